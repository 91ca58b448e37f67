"""vsg_render_level_pool and vsg_render_level_unpool on the MI355X (libvsg_render.so: the level or component
pipeline's interval list, k_pool_sums_planar / k_pool_sums_last, k_pool_combine, k_pool_count, k_pool_finish;
k_pool_intervals, k_render_fill, k_pool_gather_planar / _last) against level_pool_model.py.

Exact class: integer-valued features (|v| <= 2^15 for f32, 2048 for f16, 256 for bf16) add exactly in float64 in
any order, so sums, sums of squares, minima, maxima and groups are compared bit for bit.  General class: normal
random f32 features within area * 2^-52 * sum|x| of math.fsum, twice the proven bound of any float64 summation
order (gamma_(n-1) * sum|x| + u * |s|)."""
import ctypes as C
import itertools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import level_boundaries_cases as bc
import level_colors_cases as kc
import level_colors_model as km
import level_components_model as cm
import level_pool_model as pm
import level_regions_cases as lc
import render_model as rm
import synth
import vector_cases as vc
import vector_raster_model as vm

pytestmark = pytest.mark.gpu

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "video_segment_amd", "host")
BY_NAME = {c.name: c for c in kc.all_cases()}
MODES = (0, cm.N4, cm.N8)
LIMIT = {pm.F32: 1 << 15, pm.F16: 2048, pm.BF16: 256}
PLANAR_BLOCK, LAST_BLOCK, LONG, GROUP, QUAD, WAVES = 8, 64, 64, 16, 4, 1024      # render.h's kPool constants
PATTERN = 0x5A


@pytest.fixture(scope="module")
def vsg():
    import video_segment_amd as v
    from video_segment_amd import _lib, render
    _lib.build()
    render.build()
    assert _lib.lib().vsg_device_count() > 0
    assert (render.N4, render.N8) == (cm.N4, cm.N8)
    assert render.POOL_GROUP_DTYPE == pm.GROUP_DTYPE
    assert (render.POOL_F32, render.POOL_F16, render.POOL_BF16) == (pm.F32, pm.F16, pm.BF16)
    return v


def planes(ids, connect):
    if connect == 0:
        return ids, None
    comps, _, labels = cm.sweep(ids, connect)
    return labels, comps


def integers(C_, H, W, code, seed):
    """Integer-valued (C, H, W) float32 within the exact class of the format."""
    lim = LIMIT[code]
    return np.random.RandomState(seed).randint(-lim, lim + 1, (C_, H, W)).astype(np.float32)


def encode(X32, code):
    """The float32 map in the format `code` (bfloat16 as uint16); exact for the exact class."""
    return pm.convert(np.ascontiguousarray(X32, np.float32), code)


def laid_out(X, last):
    """A (C, H, W) view of a copy of X whose memory is channels-last or planar."""
    return np.ascontiguousarray(X.transpose(1, 2, 0)).transpose(2, 0, 1) if last else np.ascontiguousarray(X)


def kw(code):
    return {"dtype": "bf16"} if code == pm.BF16 else {}


def to_device(a, shift=0):
    """The numpy view a (non-negative strides) on the device with the same strides in elements, its first element
    `shift` elements into an allocation: a torch CUDA tensor (bfloat16 for uint16)."""
    import torch
    es = tuple(s // a.itemsize for s in a.strides)
    span = sum((n - 1) * s for n, s in zip(a.shape, es)) + 1
    flat = np.lib.stride_tricks.as_strided(a, (span,), (a.itemsize,))
    buf = np.zeros(shift + span, a.dtype)
    buf[shift:] = flat
    if a.dtype == np.uint16:
        t = torch.from_numpy(buf.view(np.int16)).cuda().view(torch.bfloat16)
    else:
        t = torch.from_numpy(buf).cuda()
    return torch.as_strided(t, a.shape, es, shift)


def host(x):
    if isinstance(x, np.ndarray):
        return x
    import torch
    if x.dtype == torch.bfloat16:
        return x.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    return x.cpu().numpy()


def same(got, want_groups, want, what, stats=pm.STATS):
    g, out = got
    g = host(g)
    if g.dtype != pm.GROUP_DTYPE:
        g = np.ascontiguousarray(g).view(pm.GROUP_DTYPE).reshape(-1)
    assert pm.same_bits(g, want_groups), (what, "groups", g, want_groups)
    assert sorted(out) == sorted(stats), what
    for s in stats:
        o = host(out[s])
        assert o.dtype == want[s].dtype and o.shape == want[s].shape, (what, s, o.shape, want[s].shape)
        if not pm.same_bits(o, want[s]):
            bad = np.argwhere(~((o == want[s]) | (np.isnan(o) & np.isnan(want[s]))))
            raise AssertionError((what, s, "first differences", bad[:4].tolist(),
                                  [(o[tuple(b)], want[s][tuple(b)]) for b in bad[:4]]))


def check_plane(r, seg, level, ids, X32, what, modes=MODES, codes=(pm.F32, pm.F16, pm.BF16), layouts=(False, True),
                device=False):
    """Every mode, format and layout of one level against the model, bit for bit.  X32 has to be in the exact
    class of every format asked for."""
    for connect in modes:
        P, comps = planes(ids, connect)
        want_groups, want = pm.pool(P, X32.astype(np.float64), comps)
        for code in codes:
            assert np.abs(X32).max() <= LIMIT[code]
            for last in layouts:
                a = laid_out(encode(X32, code), last)
                got = r.level_pool(seg, level, to_device(a) if device else a, connect, pm.STATS, **kw(code))
                same(got, want_groups, want, (what, level, connect, code, last))
        st = r.last_pool_stats()
        counts = km.stats_of(P)
        assert {k: st[k] for k in counts} == counts, (what, st)
        assert st["feature_bytes"] == counts["covered"] * X32.shape[0] * (4 if codes[-1] == pm.F32 else 2)


def renderer_of(vsg, case):
    return vsg.SegmentationRenderer(case.W, case.H), case.msg.SerializeToString()


# ---- exact class -------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", bc.WIDTHS)
def test_widths_around_wavefront_and_block_boundaries(vsg, W):
    for H in bc.HEIGHTS:
        c = BY_NAME["width_%dx%d" % (W, H)]
        r, seg = renderer_of(vsg, c.case)
        check_plane(r, seg, 0, lc.id_image(c.case.msg), integers(3, H, W, pm.BF16, W * 8 + H), c.name)
        r.close()


@pytest.mark.parametrize("channels", [1, 2, 3, 4, 5, PLANAR_BLOCK - 1, PLANAR_BLOCK, PLANAR_BLOCK + 1, 31, 32, 33,
                                      LAST_BLOCK - 1, LAST_BLOCK, LAST_BLOCK + 1])
def test_channel_counts_around_the_kernels_blocks(vsg, channels):
    c = BY_NAME["width_257x5"]
    r, seg = renderer_of(vsg, c.case)
    X = integers(channels, c.case.H, c.case.W, pm.F32, channels)
    check_plane(r, seg, 0, lc.id_image(c.case.msg), X, ("channels", channels), modes=(0, cm.N4), codes=(pm.F32,))
    X = integers(channels, c.case.H, c.case.W, pm.BF16, channels)
    check_plane(r, seg, 0, lc.id_image(c.case.msg), X, ("channels", channels), modes=(0,), codes=(pm.F16, pm.BF16),
                device=True)
    r.close()


def pool_slice(n):
    """PoolSlice: the intervals a wavefront of the sums kernels takes for a list of n."""
    s = 64
    while s > 1 and n // s < WAVES:
        s //= 2
    return s


def mixed(share):
    """256 columns: a one-pixel checker of two ids over the left 32, then runs of 63, 64 and 65 pixels (around the
    length from which all lanes sum an interval together), of 24 and 7 (the classes that groups of 16 and of 4
    lanes take) and of 1; 38 intervals per row, and as many rows as make the sums kernels give a wavefront `share`
    intervals."""
    W, per_row = 256, 38
    H = 8 if share == 1 else (WAVES * share + per_row - 1) // per_row + 1
    yy, xx = np.mgrid[0:H, 0:W]
    ids = np.where((xx + yy) % 2 == 0, 4, 6)
    ids[:, 32:95] = 20 + yy[:, 32:95] % 2
    ids[:, 95:159] = 30
    ids[:, 159:224] = 31
    ids[:, 224:248] = 32
    ids[:, 248:255] = 33
    ids[:, 255] = 20
    assert pool_slice(H * per_row) == share
    return ids.astype(np.int32)


@pytest.mark.parametrize("share", [1, 2, 4, 8, 16, 32, 64])
def test_every_number_of_intervals_a_wavefront_takes(vsg, share):
    ids = mixed(share)
    H, W = ids.shape
    r = vsg.SegmentationRenderer(W, H)
    seg = lc.desc_from_ids(ids).SerializeToString()
    check_plane(r, seg, 0, ids, integers(2, H, W, pm.F32, share), ("mixed", share), modes=(0,), codes=(pm.F32,))
    assert pool_slice(r.last_pool_stats()["intervals"]) == share
    if share in (1, 64):
        check_plane(r, seg, 0, ids, integers(9, H, W, pm.BF16, share), ("mixed 16-bit", share), modes=(0,),
                    codes=(pm.F16, pm.BF16), device=True)
    r.close()


def test_interval_lengths_around_the_thresholds_at_every_left_x(vsg):
    """One row per (left_x mod 8, length): lengths around 1, the 16-byte group (4 or 8 elements) and the length
    from which all lanes share an interval, each starting at every residue of left_x."""
    lengths = (1, 2, QUAD - 1, QUAD, QUAD + 1, 7, 8, 9, GROUP - 1, GROUP, GROUP + 1, LONG - 1, LONG, LONG + 1,
               2 * LONG + 3, 200)
    W = 8 + max(lengths) + 3
    rows = [(left, n) for left in range(8) for n in lengths]
    ids = np.full((len(rows), W), -1, np.int32)
    for y, (left, n) in enumerate(rows):
        ids[y, left:left + n] = 7 + y % 3
        ids[y, left + n + 1:] = 50           # a second interval behind a one-pixel gap
    H = len(rows)
    r = vsg.SegmentationRenderer(W, H)
    seg = lc.desc_from_ids(ids).SerializeToString()
    check_plane(r, seg, 0, ids, integers(3, H, W, pm.BF16, 3), "thresholds", modes=(0, cm.N4))
    check_plane(r, seg, 0, ids, integers(3, H, W, pm.BF16, 4), "thresholds, device", modes=(0,), device=True)
    r.close()


@pytest.mark.parametrize("code", [pm.F32, pm.F16, pm.BF16])
def test_base_pointers_off_the_16_byte_grid(vsg, code):
    c = BY_NAME["width_257x5"]
    r, seg = renderer_of(vsg, c.case)
    ids = lc.id_image(c.case.msg)
    X = integers(3, c.case.H, c.case.W, code, 11)
    want_groups, want = pm.pool(ids, X.astype(np.float64))
    shifts = (1, 2, 3) if code == pm.F32 else (1, 2, 3, 4, 5, 6, 7)       # 4, 8, 12 bytes; 2 ... 14 bytes
    for last in (False, True):
        a = laid_out(encode(X, code), last)
        for shift in shifts:
            d = to_device(a, shift)
            assert d.data_ptr() % 16 == shift * a.itemsize
            same(r.level_pool(seg, 0, d, 0, pm.STATS), want_groups, want, (code, last, shift))
    r.close()


def test_a_frame_of_one_pixel_intervals(vsg):
    c = BY_NAME["checker"]
    r, seg = renderer_of(vsg, c.case)
    check_plane(r, seg, 0, lc.id_image(c.case.msg), integers(5, c.case.H, c.case.W, pm.BF16, 1), "checker")
    assert r.last_pool_stats()["intervals"] == c.case.W * c.case.H
    r.close()


def test_a_comb_of_8192_intervals_in_one_group(vsg):
    c = BY_NAME["comb"]
    r, seg = renderer_of(vsg, c.case)
    ids = lc.id_image(c.case.msg)
    for channels in (1, 9, 65):
        check_plane(r, seg, 0, ids, integers(channels, c.case.H, c.case.W, pm.F32, channels), "comb", modes=(0,),
                    codes=(pm.F32,))
    st = r.last_pool_stats()
    assert st["largest_group_intervals"] == 8192 == st["intervals"] and st["groups"] == 1, st
    assert pool_slice(8192) < 64                # the group spans 8192 / pool_slice slices
    check_plane(r, seg, 0, ids, integers(3, c.case.H, c.case.W, pm.BF16, 2), "comb components", modes=(cm.N4,),
                codes=(pm.BF16,))
    r.close()


def test_a_group_over_many_full_slices(vsg):
    """Enough intervals for slices of 64, one group holding most of them and neighbours before and behind."""
    W, H = 512, 300
    ids = np.full((H, W), -1, np.int32)
    ids[:, 0::2] = 5
    ids[:3, 0::2] = 2
    ids[-2:, 0::2] = 9
    assert pool_slice(H * W // 2) == 64
    r = vsg.SegmentationRenderer(W, H)
    seg = lc.desc_from_ids(ids).SerializeToString()
    check_plane(r, seg, 0, ids, integers(3, H, W, pm.F32, 5), "many slices", modes=(0,), codes=(pm.F32,))
    r.close()


@pytest.mark.parametrize("name", ["hole", "three_levels"])
def test_hierarchies_at_every_level(vsg, name):
    c = BY_NAME[name]
    r, seg = renderer_of(vsg, c.case)
    for level in c.case.levels:
        check_plane(r, seg, level, lc.id_image(c.case.msg, level), integers(4, c.case.H, c.case.W, pm.BF16, level),
                    name)
    r.close()


def test_uncovered_frame_single_group_and_id_of_31_bits(vsg):
    c = BY_NAME["uncovered_frame"]
    r, seg = renderer_of(vsg, c.case)
    X = integers(3, c.case.H, c.case.W, pm.F32, 1)
    for connect in MODES:
        g, out = r.level_pool(seg, 0, X, connect, pm.STATS)
        assert len(g) == 0 and g.dtype == pm.GROUP_DTYPE and all(out[s].shape == (0, 3) for s in pm.STATS)
        st = r.last_pool_stats()
        assert all(st[k] == 0 for k in ("groups", "intervals", "covered", "largest_group_intervals", "feature_bytes"))
        assert (r.level_unpool(seg, 0, np.zeros((0, 3), np.float32), connect, fill=2.5) == 2.5).all()
    r.close()
    ids = np.full((7, 70), 6, np.int32)
    r = vsg.SegmentationRenderer(70, 7)
    check_plane(r, lc.desc_from_ids(ids).SerializeToString(), 0, ids, integers(3, 7, 70, pm.BF16, 2), "single group")
    r.close()
    c = BY_NAME["max_id"]
    r, seg = renderer_of(vsg, c.case)
    check_plane(r, seg, 0, lc.id_image(c.case.msg), integers(2, c.case.H, c.case.W, pm.BF16, 3), "max id")
    assert r.level_pool(seg, 0, integers(1, c.case.H, c.case.W, pm.F32, 3))[0]["id"].tolist() == [0, kc.MAX]
    r.close()


# ---- cross-check with the shipped call ---------------------------------------------------------------

@pytest.mark.parametrize("name", ["width_257x5", "three_levels", "comb", "checker"])
def test_byte_features_equal_level_colors(vsg, name):
    c = BY_NAME[name]
    r, seg = renderer_of(vsg, c.case)
    for level in c.case.levels:
        for connect in MODES:
            colors = r.level_colors(seg, level, c.F, connect)
            for last in (False, True):
                X = c.F.astype(np.float32)                       # (H, W, 3): channels-last as it is
                a = X.transpose(2, 0, 1) if last else np.ascontiguousarray(X.transpose(2, 0, 1))
                g, out = r.level_pool(seg, level, a, connect, pm.STATS)
                for field in ("id", "component", "area"):
                    assert np.array_equal(g[field], colors[field]), (name, level, connect, field)
                for s in pm.STATS:
                    assert np.array_equal(out[s], colors[s]), (name, level, connect, last, s)
                assert out["sum"].dtype == np.float64 and out["min"].dtype == np.float32
    r.close()


# ---- general class ------------------------------------------------------------------------------------

def test_normal_random_features_within_the_summation_bound(vsg):
    rng = np.random.RandomState(21)
    for name in ("three_levels", "width_257x5", "comb"):
        c = BY_NAME[name]
        r, seg = renderer_of(vsg, c.case)
        X = rng.standard_normal((5, c.case.H, c.case.W)).astype(np.float32)
        level = c.case.levels[-1]
        ids = lc.id_image(c.case.msg, level)
        for connect in (0, cm.N4):
            P, comps = planes(ids, connect)
            want_groups, want = pm.pool(P, X.astype(np.float64), comps)
            X64 = X.astype(np.float64)
            labels = np.unique(P[P >= 0])
            abs_sum = np.array([[math.fsum(np.abs(X64[ch][P == k]).tolist()) for ch in range(5)] for k in labels])
            sq_sum = np.array([[math.fsum((X64[ch][P == k] ** 2).tolist()) for ch in range(5)] for k in labels])
            area = want_groups["area"].astype(np.float64)[:, None]
            for last in (False, True):
                g, out = r.level_pool(seg, level, laid_out(X, last), connect, pm.STATS)
                assert pm.same_bits(g, want_groups)
                err = np.abs(out["sum"] - want["sum"])
                err_sq = np.abs(out["sum_sq"] - want["sum_sq"])
                print(name, connect, last, "max error / bound", (err / (area * 2.0 ** -52 * abs_sum)).max(),
                      (err_sq / (area * 2.0 ** -52 * sq_sum)).max())
                assert (err <= area * 2.0 ** -52 * abs_sum).all(), (name, connect, last)
                assert (err_sq <= area * 2.0 ** -52 * sq_sum).all(), (name, connect, last)
                assert pm.same_bits(out["min"], want["min"]) and pm.same_bits(out["max"], want["max"])
        r.close()


# ---- reproducibility ----------------------------------------------------------------------------------

def noise_ids(W, H, seed, regions=40):
    """A noise-like plane: short random runs of a few dozen ids."""
    rng = np.random.RandomState(seed)
    return np.repeat(rng.randint(0, regions, (H, W // 2)), 2, axis=1).astype(np.int32)


def test_the_same_call_twice_and_host_against_device_give_the_same_bytes(vsg):
    rng = np.random.RandomState(33)
    comb = BY_NAME["comb"]
    plans = [(lc.id_image(comb.case.msg), comb.case.msg.SerializeToString())]
    ids = noise_ids(512, 64, 3)
    plans.append((ids, lc.desc_from_ids(ids).SerializeToString()))
    for ids, seg in plans:
        H, W = ids.shape
        r = vsg.SegmentationRenderer(W, H)
        X = (rng.standard_normal((6, H, W)) * 1e3).astype(np.float32)
        for connect in (0, cm.N8):
            for last in (False, True):
                a = laid_out(X, last)
                first = r.level_pool(seg, 0, a, connect, pm.STATS)
                again = r.level_pool(seg, 0, a, connect, pm.STATS)
                dev = r.level_pool(seg, 0, to_device(a), connect, pm.STATS)
                for other in (again, dev):
                    assert pm.same_bits(first[0], host(other[0]).view(pm.GROUP_DTYPE).reshape(-1))
                    for s in pm.STATS:
                        assert pm.same_bits(first[1][s], host(other[1][s])), (connect, last, s)
        r.close()


# ---- strides, padding, NaN ----------------------------------------------------------------------------

def test_padding_and_uncovered_pixels_full_of_nan_are_never_read(vsg):
    c = BY_NAME["three_levels"]
    r, seg = renderer_of(vsg, c.case)
    W, H = c.case.W, c.case.H
    ids = lc.id_image(c.case.msg, 1).copy()
    X = integers(3, H, W, pm.F32, 8)
    # planar with padded rows and planes
    buf = np.full((3, H + 2, W + 5), np.nan, np.float32)
    buf[:, :H, :W] = X
    planar = buf[:, :H, :W]
    # channels-last, C = 3 with pixel_stride 4, and padded rows
    buf4 = np.full((H, W + 3, 4), np.nan, np.float32)
    buf4[:, :W, :3] = X.transpose(1, 2, 0)
    last = buf4[:, :W, :3].transpose(2, 0, 1)
    for connect in MODES:
        P, comps = planes(ids, connect)
        want_groups, want = pm.pool(P, X.astype(np.float64), comps)
        for a in (planar, last):
            for x in (a, to_device(a)):
                got = r.level_pool(seg, 1, x, connect, pm.STATS)
                same(got, want_groups, want, ("padding", connect))
                assert not any(np.isnan(host(got[1][s])).any() for s in pm.STATS)
    r.close()
    # uncovered pixels holding NaN
    hole = np.full((6, 70), 4, np.int32)
    hole[2:4, 10:60] = -1
    hole[5, 69] = -1
    Xh = integers(2, 6, 70, pm.BF16, 9)
    want_groups, want = pm.pool(hole, Xh.astype(np.float64))
    Xh[:, hole < 0] = np.nan
    r = vsg.SegmentationRenderer(70, 6)
    seg = lc.desc_from_ids(hole).SerializeToString()
    for code in (pm.F32, pm.F16, pm.BF16):
        for lay in (False, True):
            same(r.level_pool(seg, 0, laid_out(encode(Xh, code), lay), 0, pm.STATS, **kw(code)), want_groups, want,
                 ("uncovered NaN", code, lay))
    r.close()


def test_nan_and_infinities_follow_the_rule_and_touch_nothing_else(vsg):
    ids = np.zeros((4, 80), np.int32)
    ids[:, 20:40] = 1
    ids[:, 40:] = 2
    base = integers(3, 4, 80, pm.F32, 12)
    r = vsg.SegmentationRenderer(80, 4)
    seg = lc.desc_from_ids(ids).SerializeToString()
    clean_groups, clean = pm.pool(ids, base.astype(np.float64))
    X = base.copy()
    X[1, 2, 5] = np.nan                       # one NaN in group 0, channel 1
    X[1, 0, 25], X[1, 3, 30] = np.inf, -np.inf   # +inf with -inf in group 1, channel 1
    X[1][ids == 2] = np.nan                   # group 2, channel 1: nothing but NaN
    for last in (False, True):
        for x in (laid_out(X, last), to_device(laid_out(X, last))):
            g, out = r.level_pool(seg, 0, x, 0, pm.STATS)
            out = {s: host(out[s]) for s in pm.STATS}
            for s in pm.STATS:                # channels 0 and 2 are untouched
                assert pm.same_bits(out[s][:, [0, 2]], clean[s][:, [0, 2]]), s
            assert np.isnan(out["sum"][:, 1]).all()
            assert np.isnan(out["sum_sq"][0, 1]) and out["sum_sq"][1, 1] == np.inf and np.isnan(out["sum_sq"][2, 1])
            rest = np.delete(base[1][ids == 0], 2 * 20 + 5)
            assert out["min"][0, 1] == rest.min() and out["max"][0, 1] == rest.max()
            assert out["min"][1, 1] == -np.inf and out["max"][1, 1] == np.inf
            assert out["min"][2, 1] == np.inf and out["max"][2, 1] == -np.inf
    r.close()


# ---- unpool -------------------------------------------------------------------------------------------

def values_of(R, C_, seed):
    v = np.random.RandomState(seed).standard_normal((R, C_)).astype(np.float32) * 300
    v.flat[::7] = np.float32(1.00390625)       # a tie of the bfloat16 rounding
    v.flat[3::11] = np.float32(2049.0)         # a tie of the half rounding
    return v


@pytest.mark.parametrize("name", ["three_levels", "width_257x5", "hole"])
def test_unpool_equals_the_model(vsg, name):
    import torch
    from video_segment_amd import render
    c = BY_NAME[name]
    r, seg = renderer_of(vsg, c.case)
    W, H = c.case.W, c.case.H
    for level in c.case.levels:
        ids = lc.id_image(c.case.msg, level)
        for connect in MODES:
            P, _ = planes(ids, connect)
            R = len(np.unique(P[P >= 0]))
            for channels in (1, 3, 9):
                v = values_of(R, channels, R + channels)
                for code, name_ in ((pm.F32, "float32"), (pm.F16, "float16"), (pm.BF16, "bf16")):
                    want = pm.unpool(P, v, -7.25, code)
                    for last in (False, True):
                        got = r.level_unpool(seg, level, v, connect, fill=-7.25, dtype=name_, channels_last=last)
                        assert got.shape == want.shape and pm.same_bits(np.ascontiguousarray(got), want), (
                            name, level, connect, channels, code, last)
                        d = r.level_unpool(seg, level, torch.from_numpy(v).cuda(), connect, fill=-7.25, dtype=name_,
                                           channels_last=last)
                        assert d.is_cuda and pm.same_bits(host(d), want), (name, level, connect, channels, code, last)
            # wrong num_values: refused, out untouched
            out = np.full((2, H, W), 5.0, np.float32)
            for wrong in (R - 1, R + 1):
                with pytest.raises(render.VsgError) as e:
                    r.level_unpool(seg, level, np.zeros((wrong, 2), np.float32), connect, out=out)
                assert e.value.code == -1 and (out == 5.0).all()
    r.close()


def test_unpool_leaves_padding_alone_and_pools_back_to_area_times_value(vsg):
    import torch
    c = BY_NAME["three_levels"]
    r, seg = renderer_of(vsg, c.case)
    W, H = c.case.W, c.case.H
    ids = lc.id_image(c.case.msg, 1)
    P, _ = planes(ids, cm.N4)
    R = len(np.unique(P[P >= 0]))
    v = np.random.RandomState(2).randint(-200, 201, (R, 3)).astype(np.float32)
    want = pm.unpool(P, v, 0.0)
    for code, kind in ((pm.F32, np.float32), (pm.F16, np.float16)):
        # planar with padded rows and planes; channels-last with pixel_stride 4 and padded rows
        buf = np.full((3, H + 1, W + 3), 77, kind)
        buf4 = np.full((H, W + 2, 4), 77, kind)
        for b, view in ((buf, buf[:, :H, :W]), (buf4, buf4[:, :W, :3].transpose(2, 0, 1))):
            mask = np.ones(b.shape, bool)
            (mask[:, :H, :W] if b is buf else mask[:, :W, :3])[...] = False
            r.level_unpool(seg, 1, v, cm.N4, out=view)
            assert pm.same_bits(np.ascontiguousarray(view), want.astype(kind)) and (b[mask] == 77).all()
            d = to_device(view)
            r.level_unpool(seg, 1, torch.from_numpy(v).cuda(), cm.N4, out=d)
            assert pm.same_bits(host(d), want.astype(kind))
            whole = torch.as_strided(d, (d.untyped_storage().nbytes() // d.element_size(),), (1,), 0).cpu().numpy()
            flat = np.lib.stride_tricks.as_strided(view, whole.shape, (view.itemsize,))
            assert pm.same_bits(whole, flat)     # padding included
            g, out = r.level_pool(seg, 1, view, cm.N4, ("sum",))
            assert np.array_equal(out["sum"], g["area"][:, None] * v.astype(np.float64))
    r.close()


# ---- plumbing -----------------------------------------------------------------------------------------

def test_every_subset_of_the_statistics_and_every_memory_combination(vsg):
    import torch
    c = BY_NAME["three_levels"]
    r, seg = renderer_of(vsg, c.case)
    ids = lc.id_image(c.case.msg, 1)
    X = integers(9, c.case.H, c.case.W, pm.F32, 4)
    want_groups, want = pm.pool(ids, X.astype(np.float64))
    for k in range(5):
        for stats in itertools.combinations(pm.STATS, k):
            for last in (False, True):
                a = laid_out(X, last)
                same(r.level_pool(seg, 1, a, 0, stats), want_groups, want, (stats, last, "host"), stats)
                same(r.level_pool(seg, 1, to_device(a), 0, stats), want_groups, want, (stats, last, "device"), stats)
    # host input with device outputs and the reverse, through the C entry
    from video_segment_amd import render
    L = render.lib()
    R = len(want_groups)
    d_X = torch.from_numpy(X).cuda()
    d_sum = torch.zeros((R, 9), dtype=torch.float64, device="cuda")
    h_max = np.zeros((R, 9), np.float32)
    n = C.c_size_t()
    vp = C.c_void_p
    assert L.vsg_render_level_pool(r.h, seg, len(seg), 1, 0, vp(X.ctypes.data), 0, 9, X[0].size, c.case.W, 1, 0,
                                   None, vp(d_sum.data_ptr()), None, None, None, R, C.byref(n), 1) == 0
    assert pm.same_bits(d_sum.cpu().numpy(), want["sum"])
    assert L.vsg_render_level_pool(r.h, seg, len(seg), 1, 0, vp(d_X.data_ptr()), 0, 9, X[0].size, c.case.W, 1, 1,
                                   None, None, None, None, vp(h_max.ctypes.data), R, C.byref(n), 0) == 0
    assert pm.same_bits(h_max, want["max"])
    r.close()


def test_capacity_one_short_count_only_and_refusals(vsg):
    from video_segment_amd import render
    from video_segment_amd._lib import VSG_ERR_INVALID, VsgError
    c = BY_NAME["three_levels"]
    r, seg = renderer_of(vsg, c.case)
    L = render.lib()
    W, H = c.case.W, c.case.H
    X = integers(3, H, W, pm.F32, 6)
    vp = C.c_void_p

    def call(connect, outs, cap, strides=(W * H, W, 1)):
        n = C.c_size_t(77)
        rc = L.vsg_render_level_pool(r.h, seg, len(seg), 1, connect, vp(X.ctypes.data), 0, 3, *strides, 0,
                                     *[vp(o.ctypes.data) if o is not None else None for o in outs], cap,
                                     C.byref(n), 0)
        return rc, n.value

    for connect in MODES:
        P, comps = planes(lc.id_image(c.case.msg, 1), connect)
        want_groups, want = pm.pool(P, X.astype(np.float64), comps)
        k = len(want_groups)
        assert k > 1
        assert call(connect, [None] * 5, 0) == (0, k)                       # count only
        outs = [np.zeros(k + 2, pm.GROUP_DTYPE), np.zeros((k + 2, 3)), np.zeros((k + 2, 3)),
                np.zeros((k + 2, 3), np.float32), np.zeros((k + 2, 3), np.float32)]
        patterns = [np.frombuffer(bytes([PATTERN]) * o.nbytes, o.dtype).reshape(o.shape) for o in outs]
        for cap in (k - 1, 1):
            for o, p in zip(outs, patterns):
                o[...] = p
            assert call(connect, outs, cap) == (VSG_ERR_INVALID, k), cap
            assert all(pm.same_bits(o, p) for o, p in zip(outs, patterns)), cap
        # the handle is usable afterwards
        assert call(connect, outs, k) == (0, k)
        assert pm.same_bits(outs[0][:k], want_groups) and pm.same_bits(outs[0][k:], patterns[0][k:])
        for o, p, s in zip(outs[1:], patterns[1:], pm.STATS):
            assert pm.same_bits(o[:k], want[s]) and pm.same_bits(o[k:], p[k:]), s
    # disjointness is compared with the handle's size
    for strides in ((W * H, W - 1, 1), (W * H - 1, W, 1), (W, 2 * W, 1)):
        rc, _ = call(0, [None] * 5, 0, strides)
        assert rc == VSG_ERR_INVALID and b"overlap" in L.vsg_render_last_error()
    assert call(0, [None] * 5, 0, (W, 3 * W, 1))[0] == 0                     # planes interleaved row by row
    for level in (3, -1):
        with pytest.raises(VsgError) as e:
            r.level_pool(seg, level, X)
        assert e.value.code == VSG_ERR_INVALID
    with pytest.raises(ValueError):
        r.level_pool(seg, 0)
    r.close()


def test_handle_reuse_with_the_other_level_calls_before_and_after(vsg):
    by = {c.name: c for c in lc.reuse_sequence()}
    small, large = by["reuse_small"], by["reuse_large"]
    r = vsg.SegmentationRenderer(small.W, small.H)
    segs = {c.name: c.msg.SerializeToString() for c in (small, large)}
    F = kc.frame(small.W, small.H, 9)
    X = integers(5, small.H, small.W, pm.F32, 10)
    ids = {c.name: lc.id_image(c.msg, 0) for c in (small, large)}
    combos = (0, cm.N8)
    want = {(n, k): pm.pool(*planes(ids[n], k)[:1], X.astype(np.float64), planes(ids[n], k)[1])
            for n in ids for k in combos}
    colors = {n: r.level_colors(s, 0, F) for n, s in segs.items()}
    regions = {n: r.level_regions(s, 0) for n, s in segs.items()}
    allocs = []
    for _ in range(2):
        for c in (small, large, small):
            for k in combos:
                for last in (False, True):
                    same(r.level_pool(segs[c.name], 0, laid_out(X, last), k, pm.STATS), *want[c.name, k], (c.name, k))
                P = planes(ids[c.name], k)[0]
                v = values_of(len(want[c.name, k][0]), 2, 1)
                assert pm.same_bits(r.level_unpool(segs[c.name], 0, v, k), pm.unpool(P, v))
            assert km.same_bits(r.level_colors(segs[c.name], 0, F), colors[c.name])
            assert all(km.same_bits(a, b) for a, b in zip(r.level_regions(segs[c.name], 0), regions[c.name]))
            allocs.append(r.last_stats()["device_allocations"])
    assert allocs[1] > allocs[0] > 0 and allocs[3:] == [allocs[2]] * 3, allocs
    r.close()


def test_launches_do_not_depend_on_size_content_or_channels(vsg):
    counts = {}
    for name, channels in (("width_62x1", 1), ("width_257x5", 3), ("comb", 64), ("star_2x300", 9),
                           ("three_levels", 130)):
        c = BY_NAME[name]
        r, seg = renderer_of(vsg, c.case)
        X = integers(channels, c.case.H, c.case.W, pm.F32, 1)
        for connect in MODES:
            for last in (False, True):
                g, _ = r.level_pool(seg, 0, laid_out(X, last), connect, pm.STATS)
                pool_launches = r.last_pool_stats()["launches"]
                r.level_unpool(seg, 0, np.zeros((len(g), channels), np.float32), connect, channels_last=last)
                counts.setdefault((connect, last), set()).add((pool_launches, r.last_pool_stats()["launches"]))
        r.close()
    assert all(len(v) == 1 for v in counts.values()), counts


def test_the_level_of_render_is_neither_resolved_nor_changed(vsg):
    c = BY_NAME["three_levels"]
    r = vsg.SegmentationRenderer(c.case.W, c.case.H, hierarchy_level=1)
    seg = c.case.msg.SerializeToString()
    X = integers(2, c.case.H, c.case.W, pm.F32, 1)
    assert r.level is None
    for level in c.case.levels:
        g, _ = r.level_pool(seg, level, X, cm.N4)
        r.level_unpool(seg, level, np.zeros((len(g), 1), np.float32), cm.N4)
        assert r.level is None
    first = r.render(seg, c.F)
    assert r.level == 1
    for level in c.case.levels:
        g, _ = r.level_pool(seg, level, X)
        r.level_unpool(seg, level, np.zeros((len(g), 1), np.float32))
        assert r.level == 1
    assert km.same_bits(r.render(seg, c.F), first)
    r.close()


def test_vector_only_desc(vsg):
    W, H = 64, 48
    m = vc.vector_only(vc.l1_voronoi(11, W, H, 12))
    seg = m.SerializeToString()
    for w, h in ((W, H), (96, 72)):             # at its own size and scan converted at another
        r = vsg.SegmentationRenderer(w, h)
        check_plane(r, seg, 0, vm.id_plane(r.rasterize(seg), w, h), integers(3, h, w, pm.BF16, w), "vector-only",
                    codes=(pm.F32, pm.BF16))
        r.close()


STREAM = (96, 64, 16, 8)   # W, H, frames, chunk size


@pytest.fixture(scope="module")
def stream(vsg):
    """The synth stream through the dense unit and the hierarchical stage: (frames, serialized descs)."""
    W, H, N, chunk = STREAM
    fl = synth.const_flow(W, H)
    frames = [synth.soft_frame(W, H, k) for k in range(N)]
    d = vsg.DenseSegmentation(W, H, vsg.default_options(chunk_size=chunk), has_flow=True)
    reg = vsg.RegionSegmentation(W, H, vsg.default_region_options(chunk_set_size=3, chunk_set_overlap=1,
                                                                  constraint_chunks=1, min_region_num=3))
    over, segs = [], []
    for k in range(N):
        n = d.process_frame(frames[k], fl if k > 0 else None, flush=(k == N - 1))
        over += [d.result_bytes(i) for i in range(n)]
    for k, seg in enumerate(over):
        n = reg.process_frame(seg, frames[k], fl if k > 0 else None, flush=(k == N - 1))
        segs += [reg.result_bytes(i) for i in range(n)]
    d.close()
    reg.close()
    assert len(segs) == N
    return frames, segs


def test_a_real_stream_at_every_level(vsg, stream):
    W, H, N, _ = STREAM
    frames, segs = stream
    r = vsg.SegmentationRenderer(W, H)
    model_ = rm.RenderModel(W, H)
    heights = []
    for k, seg in enumerate(segs):
        m = lc.Msg()
        m.ParseFromString(seg)
        hier = model_._ingest(m)
        heights.append(len(hier))
        # every frame (a desc without a hierarchy uses the one the handle kept) in the regions' mode, a few in more
        more = k % 5 == 1 or k == N - 1
        for level in range(max(len(hier), 1)):
            check_plane(r, seg, level, model_.id_image(m, level), integers(3, H, W, pm.BF16, k), ("stream", k),
                        modes=(0, cm.N8) if more else (0,), codes=(pm.F32, pm.BF16) if more else (pm.F32,))
    assert min(heights) >= 1 and max(heights) >= 2, heights
    r.close()


def test_full_hd_level_0_and_top(vsg):
    W, H = 1920, 1080
    ids = vc.l1_voronoi(12, W, H, 300)
    m = vc.vectorize(ids)
    top = {int(i): 5 + int(i) % 7 for i in np.unique(ids)}
    lc.add_hierarchy(m, [top])
    seg = m.SerializeToString()
    lut = np.zeros(int(ids.max()) + 1, np.int32)
    for i, p in top.items():
        lut[i] = p
    X = integers(8, H, W, pm.F32, 14)
    r = vsg.SegmentationRenderer(W, H)
    for level, plane in ((0, ids), (1, lut[ids])):
        want_groups, want = pm.pool(plane, X.astype(np.float64))
        for last in (False, True):
            d = to_device(laid_out(X, last))
            same(r.level_pool(seg, level, d, 0, pm.STATS), want_groups, want, ("1080p", level, last))
            st = r.last_pool_stats()
            assert all(st[k] > 0 for k in ("plane_us", "sums_us", "table_us")) and st["paint_us"] == 0, st
            assert st["feature_bytes"] == W * H * 8 * 4
    r.close()


def test_driver_prints_the_channel_sums_of_level_colors(vsg, stream):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    W, H, N, chunk = STREAM
    base = [os.path.join(HOST, "seg_tree_synth"), "--width", str(W), "--height", str(H), "--frames", str(N),
            "--chunk_size", str(chunk), "--input", "soft", "--flow", "--region_segmentation",
            "--chunk_set_size", "3", "--chunk_set_overlap", "1", "--min_region_num", "3", "--nouse_pipeline"]
    frames, segs = stream
    r = vsg.SegmentationRenderer(W, H)
    for flags, connect in ((["--level_pool", "0"], 0),
                           (["--level_pool", "0", "--pool_components", "--components_n8"], cm.N8)):
        groups, bgr = 0, np.zeros(3, np.int64)
        for seg, F in zip(segs, frames):
            t = r.level_colors(seg, 0, F, connect)
            groups += len(t)
            bgr += t["sum"].sum(axis=0)
        covered = sum(int(r.level_colors(seg, 0, F, connect)["area"].sum()) for seg, F in zip(segs, frames))
        p = subprocess.run(base + flags, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        m = re.search(r"level_pool_groups=(\d+) level_pool_sums=([-\d.,e+]+) level_pool_fnv1a32=(\w+)", p.stdout)
        assert m, p.stdout
        sums = [float(v) for v in m.group(2).split(",")]
        assert int(m.group(1)) == groups and len(sums) == 5
        assert sums[:3] == [float(v) for v in bgr]          # B, G, R: the --level_colors sums of the same run
        assert covered == W * H * N                          # so x and y sum over every pixel of every frame
        assert sums[3:] == [N * H * W * (W - 1) / 2.0, N * W * H * (H - 1) / 2.0]
    r.close()


# ---- autograd -----------------------------------------------------------------------------------------

def test_gradients_equal_the_dense_one_hot_formulation(vsg):
    import torch
    from video_segment_amd import render
    c = BY_NAME["three_levels"]
    r, seg = renderer_of(vsg, c.case)
    W, H = c.case.W, c.case.H
    for level, connect in ((0, 0), (1, cm.N4), (2, 0)):
        P, _ = planes(lc.id_image(c.case.msg, level), connect)
        labels = np.unique(P[P >= 0])
        R = len(labels)
        onehot = torch.from_numpy((P.reshape(1, -1) == labels[:, None]).astype(np.float32)).cuda()    # (R, HW)
        area = onehot.sum(dim=1, keepdim=True)
        pool, unpool = render.region_pool(r, seg, level, connectedness=connect)
        rng = np.random.RandomState(level)
        x = torch.from_numpy(rng.randint(-64, 65, (3, H, W)).astype(np.float32)).cuda()
        weight = torch.from_numpy(rng.randint(-8, 9, (R, 3)).astype(np.float32)).cuda()
        a = x.clone().requires_grad_(True)
        b = x.clone().requires_grad_(True)
        got = pool(a)
        ref = (onehot @ b.reshape(3, -1).t()) / area
        assert got.shape == (R, 3) and torch.equal(got, ref)
        (got * weight).sum().backward()
        (ref * weight).sum().backward()
        assert torch.equal(a.grad, b.grad)
        v = torch.from_numpy(rng.randint(-64, 65, (R, 3)).astype(np.float32)).cuda()
        up_weight = torch.from_numpy(rng.randint(-8, 9, (3, H, W)).astype(np.float32)).cuda()
        a = v.clone().requires_grad_(True)
        b = v.clone().requires_grad_(True)
        got = unpool(a)
        ref = (onehot.t() @ b).t().reshape(3, H, W)
        assert torch.equal(got, ref)
        (got * up_weight).sum().backward()
        (ref * up_weight).sum().backward()
        assert torch.equal(a.grad, b.grad)
    r.close()


def test_gradients_that_are_broadcast_views(vsg):
    """sum and mean over an axis hand the backward an expanded gradient (a stride of 0), which is no layout."""
    import torch
    from video_segment_amd import render
    c = BY_NAME["three_levels"]
    r, seg = renderer_of(vsg, c.case)
    W, H = c.case.W, c.case.H
    P = lc.id_image(c.case.msg, 1)
    labels = np.unique(P[P >= 0])
    R = len(labels)
    onehot = torch.from_numpy((P.reshape(1, -1) == labels[:, None]).astype(np.float32)).cuda()
    pool, unpool = render.region_pool(r, seg, 1)
    v = torch.from_numpy(np.random.RandomState(5).randint(-64, 65, (R, 4)).astype(np.float32)).cuda()
    for reduce in (lambda t: t.sum(dim=0).sum(), lambda t: t.sum(dim=1).sum(), lambda t: t.sum(dim=2).sum(),
                   lambda t: t.sum(), lambda t: (t.permute(2, 1, 0) * 2).sum()):
        a = v.clone().requires_grad_(True)
        b = v.clone().requires_grad_(True)
        reduce(unpool(a)).backward()
        reduce((onehot.t() @ b).t().reshape(4, H, W)).backward()
        assert torch.equal(a.grad, b.grad)
    x = torch.from_numpy(np.random.RandomState(6).randint(-64, 65, (4, H, W)).astype(np.float32)).cuda()
    for view in (x, x.permute(0, 2, 1).contiguous().permute(0, 2, 1), x[:, :, :].expand(4, H, W)):
        a = view.clone(memory_format=torch.preserve_format).requires_grad_(True)
        got = pool(a)
        ref = (onehot @ view.reshape(4, -1).t()) / onehot.sum(dim=1, keepdim=True)
        assert torch.equal(got, ref)
        got.sum(dim=1).sum().backward()          # an expanded (R, C) gradient
        assert torch.equal(a.grad, (onehot.t() @ (1.0 / onehot.sum(dim=1, keepdim=True)).expand(R, 4)).t()
                           .reshape(4, H, W))
    r.close()
