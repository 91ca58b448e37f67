"""vsg_render_level_colors and vsg_render_mean_frame on the MI355X (libvsg_render.so: the level or component
pipeline's interval list, k_color_runs, k_color_table, k_color_finish, k_color_intervals, then k_render_fill
and k_render_compose) against level_colors_model.py.  Records and pictures are compared as raw bytes: there is
no tolerance anywhere in this file."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import level_adjacency_model as am
import level_boundaries_cases as bc
import level_colors_cases as kc
import level_colors_model as km
import level_components_model as cm
import level_regions_cases as lc
import render_model as rm
import synth
import vector_cases as vc
import vector_raster_model as vm

pytestmark = pytest.mark.gpu

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "video_segment_amd", "host")
CASES = kc.all_cases()
BY_NAME = {c.name: c for c in CASES}
MODES = (0, cm.N4, cm.N8)          # the regions' table, the N4 components', the N8 components'
FILL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def vsg():
    import video_segment_amd as v
    from video_segment_amd import _lib, render
    _lib.build()
    render.build()
    assert _lib.lib().vsg_device_count() > 0
    assert (render.N4, render.N8) == (cm.N4, cm.N8)
    assert render.LEVEL_COLOR_DTYPE == km.COLOR_DTYPE
    return v


def planes(ids, connect):
    if connect == 0:
        return ids, None
    comps, _, labels = cm.sweep(ids, connect)
    return labels, comps


def model(ids, F, connect):
    P, comps = planes(ids, connect)
    return km.colors(P, F, comps)


def picture_model(r, P, F, records):
    o = r.opts
    return km.picture(P, F, records, bool(o.highlight_edges), float(o.blend_alpha), bool(o.concat_with_source),
                      bool(o.has_video))


def check_stats(st, P, what):
    want = km.stats_of(P)
    assert {k: st[k] for k in want} == want, (what, st)


def check_ids(r, seg, ids, F, level, what, modes=MODES):
    """The modes of one level against the model: table, stats, the sibling calls' records, picture."""
    out = {}
    for connect in modes:
        P, comps = planes(ids, connect)
        want = km.colors(P, F, comps)
        got = r.level_colors(seg, level, F, connect)
        assert got.dtype == km.COLOR_DTYPE and got.shape == want.shape, (what, level, connect, got.shape, want.shape)
        assert km.same_bits(got, want), (what, level, connect)
        check_stats(r.last_color_stats(), P, (what, level, connect))
        # record k belongs to record k of the call the mode is named after
        if connect == 0:
            regions, _ = r.level_regions(seg, level)
            assert np.array_equal(got["id"], regions["id"]) and (got["component"] == -1).all()
            assert np.array_equal(got["area"], regions["area"])
        else:
            sib, _ = r.level_components(seg, level, connect)
            assert np.array_equal(got["id"], sib["id"]) and np.array_equal(got["component"], sib["component"])
            assert np.array_equal(got["area"], sib["area"])
        pic = r.mean_frame(seg, level, F, connect)
        assert km.same_bits(pic, picture_model(r, P, F, want)), (what, level, connect, "picture")
        check_stats(r.last_color_stats(), P, (what, level, connect, "picture"))
        out[connect] = got
    return out


def check_case(vsg, c, **options):
    r = vsg.SegmentationRenderer(c.case.W, c.case.H, **options)
    seg = c.case.msg.SerializeToString()
    out = {level: check_ids(r, seg, lc.id_image(c.case.msg, level), c.F, level, c.name) for level in c.case.levels}
    r.close()
    return out


@pytest.mark.parametrize("W", bc.WIDTHS)
def test_widths_around_wavefront_and_block_boundaries(vsg, W):
    for H in bc.HEIGHTS:
        check_case(vsg, BY_NAME["width_%dx%d" % (W, H)])


def test_a_frame_of_one_pixel_intervals(vsg):
    c = BY_NAME["checker"]
    out = check_case(vsg, c)[0]
    assert len(out[0]) == 2 and len(out[cm.N4]) == c.case.W * c.case.H and len(out[cm.N8]) == 2
    r = vsg.SegmentationRenderer(c.case.W, c.case.H)
    r.level_colors(c.case.msg.SerializeToString(), 0, c.F)
    assert r.last_color_stats()["intervals"] == c.case.W * c.case.H
    r.close()


@pytest.mark.parametrize("share", kc.SHARES)
def test_every_number_of_intervals_a_wavefront_takes(vsg, share):
    """Short and long intervals side by side in lists long enough for k_color_runs to give a wavefront 1, 2,
    ... 64 of them."""
    c = kc.mixed(share)
    ids = lc.id_image(c.case.msg)
    r = vsg.SegmentationRenderer(c.case.W, c.case.H)
    check_ids(r, c.case.msg.SerializeToString(), ids, c.F, 0, c.name, MODES if share == 1 else (0,))
    r.level_colors(c.case.msg.SerializeToString(), 0, c.F)
    assert kc.share_of(r.last_color_stats()["intervals"]) == share
    r.close()


@pytest.mark.parametrize("name", ["star_300x2", "star_2x300"])
def test_300_regions(vsg, name):
    out = check_case(vsg, BY_NAME[name])[0]
    assert all(len(t) == 301 for t in out.values())


def test_a_comb_of_8192_intervals_in_one_group(vsg):
    c = BY_NAME["comb"]
    out = check_case(vsg, c)[0]
    assert len(out[0]) == 1 and out[0]["area"].tolist() == [kc.COMB_INTERVALS]
    assert len(out[cm.N4]) == kc.COMB[0] // 2 and len(out[cm.N8]) == kc.COMB[0] // 2
    r = vsg.SegmentationRenderer(c.case.W, c.case.H)
    r.level_colors(c.case.msg.SerializeToString(), 0, c.F)
    st = r.last_color_stats()
    assert st["largest_group_intervals"] == 8192 == st["intervals"] and st["groups"] == 1, st
    r.close()


@pytest.mark.parametrize("name", ["hole", "three_levels"])
def test_hierarchies_at_every_level(vsg, name):
    c = BY_NAME[name]
    out = check_case(vsg, c)
    assert sorted(out) == list(c.case.levels)
    if name == "hole":
        assert out[0][0]["id"].tolist() == [3, 8]
    else:
        assert [len(out[level][0]) for level in (0, 1, 2)] == [48, 20, 3]


def test_id_of_31_bits(vsg):
    out = check_case(vsg, BY_NAME["max_id"])[0]
    assert out[0]["id"].tolist() == [0, kc.MAX]


def test_a_frame_without_a_covered_pixel(vsg):
    c = BY_NAME["uncovered_frame"]
    for connect, rec in check_case(vsg, c)[0].items():
        assert len(rec) == 0 and rec.dtype == km.COLOR_DTYPE
    r = vsg.SegmentationRenderer(c.case.W, c.case.H, has_video=False)
    seg = c.case.msg.SerializeToString()
    for connect in MODES:
        assert not r.mean_frame(seg, 0, c.F, connect).any()          # black throughout
        st = r.last_color_stats()
        assert all(st[k] == 0 for k in ("groups", "intervals", "covered", "largest_group_intervals")), st
    r.close()


def test_mean_rounds_half_up_at_exact_halves(vsg):
    out = check_case(vsg, BY_NAME["halves"])[0]
    assert out[0]["mean"].tolist() == [[1, 255, 8], [11, 201, 1], [9, 90, 255]]


def one_region(vsg, W, H, value=255):
    """The table of one region over a constant frame; expected values are closed forms."""
    m = lc.desc_from_ids(np.full((H, W), 6, np.int32))
    F = np.full((H, W, 3), value, np.uint8)
    r = vsg.SegmentationRenderer(W, H, has_video=False)
    rec = r.level_colors(m.SerializeToString(), 0, F)
    st = r.last_color_stats()
    r.close()
    n = W * H
    want = np.zeros(1, km.COLOR_DTYPE)
    want["id"], want["component"], want["area"] = 6, -1, n
    want["mean"] = want["min"] = want["max"] = value
    want["sum"], want["sum_sq"] = n * value, n * value * value
    assert km.same_bits(rec, want), (W, H, rec, want)
    assert (st["groups"], st["intervals"], st["covered"], st["largest_group_intervals"]) == (1, H, n, H), st
    return rec


def test_sum_of_squares_beyond_32_bits(vsg):
    rec = one_region(vsg, 640, 104)
    assert rec["sum_sq"][0, 0] == 640 * 104 * 255 * 255 > 1 << 32


def test_the_largest_partial_of_one_interval(vsg):
    rec = one_region(vsg, 10224, 2)
    assert rec["sum_sq"][0, 0] // 2 == 10224 * 255 * 255 < 1 << 32


def test_sum_beyond_32_bits(vsg):
    rec = one_region(vsg, 4096, 4113)
    assert rec["sum"][0, 0] == 4096 * 4113 * 255 > 1 << 32


def padded(F, stride, fill, offset=0):
    """F's rows `stride` bytes apart in a buffer of `fill`, starting `offset` bytes into it: (buffer, view)."""
    H, W = F.shape[:2]
    buf = np.full(offset + H * stride, fill, np.uint8)
    view = np.lib.stride_tricks.as_strided(buf[offset:], (H, W, 3), (stride, 3, 1))
    view[:] = F
    return buf, view


def test_strides_whose_padding_holds_garbage(vsg):
    import torch
    c = BY_NAME["width_65x5"]
    W, H = c.case.W, c.case.H
    seg = c.case.msg.SerializeToString()
    ids = lc.id_image(c.case.msg)
    r = vsg.SegmentationRenderer(W, H)
    for fill in (0xFF, 0x00):
        for stride in (3 * W + 1, 3 * W + 9, 3 * W + 16):
            buf, view = padded(c.F, stride, fill)
            d_buf = torch.from_numpy(buf).cuda()
            d_view = torch.as_strided(d_buf, (H, W, 3), (stride, 3, 1))
            for connect in MODES:
                P, comps = planes(ids, connect)
                want = km.colors(P, c.F, comps)
                assert km.same_bits(r.level_colors(seg, 0, view, connect), want), ("host", fill, stride, connect)
                assert km.same_bits(r.level_colors(seg, 0, d_view, connect), want), ("device", fill, stride, connect)
                pic = picture_model(r, P, c.F, want)
                assert km.same_bits(r.mean_frame(seg, 0, view, connect), pic)
                assert km.same_bits(r.mean_frame(seg, 0, d_view, connect).cpu().numpy(), pic)
            assert np.array_equal(d_buf.cpu().numpy(), buf)          # F is read only
    r.close()


def test_an_odd_stride_and_a_pointer_offset_by_one_byte(vsg):
    """The byte path of k_color_runs: neither the pointer nor the stride is a multiple of 4."""
    import torch
    for name in ("width_257x5", "width_64x3", "three_levels"):
        c = BY_NAME[name]
        W, H = c.case.W, c.case.H
        seg = c.case.msg.SerializeToString()
        ids = lc.id_image(c.case.msg)
        r = vsg.SegmentationRenderer(W, H)
        # an unaligned pointer with an aligned stride, an aligned pointer with an unaligned stride, both unaligned
        pad = 4 - 3 * W % 4
        for stride, offset in ((3 * W + pad, 1), (3 * W + pad + 1, 0), (3 * W + pad + 2, 3), (3 * W + pad + 3, 2)):
            buf, _ = padded(c.F, stride, 0xFF, offset)
            d_buf = torch.from_numpy(buf).cuda()
            d_view = torch.as_strided(d_buf, (H, W, 3), (stride, 3, 1), offset)
            assert d_buf.data_ptr() % 4 == 0 and (d_view.data_ptr() % 4 != 0 or stride % 4 != 0)
            for connect in MODES:
                P, comps = planes(ids, connect)
                want = km.colors(P, c.F, comps)
                assert km.same_bits(r.level_colors(seg, 0, d_view, connect), want), (name, stride, offset, connect)
                assert km.same_bits(r.mean_frame(seg, 0, d_view, connect).cpu().numpy(),
                                    picture_model(r, P, c.F, want)), (name, stride, offset, connect)
        r.close()


def test_device_frame_and_device_outputs_equal_the_host_paths(vsg):
    import torch
    from video_segment_amd import render
    c = BY_NAME["three_levels"]
    seg = c.case.msg.SerializeToString()
    dev = torch.device("cuda", 0)
    d_F = torch.from_numpy(c.F).cuda()
    r = vsg.SegmentationRenderer(c.case.W, c.case.H)
    for level in c.case.levels:
        for connect in MODES:
            host = r.level_colors(seg, level, c.F, connect)
            k = len(host)
            out = torch.full((k + 3, render.LEVEL_COLOR_WORDS), FILL, dtype=torch.int32, device=dev)
            got = r.level_colors(seg, level, d_F, connect, colors_out=out)
            assert got.is_cuda and got.shape == (k, 18) and got.cpu().numpy().tobytes() == host.tobytes()
            assert bool((out[k:] == FILL).all())
            # host frame with a device table, device frame with a host table
            out.fill_(FILL)
            assert r.level_colors(seg, level, c.F, connect, colors_out=out).cpu().numpy().tobytes() == host.tobytes()
            assert km.same_bits(r.level_colors(seg, level, d_F, connect), host)
            # one record too few: refused, nothing written
            out.fill_(FILL)
            with pytest.raises(render.VsgError):
                r.level_colors(seg, level, d_F, connect, colors_out=out[:k - 1])
            assert bool((out == FILL).all())
            # the picture: device in and out, host in and device out
            pic = r.mean_frame(seg, level, c.F, connect)
            d_pic = r.mean_frame(seg, level, d_F, connect)
            assert d_pic.is_cuda and km.same_bits(d_pic.cpu().numpy(), pic)
            d_out = torch.zeros((c.case.H, c.case.W, 3), dtype=torch.uint8, device=dev)
            r.mean_frame(seg, level, c.F, connect, out=d_out)
            assert km.same_bits(d_out.cpu().numpy(), pic)
    assert bool((d_F.cpu() == torch.from_numpy(c.F)).all())
    r.close()


def test_capacity_one_short_count_only_and_refusals(vsg):
    from video_segment_amd import render
    from video_segment_amd._lib import VSG_ERR_INVALID, VsgError
    c = BY_NAME["three_levels"]
    seg = c.case.msg.SerializeToString()
    L = render.lib()
    r = vsg.SegmentationRenderer(c.case.W, c.case.H)
    F = np.ascontiguousarray(c.F)
    stride = 3 * c.case.W

    def call(level, connect, out, cap, stride=stride):
        n = C.c_size_t(77)
        rc = L.vsg_render_level_colors(r.h, seg, len(seg), level, connect, F.ctypes.data_as(C.c_void_p), stride, 0,
                                       out.ctypes.data_as(C.c_void_p) if out is not None else None, cap,
                                       C.byref(n), 0)
        return rc, n.value

    for connect in MODES:
        want = model(lc.id_image(c.case.msg, 1), F, connect)
        k = len(want)
        assert k > 1
        assert call(1, connect, None, 0) == (0, k)                              # count only
        out = np.zeros(k + 2, km.COLOR_DTYPE)
        pattern = np.frombuffer(b"\x5a" * out.nbytes, km.COLOR_DTYPE)
        for cap in (k - 1, 1, 0):
            out[:] = pattern
            assert call(1, connect, out, cap) == (VSG_ERR_INVALID, k), cap
            assert km.same_bits(out, pattern), cap
        # the handle is usable afterwards
        out[:] = pattern
        assert call(1, connect, out, k) == (0, k)
        assert km.same_bits(out[:k], want) and km.same_bits(out[k:], pattern[k:])
    # the stride is compared with the handle's width
    for bad in (0, 1, stride - 1):
        rc, _ = call(0, 0, None, 0, bad)
        assert rc == VSG_ERR_INVALID and b"stride" in L.vsg_render_last_error()
    pic = np.zeros((c.case.H, c.case.W, 3), np.uint8)
    assert L.vsg_render_mean_frame(r.h, seg, len(seg), 0, 0, F.ctypes.data_as(C.c_void_p), stride - 1, 0,
                                   pic.ctypes.data_as(C.c_void_p), 0, 0) == VSG_ERR_INVALID
    assert L.vsg_render_mean_frame(r.h, seg, len(seg), 0, 0, F.ctypes.data_as(C.c_void_p), stride, 0,
                                   pic.ctypes.data_as(C.c_void_p), stride - 1, 0) == VSG_ERR_INVALID
    assert b"out_stride" in L.vsg_render_last_error()
    # levels and connectedness
    for level in (3, 4, -1):
        for connect in MODES:
            for f in (r.level_colors, r.mean_frame):
                with pytest.raises(VsgError) as e:
                    f(seg, level, F, connect)
                assert e.value.code == VSG_ERR_INVALID
    for connect in (3, -1):
        with pytest.raises(VsgError) as e:
            r.level_colors(seg, 0, F, connect)
        assert e.value.code == VSG_ERR_INVALID
    with pytest.raises(ValueError):
        r.level_colors(seg, 0)
    assert km.same_bits(r.level_colors(seg, 2, F), model(lc.id_image(c.case.msg, 2), F, 0))
    r.close()


def test_vector_only_desc(vsg):
    W, H = 64, 48
    m = vc.vector_only(vc.l1_voronoi(11, W, H, 12))
    seg = m.SerializeToString()
    r = vsg.SegmentationRenderer(W, H)
    check_ids(r, seg, vm.id_plane(r.rasterize(seg), W, H), kc.frame(W, H, 5), 0, "vector-only")
    # at another size than the desc's: scan converted at the handle's
    r2 = vsg.SegmentationRenderer(96, 72)
    check_ids(r2, seg, vm.id_plane(r2.rasterize(seg), 96, 72), kc.frame(96, 72, 6), 0, "vector-only, scaled")
    r.close()
    r2.close()


def test_handle_reuse_with_the_other_level_calls_before_and_after(vsg):
    by = {c.name: c for c in lc.reuse_sequence()}
    small, large = by["reuse_small"], by["reuse_large"]
    r = vsg.SegmentationRenderer(small.W, small.H)
    segs = {c.name: c.msg.SerializeToString() for c in (small, large)}
    F = kc.frame(small.W, small.H, 9)

    def siblings(s):
        return (r.level_regions(s, 0), r.level_components(s, 0, cm.N8, label_image=True),
                r.level_boundaries(s, 0, cm.N4, True), r.level_adjacency(s, 0, cm.N4, am.ADJACENT_N8))

    before = {n: siblings(s) for n, s in segs.items()}
    combos = (0, cm.N8)
    ids = {c.name: lc.id_image(c.msg, 0) for c in (small, large)}
    want = {(n, k): model(ids[n], F, k) for n in ids for k in combos}
    pics = {(n, k): picture_model(r, planes(ids[n], k)[0], F, want[n, k]) for n in ids for k in combos}
    allocs = []
    for _ in range(2):
        for c in (small, large, small):
            for k in combos:
                assert km.same_bits(r.level_colors(segs[c.name], 0, F, k), want[c.name, k]), (c.name, k)
                assert km.same_bits(r.mean_frame(segs[c.name], 0, F, k), pics[c.name, k]), (c.name, k)
            # the siblings between the colour calls
            for a, b in zip(siblings(segs[c.name]), before[c.name]):
                assert all(km.same_bits(x, y) for x, y in zip(a, b)), c.name
            allocs.append(r.last_stats()["device_allocations"])
    # the second round of identical calls allocates nothing
    assert allocs[1] > allocs[0] > 0 and allocs[3:] == [allocs[2]] * 3, allocs
    r.close()


def test_launches_do_not_depend_on_the_size_or_the_content(vsg):
    counts = {}
    for name in ("width_62x1", "width_257x5", "comb", "star_2x300", "three_levels"):
        c = BY_NAME[name]
        r = vsg.SegmentationRenderer(c.case.W, c.case.H)
        seg = c.case.msg.SerializeToString()
        for connect in MODES:
            r.level_colors(seg, 0, c.F, connect)
            table = r.last_color_stats()["launches"]
            r.mean_frame(seg, 0, c.F, connect)
            counts.setdefault(connect, set()).add((table, r.last_color_stats()["launches"]))
        r.close()
    assert all(len(v) == 1 for v in counts.values()), counts


PICTURE_OPTIONS = (
    dict(highlight_edges=True, blend_alpha=0.5),
    dict(highlight_edges=False, blend_alpha=0.5),
    dict(highlight_edges=True, blend_alpha=1.0),
    dict(highlight_edges=False, blend_alpha=1.0),
    dict(highlight_edges=True, concat_with_source=True),
    dict(highlight_edges=False, concat_with_source=True),
    dict(highlight_edges=True, has_video=False),
    dict(highlight_edges=False, has_video=False),
)


@pytest.mark.parametrize("options", PICTURE_OPTIONS, ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()))
def test_picture_with_the_handles_options(vsg, options):
    for name in ("three_levels", "hole", "width_257x5", "equal_means"):
        c = BY_NAME[name]
        r = vsg.SegmentationRenderer(c.case.W, c.case.H, **options)
        seg = c.case.msg.SerializeToString()
        for level in c.case.levels:
            ids = lc.id_image(c.case.msg, level)
            for connect in MODES:
                P, comps = planes(ids, connect)
                want = picture_model(r, P, c.F, km.colors(P, c.F, comps))
                got = r.mean_frame(seg, level, c.F, connect)
                assert got.shape == (r.out_rows, c.case.W, 3)
                assert km.same_bits(got, want), (name, level, connect, options)
        r.close()


def test_two_neighbours_with_equal_means_show_no_edge(vsg):
    c = BY_NAME["equal_means"]
    r = vsg.SegmentationRenderer(c.case.W, c.case.H, has_video=False)
    seg = c.case.msg.SerializeToString()
    rec = r.level_colors(seg, 0, c.F)
    assert rec["mean"].tolist() == [[100, 50, 200], [100, 50, 200], [10, 20, 30]]
    pic = r.mean_frame(seg, 0, c.F)
    assert (pic[:-1, :7] == [100, 50, 200]).all()          # columns 3 | 4: two groups, no edge
    assert (pic[:, 7] == 0).all() and (pic[:-1, 8:-1] == [10, 20, 30]).all()
    r.close()


def test_a_padded_out_stride_whose_padding_stays_untouched(vsg):
    import torch
    c = BY_NAME["width_65x5"]
    W, H = c.case.W, c.case.H
    seg = c.case.msg.SerializeToString()
    ids = lc.id_image(c.case.msg)
    for options in (dict(), dict(concat_with_source=True)):
        r = vsg.SegmentationRenderer(W, H, **options)
        rows = r.out_rows
        want = picture_model(r, ids, c.F, km.colors(ids, c.F))
        for stride in (3 * W + 1, 3 * W + 7, 3 * W + 13):
            buf = np.full((rows, stride), 0xA5, np.uint8)
            view = buf[:, :3 * W].reshape(rows, W, 3)
            assert not view.flags["C_CONTIGUOUS"] and view.base is not None
            r.mean_frame(seg, 0, c.F, 0, out=view)
            assert km.same_bits(view, want) and (buf[:, 3 * W:] == 0xA5).all(), (options, stride)
            d_buf = torch.full((rows, stride), 0xA5, dtype=torch.uint8, device="cuda")
            d_view = torch.as_strided(d_buf, (rows, W, 3), (stride, 3, 1))
            r.mean_frame(seg, 0, c.F, 0, out=d_view)
            got = d_buf.cpu().numpy()
            assert km.same_bits(got[:, :3 * W].reshape(rows, W, 3), want) and (got[:, 3 * W:] == 0xA5).all()
        r.close()


def test_the_level_of_render_is_neither_resolved_nor_changed(vsg):
    c = BY_NAME["three_levels"]
    seg = c.case.msg.SerializeToString()
    r = vsg.SegmentationRenderer(c.case.W, c.case.H, hierarchy_level=1)
    assert r.level is None
    for level in c.case.levels:
        r.level_colors(seg, level, c.F, cm.N4)
        r.mean_frame(seg, level, c.F)
        assert r.level is None
    first = r.render(seg, c.F)
    assert r.level == 1
    model_ = rm.RenderModel(c.case.W, c.case.H, hierarchy_level=1)
    assert km.same_bits(first, model_.render(c.case.msg, c.F))
    for level in c.case.levels:
        r.mean_frame(seg, level, c.F, cm.N8)
        r.level_colors(seg, level, c.F)
        assert r.level == 1
    assert km.same_bits(r.render(seg, c.F), first)
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


def test_a_real_stream_every_frame_at_every_level(vsg, stream):
    W, H, N, _ = STREAM
    frames, segs = stream
    r = vsg.SegmentationRenderer(W, H)
    model_ = rm.RenderModel(W, H)
    heights = []
    for k, seg in enumerate(segs):
        m = lc.Msg()
        m.ParseFromString(seg)
        hier = model_._ingest(m)                 # a desc without a hierarchy uses the kept one, as the handle does
        heights.append(len(hier))
        for level in range(max(len(hier), 1)):
            # every frame and level in the regions' mode, a few frames in all three
            modes = MODES if k % 5 == 1 or k == N - 1 else (0,)
            check_ids(r, seg, model_.id_image(m, level), frames[k], level, ("stream", k), modes)
    assert min(heights) >= 1 and max(heights) >= 2, heights
    r.close()


def test_full_hd_level_0_and_top(vsg):
    import torch
    W, H = 1920, 1080
    ids = vc.l1_voronoi(12, W, H, 300)
    F = kc.frame(W, H, 14)
    m = vc.vectorize(ids)                     # rasters; the vectorization is not looked at
    top = {int(i): 5 + int(i) % 7 for i in np.unique(ids)}
    lc.add_hierarchy(m, [top])
    seg = m.SerializeToString()
    lut = np.zeros(int(ids.max()) + 1, np.int32)
    for i, p in top.items():
        lut[i] = p
    r = vsg.SegmentationRenderer(W, H)
    d_F = torch.from_numpy(F).cuda()
    comps, _, labels = cm.sweep(lut[ids], cm.N4)
    for level, connect, plane, of in ((0, 0, ids, None), (1, 0, lut[ids], None), (1, cm.N4, labels, comps)):
        want = km.colors(plane, F, of)
        assert km.same_bits(r.level_colors(seg, level, d_F, connect), want), ("1080p", level, connect)
        st = r.last_color_stats()
        check_stats(st, plane, ("1080p", level, connect))
        assert all(st[k] > 0 for k in ("plane_us", "sums_us", "table_us")) and st["paint_us"] == 0, st
        pic = r.mean_frame(seg, level, d_F, connect)
        assert km.same_bits(pic.cpu().numpy(), picture_model(r, plane, F, want)), ("1080p picture", level, connect)
        assert r.last_color_stats()["paint_us"] > 0
    r.close()


def test_driver_prints_the_python_paths_sums(vsg, stream):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    W, H, N, chunk = STREAM
    frames, segs = stream
    r = vsg.SegmentationRenderer(W, H)
    base = [os.path.join(HOST, "seg_tree_synth"), "--width", str(W), "--height", str(H), "--frames", str(N),
            "--chunk_size", str(chunk), "--input", "soft", "--flow", "--region_segmentation",
            "--chunk_set_size", "3", "--chunk_set_overlap", "1", "--min_region_num", "3", "--nouse_pipeline"]
    for flags, connect in ((["--level_colors", "0"], 0),
                           (["--level_colors", "0", "--colors_components", "--components_n8"], cm.N8)):
        lists = []
        for seg, F in zip(segs, frames):
            lists += [r.level_colors(seg, 0, F, connect), r.mean_frame(seg, 0, F, connect)]
        p = subprocess.run(base + flags, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        m = re.search(r"level_colors_groups=(\d+) level_colors_fnv1a32=(\w+)", p.stdout)
        assert m, p.stdout
        assert int(m.group(1)) == sum(len(t) for t in lists[0::2])
        assert int(m.group(2), 16) == rm.fnv1a32(lists)
    r.close()
