"""CPU-side checks of the dense flow unit: the numpy model that defines it (tests/flow_model.py),
the host-only luminance hook, and the C ABI's symbols.  The GPU comparison is test_gpu_flow.py."""
import ctypes as C
import hashlib
import json
import os
import re

import numpy as np
import pytest

import flow_cases as fc
import flow_model as fm
from video_segment_amd import flow

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def library():
    flow.build()
    return flow.lib()


# ---- 1. luminance ----------------------------------------------------------------------------------
def test_luminance_hand_values():
    px = np.array([[[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255],
                    # 1868 * 4 + 8192 = 15664 -> 0; 1868 * 5 + 8192 = 17532 -> 1
                    [4, 0, 0], [5, 0, 0],
                    # 9617 * 11 + 4899 * 2 + 8192 = 123777 = 7.55 * 16384 -> 7
                    [0, 11, 2],
                    # 9617 + 8192 -> 1; 4899 + 8192 -> 0; 2 * 4899 + 8192 -> 1
                    [0, 1, 0], [0, 0, 1], [0, 0, 2]]], np.uint8)
    want = [0, 255, 29, 150, 76, 0, 1, 7, 1, 0, 1]
    # (1868 * 255 + 8192) >> 14 = 29, (9617 * 255 + 8192) >> 14 = 150, (4899 * 255 + 8192) >> 14 = 76
    assert fm.luminance(px)[0].tolist() == want


def test_luminance_rounds_half_up():
    """1868 B + 9617 G + 4899 R = 16384 k + 8192 is a value of exactly k + .5: it rounds up.  The
    byte triples that hit it are found by search."""
    b, g, r = np.meshgrid(np.arange(256), np.arange(256), np.arange(0, 256, 5), indexing="ij")
    s = 1868 * b + 9617 * g + 4899 * r
    half = np.argwhere(s % 16384 == 8192)
    assert len(half) > 0
    for bb, gg, rr in half[:50]:
        px = np.array([[[b[bb, gg, rr], g[bb, gg, rr], r[bb, gg, rr]]]], np.uint8)
        assert int(fm.luminance(px)[0, 0]) == s[bb, gg, rr] // 16384 + 1


def test_luminance_hook_equals_model(library):
    rng = np.random.RandomState(3)
    for (W, H, pad) in [(67, 45, 0), (16, 9, 7), (1, 1, 0)]:
        buf = rng.randint(0, 256, (H, W * 3 + pad), dtype=np.uint8)
        bgr = buf[:, :W * 3].reshape(H, W, 3)
        assert np.array_equal(flow.luminance(bgr), fm.luminance(bgr))


def test_gray_to_bgr_keeps_luminance():
    g = np.arange(256, dtype=np.uint8).reshape(16, 16)
    assert np.array_equal(fm.luminance(fm.gray_to_bgr(g)), g)


# ---- 2. pyramid -------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,sizes", [
    (256, 256, [(256, 256), (128, 128), (64, 64), (32, 32), (16, 16)]),
    (320, 240, [(320, 240), (160, 120), (80, 60), (40, 30)]),
    (96, 64, [(96, 64), (48, 32), (24, 16)]),
    (16, 16, [(16, 16)]),
    (15, 9, [(15, 9)]),
    (33, 31, [(33, 31), (17, 16)]),
    (4096, 4096, [(4096, 4096), (2048, 2048), (1024, 1024), (512, 512), (256, 256)]),
])
def test_pyramid_sizes(W, H, sizes):
    assert fm.pyramid_sizes(W, H) == sizes
    if W * H <= 320 * 240:
        levels = fm.pyramid(np.zeros((H, W), np.uint8))
        assert [(l.shape[1], l.shape[0]) for l in levels] == sizes


def test_pyr_down_values():
    # a constant stays constant (the taps sum to 256), at odd sizes too
    assert np.all(fm.pyr_down(np.full((31, 33), 77, np.float32)) == 77)
    # a horizontal ramp: reflect-101 at both borders, by hand for the first and last column
    src = np.tile(np.arange(17, dtype=np.float32), (16, 1))
    out = fm.pyr_down(src)
    assert out.shape == (8, 9) and out.dtype == np.float32
    assert out[0, 0] == (6 * 0 + 4 * (1 + 1) + 2 + 2) / 16.0       # taps -2, -1 -> 2, 1
    assert out[0, 4] == 8.0
    assert out[0, 8] == (6 * 16 + 4 * (15 + 15) + 14 + 14) / 16.0   # taps 17, 18 -> 15, 14


# ---- 3. identical frames ---------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(96, 64), (33, 31), (15, 9)])
def test_identical_frames_give_zero_flow(W, H):
    f = fm.value_noise(W, H, 5)
    flw, info = fm.tvl1(f, f, iterations=10, warps=2)
    assert not flw.any()
    assert info["iterations_run"] == info["scales"] * 2   # one iteration per warp, then the stop test


# ---- 4. a known motion -----------------------------------------------------------------------------
def test_translation_is_recovered():
    """Content moving by (+3, -2) per frame: the backward flow is (-3, +2).  The mean endpoint error
    16 px inside has to be below half the motion's magnitude (zero flow scores the full one)."""
    prev, cur = fm.translated_pattern(128, 96, 2, seed=7)
    flw, info = fm.tvl1(cur, prev)
    assert info["scales"] == 3
    d = flw - np.array([-3.0, 2.0], np.float32)
    epe = float(np.sqrt((d.astype(np.float64) ** 2).sum(-1))[16:-16, 16:-16].mean())
    mag = 13.0 ** 0.5
    print("mean endpoint error %.4f px, motion %.4f px" % (epe, mag))
    assert epe < 0.5 * mag


# ---- 5. no stop test of a GPU input is near its threshold -------------------------------------------
def test_stop_margins_of_gpu_inputs():
    """The device sums the error terms in another order than numpy.  Both sums are f64 sums of at most
    8 M non-negative f32 terms, so they differ by less than 8e6 * 2^-53 < 1e-9 relative: a margin of
    1e-6 means no iteration count can depend on the order."""
    infos = fc.all_infos()
    assert len(infos) > 60
    worst = min(infos, key=lambda li: li[1]["margin"])
    print("smallest margin %.3e at %s" % (worst[1]["margin"], worst[0]))
    for label, info in infos:
        assert info["margin"] >= 1e-6, (label, info)


def test_stop_cases_stop_mid_loop():
    """Every block input has a flow whose stop test fires inside a loop: later than after each warp's
    first iteration, earlier than after all of them."""
    for c in fc.STOP_CASES:
        _, infos = fc.model(*c)
        assert any(i["scales"] * c[4] < i["iterations_run"] < i["scales"] * c[4] * c[3] for i in infos[1:]), c


# ---- 6. the model's arithmetic is pinned; its counters stand beside it --------------------------------
def test_model_flows_equal_their_pins():
    """tests/golden/flow_model_pins.json holds SHA-256 sums of the model's flows for one case of each
    list, taken before the counters of info["tests"] and info["warps"] were added."""
    pins = json.load(open(os.path.join(ROOT, "tests", "golden", "flow_model_pins.json")))["cases"]
    cases = [tuple(p["case"]) for p in pins]
    assert [sum(c in l for c in cases) for l in (fc.SEQUENCE_CASES, fc.OPTION_CASES, fc.STOP_CASES)] == [1, 1, 1]
    for p, c in zip(pins, cases):
        flows, infos = fc.model(*c)
        h = hashlib.sha256()
        for f in flows[1:]:
            assert f.dtype == np.float32 and f.shape == (c[2], c[1], 2)
            h.update(f.tobytes())
        assert h.hexdigest() == p["sha256"], c
        assert [i["iterations_run"] for i in infos[1:]] == p["iterations_run"], c


def test_counters_by_hand():
    # tile sums: 33 x 9 is 2 x 2 tiles, the second column and row one pixel wide
    err = np.arange(33 * 9, dtype=np.float32).reshape(9, 33)
    t = fm.tile_sums(err)
    assert t.dtype == np.float64 and t.tolist() == [float(err[:8, :32].sum()), float(err[:8, 32].sum()),
                                                   float(err[8, :32].sum()), float(err[8, 32])]
    # warp counters on a 20 x 10 plane.  u = 0: the footprint x - 1 .. x + 2 leaves the plane at
    # x = 0 (1 column), x = W - 2 (1) and x = W - 1 (2), rows alike
    z = np.zeros((10, 20), np.float32)
    c = {}
    fm.warp3((z,), z, z, c)
    cols_in, rows_in = 20 * 4 - 4, 10 * 4 - 4
    assert c == {"outside_taps": 16 * 200 - cols_in * rows_in, "clamped": 0}
    # u1 = +30 puts every floor(x + u1) past W + 4 = 24
    fm.warp3((z,), z + np.float32(30), z, c)
    assert c == {"outside_taps": 16 * 200, "clamped": 200}
    u = z.copy()
    u[:, 0] = -4.5                  # floor = -5: clamped to -4
    u[:, 1] = -4.5                  # floor(1 - 4.5) = -4: not clamped
    fm.warp3((z,), u, z, c)
    assert c["clamped"] == 10


def test_every_stop_test_is_recorded():
    for name in ("late-block-544x136", "letterbox-96x64", "translated-33x9"):
        for info in fc.edge_model(name)[1][1:]:
            assert len(info["tests"]) == info["iterations_run"]
            assert len(info["warps"]) == info["scales"] * fc.EDGE[name][3]
            for t in info["tests"]:
                W, H = t["size"]
                assert t["lo"] + t["hi"] + t["mid"] + t["flat"] == W * H
                assert len(t["tiles"]) == -(-W // 32) * -(-H // 8)
                assert abs(t["tiles"].sum() - t["error"]) <= 1e-9 * t["error"]
                assert t["threshold"] == 0.01 * 0.01 * (W * H)


# ---- 7. the inputs of test_gpu_flow_edges.py reach what they are there for -----------------------------
def _tiles(W, H):
    return -(-W // 32) * -(-H // 8)


def test_edge_shapes_have_their_tile_counts():
    got = {n: _tiles(*fc.edge_frames(n)[0].shape[::-1]) for n in fc.edge_names("tiles")}
    assert got == {"translated-480x136": 255, "translated-544x136": 289, "translated-545x137": 324,
                   "translated-1056x200": 825, "translated-16384x16": 1024, "translated-16x2056": 257}
    assert [_tiles(*s) for s in fm.pyramid_sizes(545, 137)] == [324, 81, 25, 9]
    assert 545 % 32 == 1 and 137 % 8 == 1    # the last tile column and row are one pixel
    assert fm.pyramid_sizes(545, 137) == [(545, 137), (273, 69), (137, 35), (69, 18)]   # odd but one side


@pytest.mark.parametrize("name,row,col,tile", [("late-block-544x136", 126, 524, 271),
                                               ("late-block-1056x200", 190, 1036, 791)])
def test_late_block_decides_behind_tile_256(name, row, col, tile):
    """The frames differ only inside two tiles of index >= 256, and at the finest level a stop test
    exists that a sum over the first 256 partial sums alone would decide the other way.  The sum of
    the first 256 tiles may be exactly 0, so it is asked to lie below 0.9 x threshold, not at 1e-6
    of it; the total keeps the 1e-6 margin."""
    frames = fc.edge_frames(name)
    H, W = frames[0].shape
    tw = -(-W // 32)
    assert (row // 8) * tw + col // 32 == tile >= 256
    _, infos = fc.edge_model(name)
    _, _, iterations, warps = fc.EDGE[name]
    for k in range(1, len(frames)):
        ys, xs = np.nonzero(frames[k] != frames[0])
        assert len(ys) > 0 and set(((ys // 8) * tw + xs // 32).tolist()) == {tile, tile + tw}   # 4 rows from `row`
        info = infos[k]
        assert info["margin"] >= 1e-6
        fine = [t for t in info["tests"] if t["size"] == (W, H)]
        assert fine and len(fine[0]["tiles"]) > 256
        wrong = [t for t in fine if t["tiles"][:256].sum() <= t["threshold"] < t["error"]]
        assert wrong, "no stop test that the first 256 tiles would decide differently"
        assert any(t["tiles"][:256].sum() < 0.9 * t["threshold"] for t in wrong)
        print("%s/%d: %d of %d finest stop tests, first %.2f <= %.2f < %.2f, %d iterations" % (
            name, k, len(wrong), len(fine), wrong[0]["tiles"][:256].sum(), wrong[0]["threshold"],
            wrong[0]["error"], info["iterations_run"]))
        # stops inside a loop: later than each warp's first iteration, earlier than all of them
        assert info["scales"] * warps < info["iterations_run"] < info["scales"] * warps * iterations


def test_late_block_figures():
    info = fc.edge_model("late-block-544x136")[1][1]
    assert info["iterations_run"] == 38 and info["scales"] == 4
    assert 1.3e-3 < info["margin"] < 1.5e-3
    t = next(t for t in info["tests"] if t["size"] == (544, 136) and t["tiles"][:256].sum() <= t["threshold"] < t["error"])
    assert (round(t["tiles"][:256].sum(), 2), round(t["threshold"], 2), round(t["error"], 2)) == (6.53, 7.40, 21.47)
    t = next(t for t in fc.edge_model("late-block-1056x200")[1][1]["tests"] if t["size"] == (1056, 200))
    assert t["tiles"][:256].sum() == 0.0 and t["threshold"] < t["error"]
    for name in fc.edge_names("first"):     # the counterpart: everything happens in tile 0
        frames = fc.edge_frames(name)
        ys, xs = np.nonzero(frames[1] != frames[0])
        assert len(ys) > 0 and ys.max() < 8 and xs.max() < 32


def test_tiny_frames_run():
    runs = {n: fc.edge_model(n)[1][1]["iterations_run"] for n in fc.edge_names("tiny")}
    assert runs.pop("translated-1x1") == 2
    assert len(runs) == 5 and set(runs.values()) == {20}


def test_content_cases_reach_every_branch():
    def branches(name):
        tests = [t for i in fc.edge_model(name)[1][1:] for t in i["tests"]]
        return {b: sum(t[b] for t in tests) for b in ("lo", "hi", "mid", "flat", "gradless")}, tests

    reached = {b for name in fc.edge_names("content") for b, v in branches(name)[0].items() if v > 0}
    assert reached == {"lo", "hi", "mid", "flat", "gradless"}

    for name in fc.edge_names("content"):
        flows, _ = fc.edge_model(name)
        b, tests = branches(name)
        print(name, b)
        if name.startswith("constant"):
            assert not flows[1].any() and not np.signbit(flows[1]).any()
            # grad is 0 at every pixel of every test, so the step is zero whichever branch is taken
            assert all(t["gradless"] == t["size"][0] * t["size"][1] for t in tests) and b["mid"] == 0
    assert all(v > 0 for v in branches("letterbox-96x64")[0].values())
    b, tests = branches("constant-same")
    assert b["lo"] == b["hi"] == b["mid"] == 0 and b["flat"] == b["gradless"] > 0
    # 128 then 129: rho = -1 < -l_t * 0, so the model (and the kernel) take lo with a step of l_t * 0
    b, _ = branches("constant-128-129")
    assert b["hi"] == b["mid"] == b["flat"] == 0 and b["lo"] == b["gradless"] > 0
    # one test of the letterbox frames reaches all four at once
    assert any(min(t["lo"], t["hi"], t["mid"], t["flat"]) > 0 for t in branches("letterbox-96x64")[1])


def test_fast_motion_reaches_the_clamp():
    flows, infos = fc.edge_model("fast-160x120")
    assert fc.FAST == (12, -9)
    warps = infos[1]["warps"]
    print("clamped", [w["clamped"] for w in warps], "outside taps", [w["outside_taps"] for w in warps])
    assert sum(w["clamped"] for w in warps) > 0 and all(w["outside_taps"] > 0 for w in warps)
    assert np.abs(flows[1]).max() > 12


@pytest.mark.parametrize("W,H,sizes", [
    (131, 75, [(131, 75), (66, 38), (33, 19)]),            # the height ends it: (17, 10) is not built
    (75, 131, [(75, 131), (38, 66), (19, 33)]),
    (512, 512, [(512, 512), (256, 256), (128, 128), (64, 64), (32, 32)]),   # NSCALES alone ends it
    (544, 136, [(544, 136), (272, 68), (136, 34), (68, 17)]),
    (1056, 200, [(1056, 200), (528, 100), (264, 50), (132, 25)]),
    (16384, 16, [(16384, 16)]),
    (16, 2056, [(16, 2056)]),
    (1, 1, [(1, 1)]), (1, 40, [(1, 40)]), (40, 1, [(40, 1)]), (31, 7, [(31, 7)]), (33, 9, [(33, 9)]),
])
def test_pyramid_sizes_of_edge_shapes(W, H, sizes):
    assert fm.pyramid_sizes(W, H) == sizes
    if (W, H) == (512, 512):
        assert len(sizes) == fm.NSCALES and min((W >> 5, H >> 5)) >= 16   # a sixth level would pass the side rule
        assert fc.edge_model("translated-512x512-i3-w1")[1][1]["scales"] == 5


# ---- 8. C ABI ----------------------------------------------------------------------------------------
def test_header_symbols_exported(library):
    header = open(os.path.join(ROOT, "include", "vsg_flow.h")).read()
    declared = set(re.findall(r"\b(vsg_flow_[a-z0-9_]+)\s*\(", header))
    assert declared, "no declarations parsed"
    assert declared == set(flow.EXPORTED_SYMBOLS)
    for name in declared:
        assert hasattr(library, name), name


def test_default_options(library):
    o = flow.default_flow_options()
    assert (o.flow_type, o.iterations, o.warps, o.device) == (flow.FLOW_BACKWARD, 10, 2, -1)


def _device_count():
    try:
        import torch
        return torch.cuda.device_count()
    except ImportError:
        return 0


def test_no_cpu_fallback(library):
    """Without a HIP device creation must fail with VSG_ERR_DEVICE."""
    if _device_count() > 0:
        pytest.skip("a GPU is present")
    h = C.c_void_p()
    o = flow.default_flow_options()
    assert library.vsg_flow_create(C.byref(o), 64, 48, C.byref(h)) == -2
    assert b"no usable HIP device" in library.vsg_flow_last_error()
    with pytest.raises(flow.VsgError):
        flow.DenseFlow(64, 48)


def test_frames_one_pixel_wide_or_high_are_taken():
    """numpy leaves any stride on an axis of length 1 (a slice's, here): such a frame is packed."""
    from video_segment_amd import _capi
    canvas = np.arange(15 * 54, dtype=np.uint8).reshape(15, 54)
    for H, W in [(1, 1), (1, 9), (9, 1)]:
        f = np.ascontiguousarray(canvas[3:3 + H, 5:5 + W])
        p, stride, mem = _capi.frame_ptr(f, H, W, 1, "frame")
        assert (p.value, mem) == (f.ctypes.data, 0) and stride >= W
        assert stride == (W if H == 1 else f.strides[0])
    bgr = np.zeros((5, 8, 3), np.uint8)[1:2, 2:3]
    assert _capi.frame_ptr(bgr, 1, 1, 3, "frame")[1] == 3
    with pytest.raises(ValueError):
        _capi.frame_ptr(canvas[:, ::2], 15, 27, 1, "frame")     # pixels 2 bytes apart
    with pytest.raises(ValueError):
        _capi.frame_ptr(np.zeros((4, 1, 4), np.uint8)[..., ::2], 4, 1, 2, "frame")


def test_bad_options_are_refused(library):
    h = C.c_void_p()
    for kw in ({"iterations": 0}, {"warps": 0}, {"flow_type": 3}):
        o = flow.default_flow_options(**kw)
        assert library.vsg_flow_create(C.byref(o), 64, 48, C.byref(h)) == -1, kw
    o = flow.default_flow_options()
    assert library.vsg_flow_create(C.byref(o), 0, 48, C.byref(h)) == -1
