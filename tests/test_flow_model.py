"""CPU-side checks of the dense flow unit: the numpy model that defines it (tests/flow_model.py),
the host-only luminance hook, and the C ABI's symbols.  The GPU comparison is test_gpu_flow.py."""
import ctypes as C
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


# ---- 6. C ABI ----------------------------------------------------------------------------------------
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


def test_bad_options_are_refused(library):
    h = C.c_void_p()
    for kw in ({"iterations": 0}, {"warps": 0}, {"flow_type": 3}):
        o = flow.default_flow_options(**kw)
        assert library.vsg_flow_create(C.byref(o), 64, 48, C.byref(h)) == -1, kw
    o = flow.default_flow_options()
    assert library.vsg_flow_create(C.byref(o), 0, 48, C.byref(h)) == -1
