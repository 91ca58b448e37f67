"""The dense flow unit (libvsg_flow.so) where test_gpu_flow.py does not reach: more than 256
workgroups of the iteration kernel, one-pixel tiles and frames, the pyramid's scale cap, flat and
fast content, the bounds of the options, and buffers laid out by hand.  Same method: the model of
flow_model.py, uint32 words, no tolerance.  flow_cases.EDGE holds the inputs; test_flow_model.py
checks on the CPU that they reach what they are here for."""
import ctypes as C

import numpy as np
import pytest

import flow_cases as fc
import flow_model as fm
from test_gpu_flow import assert_bits, flow  # noqa: F401 (flow is a fixture)

pytestmark = pytest.mark.gpu

SENTINEL = 0xFFC0DEAD   # a NaN as f32; compared as a word
GUARD = 16              # words in front of and behind an output field


def expected_launches(scales, warps, iterations, calcs, host_in, host_out, has_flow=True):
    """stats["launches"] of one process call, from the sequence of flow_capi.cpp ("Dense
    flow unit"): [upload] luminance, pyrDown per further level; per calc: clear state, clear u, then
    per level clear p, gradient, per warp one warp kernel and `iterations` iteration kernels, between
    levels upsample and flip; export [and download]; one copy of the states at the end."""
    n = int(host_in) + 1 + (scales - 1)
    if not has_flow:
        return n
    calc = 2 + scales * (2 + warps * (1 + iterations)) + (scales - 1) * 2 + 1 + int(host_out)
    return n + calcs * calc + 1


def check_stats(stats, info_sum, scales, iterations, warps, calcs=1, host_in=True, host_out=True, allocs=None):
    assert stats["scales"] == scales
    assert stats["iterations_run"] == info_sum, stats
    assert stats["launches"] == expected_launches(scales, warps, iterations, calcs, host_in, host_out), stats
    assert stats["host_syncs"] == 1
    if allocs is not None:
        assert stats["device_allocations"] == allocs


def run_edge(flow, name, **extra):
    """Feeds the case's frames to a fresh handle: [(result, stats)] per frame."""
    _, _, iterations, warps = fc.EDGE[name]
    frames = fc.edge_frames(name)
    H, W = frames[0].shape
    d = flow.DenseFlow(W, H, iterations=iterations, warps=warps, **extra)
    out = []
    for f in frames:
        r = d.process_frame(f)
        out.append((r, d.last_stats()))
    d.close()
    return out


# ---- 1. every edge case against the model ------------------------------------------------------------
@pytest.mark.parametrize("name", list(fc.EDGE))
def test_edge_case_equals_model(flow, name):
    _, _, iterations, warps = fc.EDGE[name]
    frames = fc.edge_frames(name)
    flows, infos = fc.edge_model(name)
    scales = len(fm.pyramid_sizes(frames[0].shape[1], frames[0].shape[0]))
    got = run_edge(flow, name)
    assert got[0][0] is None
    first = got[0][1]
    assert first["launches"] == expected_launches(scales, warps, iterations, 1, True, True, has_flow=False)
    assert first["host_syncs"] == 1 and first["iterations_run"] == 0
    for k in range(1, len(frames)):
        r, stats = got[k]
        print("%s frame %d: %d iterations, %d launches" % (name, k, stats["iterations_run"], stats["launches"]))
        assert infos[k]["scales"] == scales
        check_stats(stats, infos[k]["iterations_run"], scales, iterations, warps,
                    allocs=first["device_allocations"])
        assert_bits(r, flows[k], "%s frame %d" % (name, k))
    if name == "translated-512x512-i3-w1":
        assert got[1][1]["scales"] == 5 == infos[1]["scales"]
    if name.startswith("constant"):
        assert not got[1][0].view(np.uint32).any()     # +0 everywhere: no sign bit either


# ---- 2. handles ----------------------------------------------------------------------------------------
def test_flow_type_both_on_late_block(flow):
    """Both fields of the frames whose only change lies behind tile 256; iterations_run is the sum of
    the two calcs."""
    name = fc.BOTH_EDGE
    _, _, iterations, warps = fc.EDGE[name]
    bwd, binfo = fc.edge_model(name)
    fwd, finfo = fc.edge_forward_model(name)
    got = run_edge(flow, name, flow_type=flow.FLOW_BOTH)
    assert got[0][0] is None
    for k in range(1, len(got)):
        b, f = got[k][0]
        assert_bits(b, bwd[k], "backward %d" % k)
        assert_bits(f, fwd[k], "forward %d" % k)
        check_stats(got[k][1], binfo[k]["iterations_run"] + finfo[k]["iterations_run"], binfo[k]["scales"],
                    iterations, warps, calcs=2, allocs=got[0][1]["device_allocations"])


def test_two_handles_alive_at_once(flow):
    """544 x 136 and 67 x 45, fed alternately: neither sees the other's frames, sizes or partial sums."""
    big, small = fc.edge_frames("late-block-544x136"), fc.frames("block", 67, 45)[:3]
    want_big, info_big = fc.edge_model("late-block-544x136")
    want_small, info_small = fc.model("block", 67, 45, 10, 2)
    a, b = flow.DenseFlow(544, 136), flow.DenseFlow(67, 45)
    for k in range(3):
        ra = a.process_frame(big[k])
        rb = b.process_frame(small[k])
        if k == 0:
            assert ra is None and rb is None
            continue
        assert_bits(ra, want_big[k], "544 x 136 frame %d" % k)
        assert_bits(rb, want_small[k], "67 x 45 frame %d" % k)
        check_stats(a.last_stats(), info_big[k]["iterations_run"], 4, 10, 2)
        check_stats(b.last_stats(), info_small[k]["iterations_run"], 2, 10, 2)
    a.close()
    b.close()


def test_restart_then_other_content(flow):
    """After restart() the handle knows nothing of the stream before it."""
    W, H = 67, 45
    split, block = fc.frames("split", W, H), fc.frames("block", W, H)
    want_split, _ = fc.model("split", W, H, 10, 2)
    want_block, info_block = fc.model("block", W, H, 10, 2)
    d = flow.DenseFlow(W, H)
    assert d.process_frame(split[0]) is None
    assert_bits(d.process_frame(split[1]), want_split[1], "before restart")
    allocs = d.last_stats()["device_allocations"]
    d.restart()
    assert d.process_frame(block[0]) is None
    for k in (1, 2, 3):
        assert_bits(d.process_frame(block[k]), want_block[k], "after restart, frame %d" % k)
        check_stats(d.last_stats(), info_block[k]["iterations_run"], 2, 10, 2, allocs=allocs)
    d.close()


# ---- 3. buffers laid out by hand, through the C ABI ----------------------------------------------------
def process_raw(flow, d, frame, stride, offset, dev_in, dev_out):
    """One process call on buffers built here.  frame: H x W x 3 (BGR) or H x W (luminance) uint8; its
    rows go `stride` bytes apart behind `offset` bytes, and the buffer ends with the last row's last
    byte.  The output field has GUARD sentinel words on both sides.  Returns (H x W x 2 f32 or None
    for a first frame, the output buffer's other words as uint32)."""
    import torch
    H, W = frame.shape[:2]
    row = frame.reshape(H, -1)
    buf_in = np.full(offset + stride * (H - 1) + row.shape[1], 0x3C, np.uint8)
    np.lib.stride_tricks.as_strided(buf_in[offset:], row.shape, (stride, 1))[:] = row
    buf_out = np.full(GUARD + H * W * 2 + GUARD, SENTINEL, np.uint32)
    keep = []
    if dev_in:
        keep.append(torch.from_numpy(buf_in).cuda())
        p_in = keep[-1].data_ptr() + offset
    else:
        p_in = buf_in.ctypes.data + offset
    if dev_out:
        t_out = torch.from_numpy(buf_out.view(np.int32)).cuda()
        p_out = t_out.data_ptr() + 4 * GUARD
    else:
        p_out = buf_out.ctypes.data + 4 * GUARD
    torch.cuda.synchronize()
    fn = flow.lib().vsg_flow_process_frame if frame.ndim == 3 else flow.lib().vsg_flow_process_luminance
    has = C.c_int(-1)
    flow.check(fn(d.h, C.c_void_p(p_in), stride, int(dev_in), C.c_void_p(p_out), None, int(dev_out), C.byref(has)))
    if dev_out:
        buf_out = t_out.cpu().numpy().view(np.uint32)
    field = buf_out[GUARD:GUARD + H * W * 2]
    rest = np.concatenate([buf_out[:GUARD], buf_out[GUARD + H * W * 2:]])
    assert has.value in (0, 1)
    if not has.value:
        assert (field == SENTINEL).all()      # nothing is written for a first frame
        return None, rest
    return field.view(np.float32).reshape(H, W, 2).copy(), rest


@pytest.mark.parametrize("dev_out", [True, False], ids=["device-out", "host-out"])
@pytest.mark.parametrize("layout", ["bgr-packed-host", "bgr-padded-device", "lum-padded-device"])
def test_raw_buffers(flow, layout, dev_out):
    """Canaries around the output field stay; a device frame with rows padded by 13 bytes behind an
    odd base offset gives the packed frame's flow."""
    packed = fc.colour_frames()
    want, infos = fc.colour_model()
    H, W = packed[0].shape[:2]
    d = flow.DenseFlow(W, H)
    for k, bgr in enumerate(packed):
        if layout == "bgr-packed-host":
            frame, stride, offset, dev_in = bgr, W * 3, 0, False
        elif layout == "bgr-padded-device":
            frame, stride, offset, dev_in = bgr, W * 3 + 13, 7, True
        else:
            frame, stride, offset, dev_in = fm.luminance(bgr), W + 13, 5, True
        got, rest = process_raw(flow, d, frame, stride, offset, dev_in, dev_out)
        assert len(rest) == 2 * GUARD and (rest == SENTINEL).all(), "words next to the field were written"
        if k == 0:
            assert got is None
            continue
        assert_bits(got, want[k], "%s frame %d" % (layout, k))
        check_stats(d.last_stats(), infos[k]["iterations_run"], 2, 10, 2, host_in=not dev_in, host_out=not dev_out)
    d.close()
