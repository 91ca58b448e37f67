"""k_render_fill and k_render_compose on the MI355X at their tile, row and alignment edges, against the numpy
model of the reference (render_model.py) byte for byte: no tolerance anywhere.  The inputs are the cases of
render_edge_cases.py; test_render_edge_cases.py shows on the CPU that each does what it is here for and that the
comparison fails for a model with one rule broken."""
import ctypes as C

import numpy as np
import pytest

import render_edge_cases as rc

pytestmark = pytest.mark.gpu
FILL = 0xAB


@pytest.fixture(scope="module")
def vsg():
    import video_segment_amd as v
    from video_segment_amd import _lib, render
    _lib.build()
    render.build()
    assert _lib.lib().vsg_device_count() > 0
    return v


# ---- options -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("o", rc.option_sets(), ids=rc.option_id)
def test_every_case_under_every_option(vsg, o):
    """One handle per size and option set, reused across the patterns of the size."""
    for (W, H) in rc.SIZES:
        r = vsg.SegmentationRenderer(W, H, **o)
        bgr = rc.frame(W, H)
        for c in rc.cases_at(W, H):
            got = r.render(rc.desc(c.name)[1], bgr if o["has_video"] else None)
            want = rc.model_render(c.name, **o)
            assert got.shape == want.shape and got.dtype == np.uint8
            assert np.array_equal(got, want), (c.name, np.argwhere((got != want).any(axis=2))[:8].tolist())
        r.close()


def test_id_images_to_host_and_in_place_at_pitch_w(vsg):
    """The device form is painted in place at row pitch W, odd for most of these widths; the values in front of
    the image and behind it keep what they held."""
    import torch
    dev = torch.device("cuda", 0)
    guard, mark = 64, -77
    for (W, H) in rc.SIZES:
        r = vsg.SegmentationRenderer(W, H)
        for c in rc.cases_at(W, H):
            want = rc.model_id_image(c.name)
            got = r.id_image(rc.desc(c.name)[1], 0)
            assert got.dtype == np.int32 and np.array_equal(got, want), c.name
            buf = torch.full((guard + W * H + guard,), mark, dtype=torch.int32, device=dev)
            out = buf[guard:guard + W * H].view(H, W)
            assert r.id_image(rc.desc(c.name)[1], 0, out=out) is out
            host = buf.cpu().numpy()
            assert np.array_equal(host[guard:guard + W * H].reshape(H, W), want), c.name
            assert (host[:guard] == mark).all() and (host[guard + W * H:] == mark).all(), c.name
        r.close()


# ---- the fill's second trip ----------------------------------------------------------------------------------
def test_stride_trip(vsg):
    """532 480 one-pixel intervals: 2048 workgroups of 256 take 524 288 of them, the rest the second trip."""
    c = rc.stride_trip_case()
    seg = rc.desc(c.name)[1]
    r = vsg.SegmentationRenderer(c.W, c.H, has_video=False, highlight_edges=False)
    got = r.render(seg)
    assert r.last_stats()["intervals"] == rc.STRIDE_TRIP_INTERVALS == 532480
    assert np.array_equal(got, rc.model_render(c.name, has_video=False, highlight_edges=False))
    ids = r.id_image(seg, 0)
    assert r.last_stats()["intervals"] == 532480
    assert np.array_equal(ids, rc.model_id_image(c.name))
    r.close()


# ---- buffers laid out by hand --------------------------------------------------------------------------------
MODES = {
    "blend": dict(has_video=True, concat_with_source=False),
    "concat": dict(has_video=True, concat_with_source=True),
    "render": dict(has_video=False, concat_with_source=False),
}
RAW_CASES = ("seams_257x17", "seams_5x3")


def render_raw(r, name, mode, offset_in, stride_in, dev_in, offset_out, stride_out, dev_out):
    """One vsg_render_frame call on byte buffers laid out by hand.  The source buffer ends with the last pixel
    of its last row; the output buffer has `offset_out` bytes in front and whole rows of `stride_out`.  Asserts
    that the source is unchanged and returns (the picture, every other byte of the output buffer, the address
    the output started at modulo 4, the same for the source)."""
    import torch
    from video_segment_amd import render
    c = rc.BY_NAME[name]
    W, H = c.W, c.H
    rows = 2 * H if MODES[mode]["concat_with_source"] else H
    keep = []
    p_in, a_in = None, 0
    if MODES[mode]["has_video"]:
        buf_in = np.full(offset_in + stride_in * (H - 1) + 3 * W, 0x3C, np.uint8)
        rows_in = np.lib.stride_tricks.as_strided(buf_in[offset_in:], (H, 3 * W), (stride_in, 1))
        rows_in[:] = rc.frame(W, H).reshape(H, 3 * W)
        before = buf_in.copy()
        if dev_in:
            t_in = torch.from_numpy(buf_in).cuda()
            base = t_in.data_ptr()
        else:
            base = buf_in.ctypes.data
        assert dev_in is False or base % 4 == 0
        p_in, a_in = base + offset_in, (base + offset_in) % 4
    buf_out = np.full(offset_out + stride_out * rows, FILL, np.uint8)
    if dev_out:
        t_out = torch.from_numpy(buf_out).cuda()
        base = t_out.data_ptr()
        assert base % 4 == 0
    else:
        base = buf_out.ctypes.data
    p_out = base + offset_out
    torch.cuda.synchronize()
    seg = rc.desc(name)[1]
    render.check(render.lib().vsg_render_frame(r.h, seg, len(seg), C.c_void_p(p_in), stride_in, int(dev_in),
                                               C.c_void_p(p_out), stride_out, int(dev_out)))
    if dev_out:
        buf_out = t_out.cpu().numpy()
    if MODES[mode]["has_video"]:
        after = t_in.cpu().numpy() if dev_in else buf_in
        assert np.array_equal(after, before), "the source buffer changed"
    view = np.lib.stride_tricks.as_strided(buf_out[offset_out:], (rows, stride_out), (stride_out, 1))
    got = view[:, :3 * W].reshape(rows, W, 3).copy()
    rest = np.concatenate([buf_out[:offset_out], view[:, 3 * W:].ravel()])
    assert len(rest) + got.size == len(buf_out)
    return got, rest, p_out % 4, a_in


def takes_dwords(mode, out_address, out_stride, src_address, src_stride):
    """LaunchCompose's rule for k_render_compose<true>."""
    ok = out_address % 4 == 0 and out_stride % 4 == 0
    if mode != "render":
        ok = ok and src_address % 4 == 0 and src_stride % 4 == 0
    return ok


OFFSETS = ((0, 0), (1, 0), (0, 1), (2, 2), (3, 1), (0, 3))      # source base, output base


@pytest.mark.parametrize("mode", list(MODES))
def test_alignment_in_device_memory(vsg, mode):
    """Source and output in device memory at every pairing of base offset and row stride.  With r = 3W rounded
    up to 4, the output strides are 3W, r, r + 4, r + 1 and the source strides 3W, r, r + 1 (3W is odd at both
    widths, 257 and 5).

    k_render_compose<true>, which moves whole threads' rows as dwords, runs for
      render          output offset 0 (the pairs (0,0) and (1,0)) and output stride r or r + 4: 4 of the 24 layouts;
      blend, concat   the pair (0,0) alone, output stride r or r + 4, source stride r: 2 of the 72 layouts.
    Every other row of the matrix runs k_render_compose<false>, which goes bytewise: an odd output offset or
    stride, and for blend and concat an odd source offset or stride too ((1,0) with an aligned output, or source
    stride 3W or r + 1 under an aligned output).  The counts are asserted from LaunchCompose's rule."""
    o = MODES[mode]
    instances = {True: 0, False: 0}
    for name in RAW_CASES:
        c = rc.BY_NAME[name]
        W, H = c.W, c.H
        r4 = (3 * W + 3) // 4 * 4
        assert 3 * W % 4 != 0
        want = rc.model_render(name, **o)
        r = vsg.SegmentationRenderer(W, H, **o)
        src_strides = (3 * W, r4, r4 + 1) if o["has_video"] else (0,)
        for (off_in, off_out) in OFFSETS:
            for stride_out in (3 * W, r4, r4 + 4, r4 + 1):
                for stride_in in src_strides:
                    got, rest, a_out, a_in = render_raw(r, name, mode, off_in, stride_in, True, off_out, stride_out, True)
                    layout = (name, off_in, off_out, stride_in, stride_out)
                    assert a_out == off_out % 4 and (not o["has_video"] or a_in == off_in % 4)
                    assert got.shape == want.shape and np.array_equal(got, want), layout
                    assert (rest == FILL).all(), layout
                    instances[takes_dwords(mode, a_out, stride_out, a_in, stride_in)] += 1
        r.close()
    if mode == "render":
        assert instances == {True: 2 * 4, False: 2 * 20}
    else:
        assert instances == {True: 2 * 2, False: 2 * 70}


@pytest.mark.parametrize("mode", list(MODES))
def test_host_memory_at_strides_the_staged_copy_does_not_share(vsg, mode):
    """Host input at 3W (odd) and 3W + 13, host output at 3W, the default stride and 3W + 7: both
    hipMemcpy2DAsync stagings between a caller's pitch and the handle's; the padding is left alone."""
    from video_segment_amd import render
    o = MODES[mode]
    for name in RAW_CASES:
        c = rc.BY_NAME[name]
        W, H = c.W, c.H
        want = rc.model_render(name, **o)
        r = vsg.SegmentationRenderer(W, H, **o)
        for stride_in in ((3 * W, 3 * W + 13) if o["has_video"] else (0,)):
            for stride_out in (3 * W, render.default_stride(W), 3 * W + 7):
                for (off_in, off_out) in ((0, 0), (1, 3)):
                    got, rest, _, _ = render_raw(r, name, mode, off_in, stride_in, False, off_out, stride_out, False)
                    layout = (name, off_in, off_out, stride_in, stride_out)
                    assert np.array_equal(got, want), layout
                    assert (rest == FILL).all(), layout
        r.close()


# ---- one handle, sparse and dense frames in turn ---------------------------------------------------------------
def test_handle_reuse_leaves_nothing_of_the_denser_frame(vsg):
    W, H = 257, 17
    names = ("uncovered_257x17", "pixels_257x17", "uncovered_257x17")
    bgr = rc.frame(W, H)
    r = vsg.SegmentationRenderer(W, H)
    allocs = []
    for _ in range(3):
        pictures, planes = [], []
        for name in names:
            seg = rc.desc(name)[1]
            pictures.append(r.render(seg, bgr))
            assert np.array_equal(pictures[-1], rc.model_render(name)), name
            planes.append(r.id_image(seg, 0))
            assert np.array_equal(planes[-1], rc.model_id_image(name)), name
        assert np.array_equal(pictures[2], pictures[0]) and not np.array_equal(pictures[1], pictures[0])
        assert np.array_equal(planes[2], planes[0])
        allocs.append(r.last_stats()["device_allocations"])
    assert allocs[0] > 0 and allocs[1] == allocs[0] and allocs[2] == allocs[0], allocs
    r.close()
