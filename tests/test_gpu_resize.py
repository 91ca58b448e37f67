"""libvsg_resize.so on the MI355X (k_resize_h, k_resize_v) against the numpy model resize_model.py:
byte equality, no tolerance anywhere.  The shapes are the smallest at which each path can go wrong:
odd widths, tiles of output columns that end inside a row, every alignment of pointers and strides,
the widest filter the horizontal pass accepts, a copied frame, and one frame of each full size."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import resize_model as rm
import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "video_segment_amd", "host")
FILL = 0xA5


@pytest.fixture(scope="module")
def rz():
    from video_segment_amd import _lib, resize
    _lib.build()
    resize.build()
    assert _lib.lib().vsg_device_count() > 0
    return resize


def noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


_case_a = {}


def case_a():
    """97 x 61 noise and its model result at 78 x 48, computed once."""
    if not _case_a:
        img = noise(97, 61, 1)
        _case_a["img"], _case_a["want"] = img, rm.resize(img, 78, 48)
        img.setflags(write=False)
        _case_a["want"].setflags(write=False)
    return _case_a["img"], _case_a["want"]


def process_raw(rz, d, img, stride_in, offset_in, dev_in, stride_out, offset_out, dev_out):
    """One vsg_resize_process call on buffers laid out by hand.  The input buffer ends with the last
    pixel of the last row.  Returns (rows x out_w*3 result bytes, every other byte of the output)."""
    import torch
    h, w = img.shape[:2]
    ow, oh = d.out_size
    buf_in = np.full(offset_in + stride_in * (h - 1) + w * 3, 0x3C, np.uint8)
    rows_in = np.lib.stride_tricks.as_strided(buf_in[offset_in:], (h, w * 3), (stride_in, 1))
    rows_in[:] = img.reshape(h, w * 3)
    buf_out = np.full(offset_out + stride_out * oh, FILL, np.uint8)
    keep = []
    if dev_in:
        t_in = torch.from_numpy(buf_in).cuda()
        p_in = t_in.data_ptr() + offset_in
        keep.append(t_in)
    else:
        p_in = buf_in.ctypes.data + offset_in
    if dev_out:
        t_out = torch.from_numpy(buf_out).cuda()
        p_out = t_out.data_ptr() + offset_out
    else:
        p_out = buf_out.ctypes.data + offset_out
    torch.cuda.synchronize()
    rz.check(rz.lib().vsg_resize_process(d.h, C.c_void_p(p_in), stride_in, int(dev_in), C.c_void_p(p_out), stride_out,
                                         int(dev_out)))
    if dev_out:
        buf_out = t_out.cpu().numpy()
    rows = np.lib.stride_tricks.as_strided(buf_out[offset_out:], (oh, stride_out), (stride_out, 1))
    got = rows[:, :ow * 3].reshape(oh, ow, 3).copy()
    rest = np.concatenate([buf_out[:offset_out], rows[:, ow * 3:].ravel()])
    return got, rest


CASES = [
    # in_w, in_h, mode, size, factor, out_w, out_h
    ("a", 97, 61, rm.TO_MIN_SIZE, 48, 1.0, 78, 48),     # odd width, non-integer ratio, width_step 236
    ("b", 96, 72, rm.TO_MAX_SIZE, 48, 1.0, 48, 36),     # exact ratio 2
    ("c", 130, 70, rm.TO_MAX_SIZE, 48, 1.0, 48, 26),    # ratio 2.7, 11 taps
    ("d", 768, 432, rm.TO_MIN_SIZE, 36, 1.0, 64, 36),   # ratio 12, 48 taps, one tile spans the whole row
    ("e", 97, 61, rm.NONE, 0, 1.0, 98, 61),             # the even-width stretch, identity vertical axis
    ("f", 96, 72, rm.BY_FACTOR, 0, 1.0, 96, 72),        # copy
    ("g", 61, 97, rm.TO_MIN_SIZE, 48, 1.0, 48, 77),     # tall frame
    # 1024 taps, the widest filter accepted: the tile narrows from 64 to 8 columns to fit its LDS budget
    ("wide", 4096, 5, rm.BY_FACTOR, 0, 1.0 / 256, 16, 1),
    # more than one tile of 64 columns and more than one block of output bytes per row
    ("tiles", 403, 9, rm.BY_FACTOR, 0, 0.75, 304, 7),
]


@pytest.mark.parametrize("name,in_w,in_h,mode,size,factor,out_w,out_h", CASES, ids=[c[0] for c in CASES])
def test_cases_equal_the_model(rz, name, in_w, in_h, mode, size, factor, out_w, out_h):
    img = noise(in_w, in_h, 2 + len(name) + in_w)
    d = rz.Downscaler(in_w, in_h, mode=mode, size=size, factor=factor)
    assert d.out_size == (out_w, out_h) and d.width_step == (out_w * 3 + 3) // 4 * 4
    want = rm.resize(img, out_w, out_h)
    got = d.process_frame(img)
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want)
    st = d.last_stats()
    assert st["host_syncs"] == 1
    if (out_w, out_h) == (in_w, in_h):
        assert np.array_equal(got, img)
        assert st["taps_h"] == 0 and st["launches"] == 0     # host to host: nothing enqueued
        import torch
        dev = d.process_frame_device(torch.from_numpy(img).cuda())
        assert np.array_equal(dev.cpu().numpy(), img) and d.last_stats()["launches"] == 1
    else:
        assert st["taps_h"] == int(rm.filter_tables(in_w, out_w)[1].max())
        assert st["taps_v"] == int(rm.filter_tables(in_h, out_h)[1].max())
        assert st["launches"] == 4      # upload, two kernels, download
        assert st["horizontal_us"] > 0 and st["vertical_us"] > 0
    d.close()


@pytest.mark.parametrize("kind", ["step", "checker"])
def test_saturation_at_both_ends(rz, kind):
    img = np.zeros((40, 64, 3), np.uint8)
    if kind == "step":
        img[:, 32:] = 255
        img[20:, :, 1] = 255 - img[20:, :, 1]
    else:
        yy, xx = np.mgrid[0:40, 0:64]
        img[((xx // 5 + yy // 3) % 2) == 1] = 255
    raw = rm.resize_f32(img, 24, 15)
    assert raw.min() < -0.5 and raw.max() > 255.5        # both clamps change a value
    d = rz.Downscaler(64, 40, mode=rm.BY_FACTOR, factor=0.375)
    assert d.out_size == (24, 15)
    got = d.process_frame(img)
    assert np.array_equal(got, rm.resize(img, 24, 15))
    assert got.min() == 0 and got.max() == 255
    d.close()


@pytest.mark.parametrize("stride_in,offset_in", [(292, 0), (292, 1), (356, 0), (291, 0)],
                         ids=["padded4", "unaligned", "padded64", "packed_odd"])
@pytest.mark.parametrize("dev_in", [False, True], ids=["host_in", "device_in"])
def test_input_strides_and_alignments(rz, stride_in, offset_in, dev_in):
    """97 * 3 = 291 bytes per row: padded to 4, padded to 4 behind an odd base pointer (the byte
    path of k_resize_h), padded by 64, and packed (odd stride: the byte path again)."""
    img, want = case_a()
    d = rz.Downscaler(97, 61, mode=rm.TO_MIN_SIZE, size=48)
    got, rest = process_raw(rz, d, img, stride_in, offset_in, dev_in, 236, 0, True)
    assert np.array_equal(got, want)
    assert (rest == FILL).all()
    d.close()


@pytest.mark.parametrize("stride_out,offset_out", [(234, 0), (236, 0), (300, 0), (301, 0), (236, 3)],
                         ids=["packed", "width_step", "wider", "odd", "unaligned"])
@pytest.mark.parametrize("dev_out", [False, True], ids=["host_out", "device_out"])
def test_output_padding_is_never_written(rz, stride_out, offset_out, dev_out):
    """78 * 3 = 234 bytes per row, not a multiple of 4: the last two bytes of a row go bytewise, and
    nothing beyond them is touched, whatever the stride and the alignment of the base."""
    img, want = case_a()
    d = rz.Downscaler(97, 61, mode=rm.TO_MIN_SIZE, size=48)
    got, rest = process_raw(rz, d, img, 291, 0, True, stride_out, offset_out, dev_out)
    assert np.array_equal(got, want)
    assert (rest == FILL).all()
    d.close()


@pytest.mark.parametrize("dev_in", [False, True], ids=["host_in", "device_in"])
@pytest.mark.parametrize("dev_out", [False, True], ids=["host_out", "device_out"])
def test_memory_kinds(rz, dev_in, dev_out):
    img, want = case_a()
    d = rz.Downscaler(97, 61, mode=rm.TO_MIN_SIZE, size=48)
    got, rest = process_raw(rz, d, img, 292, 0, dev_in, 240, 0, dev_out)
    assert np.array_equal(got, want) and (rest == FILL).all()
    st = d.last_stats()
    assert st["launches"] == 2 + (not dev_in) + (not dev_out) and st["host_syncs"] == 1
    assert (st["upload_us"] > 0) == (not dev_in) and (st["download_us"] > 0) == (not dev_out)
    d.close()


def test_process_checks_arguments(rz):
    img, _ = case_a()
    d = rz.Downscaler(97, 61, mode=rm.TO_MIN_SIZE, size=48)
    out = np.zeros((48, 236), np.uint8)
    L, p_in, p_out = rz.lib(), C.c_void_p(img.ctypes.data), C.c_void_p(out.ctypes.data)
    assert L.vsg_resize_process(d.h, None, 291, 0, p_out, 236, 0) == -1
    assert L.vsg_resize_process(d.h, p_in, 291, 0, None, 236, 0) == -1
    assert L.vsg_resize_process(d.h, p_in, 290, 0, p_out, 236, 0) == -1
    assert b"stride_in" in L.vsg_resize_last_error()
    assert L.vsg_resize_process(d.h, p_in, 291, 0, p_out, 233, 0) == -1
    assert b"stride_out" in L.vsg_resize_last_error()
    assert L.vsg_resize_process(d.h, p_in, 291, 2, p_out, 236, 0) == -1
    assert L.vsg_resize_process(d.h, p_in, 291, 0, p_out, 236, 5) == -1
    assert not out.any()
    assert L.vsg_resize_process(d.h, p_in, 291, 0, p_out, 236, 0) == 0 and out.any()
    d.close()


@pytest.mark.parametrize("in_w,in_h", [(1920, 1080), (3840, 2160)])
def test_full_size_frames(rz, in_w, in_h):
    """The production shape (--run_on_server): 1080p and 4K to 640 x 360, device memory in and out."""
    import torch
    img = noise(in_w, in_h, in_w)
    yy, xx = np.mgrid[0:in_h, 0:in_w]
    img[((xx // 37 + yy // 23) % 2) == 1, 2] |= 0xC0       # structure under the noise
    want = rm.resize(img, 640, 360)
    d = rz.Downscaler(in_w, in_h)                           # TO_MIN_SIZE 360
    assert d.out_size == (640, 360)
    got = d.process_frame_device(torch.from_numpy(img).cuda())
    assert got.is_cuda and tuple(got.shape) == (360, 640, 3)
    assert np.array_equal(got.cpu().numpy(), want)
    st = d.last_stats()
    # 3840 -> 640: centres at 6 o + 2.5, 24 taps; 1920 -> 640: centres at the integers 3 o + 1, so both
    # ends of the window are taps (of weight 0), 13
    assert st["launches"] == 2 and st["taps_h"] == (13 if in_w == 1920 else 24)
    assert st["taps_h"] == int(rm.filter_tables(in_w, 640)[1].max())
    d.close()


def test_handle_reuse_and_two_handles(rz):
    """Thirty frames on one handle allocate nothing after the first; a second handle of another
    size, used in between, does not disturb it."""
    img, want = case_a()
    other = noise(130, 70, 9)
    other_want = rm.resize(other, 48, 26)
    d = rz.Downscaler(97, 61, mode=rm.TO_MIN_SIZE, size=48)
    e = rz.Downscaler(130, 70, mode=rm.TO_MAX_SIZE, size=48)
    assert np.array_equal(d.process_frame(img), want)
    first = d.last_stats()["device_allocations"]
    assert first > 0
    for k in range(30):
        frame = img if k % 2 == 0 else np.ascontiguousarray(img[::-1])
        got = d.process_frame(frame)
        if k % 10 == 3:
            assert np.array_equal(e.process_frame(other), other_want)
        if k % 2 == 0:
            assert np.array_equal(got, want)
        st = d.last_stats()
        assert st["device_allocations"] == first and st["host_syncs"] == 1
    assert np.array_equal(d.process_frame(np.ascontiguousarray(img[::-1])), rm.resize(img[::-1], 78, 48))
    d.close()
    assert np.array_equal(e.process_frame(other), other_want)
    e.close()


def _driver(args):
    p = subprocess.run([os.path.join(HOST, "seg_tree_synth")] + args, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    m = re.search(r"frames=(\d+) first_frame_regions=(\d+) total_regions=(\d+) label_fnv1a32=(\w+)", p.stdout)
    assert m, p.stdout
    return int(m.group(1)), int(m.group(4), 16)


def test_driver_downscales_and_writes_the_original_size(rz, tmp_path):
    """seg_tree_synth --downscale_min_size 48 on a 192 x 144 source: the segmentation is that of the
    Python path on the same frames (Downscaler -> DenseSegmentation at 64 x 48), in both pipeline
    modes, and the written vectorization is scaled back to 192 x 144."""
    import torch
    import vector_cases as vc
    import video_segment_amd as vsg
    from video_segment_amd import segmentation_io as sio
    subprocess.check_call(["make", "-C", HOST, "-s"])
    W, H, N = 192, 144, 12
    d = rz.Downscaler(W, H, mode=rm.TO_MIN_SIZE, size=48)
    assert d.out_size == (64, 48)
    g = vsg.DenseSegmentation(64, 48, vsg.default_options(chunk_size=8, compute_vectorization=1), has_flow=True)
    flow = torch.from_numpy(synth.const_flow(64, 48)).cuda()
    ids = []
    for k in range(N + 1):
        if k < N:
            frame = synth.probe_frame(W, H, k)
            small = d.process_frame_device(frame)
            if k == 0:
                assert np.array_equal(small.cpu().numpy(), rm.resize(frame, 64, 48))
            n = g.process_frame(small, flow if k > 0 else None)
        else:
            n = g.process_frame(None, None, flush=True)
        ids += [g.result_id_image(i) for i in range(n)]
    assert len(ids) == N
    want_hash = synth.fnv1a32_fast(ids)
    g.close()
    d.close()

    out = str(tmp_path / "down.pb")
    base = ["--width", str(W), "--height", str(H), "--frames", str(N), "--chunk_size", "8", "--over_segment"]
    for mode in ("--use_pipeline", "--nouse_pipeline"):
        frames, got_hash = _driver(base + [mode, "--downscale_min_size", "48", "--write_to_file", "--output_file", out,
                                           "--remove_rasterization"])
        assert frames == N and got_hash == want_hash
        _, descs, _ = sio.read_segmentation_file(out)
        assert len(descs) == N
        for _, seg in descs:
            m = vc.Msg()
            m.ParseFromString(seg)
            assert (m.frame_width, m.frame_height) == (W, H) and m.rasterization_removed
            coord = np.asarray(m.vector_mesh.coord, np.float32)
            assert coord.size > 0 and coord.max() > 64        # scaled back: beyond the small frame
    # --original_width / --original_height still win
    _driver(base + ["--downscale_min_size", "48", "--write_to_file", "--output_file", out, "--remove_rasterization",
                    "--original_width", "384", "--original_height", "288"])
    m = vc.Msg()
    m.ParseFromString(sio.read_segmentation_file(out)[1][0][1])
    assert (m.frame_width, m.frame_height) == (384, 288)
    # without the flag the driver computes what it always did (the pin of tests/test_host_unit.py)
    assert _driver(["--width", "64", "--height", "48", "--frames", "8", "--flow", "0"]) == (8, 0x39AEEABB)
