"""The dense flow unit on the MI355X (libvsg_flow.so) against the numpy model that defines it
(flow_model.py), bit for bit: flows are compared as uint32 words, there is no tolerance anywhere in
this file.  flow_cases.py holds the inputs and computes each model result once."""
import os
import re
import subprocess

import numpy as np
import pytest

import flow_cases as fc
import flow_model as fm
import oracle_lib as ol

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "video_segment_amd", "host")


@pytest.fixture(scope="module")
def flow():
    import video_segment_amd  # noqa: F401
    from video_segment_amd import _lib, flow as f
    _lib.build()
    f.build()
    assert _lib.lib().vsg_device_count() > 0
    return f


def assert_bits(got, want, what):
    assert got is not None, what
    got = np.ascontiguousarray(got)
    assert got.dtype == np.float32 and got.shape == want.shape, what
    a, b = got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        y, x, c = bad[0]
        raise AssertionError("%s: %d of %d words differ, first at (x %d, y %d, c %d): %r vs model %r"
                             % (what, len(bad), a.size, x, y, c, got[y, x, c], want[y, x, c]))


def run(flow, frames, **options):
    """[(result of process_frame, stats)] of a fresh DenseFlow over the frames."""
    H, W = frames[0].shape[:2]
    d = flow.DenseFlow(W, H, **options)
    out = []
    for f in frames:
        r = d.process_frame(f)
        out.append((r, d.last_stats()))
    d.close()
    return out


# ---- 1. sequences at every size --------------------------------------------------------------------
@pytest.mark.parametrize("case", fc.SEQUENCE_CASES + fc.OPTION_CASES + fc.STOP_CASES, ids=fc.case_id)
def test_sequence_equals_model(flow, case):
    """4 luminance frames -> 3 backward flows, each bit-identical to the model's, with the model's
    number of executed iterations (the stop test is decided on the device)."""
    pattern, W, H, iterations, warps = case
    frames = fc.frames(pattern, W, H)
    flows, infos = fc.model(*case)
    got = run(flow, frames, iterations=iterations, warps=warps)
    assert got[0][0] is None
    for k in range(1, len(frames)):
        r, stats = got[k]
        assert_bits(r, flows[k], "%s frame %d" % (fc.case_id(case), k))
        assert stats["scales"] == infos[k]["scales"]
        assert stats["iterations_run"] == infos[k]["iterations_run"], (k, stats, infos[k])
        assert stats["host_syncs"] == 1


# ---- 2. options -------------------------------------------------------------------------------------
def test_bgr_strided_and_luminance_inputs_agree(flow):
    """A BGR frame with padded rows, a packed one and its luminance plane give the same flow."""
    packed = fc.colour_frames()
    H, W = packed[0].shape[:2]
    strided, lums = [], []
    for bgr in packed:
        buf = np.full((H, W * 3 + 13), 0xAB, np.uint8)
        buf[:, :W * 3] = bgr.reshape(H, W * 3)
        strided.append(buf[:, :W * 3].reshape(H, W, 3))
        lums.append(fm.luminance(bgr))
    assert strided[0].strides[0] == W * 3 + 13
    assert (packed[1][..., 0] != packed[1][..., 1]).any()
    want, _ = fc.colour_model()
    for frames in (packed, strided, lums):
        got = run(flow, frames)
        for k in (1, 2):
            assert_bits(got[k][0], want[k], "frame %d" % k)


def test_flow_type_both_and_forward(flow):
    """forward = calc(previous, current): the backward flow of the swapped pair."""
    frames = fc.frames("translated", 96, 64)
    bwd, _ = fc.model("translated", 96, 64, 10, 2)
    fwd = [None] + [fm.tvl1(frames[k - 1], frames[k])[0] for k in range(1, len(frames))]
    both = run(flow, frames, flow_type=flow.FLOW_BOTH)
    only_f = run(flow, frames, flow_type=flow.FLOW_FORWARD)
    assert both[0][0] is None and only_f[0][0] is None
    for k in range(1, len(frames)):
        b, f = both[k][0]
        assert_bits(b, bwd[k], "backward %d" % k)
        assert_bits(f, fwd[k], "forward %d" % k)
        assert_bits(only_f[k][0], fwd[k], "forward only %d" % k)
    # forward of (a, b) is what a backward handle computes for the pair fed in the other order
    swapped = run(flow, [frames[1], frames[0]])
    assert_bits(swapped[1][0], fwd[1], "swapped pair")


# ---- 3. the stop test fires inside the loop ---------------------------------------------------------
def test_stop_flag_skips_the_remaining_launches(flow):
    """The launch count does not depend on the data; the executed iterations do."""
    case = fc.STOP_CASES[0]
    _, infos = fc.model(*case)
    got = run(flow, fc.frames(*case[:3]), iterations=case[3], warps=case[4])
    launches = {s["launches"] for _, s in got[1:]}
    assert len(launches) == 1
    runs = [s["iterations_run"] for _, s in got[1:]]
    assert runs == [i["iterations_run"] for i in infos[1:]]
    assert min(runs) < infos[1]["scales"] * case[3] * case[4]


# ---- 4. memory and determinism ---------------------------------------------------------------------
def test_device_memory_determinism_restart(flow):
    import torch
    W, H = 67, 45
    frames = [fm.gray_to_bgr(g) for g in fc.frames("split", W, H)]
    want, _ = fc.model("split", W, H, 10, 2)
    d = flow.DenseFlow(W, H)
    first, allocs = [], []
    for f in frames:
        first.append(d.process_frame(f))
        s = d.last_stats()
        allocs.append(s["device_allocations"])
        assert s["host_syncs"] == 1
    assert len(set(allocs)) == 1, allocs     # nothing is allocated after creation
    for k in range(1, len(frames)):
        assert_bits(first[k], want[k], "host %d" % k)
    # restart reproduces the first run, byte for byte; device input and output equal host ones
    d.restart()
    for k, f in enumerate(frames):
        t = torch.from_numpy(f).cuda()
        r = d.process_frame_device(t)
        if k == 0:
            assert r is None
            continue
        assert r.is_cuda and tuple(r.shape) == (H, W, 2)
        assert first[k].tobytes() == r.cpu().numpy().tobytes()
        assert d.last_stats()["device_allocations"] == allocs[0]
    d.close()
    # a second handle: identical bytes again
    again = run(flow, frames)
    for k in range(1, len(frames)):
        assert first[k].tobytes() == again[k][0].tobytes()


# ---- 5. end to end: flow unit -> dense segmentation, all on the device -------------------------------
def test_flow_into_dense_segmentation_equals_oracle(flow):
    """DenseFlow (device output) feeds DenseSegmentation (device flow); the SegmentationDesc bytes
    equal the CPU oracle's fed with the MODEL's flow."""
    import torch
    import video_segment_amd as vsg
    W, H, N, chunk = fc.E2E
    frames = fc.e2e_frames()
    flows, _ = fc.e2e_model()
    d = flow.DenseFlow(W, H)
    g = vsg.DenseSegmentation(W, H, vsg.default_options(chunk_size=chunk, device=0), has_flow=True)
    o = ol.OracleStream(W, H, ol.default_options(chunk_size=chunk), has_flow=True)
    out = 0
    for k in range(N):
        t = torch.from_numpy(frames[k]).cuda()
        fl = d.process_frame_device(t)
        assert (fl is None) == (k == 0)
        ng = g.process_frame(t, fl, flush=(k == N - 1))
        no = o.process_frame(frames[k], flows[k], flush=(k == N - 1))
        assert ng == no, (k, ng, no)
        for i in range(ng):
            assert g.result_bytes(i) == o.result_bytes(i), "SegmentationDesc mismatch at %d/%d" % (k, i)
        out += ng
    assert out == N
    g.close()
    d.close()


# ---- 6. the driver: LuminanceUnit -> DenseFlowUnit in front of the dense unit ------------------------
@pytest.mark.parametrize("pipeline", ["--use_pipeline", "--nouse_pipeline"])
def test_seg_tree_synth_compute_flow(flow, tmp_path, pipeline):
    """seg_tree_synth --compute_flow --flow --save_flow: the .flow file holds the model's fields, and a
    second run that reads it through DenseFlowReaderUnit prints the same label hash."""
    from video_segment_amd import flow_io
    subprocess.check_call(["make", "-C", HOST, "-s"])
    W, H, N, chunk = fc.DRIVER
    want, _ = fc.driver_model()
    path = str(tmp_path / "computed.flow")
    base = [os.path.join(HOST, "seg_tree_synth"), "--width", str(W), "--height", str(H), "--frames", str(N),
            "--chunk_size", str(chunk), "--input", "probe", "--flow", pipeline]

    def first_line(stdout):
        return re.sub(r" seconds=\S+ fps=\S+", "", stdout.splitlines()[0])

    p = subprocess.run(base + ["--compute_flow", "--save_flow", "--flow_output_file", path], capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    r = flow_io.DenseFlowReader(path)
    r.open_and_read_header()
    assert (r.width, r.height, r.flow_type) == (W, H, flow_io.FLOW_BACKWARD)
    fields = list(r.fields(backward=True))
    r.close()
    assert len(fields) == N and fields[0] is None
    for k in range(1, N):
        assert_bits(fields[k], want[k], "field %d of the .flow file" % k)
    q = subprocess.run(base + ["--flow_file", path], capture_output=True, text=True, timeout=120)
    assert q.returncode == 0, q.stderr
    assert "label_fnv1a32=" in p.stdout
    assert first_line(p.stdout) == first_line(q.stdout)
