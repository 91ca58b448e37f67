"""Frame ingest of the stream API when the input side of a frame (staging copy, min/max, LUT upload,
filter, flow copy) runs on a side stream beside the previous frame's edge kernels.

The caller's buffers are only valid during a call: every case here recycles ONE frame buffer and ONE
flow buffer and overwrites both with the next frame's data the moment `process_frame` returns.  A
library that still read them after the call, or whose edge kernels started before the filter had
written the feature plane, would not give the oracle's bytes.  Everything is compared byte for byte
with the CPU oracle (SegmentationDesc bytes, result counts, merge statistics); the oracle's results
of a sequence are computed once and shared by the cases that feed it in different ways.
"""
import time

import numpy as np
import pytest

import oracle_lib as ol
import synth

pytestmark = pytest.mark.gpu

CHUNK = 8
N = 23          # three chunks: 8 frames, then 7 new ones each, then a flush with the last frame
SIZES = [(64, 48), (161, 97)]   # the second: no tile or row alignment


@pytest.fixture(scope="module")
def vsg():
    import video_segment_amd as v
    from video_segment_amd import _lib
    _lib.build()
    assert _lib.lib().vsg_device_count() > 0, "GPU tests need a HIP device"
    return v


def lut_miss_frame(W, H, k):
    """The bench frame squeezed into [k + 1, 254 - k] with one pixel at k and one at 255 - k: minimum
    and maximum differ in every frame, so every frame needs a bilateral LUT of its own."""
    f = np.clip(synth.bench_frame(W, H, k), k + 1, 254 - k).astype(np.uint8)
    f[0, 0, :] = k
    f[H - 1, W - 1, :] = 255 - k
    return f


_sequences = {}


def sequence(W, H):
    key = (W, H)
    if key not in _sequences:
        frames = [lut_miss_frame(W, H, k) for k in range(N)]
        flows = [synth.var_flow(W, H, k) for k in range(N)]   # another field per frame
        for f in frames + flows:
            f.setflags(write=False)
        _sequences[key] = (frames, flows)
    return _sequences[key]


_oracle = {}


def oracle_results(W, H, flow, presmoothing, flushes, restarts):
    """Per call: (the result bytes, the merge statistics or None) of the oracle; computed once."""
    key = (W, H, flow, presmoothing, flushes, restarts)
    if key not in _oracle:
        frames, flows = sequence(W, H)
        o = ol.OracleStream(W, H, ol.default_options(chunk_size=CHUNK, presmoothing=presmoothing), has_flow=flow)
        calls = []
        for k in range(N):
            first = k == 0 or (k - 1) in restarts
            n = o.process_frame(frames[k], flows[k] if (flow and not first) else None, flush=k in flushes)
            calls.append(([o.result_bytes(i) for i in range(n)],
                          np.array(o.last_merge_stats()) if n else None))
            if k in restarts:
                o.restart()
        o.close()
        assert sum(len(c[0]) for c in calls) == N
        _oracle[key] = calls
    return _oracle[key]


def feed_and_compare(vsg, W, H, flow, mode, presmoothing=2, flushes=(N - 1,), restarts=()):
    frames, flows = sequence(W, H)
    want = oracle_results(W, H, flow, presmoothing, tuple(flushes), tuple(restarts))
    g = vsg.DenseSegmentation(W, H, vsg.default_options(chunk_size=CHUNK, presmoothing=presmoothing),
                              has_flow=flow)
    if mode == "device":
        import torch
        dev = torch.device("cuda", 0)
        fbuf = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
        flbuf = torch.empty((H, W, 2), dtype=torch.float32, device=dev)

        def put(k):
            fbuf.copy_(torch.from_numpy(frames[k].copy()))
            flbuf.copy_(torch.from_numpy(flows[k].copy()))

        def ready():
            torch.cuda.current_stream().synchronize()   # what produced the buffers has to be complete
    else:
        if mode == "strided":   # rows of a wider array: stride > 3 W
            wide = np.full((H, 3 * W + 37), 0xEE, np.uint8)
            fbuf = np.lib.stride_tricks.as_strided(wide, (H, W, 3), (wide.strides[0], 3, 1))
            assert fbuf.strides[0] > 3 * W
        else:
            fbuf = np.empty((H, W, 3), np.uint8)
        flbuf = np.empty((H, W, 2), np.float32)

        def put(k):
            fbuf[...] = frames[k]
            flbuf[...] = flows[k]

        def ready():
            pass

    put(0)
    since_boundary, wall = 0, 0.0
    checked_timings = 0
    for k in range(N):
        ready()
        t0 = time.perf_counter()
        first = k == 0 or (k - 1) in restarts   # first frame of a video: its flow is absent
        n = g.process_frame(fbuf, flbuf if (flow and not first) else None, flush=k in flushes)
        wall += time.perf_counter() - t0
        # the buffers are the caller's again: the next frame's data goes in right away
        if k + 1 < N:
            put(k + 1)
        elif mode == "device":
            fbuf.fill_(255)
            flbuf.fill_(1e6)
        else:
            fbuf[...] = 255
            flbuf[...] = 1e6
        since_boundary += 1
        got = [g.result_bytes(i) for i in range(n)]
        assert n == len(want[k][0]), (k, n, len(want[k][0]))
        for i in range(n):
            assert got[i] == want[k][0][i], "result %d of call %d differs from the oracle" % (i, k)
        if n:
            assert np.array_equal(g.last_merge_stats(), want[k][1]), k
            t = g.last_timings()
            # device time of the edge kernels, one bracket per frame of the chunk, summed after the
            # graph is complete: positive, and never more than the calls took on the host
            assert t.edge_launches == since_boundary and t.preprocess_launches == since_boundary
            assert t.edges_ms > 0
            assert t.edges_ms < wall * 1e3, (t.edges_ms, wall * 1e3)
            checked_timings += 1
            since_boundary, wall = 0, 0.0
        if k in restarts:
            g.restart()
    assert checked_timings >= 3
    g.close()


@pytest.mark.parametrize("mode", ["host", "device", "strided"])
@pytest.mark.parametrize("flow", [False, True])
@pytest.mark.parametrize("W,H", SIZES)
def test_recycled_buffers_every_frame_a_lut_miss(vsg, W, H, flow, mode):
    feed_and_compare(vsg, W, H, flow, mode)


@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("flow", [False, True])
@pytest.mark.parametrize("W,H", SIZES)
def test_recycled_buffers_without_presmoothing(vsg, W, H, flow, mode):
    """presmoothing = 0: no host wait inside the preprocessing at all -- only the wait for the inputs."""
    feed_and_compare(vsg, W, H, flow, mode, presmoothing=0)


@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("flow", [False, True])
@pytest.mark.parametrize("W,H", SIZES)
def test_flush_in_the_middle_of_a_chunk(vsg, W, H, flow, mode):
    """A flush with the fourth frame of the second chunk, then more frames.  Neither the reference nor
    the oracle can take a frame straight after a flush (the flushed stream keeps its last frame buffered
    and the next one would ask for temporal edges into a graph that has one slice: the oracle's CHECK in
    AddTemporalImpl), so the stream is restarted in between, which is how a caller goes on: the frames
    after it open an unconstrained graph again and run into a boundary and the final flush."""
    feed_and_compare(vsg, W, H, flow, mode, flushes=(11, N - 1), restarts=(11,))
