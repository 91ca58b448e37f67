"""The stage filter's three ways to find an edge's list (k_filter): segment records
in the kernel's arguments, a table of records in device memory, no table (the search through the
bucket table in global memory).  VSG_FILTER_SEGS forces each of them: unset / 2 arguments where a
stage has at most 64 segments (the default), 1 always the device table, 0 no table.

Every case is a short stream (the first chunk and at least two constrained chunks) held against
the CPU oracle: the SegmentationDesc bytes of every frame and the merge statistics of every chunk.
The oracle's side of a case is computed once and shared by the three ways."""
import functools

import numpy as np
import pytest

import oracle_lib as ol
import synth
from test_gpu_parity import vsg  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

WAYS = {"arguments": None, "device_table": "1", "no_table": "0"}


def frames_of(kind, W, H, N):
    return [synth.FRAME_FNS[kind](W, H, k) for k in range(N)]


def flow_of(flow, W, H, k):
    return synth.const_flow(W, H) if flow == "const" else synth.var_flow(W, H, k)


@functools.lru_cache(maxsize=None)
def oracle_side(W, H, N, chunk, ratio, kind, flow):
    """What the oracle gives for every call: (number of results, their bytes, merge statistics)."""
    o = ol.OracleStream(W, H, ol.default_options(chunk_size=chunk, chunk_overlap_ratio=ratio), has_flow=True)
    out = []
    for k, frame in enumerate(frames_of(kind, W, H, N)):
        n = o.process_frame(frame, flow_of(flow, W, H, k) if k > 0 else None, flush=(k == N - 1))
        out.append((n, [o.result_bytes(i) for i in range(n)], o.last_merge_stats().copy() if n else None))
    o.close()
    assert sum(1 for c in out if c[0]) >= 3, "a case is the first chunk and at least two constrained ones"
    return out


def check_stream(vsg, W, H, N, chunk, ratio, kind, flow):  # noqa: F811
    want = oracle_side(W, H, N, chunk, ratio, kind, flow)
    g = vsg.DenseSegmentation(W, H, vsg.default_options(chunk_size=chunk, chunk_overlap_ratio=ratio), has_flow=True)
    for k, frame in enumerate(frames_of(kind, W, H, N)):
        n = g.process_frame(frame, flow_of(flow, W, H, k) if k > 0 else None, flush=(k == N - 1))
        assert n == want[k][0], (k, n, want[k][0])
        for i in range(n):
            assert g.result_bytes(i) == want[k][1][i], "SegmentationDesc differs: call %d, result %d" % (k, i)
        if n:
            assert np.array_equal(g.last_merge_stats(), want[k][2]), k
    g.close()


# (W, H, frames, chunk size, overlap ratio that gives the two overlap frames, generator, flow).  70 x 46 and
# 96 x 64: the width is no multiple of 64 and no stage's edge count is a multiple of the 512 edges of a
# workgroup, so the last threads of every launch repeat the last edge.
CASES = [
    (70, 46, 6, 3, 0.7, "bench", "const"),
    (70, 46, 6, 3, 0.7, "noise", "var"),
    (96, 64, 6, 3, 0.7, "blobs", "const"),
    (70, 46, 18, 7, 0.3, "blobs", "var"),
    (96, 64, 18, 7, 0.3, "bench", "var"),
    (96, 64, 18, 7, 0.3, "noise", "const"),
]


def set_way(monkeypatch, way):
    if WAYS[way] is None:
        monkeypatch.delenv("VSG_FILTER_SEGS", raising=False)
    else:
        monkeypatch.setenv("VSG_FILTER_SEGS", WAYS[way])


@pytest.mark.parametrize("way", list(WAYS))
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d_c%d_%s_%s" % (c[0], c[1], c[3], c[5], c[6]))
def test_every_way_gives_the_oracles_bytes(vsg, monkeypatch, way, case):  # noqa: F811
    set_way(monkeypatch, way)
    check_stream(vsg, *case)


@pytest.mark.parametrize("way", ["arguments", "device_table"])
def test_tail_stages_with_many_segments(vsg, monkeypatch, way):  # noqa: F811
    """Bucket groups make the stages of the tail span more (bucket, list) segments than the arguments hold,
    and more than the 512 a workgroup keeps: the table then lies in device memory and a workgroup finds
    its first segment with the two-level search.  Counted on an MI355X with a library that logged every
    filter launch: +-40 noise at 96 x 64, chunk 8: 374 stages, 22 with more than 64 segments, the longest
    table 348; the two chunk-7 streams below: 526 stages, 56 with more than 64 segments, 18 with more than
    512, the longest table 881 (with `device_table` every stage takes the table)."""
    set_way(monkeypatch, way)
    check_stream(vsg, 96, 64, 24, 8, 0.2, "noise", "const")
    check_stream(vsg, 96, 64, 18, 7, 0.3, "bench", "const")
    check_stream(vsg, 70, 46, 18, 7, 0.3, "noise", "var")


@pytest.mark.parametrize("way", list(WAYS))
def test_one_bucket_per_stage(vsg, monkeypatch, way):  # noqa: F811
    monkeypatch.setenv("VSG_GROUP_BUCKETS", "0")
    set_way(monkeypatch, way)
    check_stream(vsg, 70, 46, 18, 7, 0.3, "noise", "var")


@pytest.mark.parametrize("env", [{"VSG_INERT_MODE": "0"}, {"VSG_FORCE_ROLLBACK": "1"}])
@pytest.mark.parametrize("way", list(WAYS))
def test_deep_parent_chains_in_front_of_a_filter(vsg, monkeypatch, way, env):  # noqa: F811
    """Stages that leave their parent pointers uncompressed (every edge replayed on its own; every
    optimistic stage rolled back and replayed) put chains of depth two and more in front of the next
    filter: its compression writes parent[x0] and goes on from the first hop.  Counted on an MI355X with a
    library that counted the chains taking that branch, over the two streams: 199 966 with default
    knobs (the workers' own compression leaves such chains too), 195 500 with VSG_INERT_MODE=0 in 506
    stages, 203 730 with VSG_FORCE_ROLLBACK=1 in 6 914 stages -- the branch runs in every case here."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    set_way(monkeypatch, way)
    check_stream(vsg, 96, 64, 18, 7, 0.3, "bench", "const")
    check_stream(vsg, 70, 46, 18, 7, 0.3, "noise", "var")
