"""The state comparison of the GPU suite (node_states.py) can fail on its inputs: two mutants of the
oracle's region mean -- fused multiply-add, and sum-then-divide (oracle/Makefile, `make mutants`) --
change at least one state word of at least one region on every input of test_gpu_node_states.py and
on streaming inputs of run_streams, while the SegmentationDesc bytes and the merge statistics, all
the suite compared before, do not notice.  A condition on the inputs (their seeds are chosen for it),
not on the library.  CPU only."""
import numpy as np
import pytest

import node_state_cases as nc
import node_states as ns
import oracle_lib as ol
import synth
from test_gpu_merge_paths import twotone_frames
from test_gpu_parity import rand_frame

MUTANTS = ["fused", "sumdiv"]

# The two-pixel rows are the exception, and have to be: their one merge joins two regions of size 1,
# a = b = 0.5 exactly, and 0.5 x + 0.5 y, fma(0.5, x, 0.5 y) and (x + y) / 2 all round the exact sum
# once.  They are in the GPU cases for the smallest frame the library accepts, not for the mean.
IMMUNE = {"ramp2", "alternating2"}


def changed_regions(got, want):
    """(regions of `want` with a node whose state differs, regions of `want`)."""
    bad = ns.differing_nodes(got, want)
    return len(np.unique(want[0][bad])), len(np.unique(want[0]))


@pytest.mark.parametrize("mutant", MUTANTS)
@pytest.mark.parametrize("name", list(nc.CASES))
def test_mutant_changes_a_state_on_every_graph_case(name, mutant):
    want, want_stats = nc.oracle_result(name)
    og = nc.oracle_graph(name, ol.mutant_lib(mutant))
    got, stats = og.node_states(), og.merge_stats()
    og.close()
    changed, regions = changed_regions(got, want)
    print("%s %s: %d of %d regions changed (%.0f %%); merge statistics %s" % (
        name, mutant, changed, regions, 100.0 * changed / regions,
        "changed" if not np.array_equal(stats, want_stats) else "unchanged"))
    if name in IMMUNE:
        assert changed == 0
    else:
        assert changed > 0, "the comparison could not fail on %s: choose another seed" % name


# (W, H, N, kind, chunk): the first six are inputs of the existing streaming tests (flow, default options)
STREAMS = [(64, 48, 45, "probe", 20), (64, 48, 30, "noise", 8), (96, 64, 26, "smooth", 10),
           (128, 96, 24, "bench", 20), (192, 144, 30, "bench", 10), (160, 120, 24, "twotone", 8)]


def stream_frames(kind, W, H, N):
    if kind == "probe":
        return [synth.probe_frame(W, H, k) for k in range(N)]
    if kind == "bench":
        return [synth.bench_frame(W, H, k) for k in range(N)]
    if kind == "twotone":
        return twotone_frames(W, H, N)
    rng = np.random.default_rng(5)
    return [rand_frame(rng, W, H, kind) for _ in range(N)]


def run_oracle_stream(L, W, H, frames, chunk):
    """[(states, merge statistics) per segmented chunk], all result bytes."""
    o = ol.OracleStream(W, H, ol.default_options(chunk_size=chunk), has_flow=True, L=L)
    o.keep_node_states()
    fl = synth.const_flow(W, H)
    chunks, out = [], []
    for k, frame in enumerate(frames):
        n = o.process_frame(frame, fl if k > 0 else None, flush=(k == len(frames) - 1))
        if n:
            chunks.append((o.last_node_states(), o.last_merge_stats()))
        out += [o.result_bytes(i) for i in range(n)]
    o.close()
    return chunks, out


@pytest.mark.parametrize("W,H,N,kind,chunk", STREAMS)
def test_mutants_change_states_on_streaming_inputs(W, H, N, kind, chunk):
    frames = stream_frames(kind, W, H, N)
    want_chunks, want_bytes = run_oracle_stream(None, W, H, frames, chunk)
    for mutant in MUTANTS:
        chunks, got_bytes = run_oracle_stream(ol.mutant_lib(mutant), W, H, frames, chunk)
        assert len(chunks) == len(want_chunks)
        changed = regions = 0
        stats_changed = False
        for (got, stats), (want, want_stats) in zip(chunks, want_chunks):
            stats_changed = stats_changed or not np.array_equal(stats, want_stats)
            if not np.array_equal(ns.canon_partition(got[0]), ns.canon_partition(want[0])):
                changed += len(np.unique(want[0]))   # (another partition: everything counts as changed)
            else:
                changed += changed_regions(got, want)[0]
            regions += len(np.unique(want[0]))
        print("%s %dx%d N%d chunk %d, %s: %d of %d regions changed (%.0f %%); bytes %s, merge statistics %s" % (
            kind, W, H, N, chunk, mutant, changed, regions, 100.0 * changed / regions,
            "changed" if got_bytes != want_bytes else "unchanged", "changed" if stats_changed else "unchanged"))
        assert changed > 0


def test_keeping_states_leaves_the_stream_alone():
    """Keeping on or off: the same bytes and statistics (the oracle's timed path -- bench.py's
    cpu_baseline -- never turns it on)."""
    W, H, N, chunk = 64, 48, 20, 8
    frames = stream_frames("bench", W, H, N)
    fl = synth.const_flow(W, H)
    outs = []
    for keep in (False, True):
        o = ol.OracleStream(W, H, ol.default_options(chunk_size=chunk), has_flow=True)
        o.keep_node_states(keep)
        out = []
        for k, frame in enumerate(frames):
            n = o.process_frame(frame, fl if k > 0 else None, flush=(k == N - 1))
            out += [o.result_bytes(i) for i in range(n)]
        outs.append(out)
        o.close()
    assert outs[0] == outs[1]
