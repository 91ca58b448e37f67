"""The state the ordered merge computes -- f32 mean, size, constraint id and flags of every region --
on inputs aimed at its arithmetic (node_state_cases.py), under the default knobs and with each worker
forced: word for word what the CPU oracle's sequential replay leaves (node_states.py).  Every case
also proves, from the library's own counters, that the worker it is named for ran on that input;
where an input cannot reach a worker (KNOBS says which can), the case asserts the weaker statement
listed there instead of none.

tests/test_oracle_state_mutants.py shows that each of these inputs (bar the two-pixel rows) can
fail: a fused or a re-associated mean changes its words."""
import numpy as np
import pytest

import node_state_cases as nc
import node_states as ns
from test_gpu_parity import vsg  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

ROWS = [n for n in nc.CASES if n.startswith("ramp") or n.startswith("alternating")]
RAMPS = [n for n in ROWS if n.startswith("ramp")]


def row_edges(name):
    return nc.CASES[name][0] - 1


def counters(g):
    """What the last segment() call ran, from vsg_graph_spine_paths / _merge_paths / _diagnostics /
    _timings."""
    c = dict(g.last_spine_paths())
    c.update(g.last_merge_paths())
    d, t = g.diagnostics(), g.timings()
    c.update(stages=d["stages"], rollbacks=d["rollbacks"], optimistic_stages=d["optimistic_stages"],
             wave_edges=t.wave_kernel_edges, wave_launches=t.wave_kernel_launches,
             spine_launches=t.spine_kernel_launches, spine_edges=t.spine_kernel_edges)
    return c


def positive(k):
    return ("%s > 0" % k, lambda c: c[k] > 0)


def none(k):
    return ("%s == 0" % k, lambda c: c[k] == 0)


# A ramp row is ONE component of W - 1 edges in ONE stage (all of its edges lie in bucket 0), so which
# worker replays it follows from its length alone: the lane worker up to small_seg edges (24 unless
# VSG_SMALL_SEG says otherwise), a wavefront (or the wide worker, or the tree replay) above.  The
# stacked rows are 33 such components of 64 edges, the hub block one of some 4000.  For the other
# inputs the largest component of a stage is not known by construction: where a knob is listed without
# them, the state comparison still runs and the proof is the knob's last entry (`elsewhere`).
LANE_ONLY = [none("wave_edges"), none("wide_launches"), none("replays"), positive("stages")]
WAVE = [positive("wave_edges")]

# knob name -> (environment or function of the case name, {case: proofs}, proofs elsewhere)
def _small_seg_above(name):      # the row is on the lane worker's side of the limit
    return {"VSG_SMALL_SEG": str(max(1, row_edges(name)))}


def _small_seg_below(name):      # ... one edge past it
    return {"VSG_SMALL_SEG": str(max(1, row_edges(name) - 1))}


BIG = ["stacked", "hub"]
# past the lane worker's default limit and short of the size from which a component goes to the tree
# replay by default (VSG_SPINE_MIN, 2048 edges)
MID_RAMPS = [n for n in RAMPS if 24 < row_edges(n) < 2048]
SPINE_RAMPS = [n for n in RAMPS if row_edges(n) >= 32]                  # VSG_SPINE_MIN=32
TWO_EDGE_ROWS = [n for n in RAMPS if row_edges(n) >= 2]


def _spine(passes):
    env = {"VSG_SPINE_MIN": "32", "VSG_SPINE_FAST_MIN": "0", "VSG_SPINE_FAST": str(passes)}
    proofs = [positive("replays"), positive("spine_launches"),
              positive("streamed_passes") if passes else none("streamed_passes")]
    return (env, {n: proofs for n in SPINE_RAMPS + BIG}, [positive("stages")])


KNOBS = {
    # default knobs: rows of up to 24 edges on single lanes, longer ones on a wavefront, 4096 edges on
    # the tree replay -- as is the hub input's block: a fresh handle keeps every stage for the tree replay,
    # and hub regions are only used in stages that it cannot take (RunBucketStage: try_hubs)
    "default": ({}, dict([(n, LANE_ONLY) for n in RAMPS if row_edges(n) <= 24] +
                         [(n, WAVE) for n in MID_RAMPS + ["stacked"]] +
                         [("ramp4097", [positive("replays"), positive("spine_launches")])] +
                         [("hub", [positive("replays"), none("hub_stages")])]),
                [positive("stages")]),
    # VSG_SMALL_SEG on both sides of the row's length (rows only; the two-pixel row has one edge and
    # small_seg cannot go below 1: the lane worker on both sides)
    "small_seg_at_row": (_small_seg_above, {n: LANE_ONLY for n in RAMPS}, [positive("stages")]),
    "small_seg_below_row": (_small_seg_below, dict([(n, WAVE) for n in TWO_EDGE_ROWS] + [("ramp2", LANE_ONLY)]),
                            [positive("stages")]),
    "small_seg_1": ({"VSG_SMALL_SEG": "1"}, {n: WAVE for n in ["stacked", "temporal", "constrained"]}, [positive("stages")]),
    "small_seg_100000": ({"VSG_SMALL_SEG": "100000"},
                         {n: LANE_ONLY for n in RAMPS + BIG + ["temporal", "constrained"]}, LANE_ONLY),
    # the wide worker takes the components past the lane worker's limit
    "wide_2": ({"VSG_WIDE_MIN": "1", "VSG_WIDE_WAVES": "2"}, {n: [positive("wide_launches")] for n in MID_RAMPS + ["stacked"]},
               [positive("stages")]),
    "wide_4": ({"VSG_WIDE_MIN": "1", "VSG_WIDE_WAVES": "4"}, {n: [positive("wide_launches")] for n in MID_RAMPS + ["stacked"]},
               [positive("stages")]),
    # the tree replay (k_spine) from 32 edges, its streamed spine with 0 - 3 passes
    "spine_fast_0": _spine(0), "spine_fast_1": _spine(1), "spine_fast_2": _spine(2), "spine_fast_3": _spine(3),
    # ... so hub regions need the tree replay off: the block absorbs the outliers through k_hub_apply
    "hubs_on": ({"VSG_SPINE_MIN": "0"}, {"hub": [positive("hub_stages"), positive("hub_absorbed"), none("replays")]},
                [none("replays"), positive("stages")]),
    "hubs_off": ({"VSG_HUBS": "0", "VSG_SPINE_MIN": "0"}, {},
                 [none("hub_stages"), none("hub_absorbed"), none("replays"), positive("stages")]),
    "rle_off": ({"VSG_RLE": "0"}, {}, [none("rle_stages"), positive("stages")]),
    # optimistic stages -- and with them something to roll back -- exist in a chunk with constraints and
    # where a stage is handed to the tree replay (the 4096-edge row and the hub block, by default)
    "force_rollback": ({"VSG_FORCE_ROLLBACK": "1"},
                       {n: [positive("optimistic_stages"), positive("rollbacks")] for n in ["constrained", "ramp4097", "hub"]},
                       [none("rollbacks")]),
    # the wave worker's chains without the relaxed batch rule: no counter tells the two apart, the proof
    # is that the wave worker, whose chain code the knob changes, replayed the input
    "chain_relax_off": ({"VSG_CHAIN_RELAX": "0"}, {n: WAVE for n in MID_RAMPS + ["stacked"]}, [positive("stages")]),
}
ROW_ONLY_KNOBS = ("small_seg_at_row", "small_seg_below_row")
PARAMS = [(k, n) for k in KNOBS for n in nc.CASES if not (k in ROW_ONLY_KNOBS and n not in ROWS)]


@pytest.mark.parametrize("knob,name", PARAMS)
def test_states_match_the_oracle(vsg, monkeypatch, knob, name):
    env, proofs_by_case, elsewhere = KNOBS[knob]
    if callable(env):
        env = env(name)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    W, H, F = nc.CASES[name]
    want, want_stats = nc.oracle_result(name)
    g = vsg.DenseSegGraph(W, H, F)
    min_size, force = nc.build(name, g, False)
    g.segment(min_size, force)
    got, stats, c = g.node_states(), g.merge_stats(), counters(g)
    g.close()
    print("%s %s %s: merges %s; %s" % (knob, name, env, stats.tolist(), {k: v for k, v in c.items() if v}))
    assert np.array_equal(stats, want_stats)
    ns.assert_states_equal(got, want, "%s under %s" % (name, knob), W, H)
    proofs = proofs_by_case.get(name, elsewhere)
    for what, holds in proofs:
        assert holds(c), "%s on %s: %s does not hold: %s" % (knob, name, what, c)


def test_every_knob_proves_its_worker_somewhere():
    """(no GPU work) Every knob has at least one input with a proof of its own, and every proof list
    used is non-empty where a case is named."""
    for knob, (_, by_case, elsewhere) in KNOBS.items():
        assert by_case or elsewhere, knob
        for name, proofs in by_case.items():
            assert name in nc.CASES and proofs, (knob, name)


def test_states_after_obtain_results_and_accessors_unharmed(vsg):
    """vsg_graph_node_states borrows nothing from the read-out: called after obtain_results it returns
    the same state, and the accessors after it (index_image, region_sizes) are unchanged."""
    name = "temporal"
    W, H, F = nc.CASES[name]
    g = vsg.DenseSegGraph(W, H, F)
    min_size, force = nc.build(name, g, False)
    g.segment(min_size, force)
    before = g.node_states()
    g.obtain_results(use_flows=True)
    images = [g.index_image(t) for t in range(F)]
    sizes = g.region_sizes()
    after = g.node_states()
    for a, b in zip(before, after):
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                              b.view(np.uint32) if b.dtype == np.float32 else b)
    for t in range(F):
        assert np.array_equal(g.index_image(t), images[t])
    assert all(np.array_equal(a, b) for a, b in zip(g.region_sizes(), sizes))
    ns.assert_states_equal(after, nc.oracle_result(name)[0], name, W, H)
    g.close()


def test_stream_keeping_off_adds_nothing(vsg):
    """With keeping off (the default) a stream has no states to hand out and its chunks' diagnostics
    count the allocations and device synchronisations of a stream that never heard of the hook; with
    keeping on the results are the same bytes."""
    import synth
    from video_segment_amd._lib import VsgError
    W, H, N, chunk = 64, 48, 20, 8
    fl = synth.const_flow(W, H)
    runs = []
    for keep in (None, False, True):
        s = vsg.DenseSegmentation(W, H, vsg.default_options(chunk_size=chunk), has_flow=True)
        if keep is not None:
            s.keep_node_states(keep)
        out, diags = [], []
        for k in range(N):
            n = s.process_frame(synth.bench_frame(W, H, k), fl if k > 0 else None, flush=(k == N - 1))
            out += [s.result_bytes(i) for i in range(n)]
            if n:
                d = s.last_diagnostics()
                diags.append((d["runtime_mallocs"], d["runtime_frees"], d["device_syncs"]))
                if keep:
                    assert len(s.last_node_states()[0]) > 0
                else:
                    with pytest.raises(VsgError):
                        s.last_node_states()
        s.close()
        runs.append((out, diags))
    assert runs[0][0] == runs[1][0] == runs[2][0]
    # (the first stream warms the block cache.)  The snapshot is taken after the merge, outside what a
    # chunk's diagnostics cover: switched on, it leaves the merge's own counts alone as well
    assert runs[1][1] == runs[2][1]
