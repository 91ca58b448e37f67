"""GPU parity of the ordered merge's tree replay (merge_spine.hip RunSpineComponents and what the stage
driver does around it), with proof that each forced branch ran.

The suite's frames are far below the size from which the merge replays a component along its Kruskal
tree, so every case lowers VSG_SPINE_MIN; the other knobs force one branch of the host driver each.  A
case streams against the CPU oracle byte for byte (run_streams: result count per call, SegmentationDesc
bytes, merge statistics) and then asserts, from the library's own host counters (vsg_stream_last_spine_paths
summed over the chunks, deepest_level as a maximum), that the branch it is named for was taken.  No case
asserts `replays` alone.  VSG_SPINE_CHECK=1 (the replay's structure compared with a sequential replay on
the host) is on in every case except the ones that roll stages back."""
import numpy as np
import pytest

import synth
from test_gpu_merge_paths import frames_of as merge_frames_of
from test_gpu_parity import rand_frame, run_streams, vsg  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

BENCH_S = ("bench", 192, 144, 30, 10)   # three chunks
BENCH_L = ("bench", 256, 144, 44, 20)   # three chunks of up to 20 frames
NOISE = ("noise", 96, 64, 40, 8)
SMOOTH_L = ("smooth", 320, 240, 24, 8)


def frames_of(kind, W, H, N):
    if kind in ("noise", "bench", "twotone"):
        return merge_frames_of(kind, W, H, N)
    if kind == "blobs":
        return [synth.blobs_frame(W, H, k) for k in range(N)]
    if kind == "probe":
        return [synth.probe_frame(W, H, k) for k in range(N)]
    if kind == "smooth":
        rng = np.random.default_rng(5)
        return [rand_frame(rng, W, H, "smooth") for _ in range(N)]
    raise ValueError(kind)


def add_paths(total, stream):
    """Adds one chunk's counters to `total`: the spine paths, and what else proves a path (the side cuts
    of the merge paths, rollbacks and slab growths of the diagnostics, the kernel launch counts)."""
    for k, v in stream.last_spine_paths().items():
        if isinstance(v, list):
            total[k] = [a + b for a, b in zip(total.get(k, [0] * len(v)), v)]
        elif k == "deepest_level":
            total[k] = max(total.get(k, 0), v)
        else:
            total[k] = total.get(k, 0) + v
    mp, d, t = stream.last_merge_paths(), stream.last_diagnostics(), stream.last_timings()
    for k, v in (("spine_side_cuts", mp["spine_side_cuts"]), ("hub_stages", mp["hub_stages"]),
                 ("hub_cuts", mp["hub_cuts"]), ("group_halvings", mp["group_halvings"]),
                 ("rollbacks", d["rollbacks"]), ("slab_growths", d["slab_growths"]), ("stages", d["stages"]),
                 ("spine_pool_growths", d["spine_pool_growths"]),
                 ("wave_kernel_launches", t.wave_kernel_launches),
                 ("spine_kernel_launches", t.spine_kernel_launches)):
        total[k] = total.get(k, 0) + v
    total["chunks"] = total.get("chunks", 0) + 1


def stream_spine_paths(vsg, monkeypatch, env, kind, W, H, N, chunk):  # noqa: F811
    """Streams against the oracle under `env` and returns the counters summed over the segmented chunks."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    total = {}
    run_streams(vsg, W, H, N, None, True, chunk, frames=frames_of(kind, W, H, N),
                on_chunk=lambda stream: add_paths(total, stream))
    assert total["chunks"] >= 3, "fewer than three chunks: no constraints in play"
    print("%s %s %dx%d N=%d chunk=%d: %s" % (env, kind, W, H, N, chunk, total))
    return total


def streamed(passes):
    """The streamed spine on every replay: `passes` passes each, unless the pool refused."""
    def check(p):
        reached = p["replays"] - sum(p["pool_fallbacks"][1:])   # (replays that got to their spines)
        assert sum(p["pool_fallbacks"]) == 0, p
        assert p["streamed_passes"] == passes * p["replays"] - passes * p["streamed_refused"], p
        assert p["streamed_passes"] == passes * (reached - p["streamed_refused"]), p
    return check


def pool_too_small(p):
    assert p["top_level_fallbacks"] + p["nested_fallbacks"] > 0, p
    assert sum(p["pool_fallbacks"]) > 0, p
    # every refusal is handed on by exactly one caller
    assert sum(p["pool_fallbacks"]) == p["top_level_fallbacks"] + p["nested_fallbacks"], p
    print("pool_too_small: refusals at entry / edge arrays / tour arrays / side arrays: %s" % p["pool_fallbacks"])


def zero(*keys):
    def check(p):
        for k in keys:
            assert p[k] == 0, "%s != 0: %s" % (k, p)
    return check


def low_bucket(b):
    def check(p):
        assert p["low_bucket_failures"][b] > 0 and p["low_bucket_skips"][b] > 0, p
    return check


def ranked_plain_only_where_refused(p):
    assert p["ranked_plain"] == p["rank_sampling_refused"], p
    assert p["ranked_by_sampling"] + p["ranked_plain"] == p["replays"] - sum(p["pool_fallbacks"][1:3]), p


CHECK = {"VSG_SPINE_MIN": "32", "VSG_SPINE_CHECK": "1"}

# (name, environment, input, counters that must be > 0, further check or None).  The values each case
# reached on an MI355X are in DESIGN 4.21.
CASES = [
    ("replay_default_tail", CHECK, BENCH_S, ["replays", "components", "forest_rounds", "ranked_plain"],
     zero("ranked_by_sampling", "streamed_passes", "forest_compactions_ahead", "forest_compactions_sync")),
    ("nested_level", CHECK, BENCH_L, ["nested_replays", "deepest_level"], None),
    ("forest_one_round_ahead_compacts", dict(CHECK, VSG_BOR_COMPACT_MIN="16"), BENCH_S,
     ["forest_compactions_ahead"], zero("forest_compactions_sync")),
    ("forest_synchronous_compacts", dict(CHECK, VSG_BOR_AHEAD="0", VSG_BOR_COMPACT_MIN="16"), BENCH_S,
     ["forest_compactions_sync"], zero("forest_compactions_ahead")),
    ("sampled_ranking", dict(CHECK, VSG_RANK_SPLIT_MIN="0"), BENCH_S, ["ranked_by_sampling"],
     zero("ranked_plain", "rank_sampling_refused")),
    ("streamed_one_pass", dict(CHECK, VSG_SPINE_FAST_MIN="0", VSG_SPINE_FAST="1"), BENCH_S,
     ["streamed_passes"], streamed(1)),
    ("streamed_two_passes", dict(CHECK, VSG_SPINE_FAST_MIN="0", VSG_SPINE_FAST="2"), BENCH_S,
     ["streamed_passes"], streamed(2)),
    ("streamed_three_passes", dict(CHECK, VSG_SPINE_FAST_MIN="0", VSG_SPINE_FAST="3"), BENCH_S,
     ["streamed_passes"], streamed(3)),
    ("streamed_off", dict(CHECK, VSG_SPINE_FAST_MIN="0", VSG_SPINE_FAST="0"), BENCH_S,
     ["replays", "spine_kernel_launches"], zero("streamed_passes", "streamed_refused")),
    # (bench 256x144 N=44 chunk 20 reaches one refusal, of a nested level; the gradient reaches eight, of
    # both kinds)
    ("pool_too_small", dict(CHECK, VSG_SPINE_MAX_EDGES="4096"), SMOOTH_L,
     ["replays", "top_level_fallbacks", "nested_fallbacks"], pool_too_small),
    ("zero_pool_changes_halves", dict(CHECK, VSG_ZERO_POOL="4096"), BENCH_S, ["zero_pool_flips", "replays"], None),
    # (a rollback case: without the self check, as in test_stage_decomposition_variants)
    ("assumption_fails_and_reruns", {"VSG_SPINE_MIN": "32"}, NOISE,
     ["assumption_reruns", "limit_bucket_moves", "rollbacks"], None),
    # ---- paths that depend on the data as well (the inputs are the ones that reached them) ----------------
    ("jump_loop_ends_early", CHECK, ("blobs", 96, 64, 40, 8), ["jump_loops_ended_early", "forest_rounds"], None),
    # A noisy gradient keeps an edge inside a large component of bucket 1 chunk after chunk: the stage is
    # cut at that edge of the side cluster (spine_side_cuts), what cannot be cut is rerun without the replay
    # (low_bucket_failures[1]), and after two such chunks in a row bucket 1 goes without it for one chunk.
    ("side_cluster_cuts_and_cool_down", {"VSG_SPINE_MIN": "32"}, SMOOTH_L,
     ["spine_side_cuts", "assumption_reruns", "rollbacks"], low_bucket(1)),
    # sampling is due for every tour, and some find the pool used up by the tour's own arrays
    ("sampled_ranking_refused", dict(CHECK, VSG_SPINE_MAX_EDGES="16384", VSG_SPINE_FAST_MIN="0",
                                      VSG_RANK_SPLIT_MIN="0", VSG_BOR_COMPACT_MIN="16"), ("probe", 320, 240, 24, 8),
     ["rank_sampling_refused", "ranked_by_sampling"], ranked_plain_only_where_refused),
    # A threshold at or below the lane worker's limit (24 edges): the library raises it above that limit,
    # so no component is replayed twice.  Before that, every stream with VSG_SPINE_MIN=8 differed from the
    # oracle in its first chunk.
    ("threshold_below_the_lane_worker", dict(CHECK, VSG_SPINE_MIN="8"), BENCH_S,
     ["replays", "components", "forest_rounds", "spine_kernel_launches"], None),
    # Not reached by bench, noise, twotone, blobs, smooth or probe at 96x64 N=40 chunk 8, 192x144 N=30 chunk
    # 10 and 320x240 N=24 chunk 8, with VSG_SPINE_MIN=32 alone, with VSG_CUT_RATIO=1, and with
    # VSG_SPINE_MAX_EDGES = 4096 / 16384 / 65536 / 262144 together with VSG_SPINE_FAST_MIN=0,
    # VSG_RANK_SPLIT_MIN=0 and VSG_BOR_COMPACT_MIN=16 (126 streams, all byte-identical; VSG_SPINE_MIN=8 is
    # the same as 26, see above):
    #   forest_lists_refused == 0, streamed_refused == 0, pool_fallbacks[0] == [1] == [3] == 0 everywhere --
    #   every refusal (up to 20 per stream) came at pool_fallbacks[2], the tour's arrays.  The pool holds 16
    #   ints per edge of the stage + 64 K: the edge arrays (7 per edge) and the forest's two lists (2 per
    #   edge) always fit, a nested level is only chosen for a sixteenth of what is left, and the streamed
    #   spine's arrays (8.2 per tree edge) are taken after the tour's (18 per tree edge) are released.
    #   low_bucket_failures[0] / low_bucket_skips[0] == 0: the assumption failed in bucket 1 only.
]


@pytest.mark.parametrize("name,env,inp,must,check", CASES, ids=[c[0] for c in CASES])
def test_spine_path_runs_and_matches_oracle(vsg, monkeypatch, name, env, inp, must, check):  # noqa: F811
    paths = stream_spine_paths(vsg, monkeypatch, env, *inp)
    for k in must:
        assert paths[k] > 0, "%s: the path did not run (%s == 0): %s" % (name, k, paths)
    if check is not None:
        check(paths)
