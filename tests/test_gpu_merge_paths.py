"""GPU parity of the ordered merge's stage cuts and hub reruns (merge_stage.hip RunBucketStage /
retry_without_broken_hubs), with proof that each path ran.

At the suite's frame sizes a stage is too small for the default cut rule (a cut only above 1500 edges
per violation), so VSG_CUT_RATIO=1 lets them be cut.  VSG_HUB_CHECK=1 is on in every case: the host
checks that the hub list starts empty in every run of a stage and that every cut position lies in the
stage.  Each case streams against the CPU oracle byte for byte (run_streams: result count per call,
SegmentationDesc bytes, merge statistics) and then asserts, from the library's own counters
(vsg_stream_last_merge_paths summed over the chunks), that the path it is named for was taken."""
import numpy as np
import pytest

import synth
from test_gpu_parity import run_streams, vsg  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


def twotone_frames(W, H, N, seed=3):
    """Two large flat halves with a contrast edge of random height per frame (tools/stress_parity.py)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(N):
        img = np.zeros((H, W, 3), np.float64)
        img[:, : W // 2] = 60
        img[:, W // 2:] = 60 + rng.integers(8, 40)
        out.append(np.clip(img + rng.normal(0, 0.7, (H, W, 3)), 0, 255).astype(np.uint8))
    return out


def frames_of(kind, W, H, N):
    if kind == "noise":   # the bench shape with many small regions: +-40 per pixel and channel
        return [synth.noise_frame(W, H, k, 40) for k in range(N)]
    if kind == "bench":
        return [synth.bench_frame(W, H, k) for k in range(N)]
    if kind == "twotone":
        return twotone_frames(W, H, N)
    raise ValueError(kind)


def stream_paths(vsg, monkeypatch, env, kind, W, H, N, chunk):  # noqa: F811
    """Streams against the oracle under `env` (+ VSG_HUB_CHECK=1) and returns the merge path counters
    summed over the segmented chunks."""
    monkeypatch.setenv("VSG_HUB_CHECK", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    total = {}
    chunks = [0]

    def add(stream):
        chunks[0] += 1
        for k, v in stream.last_merge_paths().items():
            if k == "hub_reasons":
                total[k] = [a + b for a, b in zip(total.get(k, [0] * 6), v)]
            else:
                total[k] = total.get(k, 0) + v
        total["spine_launches"] = total.get("spine_launches", 0) + stream.last_timings().spine_kernel_launches

    run_streams(vsg, W, H, N, None, True, chunk, frames=frames_of(kind, W, H, N), on_chunk=add)
    assert chunks[0] >= 3, "fewer than three chunks: no constraints in play"
    print("%s %s %dx%d N=%d chunk=%d: %s" % (env, kind, W, H, N, chunk, total))
    return total


# (name, environment, input, counters that must be > 0).  Inputs chosen from the counters they reach on
# an MI355X; all at least three chunks, with flow, so the later chunks carry constraints.
CASES = [
    ("cut_in_one_bucket", {"VSG_SPINE_MIN": "0", "VSG_CUT_RATIO": "1", "VSG_GROUP_BUCKETS": "0"},
     ("bench", 192, 144, 30, 10), ["hub_cuts"]),
    ("cut_across_bucket_group", {"VSG_SPINE_MIN": "0", "VSG_CUT_RATIO": "1"},
     ("bench", 320, 240, 24, 8), ["hub_cuts", "hub_cuts_in_groups", "hub_parts_in_later_bucket"]),
    ("cut_budget_then_exclusion_list", {"VSG_SPINE_MIN": "0", "VSG_CUT_RATIO": "1", "VSG_HUB_SPLITS": "2"},
     ("noise", 96, 64, 40, 8), ["hub_cuts", "hub_exclusion_reruns"]),
    # (hub_off_reruns -- the fourth attempt, without hubs -- is reached by none of the inputs at these
    # sizes: the exclusion list settles every stage before that)
    ("no_cuts_exclusion_list", {"VSG_SPINE_MIN": "0", "VSG_HUB_SPLITS": "0"},
     ("noise", 96, 64, 40, 8), ["hub_exclusion_reruns"]),
    ("failed_group_halved", {"VSG_HUBS": "0", "VSG_FORCE_ROLLBACK": "1"},
     ("twotone", 160, 120, 24, 8), ["group_halvings"]),
    # The tree replay and the hub regions in one stream (never in one stage: the library refuses a stage
    # that has both, and a side cluster of the replay with hubs on, with VSG_ERR_INTERNAL), cuts allowed:
    # the hub absorptions stay in the stages without a replay, byte-identical.
    ("tree_replay_and_hubs", {"VSG_SPINE_MIN": "32", "VSG_CUT_RATIO": "1"},
     ("bench", 192, 144, 30, 10), ["hub_stages", "hub_absorbed", "spine_launches", "hub_cuts"]),
    # (the tree replay's side-cluster cuts, spine_side_cuts: none of these inputs reaches them; a noisy
    # gradient does -- test_gpu_spine_paths.py, side_cluster_cuts_and_cool_down)
]


@pytest.mark.parametrize("name,env,inp,must", CASES, ids=[c[0] for c in CASES])
def test_merge_path_runs_and_matches_oracle(vsg, monkeypatch, name, env, inp, must):  # noqa: F811
    paths = stream_paths(vsg, monkeypatch, env, *inp)
    for k in must:
        assert paths[k] > 0, "%s: the path did not run (%s == 0): %s" % (name, k, paths)
    if name == "no_cuts_exclusion_list":
        assert paths["hub_cuts"] == 0, paths   # (VSG_HUB_SPLITS=0: no stage is cut)


def test_long_noise_stream(vsg, monkeypatch):  # noqa: F811
    """400 frames of +-40 noise in chunks of 10 (45 segmented chunks; the suite form of
    tools/long_parity.py's noise streams): every chunk byte-identical with the default knobs, and again
    with every stage allowed to be cut."""
    W, H, chunk, N = 96, 64, 10, 400
    stream_paths(vsg, monkeypatch, {}, "noise", W, H, N, chunk)
    cut = stream_paths(vsg, monkeypatch, {"VSG_CUT_RATIO": "1"}, "noise", W, H, N, chunk)
    assert cut["hub_cuts"] > 0, cut
