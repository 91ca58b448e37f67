"""The inputs of tests/test_gpu_flow.py and their model results, computed once and shared.
test_flow_model.py checks on the CPU that no stop test of any of them is close to its threshold."""
import functools

import numpy as np

import flow_model as fm
import synth

SIZES = [(96, 64), (67, 45), (16, 16), (15, 9), (33, 31), (256, 256)]
PATTERNS = {"translated": fm.translated_pattern, "split": fm.split_pattern, "block": fm.block_pattern}
SEED = 11
FRAMES = 4

# (pattern, W, H, iterations, warps)
SEQUENCE_CASES = [(p, W, H, 10, 2) for (W, H) in SIZES for p in ("translated", "split")]
OPTION_CASES = [("translated", 96, 64, 1, 2), ("translated", 96, 64, 10, 1), ("split", 67, 45, 1, 1)]
# nearly static frames with one changed block: the stop test fires inside the loop
STOP_CASES = [("block", 96, 64, 10, 2), ("block", 67, 45, 10, 2), ("block", 256, 256, 10, 2)]
E2E = (96, 64, 20, 8)   # W, H, frames, chunk size: synth.bench_frame through DenseSegmentation


def case_id(c):
    return "%s-%dx%d-i%d-w%d" % c


@functools.lru_cache(maxsize=None)
def frames(pattern, W, H):
    return tuple(PATTERNS[pattern](W, H, FRAMES, SEED))


@functools.lru_cache(maxsize=None)
def model(pattern, W, H, iterations, warps):
    """(flows, infos) of fm.backward_flows over the case's frames; flows[0] is None."""
    flows, infos = fm.backward_flows(list(frames(pattern, W, H)), iterations, warps)
    for f in flows[1:]:
        f.setflags(write=False)
    return tuple(flows), tuple(infos)


@functools.lru_cache(maxsize=None)
def e2e_frames():
    W, H, n, _ = E2E
    return tuple(synth.bench_frame(W, H, k) for k in range(n))


@functools.lru_cache(maxsize=None)
def e2e_model():
    flows, infos = fm.backward_flows([fm.luminance(f) for f in e2e_frames()])
    for f in flows[1:]:
        f.setflags(write=False)
    return tuple(flows), tuple(infos)


@functools.lru_cache(maxsize=None)
def colour_frames():
    """3 BGR frames, 67 x 45, whose channels differ: the translated pattern with a noisy blue channel."""
    W, H = 67, 45
    rng = np.random.RandomState(4)
    out = []
    for g in fm.translated_pattern(W, H, 3, seed=21):
        bgr = fm.gray_to_bgr(g)
        bgr[..., 0] = np.clip(bgr[..., 0].astype(int) + rng.randint(-20, 20, (H, W)), 0, 255)
        bgr.setflags(write=False)
        out.append(bgr)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def colour_model():
    return fm.backward_flows([fm.luminance(f) for f in colour_frames()])


DRIVER = (64, 48, 14, 10)   # W, H, frames, chunk size: seg_tree_synth --input probe --compute_flow


@functools.lru_cache(maxsize=None)
def driver_model():
    W, H, n, _ = DRIVER
    flows, infos = fm.backward_flows([fm.luminance(synth.probe_frame(W, H, k)) for k in range(n)])
    return tuple(flows), tuple(infos)


def all_infos():
    """(label, info) of every flow the GPU tests compare."""
    out = []
    for c in SEQUENCE_CASES + OPTION_CASES + STOP_CASES:
        out += [(case_id(c) + "/%d" % k, i) for k, i in enumerate(model(*c)[1]) if i is not None]
    out += [("e2e/%d" % k, i) for k, i in enumerate(e2e_model()[1]) if i is not None]
    out += [("colour/%d" % k, i) for k, i in enumerate(colour_model()[1]) if i is not None]
    out += [("driver/%d" % k, i) for k, i in enumerate(driver_model()[1]) if i is not None]
    # flow_type both: forward = calc(previous, current) over the translated 96 x 64 frames
    fr = frames("translated", 96, 64)
    out += [("forward/%d" % k, fm.tvl1(fr[k - 1], fr[k])[1]) for k in range(1, FRAMES)]
    return out
