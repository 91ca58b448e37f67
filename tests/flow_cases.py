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


# ---- test_gpu_flow_edges.py: shapes, content and options the cases above do not reach ----------------
# name -> (group, frames() -> list of gray frames, iterations, warps); one flow per case unless the
# maker says otherwise
EDGE = {}
FAST = (12, -9)   # (dx, dy) of the fast-motion case


def _edge(group, name, maker, iterations=10, warps=2):
    assert name not in EDGE
    EDGE[name] = (group, maker, iterations, warps)


def _translated(W, H, **kw):
    return lambda: fm.translated_pattern(W, H, 2, SEED, **kw)


def _block(W, H, row, col, n=2):
    return lambda: fm.block_pattern(W, H, n, SEED, row, col)


# workgroups of the iteration kernel at the finest level: below, at and far above 256
for _W, _H in [(480, 136), (544, 136), (545, 137), (1056, 200), (16384, 16), (16, 2056)]:
    _edge("tiles", "translated-%dx%d" % (_W, _H), _translated(_W, _H))
# the only changed pixels lie in a tile of index 256 or above (271 and 288 of 289, 791 and 824 of 825) ...
_edge("late", "late-block-544x136", _block(544, 136, 126, 524, n=3))   # 3 frames: also fed to two handles
_edge("late", "late-block-1056x200", _block(1056, 200, 190, 1036))
# ... and in tile 0, as the counterpart
_edge("first", "first-block-544x136", _block(544, 136, 2, 2))
_edge("first", "first-block-1056x200", _block(1056, 200, 2, 2))
for _W, _H in [(1, 1), (2, 2), (1, 40), (40, 1), (31, 7), (33, 9)]:
    _edge("tiny", "translated-%dx%d" % (_W, _H), _translated(_W, _H))
_edge("pyramid", "translated-131x75", _translated(131, 75))
_edge("pyramid", "translated-75x131", _translated(75, 131))
_edge("pyramid", "translated-512x512-i3-w1", _translated(512, 512), 3, 1)
_edge("content", "constant-same", lambda: fm.constant_pattern(67, 45, (128, 128)))
_edge("content", "constant-128-129", lambda: fm.constant_pattern(67, 45, (128, 129)))
_edge("content", "letterbox-96x64", lambda: fm.letterbox_pattern(96, 64, 2, SEED))
_edge("content", "checker-96x64", lambda: fm.checker_pattern(96, 64, 2))
_edge("content", "fast-160x120", _translated(160, 120, dx=FAST[0], dy=FAST[1]))
_edge("options", "translated-67x45-i30-w3", _translated(67, 45), 30, 3)
_edge("options", "translated-33x31-i1-w64", _translated(33, 31), 1, 64)
_edge("options", "block-15x9-i1000-w1", lambda: fm.block_pattern(15, 9, 2, SEED), 1000, 1)


def edge_names(*groups):
    return [n for n, e in EDGE.items() if e[0] in groups]


@functools.lru_cache(maxsize=None)
def edge_frames(name):
    out = EDGE[name][1]()
    for f in out:
        f.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def edge_model(name):
    """(flows, infos) of the case's backward flows, as model()."""
    _, _, iterations, warps = EDGE[name]
    flows, infos = fm.backward_flows(list(edge_frames(name)), iterations, warps)
    for f in flows[1:]:
        f.setflags(write=False)
    return tuple(flows), tuple(infos)


@functools.lru_cache(maxsize=None)
def edge_forward_model(name):
    """The same for the forward flows: calc(previous, current)."""
    _, _, iterations, warps = EDGE[name]
    fr = edge_frames(name)
    res = [fm.tvl1(fr[k - 1], fr[k], iterations, warps) for k in range(1, len(fr))]
    for f, _ in res:
        f.setflags(write=False)
    return (None,) + tuple(f for f, _ in res), (None,) + tuple(i for _, i in res)


BOTH_EDGE = "late-block-544x136"   # flow_type both is run on these frames


def all_infos():
    """(label, info) of every flow the GPU tests compare."""
    out = []
    for name in EDGE:
        out += [(name + "/%d" % k, i) for k, i in enumerate(edge_model(name)[1]) if i is not None]
    out += [(BOTH_EDGE + "/forward/%d" % k, i) for k, i in enumerate(edge_forward_model(BOTH_EDGE)[1])
            if i is not None]
    for c in SEQUENCE_CASES + OPTION_CASES + STOP_CASES:
        out += [(case_id(c) + "/%d" % k, i) for k, i in enumerate(model(*c)[1]) if i is not None]
    out += [("e2e/%d" % k, i) for k, i in enumerate(e2e_model()[1]) if i is not None]
    out += [("colour/%d" % k, i) for k, i in enumerate(colour_model()[1]) if i is not None]
    out += [("driver/%d" % k, i) for k, i in enumerate(driver_model()[1]) if i is not None]
    # flow_type both: forward = calc(previous, current) over the translated 96 x 64 frames
    fr = frames("translated", 96, 64)
    out += [("forward/%d" % k, fm.tvl1(fr[k - 1], fr[k])[1]) for k in range(1, FRAMES)]
    return out
