"""The inputs of tests/test_gpu_build_edges.py and tests/test_gpu_readout_edges.py: frames at the
sizes where the graph-build and read-out kernels change path (tile edges, 64-lane steps, column
strides, row padding), and their oracle results, computed once and shared.
test_edge_shape_cases.py checks on the CPU that every case does what it is here for."""
import functools

import numpy as np

import oracle_lib as ol
import synth
from test_gpu_parity import rand_frame

# ---- piecewise-constant features: regions that hang together by diagonals only -----------------
PALETTE = np.array([(0.1, 0.2, 0.3), (0.9, 0.8, 0.7), (0.5, 0.1, 0.9)], np.float32)


def _xy(W, H):
    return np.arange(W)[None, :], np.arange(H)[:, None]


def _checker(W, H, t):
    x, y = _xy(W, H)
    return (x + y + t) % 2


def _diag3(W, H, t):
    x, y = _xy(W, H)
    return (x + y + t) % 3


def _anti3(W, H, t):
    x, y = _xy(W, H)
    return (x - y + t) % 3


def _stairs(W, H, t):
    x, y = _xy(W, H)
    return (((x + y) % 7 == 0) | ((x - y) % 5 == 0)).astype(np.int64)


def _sparse(W, H, t):
    return (np.random.default_rng(7).random((H, W)) < 0.3).astype(np.int64)


PATTERNS = {"checker": _checker, "diag3": _diag3, "anti3": _anti3, "stairs": _stairs, "sparse": _sparse}


@functools.lru_cache(maxsize=None)
def features(pattern, W, H, t):
    """H x W x 3 f32 features of frame t (read-only)."""
    f = np.ascontiguousarray(PALETTE[PATTERNS[pattern](W, H, t)])
    f.setflags(write=False)
    return f


# ---- read-out shapes (W, H, F, min_region_size) ---------------------------------------------------
H1_SHAPE = (70, 1, 2, 0)                      # LaunchEnforceN4 returns early, no bottom edges
READOUT_SHAPES = [
    (2, 2, 1, 0), (2, 7, 2, 0), (3, 2, 1, 0),       # smallest frames
    (63, 5, 2, 0), (64, 9, 2, 0), (65, 9, 2, 0),    # 64-lane step edges of the run kernels
    (257, 6, 2, 0),                                 # second trip of k_n4_row_flags' 256 stride
    (1030, 5, 1, 0),                                # second trip of k_enforce_n4's 1024 stride
    (129, 33, 3, 2),                                # several frames, min-size merging
    H1_SHAPE,
]
READOUT_CASES = [(p,) + s for s in READOUT_SHAPES for p in PATTERNS]
# Cases in which the oracle's N4 pass moves no pixel (everything else has to move some).
N4_IDLE_CASES = {(p,) + H1_SHAPE for p in PATTERNS} | {
    ("diag3", 2, 2, 1, 0), ("anti3", 2, 2, 1, 0), ("sparse", 2, 2, 1, 0), ("sparse", 3, 2, 1, 0)}
FLAG_CASES = [(p,) + s for s in ((65, 9, 2, 0), (129, 33, 3, 2)) for p in ("checker", "diag3", "sparse")]
FLOW_CASES = [(p, 129, 33, 3, 2) for p in ("diag3", "sparse")]
UNHASHED_CASES = [(p,) + s for s in ((1030, 5, 1, 0), (129, 33, 3, 2)) for p in PATTERNS]
WIDE_CASE = ("diag3", 4100, 3, 1, 0)          # 16 * 4100 bytes of LDS: just past 64 KiB


def readout_id(c):
    return "%s-%dx%dx%d-min%d" % c


def build_graph(graph, case, use_flows=False, oracle=False):
    """Feeds the frames of a read-out case to a DenseSegGraph or an OracleGraph; returns the flows
    (one per frame, None for the first) or None."""
    pattern, W, H, F, _ = case
    fl = synth.const_flow(W, H) if use_flows else None
    prev = None
    for t in range(F):
        feat = features(pattern, W, H, t)
        if oracle:
            graph.add_frame(feat)
            if t:
                graph.add_temporal(feat, prev, fl)
        else:
            graph.add_frame_features(feat)
            if t:
                graph.add_temporal(fl)
        prev = feat
    return ([None] + [fl] * (F - 1)) if use_flows else None


@functools.lru_cache(maxsize=None)
def oracle_readout(case, use_flows=False, enforce_n4=True, enforce_connected=True):
    """The oracle's graph of a read-out case after segment + obtain_results (only read it)."""
    _, W, H, F, min_size = case
    og = ol.OracleGraph(W, H, F)
    flows = build_graph(og, case, use_flows, oracle=True)
    og.segment(min_size, False)
    og.obtain_results(flows, enforce_n4, enforce_connected)
    return og


# ---- bilateral / min-max frames -------------------------------------------------------------------
FRAME_SIZES = [(2, 1), (2, 2), (3, 9), (9, 3), (8, 8), (64, 64), (65, 63), (63, 65), (129, 65),
               (128, 127), (1400, 3), (1089, 961)]
BIG_SIZE = (1089, 961)        # 18 x 16 = 288 tiles > 256; last tile column and row are 1 px wide
FRAME_KINDS = ["noise", "const", "extremes"]
PADS = [0, 1, 5, 13, 16]
EXTREME_BASE, EXTREME_MIN, EXTREME_MAX = 100, 3, 255


def extreme_rows(W, H, pad):
    """(row whose first byte holds the minimum, row whose last byte holds the maximum).  With the
    rows `stride` bytes apart from a 16-byte aligned start, k_minmax_u8 reads a row's first byte as
    a head byte where the row starts unaligned and its last byte as a tail byte where it ends
    unaligned: such rows are taken where the frame has them."""
    stride = 3 * W + pad
    lo = next((y for y in range(H) if (y * stride) % 16), 0)
    hi = next((y for y in range(H) if y != lo and (y * stride + 3 * W) % 16),
              next((y for y in range(H) if y != lo), 0))
    return lo, hi


@functools.lru_cache(maxsize=None)
def padded_frame(W, H, kind, pad):
    """(H x W x 3 u8 view whose rows are 3 W + pad bytes apart, the buffer behind it).  The padding
    holds 0x00 and 0xFF in turn (by byte, starting with the row's parity): a read of it changes the
    frame's min / max and with it the scale of the bilateral LUT."""
    rng = np.random.default_rng(1)
    buf = np.empty((H, W * 3 + pad), np.uint8)
    if kind == "extremes":
        frame = np.full((H, W * 3), EXTREME_BASE, np.uint8)
        lo, hi = extreme_rows(W, H, pad)
        frame[hi, W * 3 - 1] = EXTREME_MAX
        frame[lo, 0] = EXTREME_MIN
    else:
        frame = rand_frame(rng, W, H, kind).reshape(H, W * 3)
    buf[:, :W * 3] = frame
    fill = ((np.arange(pad)[None, :] + np.arange(H)[:, None]) % 2) * 0xFF
    buf[:, W * 3:] = fill.astype(np.uint8)
    buf.setflags(write=False)
    view = np.lib.stride_tricks.as_strided(buf, (H, W, 3), (buf.strides[0], 3, 1), writeable=False)
    return view, buf


def _bilateral_cases():
    """(W, H, kind, pad, presmoothing): the cross product pruned to 58 graphs.  Every size runs all
    kinds with the bilateral filter and one kind with each other mode, the pads rotate so that every
    pad meets `extremes`; the 288-tile frame runs once per mode."""
    out = []
    for i, (W, H) in enumerate(FRAME_SIZES):
        pad = [PADS[(i + k) % len(PADS)] for k in range(5)]
        if (W, H) == BIG_SIZE:
            out += [(W, H, "noise", pad[0], 2), (W, H, "extremes", pad[3], 0), (W, H, "noise", pad[4], 1)]
            continue
        out += [(W, H, "noise", pad[0], 2), (W, H, "const", pad[1], 2), (W, H, "extremes", pad[2], 2),
                (W, H, "extremes", pad[3], 0), (W, H, "noise", pad[4], 1)]
    return out


BILATERAL_CASES = _bilateral_cases()


def bilateral_id(c):
    return "%dx%d-%s-pad%d-pre%d" % c


@functools.lru_cache(maxsize=None)
def oracle_smoothed(W, H, kind, pad, presmoothing):
    out = ol.preprocess(padded_frame(W, H, kind, pad)[0], presmoothing)
    out.setflags(write=False)
    return out


# ---- edge-key frames ------------------------------------------------------------------------------
# 2048 / 2049 pixels: on and one past a tile of k_spatial_keys; 1024 / 1025: of k_temporal_keys.
KEY_SIZES = [(2, 1), (2, 2), (2, 1024), (1024, 2), (3, 683), (2049, 1), (2, 512), (5, 205)]
TILE_EDGE_SIZES = KEY_SIZES[2:]
TWO_TILE_SIZES = [(2, 1024), (1024, 2), (3, 683), (2049, 1)]
BELOW_2_31 = 2147483520.0     # the largest f32 below 2^31
_SPECIAL = [np.inf, -np.inf, np.nan, 1e12, -1e12, BELOW_2_31]
# (flow x, flow y, side of the frame it is applied on); None keeps the pixel's noise value.
BORDER_SET = (
    [(-0.5, None, "left"), (-1.0, None, "left"), (-1.5, None, "left"),
     (0.99, None, "right"), (1.0, None, "right"),
     (None, -0.5, "top"), (None, -1.0, "top"), (None, -1.5, "top"),
     (None, 0.99, "bottom"), (None, 1.0, "bottom")] +
    [(v, None, ("left", "right", "top", "bottom")[k % 4]) for k, v in enumerate(_SPECIAL)] +
    [(None, v, ("top", "bottom", "left", "right")[k % 4]) for k, v in enumerate(_SPECIAL)] +
    [(-0.5, -0.5, "tl"), (0.99, -1.0, "tr"), (-1.5, 1.0, "bl"), (1.0, 0.99, "br")])


def _side_pixels(W, H, side):
    corner = {"tl": (0, 0), "tr": (0, W - 1), "bl": (H - 1, 0), "br": (H - 1, W - 1)}
    if side in corner:
        return [corner[side]]
    if side in ("left", "right"):
        x = 0 if side == "left" else W - 1
        ys = list(range(1, H - 1)) or list(range(H))
        return [(y, x) for y in ys]
    y = 0 if side == "top" else H - 1
    xs = list(range(1, W - 1)) or list(range(W))
    return [(y, x) for x in xs]


@functools.lru_cache(maxsize=None)
def key_inputs(W, H):
    """(f0, f1, flow, placed): two feature frames, the backward flow of the second and where the rows
    of BORDER_SET ended up -- placed[(y, x)] = index of the row that owns the pixel (a small frame
    has fewer border pixels than the set has rows: later rows overwrite earlier ones)."""
    rng = np.random.default_rng(2)
    f0 = rng.random((H, W, 3), dtype=np.float32)
    f1 = (f0 + rng.normal(0, 0.02, (H, W, 3))).astype(np.float32)
    flow = rng.normal(0, 3.0, (H, W, 2)).astype(np.float32)
    placed = {}
    cursor = {}
    for k, (fx, fy, side) in enumerate(BORDER_SET):
        px = _side_pixels(W, H, side)
        y, x = px[cursor.get(side, 0) % len(px)]
        cursor[side] = cursor.get(side, 0) + 1
        if (y, x) in placed:       # the earlier row leaves: back to plain noise in both parts
            flow[y, x] = np.random.default_rng(1000 + k).normal(0, 3.0, 2).astype(np.float32)
        if fx is not None:
            flow[y, x, 0] = fx
        if fy is not None:
            flow[y, x, 1] = fy
        placed[(y, x)] = k
    for a in (f0, f1, flow):
        a.setflags(write=False)
    return f0, f1, flow, placed


def _trunc_x86(v):
    """int(float) as cvttss2si does it: NaN and everything outside [-2^31, 2^31) give INT_MIN."""
    if not (v >= -2147483648.0 and v < 2147483648.0):
        return -2 ** 31
    return int(v)


def model_prev_xy(W, H, flow):
    """The previous-frame location (x, y planes) every pixel's temporal edges go to: the pixel
    position plus its flow in f32, truncated, clamped to the frame."""
    px = np.empty((H, W), np.int64)
    py = np.empty((H, W), np.int64)
    for y in range(H):
        for x in range(W):
            px[y, x] = min(W - 1, max(0, _trunc_x86(np.float32(x) + flow[y, x, 0])))
            py[y, x] = min(H - 1, max(0, _trunc_x86(np.float32(y) + flow[y, x, 1])))
    return px, py


@functools.lru_cache(maxsize=None)
def oracle_keys(W, H, l1, with_flow):
    """(spatial buckets of f0, of f1, temporal buckets of f1 over f0, prev_idx) from the oracle."""
    f0, f1, flow, _ = key_inputs(W, H)
    tb, pidx = ol.temporal_buckets(f1, f0, flow if with_flow else None, l1)
    out = (ol.spatial_buckets(f0, l1), ol.spatial_buckets(f1, l1), tb, pidx)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _oracle_merge(W, H, min_size):
    f0, f1, flow, _ = key_inputs(W, H)
    og = ol.OracleGraph(W, H, 2)
    og.add_frame(f0)
    og.add_frame(f1)
    og.add_temporal(f1, f0, flow)
    og.segment(min_size, False)
    out = (og.merge_stats(), og.node_roots(), og.node_states())
    for a in (out[0], out[1]) + out[2]:
        a.setflags(write=False)
    return out


def oracle_merge(W, H, min_size):
    """(merge_stats, node_roots) of the oracle's two-frame graph over key_inputs with flow."""
    return _oracle_merge(W, H, min_size)[:2]


def oracle_merge_states(W, H, min_size):
    """The same graph's node states (node_states.py) after the merge."""
    return _oracle_merge(W, H, min_size)[2]
