"""Inputs aimed at the arithmetic of the ordered merge (tests/test_gpu_node_states.py on the GPU,
tests/test_oracle_state_mutants.py on the CPU): tiny graphs whose f32 features are chosen, so that
the region means go through long chains of roundings.

A case is a name; build(name, graph) feeds it to a DenseSegGraph or an OracleGraph (the two differ in
add_frame / add_temporal only) and returns the arguments of segment().  Every array is built once
and is read-only.

An edge's weight is the RMS of the three channel differences and its bucket int(weight * 2048); the
merge walks the buckets in order and, inside a bucket, the edges in slot order.  Regions merge while
their means are closer than 0.05.
"""
import functools

import numpy as np

import synth

# 24: the lane worker's limit in edges (rows of 25 and 26 px are on and one past it); 64: one batch of
# the wave worker's chain; 129, 4097: more than one batch, by a little and by a lot.
ROW_WIDTHS = [2, 24, 25, 26, 63, 64, 65, 129, 4097]
BUCKET = 1.0 / 2048.0
# Seeds of the rows' jitter, chosen so that both mutants of the oracle's mean (oracle/Makefile) end in
# other words than the oracle does: tests/test_oracle_state_mutants.py asserts it.  (A fused mean
# differs in about one merge out of fifty, and a later merge can round the difference away.)
RAMP_SEEDS = {63: 2, 64: 2}         # default 1
ALTERNATING_SEEDS = {129: 3}        # default 2


def _frozen(a):
    a = np.ascontiguousarray(a, np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def ramp_row(W, seed=1):
    """1 x W: a slow ramp (one bucket's width over the whole row) with per-pixel, per-channel jitter.
    Every edge lies in bucket 0, so the row is one component of one stage and the region that starts
    at the left end absorbs it pixel by pixel, in rank order: a chain of W - 1 unequal merges."""
    rng = np.random.default_rng([seed, W])
    ramp = 0.3 + 0.4 * BUCKET * np.arange(W) / max(W - 1, 1)
    f = ramp[:, None] + rng.uniform(-0.1 * BUCKET, 0.1 * BUCKET, (W, 3))
    return _frozen(f[None])


def _valuation3(n):
    v = 0
    while n % 3 == 0:
        n //= 3
        v += 1
    return v


@functools.lru_cache(maxsize=None)
def alternating_row(W, seed=2):
    """1 x W: the step between x - 1 and x alternates in sign and lies in bucket 2 v + 1, v the 3-adic
    valuation of x.  Bucket 1 joins the pixels of every triple (1 + 1, then 2 + 1), bucket 3 the
    triples of every nonet (3 + 3: a tie, rep_2 survives and the roles of a and b swap; then 6 + 3),
    and so on: equal-sized regions whose size is no power of two meet at every level."""
    rng = np.random.default_rng([seed, W])
    f = np.empty((W, 3))
    f[0] = 0.5 + rng.uniform(-0.1 * BUCKET, 0.1 * BUCKET, 3)
    for x in range(1, W):
        step = (2 * _valuation3(x) + 1.5) * BUCKET * (1.0 if x % 2 else -1.0)
        f[x] = f[x - 1] + step + rng.uniform(-0.1 * BUCKET, 0.1 * BUCKET, 3)
    return _frozen(f[None])


STACK_ROWS, STACK_W = 33, 65


@functools.lru_cache(maxsize=None)
def stacked_rows(seed=3):
    """33 ramp rows of 65 px (each with its own jitter) separated by rows that alternate between 0.95
    and 0.05 from pixel to pixel: 33 independent chains in the first stage, and edges that fail (and
    finalize the rows) in the last buckets."""
    H = 2 * STACK_ROWS - 1
    f = np.empty((H, STACK_W, 3), np.float32)
    for r in range(STACK_ROWS):
        f[2 * r] = ramp_row(STACK_W, seed + 10 * r)[0]
        if r + 1 < STACK_ROWS:
            f[2 * r + 1] = np.where(np.arange(STACK_W) % 2 == 0, 0.95, 0.05)[:, None]
    return _frozen(f)


HUB_BLOCK = 32


@functools.lru_cache(maxsize=None)
def hub_frame(seed=4):
    """A flat (jittered inside bucket 0) 32 x 32 block ringed by single-pixel outliers, each far from
    the block and from its neighbours on the ring: with min_region_size > 1 the block is finalized by
    the first outlier edge that fails and then absorbs the outliers one by one (through k_hub_apply
    where hub regions are in use: VSG_SPINE_MIN=0, a fresh handle keeps its stages for the tree replay)."""
    rng = np.random.default_rng(seed)
    n = HUB_BLOCK + 2
    f = 0.5 + rng.uniform(-0.1 * BUCKET, 0.1 * BUCKET, (n, n, 3))
    ring = np.ones((n, n), bool)
    ring[1:-1, 1:-1] = False
    k = int(ring.sum())
    levels = np.where(np.arange(k) % 2 == 0, 0.1, 0.9)[:, None] + rng.uniform(-0.05, 0.05, (k, 3))
    f[ring] = levels
    # ... but one, 0.08 above the block: its edge fails some 550 buckets before the others' do, in a stage
    # of its own, so the block is finalized (and has absorbed it) when the stages of the outliers are
    # filtered -- what a hub region is (device_graph.h: kFlagHub)
    f[0, 5] = f[1, 5] + 0.08
    return _frozen(f)


TEMPORAL_WH = (40, 30)


@functools.lru_cache(maxsize=None)
def temporal_frames(seed=5):
    """Two 40 x 30 frames: a two-dimensional ramp (too steep for one region) with jitter spread over a few buckets, the
    second frame the first plus noise; connected by the nine-neighbour temporal edges under a constant
    flow."""
    W, H = TEMPORAL_WH
    rng = np.random.default_rng(seed)
    x, y = np.arange(W)[None, :, None], np.arange(H)[:, None, None]
    f0 = 0.3 + 0.25 * x / W + 0.2 * y / H + rng.uniform(-6 * BUCKET, 6 * BUCKET, (H, W, 3))
    f1 = f0 + rng.uniform(-2 * BUCKET, 2 * BUCKET, (H, W, 3))
    return _frozen(f0), _frozen(f1)


CONS_WH, CONS_REAL = (32, 24), 3


@functools.lru_cache(maxsize=None)
def constrained_chunk(seed=6):
    """A second chunk: a virtual slice, a constrained slice and two plain ones, 32 x 24.  The labels
    are 8 x 8 blocks (the constrained slice's shifted by two pixels); the features follow the
    constrained labels closely enough for forced merges, except that every block with an odd label
    is split in two halves 0.5 apart: regions of one constraint further apart than 0.15, which drops
    constraints."""
    W, H = CONS_WH
    rng = np.random.default_rng(seed)
    x, y = np.arange(W)[None, :], np.arange(H)[:, None]
    labels_v = ((y // 8) * (W // 8) + x // 8).astype(np.int32)
    labels_c = np.roll(labels_v, 2, axis=1).astype(np.int32)
    base = 0.2 + 0.05 * (labels_c % 7) + np.where((labels_c % 2 == 1) & (y % 8 >= 4), 0.5, 0.0)
    frames = []
    for t in range(CONS_REAL):
        frames.append(_frozen(base[:, :, None] + rng.uniform(-2 * BUCKET, 2 * BUCKET, (H, W, 3))))
    labels_v.setflags(write=False)
    labels_c.setflags(write=False)
    return labels_v, labels_c, tuple(frames)


# name -> (W, H, slices)
def _cases():
    out = {}
    for W in ROW_WIDTHS:
        out["ramp%d" % W] = (W, 1, 1)
        out["alternating%d" % W] = (W, 1, 1)
    out["stacked"] = (STACK_W, 2 * STACK_ROWS - 1, 1)
    out["hub"] = (HUB_BLOCK + 2, HUB_BLOCK + 2, 1)
    out["temporal"] = TEMPORAL_WH + (2,)
    out["constrained"] = CONS_WH + (CONS_REAL + 1,)
    return out


CASES = _cases()


def build(name, g, oracle):
    """Feeds case `name` to graph g; returns (min_region_size, force_constraints) for segment()."""
    if name.startswith("ramp") or name.startswith("alternating"):
        W = CASES[name][0]
        f = (ramp_row(W, RAMP_SEEDS.get(W, 1)) if name.startswith("ramp")
             else alternating_row(W, ALTERNATING_SEEDS.get(W, 2)))
        (g.add_frame if oracle else g.add_frame_features)(f)
        return 0, False
    if name == "stacked":
        (g.add_frame if oracle else g.add_frame_features)(stacked_rows())
        return 0, False
    if name == "hub":
        (g.add_frame if oracle else g.add_frame_features)(hub_frame())
        return 4, False
    if name == "temporal":
        f0, f1 = temporal_frames()
        fl = synth.const_flow(*TEMPORAL_WH)
        if oracle:
            g.add_frame(f0)
            g.add_frame(f1)
            g.add_temporal(f1, f0, fl)
        else:
            g.add_frame_features(f0)
            g.add_frame_features(f1)
            g.add_temporal(fl)
        return 6, False
    if name == "constrained":
        labels_v, labels_c, frames = constrained_chunk()
        fl = synth.const_flow(*CONS_WH)
        g.add_virtual_frame(labels_v)
        prev = None
        for t, feat in enumerate(frames):
            if oracle:
                g.add_frame(feat, labels_c if t == 0 else None)
                g.add_temporal(feat if t else None, prev, fl, is_virtual=(t == 0))
            else:
                g.add_frame_features(feat, constraint_ids=labels_c if t == 0 else None)
                g.add_temporal(fl, is_virtual=(t == 0))
            prev = feat
        return 5, True
    raise ValueError(name)


def oracle_graph(name, L=None):
    """A fresh oracle graph of the case, segmented (L: a mutant library, oracle_lib.mutant_lib)."""
    import oracle_lib as ol
    W, H, F = CASES[name]
    og = ol.OracleGraph(W, H, F, L=L)
    min_size, force = build(name, og, True)
    og.segment(min_size, force)
    return og


@functools.lru_cache(maxsize=None)
def oracle_result(name):
    """(node states, merge statistics) of the unmodified oracle on the case: computed once, read-only."""
    og = oracle_graph(name)
    out = (og.node_states(), og.merge_stats())
    og.close()
    for a in out[0] + (out[1],):
        a.setflags(write=False)
    return out
