"""Plain numpy model of the boundary distance calls (not collected by pytest; the boundary distance tests
compare the product against it byte for byte).

The definition, from include/vsg_render.h.  The edge set of a plane P is E = {(x, y): P(x, y) != P(x + 1, y) with
x + 1 < W, or P(x, y) != P(x, y + 1) with y + 1 < H}, -1 counting as a value (persistence_model.edge_mask).
D(x, y) = min over (u, v) in E of (x - u)^2 + (y - v)^2 as an int32, NONE = 0x7fffffff everywhere when E is empty.
The benchmark takes a label plane B, B' = max(B, -1), G = E(B'), and gives per level l of the persistence plane Q
(L levels) seg_edges = #{Q > l}, seg_matched = #{Q > l and D_G <= T}, gt_edges = |G| and
gt_matched = #{p in G: D_l(p) <= T} with D_l the distance to {Q > l}.

`distance` is the exact separable minimum in int64: the vertical distance to the nearest edge pixel of every
column, then per row the minimum over all columns.  `benchmark` goes level by level through per-level
distances; it deliberately does not use the device's disc-maximum route."""
import numpy as np

from persistence_model import edge_mask  # noqa: F401 (part of the model)

NONE = 0x7fffffff
MAX_TOLERANCE_SQ = 4096
_FAR = np.int64(1) << 40

SCORE_DTYPE = np.dtype([("seg_edges", np.int64), ("seg_matched", np.int64), ("gt_edges", np.int64),
                        ("gt_matched", np.int64)])


def column_distance(mask):
    """g: H x W int64, the vertical distance to the nearest set pixel of the column, _FAR without one."""
    mask = np.asarray(mask, bool)
    H, W = mask.shape
    rows = np.arange(H, dtype=np.int64)[:, None]
    last = np.maximum.accumulate(np.where(mask, rows, -_FAR), axis=0)            # last set row at or above
    first = np.minimum.accumulate(np.where(mask, rows, _FAR)[::-1], axis=0)[::-1]  # first set row at or below
    return np.minimum(np.where(last < 0, _FAR, rows - last), np.where(first >= _FAR, _FAR, first - rows))


def distance(mask):
    """D: H x W int32 of the boolean edge set `mask`."""
    mask = np.asarray(mask, bool)
    H, W = mask.shape
    if not mask.any():
        return np.full((H, W), NONE, np.int32)
    g = column_distance(mask)
    gsq = np.where(g >= _FAR, _FAR, g * g)
    cols = np.arange(W, dtype=np.int64)
    out = np.empty((H, W), np.int64)
    for x in range(W):
        out[:, x] = (gsq + ((cols - x) ** 2)[None, :]).min(axis=1)
    assert out.max() < NONE
    return out.astype(np.int32)


def brute_distance(mask):
    """The same by the all-pairs minimum; for small frames."""
    mask = np.asarray(mask, bool)
    H, W = mask.shape
    ys, xs = np.nonzero(mask)
    if len(ys) == 0:
        return np.full((H, W), NONE, np.int32)
    yy, xx = np.mgrid[0:H, 0:W]
    d = (yy[:, :, None] - ys[None, None, :]).astype(np.int64) ** 2 + (xx[:, :, None] - xs[None, None, :]) ** 2
    return d.min(axis=2).astype(np.int32)


def other_edges(other):
    """G of a label plane."""
    return edge_mask(np.maximum(np.asarray(other, np.int64), -1))


def level_distances(q, L):
    """[D of {Q > l} for l in [0, L)]."""
    q = np.asarray(q)
    return [distance(q > l) for l in range(L)]


def benchmark(q, L, other, T, d_other=None, d_levels=None):
    """The L records, level by level.  d_other = distance(other_edges(other)) and d_levels = level_distances(q, L)
    may be handed in by a caller that asks for several T."""
    q = np.asarray(q)
    g = other_edges(other)
    near_g = (distance(g) if d_other is None else d_other) <= T
    out = np.zeros(L, SCORE_DTYPE)
    for l in range(L):
        e = q > l
        d_l = distance(e) if d_levels is None else d_levels[l]
        out[l] = (int(e.sum()), int((e & near_g).sum()), int(g.sum()), int((g & (d_l <= T)).sum()))
    return out


def disc_maximum(q, T):
    """M(p) = max of Q over the pixels q with |p - q|^2 <= T (the frame's outside counts as 0)."""
    q = np.asarray(q, np.int64)
    H, W = q.shape
    r = int(np.floor(np.sqrt(T)))
    while (r + 1) * (r + 1) <= T:
        r += 1
    while r * r > T:
        r -= 1
    pad = np.zeros((H + 2 * r, W + 2 * r), np.int64)
    pad[r:r + H, r:r + W] = q
    out = np.zeros((H, W), np.int64)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if dx * dx + dy * dy <= T:
                out = np.maximum(out, pad[r + dy:r + dy + H, r + dx:r + dx + W])
    return out


def suffix_counts(values, L):
    """out[l] = the number of entries of `values` that are > l, l in [0, L)."""
    hist = np.bincount(np.asarray(values, np.int64).ravel(), minlength=L + 1)[:L + 1]
    return hist[::-1].cumsum()[::-1][1:]


def scores(records):
    """precision, recall, F per level as float64 with 0 / 0 = 0, and the lowest level of the best F."""
    def quotient(a, b):
        return np.array([x / y if y else 0.0 for x, y in zip(a.tolist(), b.tolist())], np.float64)
    p = quotient(records["seg_matched"], records["seg_edges"])
    r = quotient(records["gt_matched"], records["gt_edges"])
    f = quotient(2 * p * r, p + r)
    return p, r, f, (int(np.argmax(f)) if len(f) else None)
