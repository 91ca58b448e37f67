"""Plain numpy model of vsg_render_level_pool and vsg_render_level_unpool (not collected by pytest; the level pool
tests compare the product against it).

The definition.  P is a plane of W x H, a negative value "no group"; a group g >= 0 is a value of P.  X is the
(C, H, W) feature map; every element is first widened exactly to float64.
  groups   one per group by ascending group: id, component (-1, or those of the component list P is the label
           image of), area = pixels of g.
  sum      [k][c] the sum of X[c] over the pixels of group k, correctly rounded (math.fsum); sum_sq likewise of
           the squares, which are exact in float64.  A NaN among the values makes both NaN; +inf with -inf makes
           the sum NaN and leaves sum_sq +inf.
  min/max  the extreme non-NaN values as float32; +inf / -inf when the group has none.
  unpool   out[c, y, x] = values[k, c] of the group k at (x, y), `fill` where P < 0, converted to the output's
           format with round-to-nearest-even.
bfloat16 maps are uint16 arrays of the upper halves of float32 values."""
import fractions
import math

import numpy as np

GROUP_DTYPE = np.dtype([("id", np.int32), ("component", np.int32), ("area", np.int32), ("reserved", np.int32)])
F32, F16, BF16 = 0, 1, 2
STATS = ("sum", "sum_sq", "min", "max")


def from_bf16(bits):
    """The float32 values of bfloat16 bit patterns (uint16)."""
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def to_bf16(x):
    """float32 to bfloat16 bit patterns, round to nearest even; a NaN stays one."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    rounded = (u + 0x7fff + ((u >> 16) & 1)) >> 16
    nan = (u & 0x7fffffff) > 0x7f800000
    return np.where(nan, (u >> 16) | 0x40, rounded).astype(np.uint16)


def widen(X, dtype):
    """The map as float64, every element exactly."""
    X = np.asarray(X)
    if dtype == BF16:
        assert X.dtype == np.uint16
        return from_bf16(X).astype(np.float64)
    assert X.dtype == (np.float32 if dtype == F32 else np.float16)
    return X.astype(np.float64)


def convert(x, dtype):
    """float32 values in the format `dtype`, round to nearest even (bfloat16 as uint16)."""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore"):   # a value beyond the half range becomes an infinity, as on the device
        return x if dtype == F32 else x.astype(np.float16) if dtype == F16 else to_bf16(x)


def _order(P):
    P = np.asarray(P, np.int32)
    p = P.ravel()
    covered = np.flatnonzero(p >= 0)
    groups = np.unique(p[covered])
    order = covered[np.argsort(p[covered], kind="stable")]
    first = np.searchsorted(p[order], groups)
    return groups, order, first


def groups_of(P, comps=None):
    groups, order, first = _order(P)
    out = np.zeros(len(groups), GROUP_DTYPE)
    if comps is None:
        out["id"], out["component"] = groups, -1
    else:
        out["id"], out["component"] = comps["id"][groups], comps["component"][groups]
    out["area"] = np.diff(np.r_[first, len(order)])
    return out


def _sum(values):
    """The correctly rounded sum; NaN and infinities as IEEE addition has them."""
    if np.isfinite(values).all():
        return math.fsum(values.tolist())
    with np.errstate(invalid="ignore"):
        return float(np.sum(values))


def pool(P, X64, comps=None):
    """(groups, {"sum", "sum_sq", "min", "max"}) of the plane P and the widened (C, H, W) map X64."""
    X64 = np.asarray(X64, np.float64)
    C = X64.shape[0]
    assert X64.shape[1:] == np.asarray(P).shape
    g = groups_of(P, comps)
    groups, order, first = _order(P)
    R = len(groups)
    out = {"sum": np.zeros((R, C)), "sum_sq": np.zeros((R, C)),
           "min": np.full((R, C), np.inf, np.float32), "max": np.full((R, C), -np.inf, np.float32)}
    if not R:
        return g, out
    v = X64.reshape(C, -1)[:, order]                     # (C, covered), grouped
    ends = np.r_[first[1:], len(order)]
    # integer values whose sums of squares stay below 2^53 add exactly in any order
    exact = np.isfinite(v).all() and (v == np.rint(v)).all() and float((v * v).sum(axis=1).max()) < 2.0 ** 53
    if exact:
        out["sum"] = np.add.reduceat(v, first, axis=1).T.copy()
        out["sum_sq"] = np.add.reduceat(v * v, first, axis=1).T.copy()
    for k in range(R):
        seg = v[:, first[k]:ends[k]]
        for c in range(C):
            x = seg[c]
            if not exact:
                out["sum"][k, c] = _sum(x)
                out["sum_sq"][k, c] = _sum(x * x)
            real = x[~np.isnan(x)]
            if len(real):
                out["min"][k, c], out["max"][k, c] = real.min(), real.max()
    return g, out


def pool_literal(P, X64, comps=None):
    """The same from a double loop over the pixels that walks the definition word for word, the sums in exact
    rational arithmetic; for small planes of finite values."""
    P = np.asarray(P, np.int32)
    H, W = P.shape
    C = X64.shape[0]
    acc = {}
    for y in range(H):
        for x in range(W):
            k = int(P[y, x])
            if k < 0:
                continue
            a = acc.setdefault(k, {"area": 0, "sum": [fractions.Fraction(0)] * C, "sum_sq": [fractions.Fraction(0)] * C,
                                   "min": [math.inf] * C, "max": [-math.inf] * C})
            a["area"] += 1
            for c in range(C):
                v = float(X64[c, y, x])
                f = fractions.Fraction(v)
                a["sum"][c] = a["sum"][c] + f
                a["sum_sq"][c] = a["sum_sq"][c] + f * f
                a["min"][c] = min(a["min"][c], v)
                a["max"][c] = max(a["max"][c], v)
    R = len(acc)
    g = np.zeros(R, GROUP_DTYPE)
    out = {"sum": np.zeros((R, C)), "sum_sq": np.zeros((R, C)),
           "min": np.zeros((R, C), np.float32), "max": np.zeros((R, C), np.float32)}
    for k, key in enumerate(sorted(acc)):
        a = acc[key]
        g[k]["id"] = key if comps is None else comps["id"][key]
        g[k]["component"] = -1 if comps is None else comps["component"][key]
        g[k]["area"] = a["area"]
        for c in range(C):
            out["sum"][k, c], out["sum_sq"][k, c] = float(a["sum"][c]), float(a["sum_sq"][c])
            out["min"][k, c], out["max"][k, c] = a["min"][c], a["max"][c]
    return g, out


def unpool(P, values, fill=0.0, dtype=F32):
    """The (C, H, W) map of the values (R, C) float32 in the format `dtype`."""
    P = np.asarray(P, np.int32)
    values = np.asarray(values, np.float32)
    groups = np.unique(P[P >= 0])
    assert values.ndim == 2 and len(groups) == len(values)
    C = values.shape[1]
    out = np.full((C,) + P.shape, fill, np.float32)
    if len(groups):
        out[:, P >= 0] = values[np.searchsorted(groups, P[P >= 0])].T
    return convert(out, dtype)


def moments(groups, sum_, sum_sq):
    area = groups["area"].astype(np.float64)[:, None]
    mean = sum_ / area
    return mean, np.maximum(sum_sq / area - mean * mean, 0.0)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
