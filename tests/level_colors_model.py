"""Plain numpy model of the colour table of a hierarchy level and of its mean-colour picture (not collected by
pytest; the level colour tests compare the product against it byte for byte).

The definition.  P is a plane of W x H, a negative value "no group"; a group g >= 0 is a value of P.  F is
the H x W x 3 uint8 frame, channels in B, G, R order.
  records  one per group by ascending group: area = pixels of g; sum[c], sum_sq[c], min[c], max[c] over the
           bytes F[y, x, c] of those pixels; mean[c] = (2 * sum[c] + area) // (2 * area), sum / area rounded
           half up.  Everything is an integer.
  plane    C[y, x] = mean of the group at (x, y), 0 where P < 0.
  picture  what the renderer makes of C: render_model's own edge rule and blend, not restated here.
`colors` groups the pixels with a sort and np.add.reduceat on int64; there is no run logic in it.
`stats_of` counts what the product's interval list holds."""
import numpy as np

import level_regions_model as lm
import render_model as rm

COLOR_DTYPE = np.dtype([
    ("id", np.int32), ("component", np.int32), ("area", np.int32),
    ("mean", np.uint8, (3,)), ("reserved0", np.uint8),
    ("sum", np.int64, (3,)), ("sum_sq", np.int64, (3,)),
    ("min", np.uint8, (3,)), ("max", np.uint8, (3,)), ("reserved1", np.uint8, (2,)),
])
OFFSETS = {"id": 0, "component": 4, "area": 8, "mean": 12, "reserved0": 15, "sum": 16, "sum_sq": 40, "min": 64,
           "max": 67, "reserved1": 70}


def _check(P, F):
    P, F = np.asarray(P, np.int32), np.asarray(F)
    assert P.ndim == 2 and F.shape == P.shape + (3,) and F.dtype == np.uint8
    return P, F


def colors(P, F, comps=None):
    """The records of the planes P and F.  id = group and component = -1, or, with the component list of
    level_components_model that P is the label image of, that component's id and component."""
    P, F = _check(P, F)
    p = P.ravel()
    covered = np.flatnonzero(p >= 0)
    groups = np.unique(p[covered])
    out = np.zeros(len(groups), COLOR_DTYPE)
    if comps is None:
        out["id"], out["component"] = groups, -1
    else:
        out["id"], out["component"] = comps["id"][groups], comps["component"][groups]
    if not len(groups):
        return out
    order = covered[np.argsort(p[covered], kind="stable")]
    first = np.searchsorted(p[order], groups)
    v = F.reshape(-1, 3)[order].astype(np.int64)
    area = np.diff(np.r_[first, len(order)]).astype(np.int64)
    out["area"] = area
    out["sum"] = np.add.reduceat(v, first, axis=0)
    out["sum_sq"] = np.add.reduceat(v * v, first, axis=0)
    out["min"] = np.minimum.reduceat(v, first, axis=0)
    out["max"] = np.maximum.reduceat(v, first, axis=0)
    out["mean"] = (2 * out["sum"] + area[:, None]) // (2 * area[:, None])
    return out


def colors_literal(P, F, comps=None):
    """The same table from a double loop over the pixels that walks the definition word for word, in Python
    integers; for small planes."""
    P, F = _check(P, F)
    H, W = P.shape
    acc = {}
    for y in range(H):
        for x in range(W):
            g = int(P[y, x])
            if g < 0:
                continue
            a = acc.setdefault(g, {"area": 0, "sum": [0] * 3, "sum_sq": [0] * 3, "min": [255] * 3, "max": [0] * 3})
            a["area"] += 1
            for c in range(3):
                b = int(F[y, x, c])
                a["sum"][c] += b
                a["sum_sq"][c] += b * b
                a["min"][c] = min(a["min"][c], b)
                a["max"][c] = max(a["max"][c], b)
    out = np.zeros(len(acc), COLOR_DTYPE)
    for k, g in enumerate(sorted(acc)):
        a = acc[g]
        out[k]["id"] = g if comps is None else comps["id"][g]
        out[k]["component"] = -1 if comps is None else comps["component"][g]
        out[k]["area"] = a["area"]
        for c in range(3):
            # sum / area rounded half up: floor(sum / area + 1 / 2)
            out[k]["mean"][c] = (2 * a["sum"][c] + a["area"]) // (2 * a["area"])
            out[k]["sum"][c], out[k]["sum_sq"][c] = a["sum"][c], a["sum_sq"][c]
            out[k]["min"][c], out[k]["max"][c] = a["min"][c], a["max"][c]
    return out


def mean_plane(P, records):
    """C: H x W x 3 uint8, the mean of every pixel's group, 0 where P < 0.  records: those of colors(P, .)."""
    P = np.asarray(P, np.int32)
    groups = np.unique(P[P >= 0])
    assert len(groups) == len(records)
    plane = np.zeros(P.shape + (3,), np.uint8)
    if len(groups):
        plane[P >= 0] = records["mean"][np.searchsorted(groups, P[P >= 0])]
    return plane


def picture(P, F, records, highlight_edges=True, blend_alpha=0.5, concat_with_source=False, has_video=True):
    """The mean-colour picture: render_model.RenderModel.render's steps after its fill, on C."""
    P, F = _check(P, F)
    plane = mean_plane(P, records)
    if highlight_edges:
        plane = rm.highlight_edges(plane)
    if concat_with_source:
        return np.concatenate([plane, F], axis=0)
    if has_video:
        return rm.add_weighted(F, plane, blend_alpha)
    return plane


def stats_of(P):
    """The stats' groups, intervals, covered and largest_group_intervals: the intervals are the maximal runs of
    P per row, -1 belonging to none."""
    P = np.asarray(P, np.int32)
    _, _, _, rid = lm.runs_of(P)
    counts = np.unique(rid, return_counts=True)[1]
    return {"groups": len(counts), "intervals": len(rid), "covered": int((P >= 0).sum()),
            "largest_group_intervals": int(counts.max()) if len(counts) else 0}


def moments(records):
    """(mean, variance) per record and channel as float64, what render.color_moments returns."""
    area = records["area"].astype(np.float64)[:, None]
    mean = records["sum"].astype(np.float64) / area
    return mean, np.maximum(records["sum_sq"].astype(np.float64) / area - mean * mean, 0.0)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
