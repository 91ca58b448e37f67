"""Plain numpy model of the volume session's table: a hierarchy level's region ids (supervoxels) accumulated over
the frames of a sequence (not collected by pytest; the volume tests compare the product against it byte for byte).

The definition.  A sequence is a list of adds (frame, P, F, B): `frame` >= 0 the caller's frame index, P the
H x W id plane of the level (negative: no region), F the H x W x 3 uint8 BGR frame (None without colours), B the
H x W int32 label plane (negative: no label; None without labels).  A voxel is a pixel of an add; an index that is
added twice gives every pixel twice.
  rows   one per id by ascending id: first_frame / last_frame / frames = the smallest and the largest `frame`
         and the number of adds in which it has a pixel; the box over all its voxels; volume = its voxels,
         unlabelled = those with B < 0; sum_x, sum_y, sum_t over its voxels with t = frame; sum[c], sum_sq[c],
         min[c], max[c] over the bytes F[y, x, c] of its voxels
  cols   one per label by ascending label: volume = voxels of the label, uncovered = those with P < 0, and the
         same first_frame / last_frame / frames
  pairs  one per (id, label) with count = voxels with both > 0, by (row, label); frames = the adds in which the
         two share a pixel
best_label of a row is the label of its largest count, the smallest such label; best_row of a column the row of
its largest count, the smallest such row.  first_pair of a row is the number of pairs of the rows before it.
Without labels there are no cols and no pairs, unlabelled = best_count = 0 and best_label = -1; without colours
the colour fields are 0.  `volume` takes everything from sorts over the voxels of all adds at once; it knows
nothing of frames' tables, of runs or of merging."""
import numpy as np

ROW_DTYPE = np.dtype([
    ("id", np.int32), ("first_frame", np.int32), ("last_frame", np.int32), ("frames", np.int32),
    ("min_x", np.int32), ("min_y", np.int32), ("max_x", np.int32), ("max_y", np.int32),
    ("first_pair", np.int32), ("num_pairs", np.int32), ("best_label", np.int32), ("reserved0", np.int32),
    ("volume", np.int64), ("unlabelled", np.int64), ("best_count", np.int64),
    ("sum_x", np.int64), ("sum_y", np.int64), ("sum_t", np.int64),
    ("sum", np.int64, (3,)), ("sum_sq", np.int64, (3,)),
    ("min", np.uint8, (3,)), ("max", np.uint8, (3,)), ("reserved1", np.uint8, (2,)),
])
COL_DTYPE = np.dtype([
    ("label", np.int32), ("num_pairs", np.int32), ("best_row", np.int32),
    ("first_frame", np.int32), ("last_frame", np.int32), ("frames", np.int32),
    ("volume", np.int64), ("uncovered", np.int64), ("best_count", np.int64),
])
PAIR_DTYPE = np.dtype([("row", np.int32), ("col", np.int32), ("label", np.int32), ("frames", np.int32),
                       ("count", np.int64)])
ROW_OFFSETS = {"id": 0, "first_frame": 4, "last_frame": 8, "frames": 12, "min_x": 16, "min_y": 20, "max_x": 24,
               "max_y": 28, "first_pair": 32, "num_pairs": 36, "best_label": 40, "reserved0": 44, "volume": 48,
               "unlabelled": 56, "best_count": 64, "sum_x": 72, "sum_y": 80, "sum_t": 88, "sum": 96, "sum_sq": 120,
               "min": 144, "max": 147, "reserved1": 150}
COL_OFFSETS = {"label": 0, "num_pairs": 4, "best_row": 8, "first_frame": 12, "last_frame": 16, "frames": 20,
               "volume": 24, "uncovered": 32, "best_count": 40}
PAIR_OFFSETS = {"row": 0, "col": 4, "label": 8, "frames": 12, "count": 16}


def _voxels(adds, colors, labels):
    """Everything per voxel of the sequence, as flat int64 arrays: id, label, frame, add, x, y, and the bytes."""
    cols = {k: [] for k in ("p", "b", "t", "k", "x", "y", "f")}
    for k, (frame, P, F, B) in enumerate(adds):
        P = np.asarray(P, np.int32)
        H, W = P.shape
        yy, xx = np.mgrid[0:H, 0:W]
        n = W * H
        cols["p"].append(np.maximum(P, -1).astype(np.int64).ravel())
        cols["b"].append(np.maximum(np.asarray(B, np.int32), -1).astype(np.int64).ravel() if labels
                         else np.full(n, -1, np.int64))
        cols["t"].append(np.full(n, int(frame), np.int64))
        cols["k"].append(np.full(n, k, np.int64))
        cols["x"].append(xx.astype(np.int64).ravel())
        cols["y"].append(yy.astype(np.int64).ravel())
        if colors:
            F = np.asarray(F)
            assert F.shape == (H, W, 3) and F.dtype == np.uint8
        cols["f"].append(F.reshape(-1, 3).astype(np.int64) if colors else np.zeros((n, 3), np.int64))
    if not adds:
        return {k: np.zeros((0, 3) if k == "f" else 0, np.int64) for k in cols}
    return {k: np.concatenate(v) for k, v in cols.items()}


def _sum_by(index, n, values):
    out = np.zeros((n,) + values.shape[1:], np.int64)
    np.add.at(out, index, values)                      # int64 throughout: no float in between
    return out


def _span(index, n, t, k):
    """first_frame, last_frame and the number of distinct adds of every group."""
    first, last = np.full(n, np.iinfo(np.int64).max), np.full(n, -1, np.int64)
    np.minimum.at(first, index, t)
    np.maximum.at(last, index, t)
    adds = np.unique(np.stack([index, k], axis=1), axis=0)[:, 0] if len(index) else index
    return first, last, np.bincount(adds, minlength=n)


def volume(adds, colors=True, labels=True):
    """(rows, cols, pairs) of the sequence of adds (frame, P, F, B)."""
    v = _voxels(adds, colors, labels)
    p, b = v["p"], v["b"]
    ids, labs = np.unique(p[p >= 0]), np.unique(b[b >= 0])
    rows, cols = np.zeros(len(ids), ROW_DTYPE), np.zeros(len(labs), COL_DTYPE)
    rows["id"], cols["label"] = ids, labs
    rows["best_label"], cols["best_row"] = -1, -1
    cov = p >= 0
    gi = np.searchsorted(ids, p[cov])
    n = len(ids)
    rows["volume"] = np.bincount(gi, minlength=n)
    rows["unlabelled"] = np.bincount(np.searchsorted(ids, p[cov & (b < 0)]), minlength=n) if labels else 0
    rows["first_frame"], rows["last_frame"], rows["frames"] = _span(gi, n, v["t"][cov], v["k"][cov])
    for name, key in (("sum_x", "x"), ("sum_y", "y"), ("sum_t", "t")):
        rows[name] = _sum_by(gi, n, v[key][cov])
    for name, key, fn, start in (("min_x", "x", np.minimum, 2 ** 31 - 1), ("min_y", "y", np.minimum, 2 ** 31 - 1),
                                 ("max_x", "x", np.maximum, -1), ("max_y", "y", np.maximum, -1)):
        acc = np.full(n, start, np.int64)
        fn.at(acc, gi, v[key][cov])
        rows[name] = acc
    if colors:
        f = v["f"][cov]
        rows["sum"], rows["sum_sq"] = _sum_by(gi, n, f), _sum_by(gi, n, f * f)
        lo, hi = np.full((n, 3), 255, np.int64), np.zeros((n, 3), np.int64)
        np.minimum.at(lo, gi, f)
        np.maximum.at(hi, gi, f)
        rows["min"], rows["max"] = lo, hi
    lab = b >= 0
    li = np.searchsorted(labs, b[lab])
    m = len(labs)
    cols["volume"] = np.bincount(li, minlength=m)
    cols["uncovered"] = np.bincount(np.searchsorted(labs, b[lab & (p < 0)]), minlength=m)
    cols["first_frame"], cols["last_frame"], cols["frames"] = _span(li, m, v["t"][lab], v["k"][lab])
    both = cov & lab
    # row and col index of every voxel with both, as one int64 that sorts by (row, col), that is by (id, label)
    cell = np.searchsorted(ids, p[both]) * max(m, 1) + np.searchsorted(labs, b[both])
    cells, counts = np.unique(cell, return_counts=True)
    pairs = np.zeros(len(cells), PAIR_DTYPE)
    pairs["row"], pairs["col"] = cells // max(m, 1), cells % max(m, 1)
    pairs["label"], pairs["count"] = labs[pairs["col"]] if len(cells) else 0, counts
    shared = np.unique(np.stack([cell, v["k"][both]], axis=1), axis=0)[:, 0] if len(cell) else cell
    pairs["frames"] = np.unique(shared, return_counts=True)[1] if len(cell) else 0
    rows["num_pairs"] = np.bincount(pairs["row"], minlength=n)
    rows["first_pair"] = np.cumsum(rows["num_pairs"]) - rows["num_pairs"]
    cols["num_pairs"] = np.bincount(pairs["col"], minlength=m)
    if not labels:
        rows["first_pair"] = 0
    # the first pair of every row in (row, largest count, smallest label) order, and the same for the columns
    order = np.lexsort((pairs["label"], -pairs["count"], pairs["row"]))
    first = order[np.r_[True, np.diff(pairs["row"][order]) != 0]] if len(order) else order
    rows["best_label"][pairs["row"][first]] = pairs["label"][first]
    rows["best_count"][pairs["row"][first]] = pairs["count"][first]
    order = np.lexsort((pairs["row"], -pairs["count"], pairs["col"]))
    first = order[np.r_[True, np.diff(pairs["col"][order]) != 0]] if len(order) else order
    cols["best_row"][pairs["col"][first]] = pairs["row"][first]
    cols["best_count"][pairs["col"][first]] = pairs["count"][first]
    return rows, cols, pairs


def volume_literal(adds, colors=True, labels=True):
    """The same table from a loop over the voxels that walks the definition word for word, in Python integers; for
    small sequences."""
    R, Cl, Pr = {}, {}, {}
    for k, (frame, P, F, B) in enumerate(adds):
        P = np.asarray(P, np.int32)
        H, W = P.shape
        for y in range(H):
            for x in range(W):
                g = int(P[y, x])
                l = int(B[y, x]) if labels else -1
                if g >= 0:
                    r = R.setdefault(g, {"t": [], "k": set(), "x": [], "y": [], "un": 0, "f": []})
                    r["t"].append(int(frame))
                    r["k"].add(k)
                    r["x"].append(x)
                    r["y"].append(y)
                    r["un"] += 1 if (labels and l < 0) else 0
                    if colors:
                        r["f"].append([int(F[y, x, c]) for c in range(3)])
                if l >= 0:
                    c = Cl.setdefault(l, {"t": [], "k": set(), "n": 0, "un": 0})
                    c["t"].append(int(frame))
                    c["k"].add(k)
                    c["n"] += 1
                    c["un"] += 1 if g < 0 else 0
                if g >= 0 and l >= 0:
                    q = Pr.setdefault((g, l), {"k": set(), "n": 0})
                    q["k"].add(k)
                    q["n"] += 1
    ids, labs = sorted(R), sorted(Cl)
    rows, cols, pairs = np.zeros(len(ids), ROW_DTYPE), np.zeros(len(labs), COL_DTYPE), np.zeros(len(Pr), PAIR_DTYPE)
    for e, (g, l) in enumerate(sorted(Pr)):
        pairs[e] = (ids.index(g), labs.index(l), l, len(Pr[g, l]["k"]), Pr[g, l]["n"])
    before = 0
    for i, g in enumerate(ids):
        r, out = R[g], rows[i]
        mine = [e for e in range(len(pairs)) if pairs[e]["row"] == i]
        best = max(mine, key=lambda e: (int(pairs[e]["count"]), -int(pairs[e]["label"]))) if mine else None
        out["id"], out["first_frame"], out["last_frame"], out["frames"] = g, min(r["t"]), max(r["t"]), len(r["k"])
        out["min_x"], out["min_y"], out["max_x"], out["max_y"] = min(r["x"]), min(r["y"]), max(r["x"]), max(r["y"])
        out["first_pair"], out["num_pairs"] = (before if labels else 0), len(mine)
        out["best_label"] = pairs[best]["label"] if mine else -1
        out["best_count"] = pairs[best]["count"] if mine else 0
        out["volume"], out["unlabelled"] = len(r["t"]), r["un"]
        out["sum_x"], out["sum_y"], out["sum_t"] = sum(r["x"]), sum(r["y"]), sum(r["t"])
        for c in range(3 if colors else 0):
            vals = [f[c] for f in r["f"]]
            out["sum"][c], out["sum_sq"][c] = sum(vals), sum(b * b for b in vals)
            out["min"][c], out["max"][c] = min(vals), max(vals)
        before += len(mine)
    for j, l in enumerate(labs):
        c = Cl[l]
        mine = [e for e in range(len(pairs)) if pairs[e]["col"] == j]
        best = max(mine, key=lambda e: (int(pairs[e]["count"]), -int(pairs[e]["row"]))) if mine else None
        cols[j] = (l, len(mine), pairs[best]["row"] if mine else -1, min(c["t"]), max(c["t"]), len(c["k"]), c["n"],
                   c["un"], pairs[best]["count"] if mine else 0)
    return rows, cols, pairs


def stats_of(adds, colors=True, labels=True):
    """What vsg_render_last_volume_stats reports after the last add of the sequence: the session's totals, and
    the keys that add brought."""
    rows, cols, pairs = volume(adds, colors, labels)
    rows0, cols0, pairs0 = volume(adds[:-1], colors, labels)
    covered = sum(int((np.asarray(P) >= 0).sum()) for _, P, _, _ in adds)
    labelled = sum(int((np.asarray(B) >= 0).sum()) for _, _, _, B in adds) if labels else 0
    return {"frames": len(adds), "rows": len(rows), "cols": len(cols), "pairs": len(pairs),
            "new_rows": len(rows) - len(rows0), "new_cols": len(cols) - len(cols0),
            "new_pairs": len(pairs) - len(pairs0), "covered": covered, "labelled": labelled,
            "both": int(pairs["count"].sum())}


def scores_direct(adds):
    """What render.volume_scores derives from the table, straight from the voxels: (n, ue_sum, mean_duration)."""
    v = _voxels(adds, False, True)
    p, b, k = v["p"], v["b"], v["k"]
    n = ue_sum = 0
    durations = []
    for g in np.unique(p[p >= 0]):
        inside = b[(p == g) & (b >= 0)]
        n += len(inside)
        ue_sum += sum(min(int((inside == l).sum()), len(inside) - int((inside == l).sum())) for l in np.unique(inside))
        durations.append(len(np.unique(k[p == g])))
    return n, ue_sum, (float(np.mean(durations)) if durations else None)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_tables(got, want):
    return all(same_bits(g, w) for g, w in zip(got, want))
