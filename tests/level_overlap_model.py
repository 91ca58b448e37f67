"""Plain numpy model of the overlap (contingency) table of a hierarchy level and a plane of labels (not
collected by pytest; the level overlap tests compare the product against it byte for byte).

The definition.  P and B are planes of W x H.  A negative value of P is "no group", a negative value of B
"no label".  A group g >= 0 is a value of P, a label l >= 0 a value of B.
  rows   one per group by ascending group: area = pixels of g, unlabelled = those of them with B < 0
  cols   one per label by ascending label: area = pixels of l, uncovered = those of them with P < 0
  pairs  one per (g, l) with count = pixels with P = g and B = l > 0, by (row, label)
best_label of a row is the label of its largest count, the smallest such label; best_row of a column the
row of its largest count, the smallest such row.  `overlap` takes all of it from np.unique on the pixel
pairs; there is no run logic in it.  `runs_of` counts what the product's sort sees."""
import numpy as np

ROW_DTYPE = np.dtype([("id", np.int32), ("component", np.int32), ("first_pair", np.int32), ("num_pairs", np.int32),
                      ("area", np.int32), ("unlabelled", np.int32), ("best_label", np.int32),
                      ("best_count", np.int32)])
COL_DTYPE = np.dtype([("label", np.int32), ("area", np.int32), ("uncovered", np.int32), ("num_pairs", np.int32),
                      ("best_row", np.int32), ("best_count", np.int32)])
PAIR_DTYPE = np.dtype([("row", np.int32), ("col", np.int32), ("label", np.int32), ("count", np.int32)])


def _planes(P, B):
    P, B = np.asarray(P, np.int32), np.asarray(B, np.int32)
    assert P.shape == B.shape and P.ndim == 2
    return np.maximum(P, -1).astype(np.int64).ravel(), np.maximum(B, -1).astype(np.int64).ravel()


def overlap(P, B, comps=None):
    """(rows, cols, pairs) of the planes P and B.  id = group and component = -1, or, with the component
    list of level_components_model that P is the label image of, that component's id and component."""
    p, b = _planes(P, B)
    groups, labels = np.unique(p[p >= 0]), np.unique(b[b >= 0])
    rows, cols = np.zeros(len(groups), ROW_DTYPE), np.zeros(len(labels), COL_DTYPE)
    if comps is None:
        rows["id"], rows["component"] = groups, -1
    else:
        rows["id"], rows["component"] = comps["id"][groups], comps["component"][groups]
    cols["label"] = labels
    rows["area"] = np.bincount(np.searchsorted(groups, p[p >= 0]), minlength=len(groups))
    rows["unlabelled"] = np.bincount(np.searchsorted(groups, p[(p >= 0) & (b < 0)]), minlength=len(groups))
    cols["area"] = np.bincount(np.searchsorted(labels, b[b >= 0]), minlength=len(labels))
    cols["uncovered"] = np.bincount(np.searchsorted(labels, b[(b >= 0) & (p < 0)]), minlength=len(labels))
    both = (p >= 0) & (b >= 0)
    # group and label are below 2^31: the pair as one int64 sorts by (group, label)
    cell, counts = np.unique(p[both] << 32 | b[both], return_counts=True)
    cells = np.stack([cell >> 32, cell & 0xFFFFFFFF], axis=1).reshape(-1, 2)
    pairs = np.zeros(len(cells), PAIR_DTYPE)                 # np.unique sorts by (group, label)
    pairs["row"] = np.searchsorted(groups, cells[:, 0])
    pairs["col"] = np.searchsorted(labels, cells[:, 1])
    pairs["label"], pairs["count"] = cells[:, 1], counts
    rows["num_pairs"] = np.bincount(pairs["row"], minlength=len(groups))
    rows["first_pair"] = np.cumsum(rows["num_pairs"]) - rows["num_pairs"]
    cols["num_pairs"] = np.bincount(pairs["col"], minlength=len(labels))
    rows["best_label"], cols["best_row"] = -1, -1
    # the first pair of every row in (row, largest count, smallest label) order, and the same for the columns
    order = np.lexsort((pairs["label"], -pairs["count"].astype(np.int64), pairs["row"]))
    first = order[np.r_[True, np.diff(pairs["row"][order]) != 0]] if len(order) else order
    rows["best_label"][pairs["row"][first]] = pairs["label"][first]
    rows["best_count"][pairs["row"][first]] = pairs["count"][first]
    order = np.lexsort((pairs["row"], -pairs["count"].astype(np.int64), pairs["col"]))
    first = order[np.r_[True, np.diff(pairs["col"][order]) != 0]] if len(order) else order
    cols["best_row"][pairs["col"][first]] = pairs["row"][first]
    cols["best_count"][pairs["col"][first]] = pairs["count"][first]
    return rows, cols, pairs


def overlap_literal(P, B, comps=None):
    """The same table from a double loop over the pixels that walks the definition word for word; for
    small planes."""
    P, B = np.asarray(P, np.int32), np.asarray(B, np.int32)
    H, W = P.shape
    area, unlabelled, label_area, uncovered, cells = {}, {}, {}, {}, {}
    for y in range(H):
        for x in range(W):
            g, l = int(P[y, x]), int(B[y, x])
            if g >= 0:
                area[g] = area.get(g, 0) + 1
                if l < 0:
                    unlabelled[g] = unlabelled.get(g, 0) + 1
            if l >= 0:
                label_area[l] = label_area.get(l, 0) + 1
                if g < 0:
                    uncovered[l] = uncovered.get(l, 0) + 1
            if g >= 0 and l >= 0:
                cells[g, l] = cells.get((g, l), 0) + 1
    groups, labels = sorted(area), sorted(label_area)
    rows, cols = np.zeros(len(groups), ROW_DTYPE), np.zeros(len(labels), COL_DTYPE)
    pairs = np.zeros(len(cells), PAIR_DTYPE)
    for e, (g, l) in enumerate(sorted(cells)):
        pairs[e] = (groups.index(g), labels.index(l), l, cells[g, l])
    for k, g in enumerate(groups):
        mine = [e for e in range(len(pairs)) if pairs[e]["row"] == k]
        best = max(mine, key=lambda e: (pairs[e]["count"], -pairs[e]["label"])) if mine else None
        rows[k] = (g if comps is None else comps["id"][g], -1 if comps is None else comps["component"][g],
                   mine[0] if mine else (rows[k - 1]["first_pair"] + rows[k - 1]["num_pairs"] if k else 0), len(mine),
                   area[g], unlabelled.get(g, 0), pairs[best]["label"] if mine else -1,
                   pairs[best]["count"] if mine else 0)
    for c, l in enumerate(labels):
        mine = [e for e in range(len(pairs)) if pairs[e]["col"] == c]
        best = max(mine, key=lambda e: (pairs[e]["count"], -pairs[e]["row"])) if mine else None
        cols[c] = (l, label_area[l], uncovered.get(l, 0), len(mine), pairs[best]["row"] if mine else -1,
                   pairs[best]["count"] if mine else 0)
    return rows, cols, pairs


def runs_of(P, B):
    """The stats' `runs`: the maximal runs, per frame row, of constant (P, B) with at least one of the two
    non-negative.  A run ends with its row."""
    P, B = np.asarray(P, np.int32), np.asarray(B, np.int32)
    p, b = np.maximum(P, -1), np.maximum(B, -1)
    head = np.ones(P.shape, bool)
    head[:, 1:] = (p[:, 1:] != p[:, :-1]) | (b[:, 1:] != b[:, :-1])
    return int((head & ((p >= 0) | (b >= 0))).sum())


def totals(P, B):
    """The stats' covered, labelled and both."""
    p, b = _planes(P, B)
    return int((p >= 0).sum()), int((b >= 0).sum()), int(((p >= 0) & (b >= 0)).sum())


def scores_direct(P, B):
    """What overlap_scores computes, straight from the planes: (n, asa_sum, ue_sum).  n: the pixels with a
    group and a label.  asa_sum: every group counts the pixels of the label it shares most pixels with.
    ue_sum: every (group, label) that meet counts the smaller of the group's labelled pixels inside and
    outside the label."""
    P, B = np.asarray(P, np.int32), np.asarray(B, np.int32)
    n = asa_sum = ue_sum = 0
    for g in np.unique(P[P >= 0]):
        inside = B[(P == g) & (B >= 0)]
        n += len(inside)
        counts = [int((inside == l).sum()) for l in np.unique(inside)]
        asa_sum += max(counts) if counts else 0
        ue_sum += sum(min(c, len(inside) - c) for c in counts)
    return n, asa_sum, ue_sum


def pairs_of(rows, pairs, k):
    return pairs[rows[k]["first_pair"]:rows[k]["first_pair"] + rows[k]["num_pairs"]]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
