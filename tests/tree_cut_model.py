"""Plain numpy model of the tree cut (not collected by pytest; the tree cut tests compare the product against
it byte for byte).

The definition.  The hierarchy has L = max(1, levels) levels and the ancestors A_l(r) of persistence_model.
A node is a pair (l, id) with id = A_l(r) for a region r of the level-0 id image P0; its pixels are those whose
level-0 region r has A_l(r) = id, its leaves those regions, its children the distinct (l - 1, A_{l-1}(r)) of
its leaves.  Every node has a gain g(n), an integer:
  labels      g(n) = best(n) - penalty, best(n) the largest number of pixels n shares with one label >= 0 of
              the plane B (ties: the smallest label; no labelled pixel: label -1, count 0)
  gain table  (level, id, gain) entries, strictly ascending by (level, id), |gain| <= 2^32: the gain of the
              node an entry names, 0 for a node no entry names; entries that name no node are ignored
Bottom-up, opt(n) = g(n) at level 0; above, S(n) is the sum of opt over the children, keep(n) <=> g(n) >= S(n)
(a tie keeps the coarser node) and opt(n) = max(g(n), S(n)).  Leaves always keep.  A region's selected node is
the first kept one met when descending from the top.  The records are the selected nodes by ascending (level,
id), the plane holds for every pixel the index of its record (-1 where P0 is -1), total is the sum of the
selected gains.  `Tree` walks this definition word for word; `enumerate_cuts` lists every partition into nodes."""
import itertools

import numpy as np

import persistence_model as pm

NODE_DTYPE = np.dtype([
    ("level", np.int32), ("id", np.int32), ("area", np.int32), ("leaves", np.int32), ("children", np.int32),
    ("best_label", np.int32), ("best_count", np.int32), ("reserved", np.int32),
    ("gain", np.int64), ("split_value", np.int64)])
GAIN_DTYPE = np.dtype([("level", np.int32), ("id", np.int32), ("gain", np.int64)])
MAX_GAIN = 1 << 32
MAX_ENTRIES = 1 << 27


class Tree:
    """The nodes of all levels of one frame.  nodes: the (level, id) keys, ascending.  Of every node: leaves (the
    columns of the ancestor table), children (keys), parent (key or None), area."""

    def __init__(self, ids0, hierarchy):
        self.ids0 = np.maximum(np.asarray(ids0, np.int64), -1)
        self.ids, self.table = pm.ancestors(self.ids0, hierarchy)
        self.L = self.table.shape[0]
        covered = self.ids0[self.ids0 >= 0]
        self.leaf_area = np.bincount(np.searchsorted(self.ids, covered), minlength=len(self.ids)).astype(np.int64)
        self.leaves, self.children, self.parent = {}, {}, {}
        for l in range(self.L):
            for k in range(len(self.ids)):
                key = (l, int(self.table[l, k]))
                self.leaves.setdefault(key, []).append(k)
        for key in self.leaves:
            l = key[0]
            self.children[key] = sorted({(l - 1, int(self.table[l - 1, k])) for k in self.leaves[key]}) if l else []
            for c in self.children[key]:
                self.parent[c] = key
        self.nodes = sorted(self.leaves)
        self.area = {key: int(self.leaf_area[self.leaves[key]].sum()) for key in self.nodes}

    def top(self):
        return [key for key in self.nodes if key[0] == self.L - 1]

    def best_labels(self, B):
        """{node: (best_label, best_count)} against the label plane B."""
        b = np.maximum(np.asarray(B, np.int64), -1)
        assert b.shape == self.ids0.shape
        both = (self.ids0 >= 0) & (b >= 0)
        per_leaf = [dict() for _ in self.ids]
        if both.any():
            cells, counts = np.unique(np.stack([np.searchsorted(self.ids, self.ids0[both]), b[both]], axis=1),
                                      axis=0, return_counts=True)
            for (k, label), c in zip(cells.tolist(), counts.tolist()):
                per_leaf[k][label] = c
        out = {}
        for key in self.nodes:
            shared = {}
            for k in self.leaves[key]:
                for label, c in per_leaf[k].items():
                    shared[label] = shared.get(label, 0) + c
            if shared:
                count = max(shared.values())
                out[key] = (min(label for label, c in shared.items() if c == count), count)
            else:
                out[key] = (-1, 0)
        return out


def check_gains(gains):
    """Raises ValueError for a table the call refuses."""
    gains = np.asarray(gains, GAIN_DTYPE)
    keys = [(int(g["level"]), int(g["id"])) for g in gains]
    for a, b in zip(keys, keys[1:]):
        if not a < b:
            raise ValueError("the gain table is not strictly ascending by (level, id)")
    if any(abs(int(g)) > MAX_GAIN for g in gains["gain"]):
        raise ValueError("a gain is out of range")
    return gains


def node_gains(tree, labels=None, penalty=0, gains=None):
    """({node: gain}, {node: (best_label, best_count)})."""
    if (labels is None) == (gains is None):
        raise ValueError("exactly one of labels and gains")
    if not 0 <= penalty <= MAX_GAIN:
        raise ValueError("penalty out of range")
    if labels is not None:
        best = tree.best_labels(labels)
        return {key: best[key][1] - penalty for key in tree.nodes}, best
    listed = {(int(g["level"]), int(g["id"])): int(g["gain"]) for g in check_gains(gains)}
    return {key: listed.get(key, 0) for key in tree.nodes}, {key: (-1, 0) for key in tree.nodes}


def solve(tree, g):
    """(keep, opt, S) of every node, bottom-up."""
    keep, opt, split = {}, {}, {}
    for key in tree.nodes:                           # ascending level: children come first
        kids = tree.children[key]
        split[key] = sum(opt[c] for c in kids)
        keep[key] = not kids or g[key] >= split[key]
        opt[key] = g[key] if keep[key] else split[key]
    return keep, opt, split


def selected_levels(tree, keep):
    """l* of every leaf (column of the ancestor table)."""
    out = np.zeros(len(tree.ids), np.int64)
    for k in range(len(tree.ids)):
        for l in range(tree.L - 1, -1, -1):
            if keep[(l, int(tree.table[l, k]))]:
                out[k] = l
                break
    return out


def cut(ids0, hierarchy, labels=None, penalty=0, gains=None, tree=None):
    """(records, plane, total) of the frame.  tree: Tree(ids0, hierarchy) made before, to share it."""
    tree = tree or Tree(ids0, hierarchy)
    g, best = node_gains(tree, labels, penalty, gains)
    keep, opt, split = solve(tree, g)
    star = selected_levels(tree, keep)
    chosen = sorted({(int(star[k]), int(tree.table[star[k], k])) for k in range(len(tree.ids))})
    records = np.zeros(len(chosen), NODE_DTYPE)
    for i, key in enumerate(chosen):
        kids = tree.children[key]
        records[i] = (key[0], key[1], tree.area[key], len(tree.leaves[key]), len(kids), best[key][0], best[key][1], 0,
                      g[key], split[key] if kids else 0)
    place = {key: i for i, key in enumerate(chosen)}
    leaf_record = np.array([place[(int(star[k]), int(tree.table[star[k], k]))] for k in range(len(tree.ids))],
                           np.int32)
    plane = np.full(tree.ids0.shape, -1, np.int32)
    covered = tree.ids0 >= 0
    if len(tree.ids):
        plane[covered] = leaf_record[np.searchsorted(tree.ids, tree.ids0[covered])]
    total = sum(g[key] for key in chosen)
    assert total == sum(opt[key] for key in tree.top())
    return records, plane, int(total)


def level_plane(records, plane):
    """The level of the record that covers each pixel, -1 where none does."""
    out = np.full(plane.shape, -1, np.int64)
    out[plane >= 0] = records["level"][plane[plane >= 0]]
    return out


def enumerate_cuts(tree):
    """Every partition of the frame into nodes, as tuples of keys; for small trees."""
    def below(key):
        out = [(key,)]
        kids = tree.children[key]
        if kids:
            for parts in itertools.product(*[below(c) for c in kids]):
                out.append(tuple(itertools.chain.from_iterable(parts)))
        return out
    return [tuple(itertools.chain.from_iterable(parts)) for parts in itertools.product(*[below(t) for t in tree.top()])]


def consistent(records, plane, total, ids0):
    """The records partition the covered pixels, are ordered, and sum to total."""
    ids0 = np.asarray(ids0)
    keys = [(int(r["level"]), int(r["id"])) for r in records]
    assert keys == sorted(set(keys))
    assert ((plane >= 0) == (ids0 >= 0)).all()
    assert np.array_equal(np.bincount(plane[plane >= 0], minlength=len(records)), records["area"])
    assert int(records["gain"].sum()) == total and not records["reserved"].any()
    assert (records["split_value"][records["children"] == 0] == 0).all()
    return True


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
