"""Frames for the tree cut tests (not collected by pytest), built from persistence_cases and
level_regions_cases.  A case is (name, msg, W, H, labels, penalties, gains): the desc, a label plane, the
penalties to cut it with and a gain table.  Each is one of the smallest shapes at which a kernel can still go
wrong."""
import collections

import numpy as np

import level_regions_cases as lc
import persistence_cases as pc
import render_model as rm
import tree_cut_model as tm

Case = collections.namedtuple("Case", "name msg W H labels penalties gains")
MAX_LABEL = (1 << 31) - 1
PENALTIES = (0, 1, 2, 3, 1 << 32)


def ids_of(msg):
    return lc.id_image(msg, 0)


def table(entries):
    out = np.zeros(len(entries), tm.GAIN_DTYPE)
    for i, e in enumerate(sorted(entries)):
        out[i] = e
    return out


def random_gains(msg, seed):
    """A gain for about two nodes in three, small enough for ties, and two entries that name no node."""
    tree = tm.Tree(ids_of(msg), rm.hierarchy_of(msg))
    rng = np.random.RandomState(seed)
    entries = [(l, i, int(rng.randint(-4, 9))) for (l, i) in tree.nodes if rng.randint(3)]
    present = set(tree.nodes)
    for absent in ((0, 123456789), (tree.L + 3, 0), (-1, 5)):
        if absent not in present:
            entries.append(absent + (7,))
    return table(entries)


def shifted_labels(ids, modulo=5):
    """The id image moved by (3, 4), folded into a few labels, with holes: no label where the id was -1 and in
    one column."""
    ids = np.asarray(ids, np.int64)
    moved = np.roll(ids, (3, 4), (0, 1))
    out = np.where(moved >= 0, moved % modulo, -1).astype(np.int32)
    out[:, ids.shape[1] // 2] = -7
    return out


def from_case(c, labels=None, penalties=PENALTIES, gains=None, name=None):
    ids = ids_of(c.msg)
    return Case(name or c.name, c.msg, c.W, c.H, shifted_labels(ids) if labels is None else labels, tuple(penalties),
                random_gains(c.msg, len(c.name) + c.W) if gains is None else gains)


def ladder_splits(L):
    return sorted({k for k in (1, 2, (L + 1) // 2, L - 1, L) if 1 <= k <= L})


def ladders():
    """ladder(L) has the columns 0 .. L; at level l the columns 0 .. l are one region.  The labels are 0 left of
    column k and 1 from it on: the rungs climb to level k - 1 (with penalty 0 every rung below is a tie,
    g == S), the columns from k on are single-child chains that climb to the top.  With penalty 2 the rung of
    level k is a tie as well: 2 k - 2 against (2 k - 2) + (2 - 2)."""
    out = []
    for L in pc.LADDER_HEIGHTS:
        c = pc.ladder(L)
        for k in ladder_splits(L):
            labels = np.tile((np.arange(L + 1) >= k).astype(np.int32), (2, 1))
            out.append(from_case(c, labels, name="%s_split_%d" % (c.name, k)))
    return out


def chain():
    """Two regions that pass through four levels unchanged but for their names: every level is a tie, the cut is
    the top."""
    ids = np.array([[0, 0, 0, 1], [0, 0, 1, 1]], np.int32)
    maps = [{0: 10, 1: 11}, {10: 20, 11: 21}, {20: 30, 21: 31}]
    c = pc.case("chain_4", ids, maps)
    return from_case(c, np.array([[0, 0, 0, 1], [0, 1, 1, 1]], np.int32))


def max_id():
    c = pc.max_id()
    ids = ids_of(c.msg)
    labels = np.where(ids == 0, MAX_LABEL, 0).astype(np.int32)
    labels[0, 0] = 0
    labels[-1, -1] = MAX_LABEL
    return from_case(c, labels)


def unlabelled():
    """Every label negative: best_label -1 and best_count 0 everywhere."""
    c = [x for x in pc.reused() if x.name == "uncovered"][0]
    return from_case(c, np.full((c.H, c.W), -3, np.int32), name="uncovered_unlabelled")


def dense():
    """64 x 64 one-pixel regions, five levels (2 x 2 blocks merge at every level), seven labels in diagonal
    stripes: 20480 node keys, and more pair keys than one tile of the sort holds."""
    W = H = 64
    yy, xx = np.mgrid[0:H, 0:W]
    ids = (yy * W + xx).astype(np.int32)
    maps, below = [], {int(i): (int(i) // W, int(i) % W) for i in ids.ravel()}
    for l in range(1, 5):
        step = 1 << l
        name = lambda y, x: 100000 * l + (y // step) * W + x // step
        maps.append({i: name(y, x) for i, (y, x) in below.items()})
        below = {name(y, x): (y // step * step, x // step * step) for (y, x) in below.values()}
    c = pc.case("dense_64", ids, maps)
    labels = ((xx + 2 * yy) // 9 % 7).astype(np.int32)
    return from_case(c, labels, penalties=(0, 1, 3, 20, 1 << 32))


def big_gains():
    """2^32 on three leaves and -2^32 on their parent, and the other way round one level up: the sums pass 32
    bits in both directions."""
    ids = np.array([[0, 1, 2, 3, 4, 5]], np.int32)
    maps = [{0: 10, 1: 10, 2: 10, 3: 11, 4: 11, 5: 11}, {10: 20, 11: 20}]
    c = pc.case("big_gains", ids, maps)
    big = 1 << 32
    gains = table([(0, 0, big), (0, 1, big), (0, 2, big), (1, 10, -big), (0, 3, -big), (0, 4, -big), (0, 5, -big),
                   (1, 11, big), (2, 20, big)])
    return from_case(c, gains=gains)


def bad_tables():
    """(what, table) the call refuses, for big_gains' frame."""
    return [("unsorted", np.array([(0, 1, 1), (0, 0, 1)], tm.GAIN_DTYPE)),
            ("unsorted level", np.array([(1, 10, 1), (0, 0, 1)], tm.GAIN_DTYPE)),
            ("duplicate", np.array([(0, 0, 1), (0, 1, 2), (0, 1, 2)], tm.GAIN_DTYPE)),
            ("gain too large", np.array([(0, 0, 1), (0, 1, (1 << 32) + 1)], tm.GAIN_DTYPE)),
            ("gain too small", np.array([(0, 0, -(1 << 32) - 1), (0, 1, 0)], tm.GAIN_DTYPE))]


def all_cases():
    out = ladders() + [chain()]
    out += [from_case(c) for c in pc.widths() + pc.narrow()]
    out += [max_id(), from_case(pc.out_of_order())]
    out += [from_case(c) for c in pc.reused()]
    out += [unlabelled(), dense(), big_gains()]
    return out
