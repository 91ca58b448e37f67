"""The tree cut's numpy model against the enumeration of every cut on small random trees, the consequences the
definition promises, and the internal consistency of every case of tree_cut_cases.  No device."""
import numpy as np
import pytest

import level_overlap_model as om
import level_regions_cases as lc
import render_model as rm
import tree_cut_cases as tc
import tree_cut_model as tm

CASES = tc.all_cases()


def random_tree(rng):
    """(ids0, desc) with up to 9 leaves and up to 6 levels; every level merges some neighbours of the level
    below, or none (single-child chains)."""
    n = int(rng.randint(1, 10))
    L = int(rng.randint(1, 7))
    widths = rng.randint(1, 4, n)
    ids = np.repeat(np.arange(n, dtype=np.int32), widths)[None, :].repeat(2, 0)
    maps, below = [], list(range(n))
    for l in range(1, L):
        groups, g = [], 0
        for i in range(len(below)):
            if i and rng.randint(3) == 0:
                g += 1
            groups.append(g)
        maps.append({b: 100 * l + grp for b, grp in zip(below, groups)})
        below = sorted(set(maps[-1].values()))
    return ids, lc.desc_from_ids(ids, maps)


def value_of(parts, g):
    return sum(g[key] for key in parts)


@pytest.mark.parametrize("seed", range(8))
def test_model_equals_the_enumeration_of_every_cut(seed):
    rng = np.random.RandomState(seed)
    ties = 0
    for _ in range(50):
        ids, msg = random_tree(rng)
        hier = rm.hierarchy_of(msg)
        tree = tm.Tree(ids, hier)
        labels = rng.randint(-1, 4, ids.shape).astype(np.int32)
        gains = tc.table([(l, i, int(rng.randint(-5, 6))) for (l, i) in tree.nodes if rng.randint(4)])
        cuts = tm.enumerate_cuts(tree)
        for source in [dict(labels=labels, penalty=p) for p in (0, 1, 2, 5)] + [dict(gains=gains)]:
            g, _ = tm.node_gains(tree, **source)
            records, plane, total = tm.cut(ids, hier, tree=tree, **source)
            assert tm.consistent(records, plane, total, ids)
            best = max(value_of(parts, g) for parts in cuts)
            assert total == best
            optimal = [parts for parts in cuts if value_of(parts, g) == best]
            mine = tuple(sorted((int(r["level"]), int(r["id"])) for r in records))
            assert mine in [tuple(sorted(parts)) for parts in optimal]
            # a tie keeps the coarser node: every optimal cut refines the model's
            assert len(mine) == min(len(parts) for parts in optimal)
            ties += len(optimal) > 1
    assert ties > 0


@pytest.mark.parametrize("seed", range(4))
def test_consequences(seed):
    rng = np.random.RandomState(100 + seed)
    for _ in range(25):
        ids, msg = random_tree(rng)
        hier = rm.hierarchy_of(msg)
        tree = tm.Tree(ids, hier)
        labels = rng.randint(-1, 4, ids.shape).astype(np.int32)
        rows, _, _ = om.overlap(ids, labels)
        # penalty 0: the level-0 numerator, by the coarsest partition that reaches it
        records, plane, total = tm.cut(ids, hier, labels=labels, tree=tree)
        assert int(records["best_count"].sum()) == int(rows["best_count"].sum()) == total
        best = tree.best_labels(labels)
        reach = [parts for parts in tm.enumerate_cuts(tree) if sum(best[k][1] for k in parts) == total]
        assert len(records) == min(len(parts) for parts in reach)
        assert all(sum(best[k][1] for k in parts) <= total for parts in tm.enumerate_cuts(tree))
        # a penalty above every count: the top level
        records, plane, _ = tm.cut(ids, hier, labels=labels, penalty=ids.size + 1, tree=tree)
        assert [(int(r["level"]), int(r["id"])) for r in records] == tree.top()
        # nested cuts
        counts, levels = [], []
        for p in range(0, ids.size + 2):
            records, plane, _ = tm.cut(ids, hier, labels=labels, penalty=p, tree=tree)
            counts.append(len(records))
            levels.append(tm.level_plane(records, plane))
        assert all(a >= b for a, b in zip(counts, counts[1:])), counts
        assert all((a <= b).all() for a, b in zip(levels, levels[1:]))


def test_every_case_is_consistent_and_has_what_it_is_there_for():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    stars, tie_found, wide = {}, False, False
    for c in CASES:
        ids, hier = tc.ids_of(c.msg), rm.hierarchy_of(c.msg)
        assert ids.shape == (c.H, c.W) and c.labels.shape == ids.shape and c.labels.dtype == np.int32
        tree = tm.Tree(ids, hier)
        tm.check_gains(c.gains)
        for source in [dict(labels=c.labels, penalty=p) for p in c.penalties] + [dict(gains=c.gains)]:
            records, plane, total = tm.cut(ids, hier, tree=tree, **source)
            assert tm.consistent(records, plane, total, ids), c.name
            g, _ = tm.node_gains(tree, **source)
            _, _, split = tm.solve(tree, g)
            tie_found |= any(len(tree.children[k]) > 1 and g[k] == split[k] for k in tree.nodes)
            wide |= abs(total) > 1 << 32
            if c.name.startswith("ladder_") and "labels" in source:
                stars.setdefault(tree.L, set()).update(int(x) for x in records["level"])
        if c.name == "chain_4":
            records, _, _ = tm.cut(ids, hier, labels=c.labels, tree=tree)
            assert sorted(records["level"].tolist()) == [3, 3]
    assert tie_found and wide
    # over the ladders' splits l* takes the bottom, the top and values between
    for L, seen in stars.items():
        assert 0 in seen and L - 1 in seen, (L, seen)
        assert L < 4 or len(seen) >= 3, (L, seen)
    by_name = {c.name: c for c in CASES}
    empty = by_name["uncovered_frame"]
    records, plane, total = tm.cut(tc.ids_of(empty.msg), rm.hierarchy_of(empty.msg), labels=empty.labels)
    assert len(records) == 0 and total == 0 and (plane == -1).all()
    records, _, _ = tm.cut(tc.ids_of(by_name["uncovered_unlabelled"].msg), [], labels=by_name["uncovered_unlabelled"].labels)
    assert (records["best_label"] == -1).all() and not records["best_count"].any()
    dense = by_name["dense_64"]
    assert tm.Tree(tc.ids_of(dense.msg), rm.hierarchy_of(dense.msg)).L == 5
    assert (dense.labels >= 0).all() and len(np.unique(dense.labels)) == 7


def test_bad_tables_and_sources_are_refused():
    for what, bad in tc.bad_tables():
        with pytest.raises(ValueError):
            tm.check_gains(bad)
    c = {c.name: c for c in CASES}["big_gains"]
    ids, hier = tc.ids_of(c.msg), rm.hierarchy_of(c.msg)
    with pytest.raises(ValueError):
        tm.cut(ids, hier)
    with pytest.raises(ValueError):
        tm.cut(ids, hier, labels=c.labels, gains=c.gains)
    for p in (-1, (1 << 32) + 1):
        with pytest.raises(ValueError):
            tm.cut(ids, hier, labels=c.labels, penalty=p)
    records, _, total = tm.cut(ids, hier, gains=c.gains)
    big = 1 << 32
    assert total == 4 * big and [(int(r["level"]), int(r["id"])) for r in records] == [(0, 0), (0, 1), (0, 2), (1, 11)]
    assert records["split_value"][3] == -3 * big
