"""The three definitions of a level's connected components in level_components_model.py against each
other: the reference's ConnectedComponents restated literally on the literal level regions, the sweep
over the sorted runs, and the flood fill of the id image.  Bits, not tolerances; both connectednesses."""
import numpy as np
import pytest

import level_components_cases as cc
import level_components_model as cm
import level_regions_cases as lc
import level_regions_model as lm
import render_model as rm

CASES = cc.all_cases()
BY_NAME = {c.name: c for c in CASES}
MODES = (cm.N4, cm.N8)


def three_ways(ids, connect, regions=None):
    """sweep, literal and pixels on one id image, asserted equal; returns the result and the counts."""
    H, W = ids.shape
    stats, lit_stats = {}, {}
    want = cm.sweep(ids, connect, stats)
    got = cm.literal(*(regions if regions is not None else lm.runs(ids)), W, H, connect, lit_stats)
    assert cm.same(got, want), "literal"
    assert cm.same(cm.pixels(ids, connect), want), "pixels"
    assert stats == lit_stats
    # two sorted lists of disjoint, non-touching intervals have fewer neighbour pairs than intervals
    assert stats["links"] < 2 * stats["runs"] or stats["runs"] == 0
    return want, stats


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_literal_sweep_and_pixels_agree(case):
    hier = rm.hierarchy_of(case.msg)
    for level in case.levels:
        ids = lc.id_image(case.msg, level)
        regions = lm.literal(case.msg, level, hier)
        for connect in MODES:
            (comps, intervals, labels), _ = three_ways(ids, connect, regions)
            assert np.array_equal(labels == -1, ids == -1)
            assert int(comps["area"].sum()) == int((ids != -1).sum())
            assert comps.dtype.itemsize == 64


def test_random_id_images():
    rng = np.random.RandomState(20)
    for k in range(300):
        H, W = (1, 1) if k == 0 else (int(rng.randint(1, 41)), int(rng.randint(1, 41)))
        n_ids = int(rng.randint(2, 7))
        names = np.concatenate([[-1], rng.permutation(40)[:n_ids] * ((1 << 30) // 40)]).astype(np.int32)
        # blobs rather than noise on every other image: a coarse random grid blown up
        if k % 2:
            coarse = rng.randint(0, n_ids + 1, ((H + 3) // 4, (W + 2) // 3))
            ids = names[np.kron(coarse, np.ones((4, 3), np.int64))[:H, :W]]
        else:
            ids = names[rng.randint(0, n_ids + 1, (H, W))]
        for connect in MODES:
            three_ways(ids.astype(np.int32), connect)


def test_expected_counts_of_the_named_cases():
    def count(name, level, connect):
        comps, _, _ = cm.sweep(lc.id_image(BY_NAME[name].msg, level), connect)
        return comps

    for connect in MODES:
        assert len(count("checker", 0, connect)) == 6144
    n4 = count("checker", 1, cm.N4)
    assert len(n4) == 6144 and set(n4["region_components"].tolist()) == {3072}
    assert n4["component"].tolist() == list(range(3072)) * 2
    n8 = count("checker", 1, cm.N8)
    assert len(n8) == 2 and n8["region_components"].tolist() == [1, 1] and n8["num_intervals"].tolist() == [3072] * 2
    for name in ("serpentine", "spiral", "comb_up", "comb_down", "fan_down", "fan_up", "fan_offset"):
        for connect in MODES:
            comps = count(name, 0, connect)
            assert len(comps) == 1, name
    assert count("serpentine", 0, cm.N4)["num_intervals"][0] > 2000
    assert count("spiral", 0, cm.N4)["num_intervals"][0] > 1000
    assert len(count("fan_diagonal", 0, cm.N4)) == 256 and len(count("fan_diagonal", 0, cm.N8)) == 1
    rings = count("rings", 0, cm.N8)
    assert rings["id"].tolist() == [11, 11, 12] and rings["component"].tolist() == [0, 1, 0]
    assert rings["region_components"].tolist() == [2, 2, 1]
    inter = count("interleaved", 0, cm.N4)
    assert len(inter) == 72 and len(count("interleaved", 0, cm.N8)) == 2
    assert sorted(set(inter["id"].tolist())) == [7, 1 << 30]
    assert [len(count("parts", 1, c)) for c in MODES] == [4, 3]


def test_components_are_ordered_by_their_first_pixel():
    ids = np.array([[-1, 5, -1, 5],
                    [5, -1, -1, 5],
                    [5, -1, 5, -1]], np.int32)
    comps, intervals, labels = cm.sweep(ids, cm.N4)
    assert labels.tolist() == [[-1, 0, -1, 1], [2, -1, -1, 1], [2, -1, 3, -1]]
    assert comps["first_interval"].tolist() == [0, 1, 3, 5] and comps["component"].tolist() == [0, 1, 2, 3]
    comps, intervals, labels = cm.sweep(ids, cm.N8)
    assert labels.tolist() == [[-1, 0, -1, 1], [0, -1, -1, 1], [0, -1, 1, -1]]
    # a component keeps its intervals in list order
    assert intervals.tolist() == [[0, 1, 1, 5], [1, 0, 0, 5], [2, 0, 0, 5], [0, 3, 3, 5], [1, 3, 3, 5], [2, 2, 2, 5]]


def test_touching_intervals_are_outside_the_definition():
    """level_regions_cases.touching_counter_example: a rasterization with the touching intervals [0, 3]
    and [4, 7] in one row.  ConnectedComponents does not call them neighbours under N4 (max(left) = 4 >
    min(right) = 3) although their pixels are 4-adjacent; the id plane shows one run, and the library
    works on maximal runs, which never touch."""
    raster = [(0, 0, 3), (0, 4, 7)]
    assert len(cm.connected_components(raster, cm.N4)[0]) == 2
    assert len(cm.connected_components(raster, cm.N8)[0]) == 1
    m = lc.touching_counter_example()
    ids = lc.id_image(m, 1)
    for connect in MODES:
        comps, intervals, _ = cm.sweep(ids, connect)
        assert len(comps) == 1 and intervals.tolist() == [[0, 0, 7, 9], [1, 2, 5, 9]]
        assert cm.same(cm.pixels(ids, connect), cm.sweep(ids, connect))
