"""The numpy model of the boundary distance calls against itself: the separable minimum against the all-pairs
minimum, the closed forms of the planted frames, the two identities the device's benchmark rests on, and the
monotonicity of the records.  Needs no device."""
import numpy as np
import pytest

import boundary_distance_cases as dc
import boundary_distance_model as dm
import level_regions_cases as lc
import persistence_model as pm
import render_model as rm

PLANTED = {c.name: c for c in dc.planted()}


def q_of(case):
    ids0 = lc.id_image(case.msg, 0)
    hier = rm.hierarchy_of(case.msg)
    return ids0, pm.plane(ids0, pm.ancestors(ids0, hier)), pm.height(hier)


@pytest.mark.parametrize("seed", range(6))
def test_separable_minimum_equals_the_all_pairs_minimum(seed):
    rs = np.random.RandomState(seed)
    H, W = rs.randint(1, 24), rs.randint(1, 40)
    for density in (0.0, 0.02, 0.3, 1.0):
        mask = rs.rand(H, W) < density
        d = dm.distance(mask)
        assert d.dtype == np.int32 and np.array_equal(d, dm.brute_distance(mask)), (H, W, density)
        assert np.array_equal(d == 0, mask) or not mask.any()
        if not mask.any():
            assert (d == dm.NONE).all()


def test_closed_forms_of_the_planted_frames():
    yy, xx = np.mgrid[0:dc.PH, 0:dc.PW].astype(np.int64)
    ids = lc.id_image(PLANTED["first_column"].msg, 0)
    assert np.array_equal(dm.distance(pm.edge_mask(ids)), xx ** 2)
    ids = lc.id_image(PLANTED["first_row"].msg, 0)
    assert np.array_equal(dm.distance(pm.edge_mask(ids)), yy ** 2)
    ids = lc.id_image(PLANTED["corner"].msg, 0)
    mask = pm.edge_mask(ids)
    W, H = dc.PW, dc.PH
    assert sorted(zip(*np.nonzero(mask))) == [(H - 2, W - 1), (H - 1, W - 2)]
    want = np.minimum((xx - (W - 2)) ** 2 + (yy - (H - 1)) ** 2, (xx - (W - 1)) ** 2 + (yy - (H - 2)) ** 2)
    assert np.array_equal(dm.distance(mask), want)
    for name in ("uniform", "uncovered_300x200", "thin_1x1", "thin_uniform_290x1"):
        ids = lc.id_image(PLANTED[name].msg, 0)
        assert (dm.distance(pm.edge_mask(ids)) == dm.NONE).all(), name
    ids = lc.id_image(PLANTED["every_pixel"].msg, 0)
    d = dm.distance(pm.edge_mask(ids))
    assert d[-1, -1] == 1 and d.ravel()[:-1].max() == 0      # only the last pixel has no right or below neighbour
    d = dm.distance(pm.edge_mask(lc.id_image(PLANTED["thin_290x1"].msg, 0)))
    assert d.shape == (1, 290) and d[0, 96] == 0 and d[0, 0] == 96 ** 2 and d[0, 289] == (289 - 193) ** 2


@pytest.mark.parametrize("name", ["blobs", "first_column", "corner", "thin_1x290"])
def test_the_two_identities_and_the_records(name):
    case = PLANTED[name]
    ids0, q, L = q_of(case)
    for other_name, other in dc.others(case, ids0)[:2]:
        g = dm.other_edges(other)
        d_g = dm.distance(g)
        previous = None
        for T in dc.TOLERANCES:
            want = dm.benchmark(q, L, other, T)
            assert want.dtype.itemsize == 32 and len(want) == L
            # seg_matched: one distance transform of G, a histogram of Q over the near pixels, suffix sums
            assert np.array_equal(dm.suffix_counts(q[d_g <= T], L), want["seg_matched"]), (other_name, T)
            # gt_matched: the disc maximum of Q at the pixels of G, a histogram, suffix sums
            m = dm.disc_maximum(q, T)
            assert np.array_equal(dm.suffix_counts(m[g], L), want["gt_matched"]), (other_name, T)
            assert np.array_equal(dm.suffix_counts(q, L), want["seg_edges"])
            assert want["seg_edges"].tolist() == [int((q > l).sum()) for l in range(L)]
            assert (want["gt_edges"] == int(g.sum())).all()
            # monotone in l: a higher level has fewer edges and matches fewer of either side
            for field in ("seg_edges", "seg_matched", "gt_matched"):
                assert (np.diff(want[field]) <= 0).all(), (field, T)
            assert (want["seg_matched"] <= want["seg_edges"]).all() and (want["gt_matched"] <= want["gt_edges"]).all()
            # monotone in T
            if previous is not None:
                assert (want["seg_matched"] >= previous["seg_matched"]).all()
                assert (want["gt_matched"] >= previous["gt_matched"]).all()
            previous = want


def test_shift_by_3_4_flips_between_24_and_25():
    """A vertical boundary moved by (3, 4) lies 3 away; an anti-diagonal one x + y = c lands on x + y = c + 7,
    whose nearest pixels are (3, 4) and (4, 3) away: 25, not 24."""
    case = PLANTED["first_column"]
    ids0, q, L = q_of(case)
    other = dc.shifted(ids0)
    g = dm.other_edges(other)
    assert np.array_equal(np.nonzero(g.any(axis=0))[0], [3])      # the boundary moved from column 0 to column 3
    at = {T: dm.benchmark(q, L, other, T) for T in (4, 9)}
    assert at[4]["seg_matched"][0] == 0 and at[9]["seg_matched"][0] == dc.PH
    assert at[4]["gt_matched"][0] == 0 and at[9]["gt_matched"][0] == dc.PH
    yy, xx = np.mgrid[0:40, 0:40]
    ids0 = (xx + yy >= 40).astype(np.int32)
    q = pm.edge_mask(ids0).astype(np.int32)
    other = dc.shifted(ids0)
    a, b = dm.benchmark(q, 1, other, 24), dm.benchmark(q, 1, other, 25)
    inner = int(q[8:32, 8:32].sum())
    assert a["seg_matched"][0] < inner / 2 and b["seg_matched"][0] >= inner
    case = PLANTED["blobs"]
    ids0, q, L = q_of(case)
    other = dc.shifted(ids0)
    a, b = dm.benchmark(q, L, other, 24), dm.benchmark(q, L, other, 25)
    assert b["seg_matched"][0] > a["seg_matched"][0] and b["gt_matched"][0] > a["gt_matched"][0]


def test_scores_quotients():
    rec = np.zeros(3, dm.SCORE_DTYPE)
    rec[0] = (10, 5, 8, 8)
    rec[1] = (4, 4, 8, 2)
    p, r, f, best = dm.scores(rec)
    assert p.tolist() == [0.5, 1.0, 0.0] and r.tolist() == [1.0, 0.25, 0.0]
    assert f.tolist() == [2 * 0.5 / 1.5, 2 * 0.25 / 1.25, 0.0] and best == 0
