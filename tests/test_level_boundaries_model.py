"""The two definitions of level_boundaries_model.py agree: the reference's GetBoundary restated literally
and the set form the device code is written to, on every case plane and on random masks; and the region
and component modes of the set form are consistent with each other.  CPU only."""
import numpy as np
import pytest

import level_boundaries_cases as bc
import level_boundaries_model as bm
import level_components_model as cm
import level_regions_cases as lc

CASES = bc.all_cases()
SMALL = [c for c in CASES if c.W * c.H <= 2048]      # the literal form is a Python loop over bytes


def planes_of(c):
    return [lc.id_image(c.msg, level) for level in c.levels]


def check_mask(mask):
    """The literal form against the set form for one mask; returns the outer mode's guard reads."""
    mask = np.asarray(mask, bool)
    runs = bm.runs_of_mask(mask)
    got, guard = bm.get_boundary_literal(runs, mask.shape[1], True)
    assert got == bm.of_mask(mask, False)
    assert guard == 0
    got, guard = bm.get_boundary_literal(runs, mask.shape[1], False)
    assert got == [(x + 1, y) for x, y in bm.of_mask(mask, True)]      # the reference's x is one too large
    return guard


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_literal_equals_set_form_on_every_group_of_every_case(case):
    for plane in planes_of(case):
        for g in np.unique(plane[plane >= 0])[:12]:
            check_mask(plane == g)


def test_literal_equals_set_form_on_random_masks():
    rng = np.random.RandomState(5)
    guard = 0
    for k in range(300):
        H, W = rng.randint(1, 10), rng.randint(1, 12)
        mask = rng.rand(H, W) < rng.choice([0.15, 0.5, 0.85])
        if not mask.any():
            mask[rng.randint(H), rng.randint(W)] = True
        guard += check_mask(mask)
    # the outer mode does read outside its buffer: a mask with a pixel in column 0 reads the byte before
    assert guard > 0
    _, one = bm.get_boundary_literal([(0, 0, 0)], 1, False)
    assert one > 0


def test_an_empty_rasterization_has_no_boundary():
    assert bm.get_boundary_literal([], 5, True) == ([], 0) and bm.get_boundary_literal([], 5, False) == ([], 0)
    for outer in (False, True):
        records, points = bm.boundaries(np.full((3, 4), -1, np.int32), outer)
        assert records.shape == (0,) and points.shape == (0, 2) and points.dtype == np.int32


def test_counts_of_the_simple_planes():
    W, H = 7, 4
    records, points = bm.boundaries(np.full((H, W), 3, np.int32), True)
    assert records.tolist() == [(3, -1, 0, 2 * W + 2 * H)]
    assert not any((x in (-1, W)) and (y in (-1, H)) for x, y in points.tolist())         # no corners
    assert all(x in (-1, W) or y in (-1, H) for x, y in points.tolist())
    records, _ = bm.boundaries(np.full((H, W), 3, np.int32), False)
    assert records.tolist() == [(3, -1, 0, 2 * W + 2 * H - 4)]
    by_name = {c.name: c for c in CASES}
    plane = planes_of(by_name["pixel_checker"])[0]
    records, points = bm.boundaries(plane, False)
    assert records["num_points"].sum() == plane.size                                     # every pixel is inner
    _, outer = bm.boundaries(plane, True)
    inside = [(x, y) for x, y in outer.tolist() if 0 < x < plane.shape[1] - 1 and 0 < y < plane.shape[0] - 1]
    assert len(inside) == 4 * (plane.shape[1] - 2) * (plane.shape[0] - 2)                # of four groups each
    plane = planes_of(by_name["flanked"])[0]
    records, points = bm.boundaries(plane, True)
    five = points[records[0]["first_point"]:][:records[0]["num_points"]].tolist()
    assert records[0]["id"] == 5 and len(set(map(tuple, five))) == len(five)             # listed once
    for p in ([2, 2], [6, 2], [10, 1], [3, 6], [7, 6], [12, 6]):
        assert five.count(p) == 1, p


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_components_boundaries_make_up_their_regions(case):
    for plane in planes_of(case):
        for connect in (cm.N4, cm.N8):
            comps, _, labels = cm.sweep(plane, connect)
            for outer in (False, True):
                r_rec, r_pts = bm.boundaries(plane, outer)
                c_rec, c_pts = bm.boundaries(labels, outer, comps)
                assert len(c_rec) == len(comps) and len(r_rec) == len(np.unique(comps["id"]))
                assert np.array_equal(c_rec["id"], comps["id"]) and np.array_equal(c_rec["component"], comps["component"])
                for r in r_rec:
                    want = r_pts[r["first_point"]:r["first_point"] + r["num_points"]]
                    parts = [c_pts[c["first_point"]:c["first_point"] + c["num_points"]]
                             for c in c_rec[c_rec["id"] == r["id"]]]
                    got = np.concatenate(parts)
                    if outer:
                        got = np.unique(got[:, ::-1], axis=0)[:, ::-1]        # a set: sorted by (y, x), once
                    else:
                        got = got[np.lexsort((got[:, 0], got[:, 1]))]          # a list: nothing is shared
                    assert np.array_equal(got, want), (case.name, connect, outer, int(r["id"]))
