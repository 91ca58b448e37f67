"""level_colors_model.py against a brute-force double loop, closed forms and hand-made halves.  CPU only."""
import numpy as np
import pytest

import level_colors_cases as kc
import level_colors_model as km
import level_components_model as cm
import level_regions_cases as lc
import render_model as rm

SMALL = kc.small()


def planes(c, level, connect):
    ids = lc.id_image(c.case.msg, level)
    if connect == 0:
        return ids, None
    comps, _, labels = cm.sweep(ids, connect)
    return labels, comps


def test_the_dtype_has_the_documented_layout():
    d = km.COLOR_DTYPE
    assert d.itemsize == 72
    assert {n: d.fields[n][1] for n in d.names} == km.OFFSETS


def test_there_are_small_cases_of_every_kind():
    names = {c.name for c in SMALL}
    assert {"checker", "star_300x2", "star_2x300", "hole", "max_id", "uncovered_frame", "halves",
            "equal_means"} <= names
    assert any(n.startswith("width_") for n in names)
    assert all(c.F.shape == (c.case.H, c.case.W, 3) and c.F.dtype == np.uint8 for c in kc.all_cases())


@pytest.mark.parametrize("name", [c.name for c in SMALL])
def test_model_equals_the_double_loop(name):
    c = {k.name: k for k in SMALL}[name]
    for level in c.case.levels:
        for connect in (0, cm.N4, cm.N8):
            P, comps = planes(c, level, connect)
            got, want = km.colors(P, c.F, comps), km.colors_literal(P, c.F, comps)
            assert km.same_bits(got, want), (name, level, connect)
            assert (got["reserved0"] == 0).all() and (got["reserved1"] == 0).all()
            assert got["area"].sum() == (P >= 0).sum()


def test_three_levels_at_every_level():
    c = kc.of(lc.three_levels())
    for level in c.case.levels:
        for connect in (0, cm.N4, cm.N8):
            P, comps = planes(c, level, connect)
            assert km.same_bits(km.colors(P, c.F, comps), km.colors_literal(P, c.F, comps)), (level, connect)


@pytest.mark.parametrize("value", [0, 1, 128, 255])
def test_constant_frames_have_closed_forms(value):
    ids = lc.boundary_ids(65, 5)
    F = np.full(ids.shape + (3,), value, np.uint8)
    F[..., 1] = 255 - value
    rec = km.colors(ids, F)
    area = rec["area"].astype(np.int64)
    for c, v in enumerate((value, 255 - value, value)):
        assert np.array_equal(rec["sum"][:, c], area * v) and np.array_equal(rec["sum_sq"][:, c], area * v * v)
        assert (rec["min"][:, c] == v).all() and (rec["max"][:, c] == v).all() and (rec["mean"][:, c] == v).all()
    mean, var = km.moments(rec)
    assert (var == 0).all() and np.array_equal(mean[:, 0], np.full(len(rec), float(value)))


def test_wide_accumulators_closed_forms():
    """Where a 32-bit sum of squares would wrap (a 32-bit sum wraps from 4096 x 4113 on, which the device test
    checks against the same closed form)."""
    W, H = 640, 104
    rec = km.colors(np.zeros((H, W), np.int32), np.full((H, W, 3), 255, np.uint8))
    assert rec["sum"].tolist() == [[W * H * 255] * 3] and rec["sum_sq"].tolist() == [[W * H * 255 * 255] * 3]
    assert rec["mean"].tolist() == [[255] * 3]
    assert 640 * 104 * 255 * 255 > 1 << 32 and 4096 * 4113 * 255 > 1 << 32 and 10224 * 255 * 255 < 1 << 32


def test_mean_rounds_half_up_at_exact_halves():
    c = kc.halves()
    rec = km.colors(lc.id_image(c.case.msg), c.F)
    assert rec["area"].tolist() == [2, 4, 1]
    assert rec["sum"].tolist() == [[1, 509, 15], [42, 802, 2], [9, 90, 255]]
    # 0.5 -> 1, 254.5 -> 255, 7.5 -> 8; 10.5 -> 11, 200.5 -> 201, 0.5 -> 1
    assert rec["mean"].tolist() == [[1, 255, 8], [11, 201, 1], [9, 90, 255]]
    assert km.same_bits(rec, km.colors_literal(lc.id_image(c.case.msg), c.F))


def test_mean_plane_and_picture_go_through_the_render_models_rules():
    c = kc.equal_means()
    P = lc.id_image(c.case.msg)
    rec = km.colors(P, c.F)
    assert rec["mean"].tolist() == [[100, 50, 200], [100, 50, 200], [10, 20, 30]]
    plane = km.mean_plane(P, rec)
    assert (plane[:, :8] == [100, 50, 200]).all() and (plane[:, 8:] == [10, 20, 30]).all()
    pic = km.picture(P, c.F, rec, has_video=False)
    assert km.same_bits(pic, rm.highlight_edges(plane))
    assert (pic[:, 3] == [100, 50, 200]).all()          # no edge between the two groups with equal means
    assert (pic[:, 7] == 0).all() and (pic[:, 8] == [10, 20, 30]).all()
    assert km.same_bits(km.picture(P, c.F, rec, blend_alpha=0.5),
                        rm.add_weighted(c.F, rm.highlight_edges(plane), 0.5))
    assert km.same_bits(km.picture(P, c.F, rec, highlight_edges=False, concat_with_source=True),
                        np.concatenate([plane, c.F], axis=0))
    # uncovered pixels are black
    hole = {k.name: k for k in kc.all_cases()}["hole"]
    Ph = lc.id_image(hole.case.msg)
    assert (km.mean_plane(Ph, km.colors(Ph, hole.F))[Ph < 0] == 0).all()


def test_stats_of_the_comb():
    c = kc.comb()
    st = km.stats_of(lc.id_image(c.case.msg))
    assert st == {"groups": 1, "intervals": kc.COMB_INTERVALS, "covered": kc.COMB_INTERVALS,
                  "largest_group_intervals": kc.COMB_INTERVALS}
    assert km.stats_of(np.full((3, 4), -1, np.int32)) == {"groups": 0, "intervals": 0, "covered": 0,
                                                          "largest_group_intervals": 0}


def test_moments_against_numpy():
    c = kc.of(lc.three_levels())
    P = lc.id_image(c.case.msg, 1)
    rec = km.colors(P, c.F)
    mean, var = km.moments(rec)
    for k, g in enumerate(np.unique(P)):
        px = c.F[P == g].astype(np.float64)
        assert np.allclose(mean[k], px.mean(axis=0), rtol=1e-12) and np.allclose(var[k], px.var(axis=0), rtol=1e-9)
