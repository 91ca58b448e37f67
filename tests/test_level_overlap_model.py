"""level_overlap_model.py against a brute-force double loop, its identities, and overlap_scores against a
direct evaluation on the planes.  Pins the definition; needs neither the library nor a device."""
import numpy as np
import pytest

import level_components_model as cm
import level_overlap_cases as oc
import level_overlap_model as om
import level_regions_cases as lc

CASES = oc.all_cases()
SMALL = oc.small()


def planes(c, connect):
    ids = lc.id_image(c.case.msg, 0)
    if connect == 0:
        return ids, None
    comps, _, labels = cm.sweep(ids, connect)
    return labels, comps


def test_there_are_small_cases_of_every_kind():
    names = {c.name for c in SMALL}
    for name in ("width_62x1", "width_257x5", "wrap_64x3", "same_hole", "void", "uncovered_frame", "checker_offset",
                 "labels_300x2", "regions_2x300", "max_values"):
        assert name in names, name


@pytest.mark.parametrize("name", [c.name for c in SMALL])
def test_model_equals_the_double_loop(name):
    c = {k.name: k for k in SMALL}[name]
    for connect in (0, cm.N4, cm.N8):
        P, comps = planes(c, connect)
        got, want = om.overlap(P, c.B, comps), om.overlap_literal(P, c.B, comps)
        for g, w, dtype in zip(got, want, (om.ROW_DTYPE, om.COL_DTYPE, om.PAIR_DTYPE)):
            assert g.dtype == dtype and om.same_bits(g, w), (name, connect)


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_identities(name):
    c = {k.name: k for k in CASES}[name]
    for connect in (0, cm.N4, cm.N8):
        P, comps = planes(c, connect)
        rows, cols, pairs = om.overlap(P, c.B, comps)
        covered, labelled, both = om.totals(P, c.B)
        count = pairs["count"].astype(np.int64)
        assert (count > 0).all()
        assert np.array_equal(rows["area"] - rows["unlabelled"],
                              np.bincount(pairs["row"], weights=count, minlength=len(rows)).astype(np.int64))
        assert np.array_equal(cols["area"] - cols["uncovered"],
                              np.bincount(pairs["col"], weights=count, minlength=len(cols)).astype(np.int64))
        assert rows["area"].sum(dtype=np.int64) == covered and cols["area"].sum(dtype=np.int64) == labelled
        assert count.sum() == both <= min(covered, labelled)
        assert np.array_equal(cols["label"][pairs["col"]], pairs["label"])
        # grouped by row in row order, within a row by ascending label = ascending col
        key = pairs["row"].astype(np.int64) << 32 | pairs["col"]
        assert (np.diff(key) > 0).all()
        assert (np.diff(cols["label"].astype(np.int64)) > 0).all()
        assert np.array_equal(rows["first_pair"], np.cumsum(rows["num_pairs"]) - rows["num_pairs"])
        # a run is at least a pixel with a group or a label, and every cell of the table has a run
        live = int(((np.asarray(P) >= 0) | (c.B >= 0)).sum())
        assert len(pairs) <= om.runs_of(P, c.B) <= live and (om.runs_of(P, c.B) > 0) == (live > 0)


def test_named_cases_are_what_they_say():
    by = {c.name: c for c in CASES}
    for name in ("wrap_64x3", "wrap_257x3"):
        c = by[name]
        rows, cols, pairs = om.overlap(lc.id_image(c.case.msg), c.B)
        assert om.runs_of(lc.id_image(c.case.msg), c.B) == c.case.H and len(pairs) == 1
    c = by["checker_offset"]
    assert om.runs_of(lc.id_image(c.case.msg), c.B) == c.case.W * c.case.H
    for name in ("same_hole", "same_three_levels"):
        P = lc.id_image(by[name].case.msg)
        rows, cols, pairs = om.overlap(P, by[name].B)
        assert len(rows) == len(cols) == len(pairs) and np.array_equal(pairs["row"], pairs["col"])
        assert np.array_equal(pairs["count"], rows["area"]) and np.array_equal(rows["best_label"], rows["id"])
    rows, cols, pairs = om.overlap(lc.id_image(by["void"].case.msg), by["void"].B)
    assert len(cols) == len(pairs) == 0 and len(rows) > 0 and np.array_equal(rows["unlabelled"], rows["area"])
    rows, cols, pairs = om.overlap(lc.id_image(by["uncovered_frame"].case.msg), by["uncovered_frame"].B)
    assert len(rows) == len(pairs) == 0 and len(cols) == 2 and np.array_equal(cols["uncovered"], cols["area"])
    for name in ("labels_300x2", "labels_2x300"):
        rows, cols, pairs = om.overlap(lc.id_image(by[name].case.msg), by[name].B)
        assert rows["num_pairs"].tolist() == [oc.MANY] and rows["unlabelled"].tolist() == [oc.MANY]
    for name in ("regions_300x2", "regions_2x300"):
        rows, cols, pairs = om.overlap(lc.id_image(by[name].case.msg), by[name].B)
        assert cols["num_pairs"].tolist() == [oc.MANY] and len(rows) == oc.MANY + 1
        assert cols["best_row"].tolist() == [1]          # every count is 1: the smallest row wins
    rows, cols, pairs = om.overlap(lc.id_image(by["max_values"].case.msg), by["max_values"].B)
    assert rows["id"].tolist() == [0, oc.MAX] and cols["label"].tolist() == [0, oc.MAX]
    assert pairs[-1].tolist() == (1, 1, oc.MAX, 4)


def test_ties_go_to_the_smallest_label_and_the_smallest_row():
    P = np.array([[1, 1, 2, 2], [1, 1, 2, 2]], np.int32)
    B = np.array([[5, 3, 3, 5], [3, 5, 5, 3]], np.int32)
    rows, cols, _ = om.overlap(P, B)
    assert rows["best_label"].tolist() == [3, 3] and rows["best_count"].tolist() == [2, 2]
    assert cols["best_row"].tolist() == [0, 0] and cols["best_count"].tolist() == [2, 2]


@pytest.mark.parametrize("name", [c.name for c in SMALL])
def test_overlap_scores_equal_a_direct_evaluation(name):
    from video_segment_amd import render
    c = {k.name: k for k in SMALL}[name]
    P = lc.id_image(c.case.msg)
    rows, _, pairs = om.overlap(P, c.B)
    s = render.overlap_scores(rows, pairs)
    n, asa_sum, ue_sum = om.scores_direct(P, c.B)
    assert (s["n"], s["asa_sum"], s["ue_sum"]) == (n, asa_sum, ue_sum)
    assert all(isinstance(s[k], int) for k in ("n", "asa_sum", "ue_sum"))
    if n == 0:
        assert s["asa"] is None and s["ue"] is None
    else:
        assert isinstance(s["asa"], float) and s["asa"] == asa_sum / n and s["ue"] == ue_sum / n
        assert 0.0 < s["asa"] <= 1.0 and 0.0 <= s["ue"] <= 1.0


def test_scores_of_a_perfect_and_of_a_void_table():
    from video_segment_amd import render
    P = lc.id_image({c.name: c for c in CASES}["same_three_levels"].case.msg)
    rows, _, pairs = om.overlap(P, P)
    s = render.overlap_scores(rows, pairs)
    assert s["asa"] == 1.0 and s["ue"] == 0.0 and s["n"] == P.size
    rows, _, pairs = om.overlap(P, np.full(P.shape, -1, np.int32))
    s = render.overlap_scores(rows, pairs)
    assert s == {"n": 0, "asa_sum": 0, "ue_sum": 0, "asa": None, "ue": None}
