"""The two definitions of a level's regions in level_regions_model.py against each other, on the cases
the GPU tests use: the reference restated literally (parent map, MergeRasterization fold, area,
ShapeMomentsFromRasterization) and the maximal runs of the id plane.  Bits, not tolerances."""
import numpy as np
import pytest

import level_regions_cases as lc
import level_regions_model as lm
import render_model as rm

CASES = lc.all_cases()


def permutations():
    rng = np.random.RandomState(7)
    yield "reversed", lambda c: c[::-1]
    yield "rotated", lambda c: c[len(c) // 2:] + c[:len(c) // 2]
    yield "shuffled", lambda c: [c[k] for k in rng.permutation(len(c))]


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_literal_and_runs_agree(case):
    hier = rm.hierarchy_of(case.msg)
    for level in case.levels:
        want_r, want_i = lm.runs(lc.id_image(case.msg, level))
        got_r, got_i = lm.literal(case.msg, level, hier)
        assert lm.same_bits(got_i, want_i), (case.name, level)
        assert lm.same_bits(got_r, want_r), (case.name, level)
        assert int(want_r["area"].sum()) == int((lc.id_image(case.msg, level) != -1).sum())
        # the checker's level 1 folds 3 072 children per region: once is enough for it
        if case.name == "checker" and level == 1:
            continue
        for name, order in permutations():
            got_r, got_i = lm.literal(case.msg, level, hier, child_order=order)
            assert lm.same_bits(got_i, want_i) and lm.same_bits(got_r, want_r), (case.name, level, name)


def test_every_case_serializes_and_parses_back():
    """The GPU tests hand the library the serialized message: every required field has to be set."""
    for m in [c.msg for c in CASES] + [lc.touching_counter_example()]:
        back = lc.Msg()
        back.ParseFromString(m.SerializeToString())
        assert back == m


def test_expected_counts_of_the_named_cases():
    by_name = {c.name: c for c in CASES}
    c = by_name["checker"]
    r0, i0 = lm.runs(lc.id_image(c.msg, 0))
    r1, i1 = lm.runs(lc.id_image(c.msg, 1))
    assert len(r0) == 6144 and len(i0) == 6144
    assert len(r1) == 2 and r1["num_intervals"].tolist() == [3072, 3072] and len(i1) == 6144
    r, i = lm.runs(lc.id_image(by_name["one_region_9x5"].msg, 0))
    assert len(r) == 1 and i.tolist() == [[y, 0, 8, 3] for y in range(5)]     # a run ends with its row
    r, i = lm.runs(lc.id_image(by_name["uncovered_frame"].msg, 0))
    assert len(r) == 0 and i.shape == (0, 4)
    r, i = lm.runs(lc.id_image(by_name["boundary_1025x5"].msg, 0))
    assert [1, 0, 1024, 7] in i.tolist()
    t = by_name["three_levels"]
    counts = [len(lm.runs(lc.id_image(t.msg, level))[0]) for level in (0, 1, 2)]
    assert counts == [48, 20, 3]
    r2, i2 = lm.runs(lc.id_image(t.msg, 2))
    assert (i2[:, 1] == 0).all() and (i2[:, 2] == 63).all()                    # children adjacent in a row merge
    r1, _ = lm.runs(lc.id_image(t.msg, 1))
    assert r1["num_intervals"].max() == 16 and r1["id"].max() > (1 << 30) - 60


def test_the_order_of_the_sums_shows_in_the_bits():
    c = {c.name: c for c in CASES}["moments"]
    regions, intervals = lm.runs(lc.id_image(c.msg, 0))
    assert len(regions) == 2 and (intervals[:, 1] >= 3000).all() and regions["num_intervals"].max() >= 1680
    back = lm.reversed_moments(regions, intervals)
    changed = [f for f in lm.FLOAT_FIELDS if regions[f].view(np.uint32).tolist() != back[f].view(np.uint32).tolist()]
    assert changed, "summing in reverse order gives the same bits: the comparison would prove nothing"
    assert "size" not in changed


def test_touching_intervals_inside_one_region_are_where_the_two_differ():
    """The header's statement: with touching intervals inside one region the reference's result
    depends on which rows a second child shares; the library returns the maximal runs."""
    m = lc.touching_counter_example()
    hier = rm.hierarchy_of(m)
    lit_r, lit_i = lm.literal(m, 1, hier)
    run_r, run_i = lm.runs(lc.id_image(m, 1))
    assert lit_i.tolist() == [[0, 0, 3, 9], [0, 4, 7, 9], [1, 2, 5, 9]]
    assert run_i.tolist() == [[0, 0, 7, 9], [1, 2, 5, 9]]
    assert lit_r["area"].tolist() == run_r["area"].tolist() == [12]
    # a second child in that row makes the reference join them
    extra = m.region.add()
    extra.id = 7
    s = extra.raster.scan_inter.add()
    s.y, s.left_x, s.right_x = 0, 9, 9
    m.frame_width = 10
    lc.add_hierarchy(m, [{5: 9, 6: 9, 7: 9}])
    lit_r, lit_i = lm.literal(m, 1, rm.hierarchy_of(m))
    assert lit_i.tolist() == [[0, 0, 7, 9], [0, 9, 9, 9], [1, 2, 5, 9]]
    assert lm.same_bits(lit_i, lm.runs(lc.id_image(m, 1))[1])
