"""volume_model.py, the numpy model the volume session tests compare the product with: against a loop over the
voxels that walks the definition, against the field-wise sum over the frames of the per-frame models
(level_regions_model, level_colors_model, level_overlap_model), and its documented identities.  Needs no device."""
import numpy as np
import pytest

import level_colors_model as km
import level_overlap_model as om
import level_regions_model as lm
import volume_cases as vcs
import volume_model as vm

SMALL = vcs.small()
ALL = vcs.all_sequences()
FLAGS = ((True, True), (True, False), (False, True), (False, False))


def test_layouts():
    for dtype, offsets, size in ((vm.ROW_DTYPE, vm.ROW_OFFSETS, 152), (vm.COL_DTYPE, vm.COL_OFFSETS, 48),
                                 (vm.PAIR_DTYPE, vm.PAIR_OFFSETS, 24)):
        assert dtype.itemsize == size
        assert {n: dtype.fields[n][1] for n in dtype.names} == offsets


@pytest.mark.parametrize("s", SMALL, ids=lambda s: s.name)
def test_model_equals_the_voxel_loop(s):
    for colors, labels in FLAGS:
        for upto in range(len(s.adds) + 1):
            adds = vcs.model_adds(s, upto)
            assert vm.same_tables(vm.volume(adds, colors, labels), vm.volume_literal(adds, colors, labels)), \
                (s.name, colors, labels, upto)


def summed(adds):
    """The table as the sum over the adds of the per-frame tables, merged in dictionaries: what a caller had to do
    on the host before there was a session."""
    R, Cl, Pr = {}, {}, {}
    for k, (frame, P, F, B) in enumerate(adds):
        regions, _ = lm.runs(P)
        colors = km.colors(P, F)
        rows, cols, pairs = om.overlap(P, B)
        assert np.array_equal(regions["id"], colors["id"]) and np.array_equal(regions["id"], rows["id"])
        ys, lx, rx, rid = lm.runs_of(P)
        for reg, col, row in zip(regions, colors, rows):
            mine = rid == reg["id"]
            length = (rx[mine] - lx[mine] + 1).astype(np.int64)
            r = R.setdefault(int(reg["id"]), np.zeros((), vm.ROW_DTYPE))
            if r["frames"] == 0:
                r["id"], r["first_frame"], r["last_frame"] = reg["id"], frame, frame
                r["min_x"], r["min_y"], r["max_x"], r["max_y"] = reg["min_x"], reg["min_y"], reg["max_x"], reg["max_y"]
                r["min"], r["max"] = col["min"], col["max"]
            r["first_frame"], r["last_frame"] = min(r["first_frame"], frame), max(r["last_frame"], frame)
            r["frames"] += 1
            for lo, hi in (("min_x", "max_x"), ("min_y", "max_y"), ("min", "max")):
                src = reg if lo != "min" else col
                r[lo], r[hi] = np.minimum(r[lo], src[lo]), np.maximum(r[hi], src[hi])
            r["volume"] += int(reg["area"])
            r["unlabelled"] += int(row["unlabelled"])
            r["sum_x"] += int(((lx[mine] + rx[mine]).astype(np.int64) * length // 2).sum())
            r["sum_y"] += int((ys[mine].astype(np.int64) * length).sum())
            r["sum_t"] += int(frame) * int(reg["area"])
            r["sum"] += col["sum"]
            r["sum_sq"] += col["sum_sq"]
        for c in cols:
            out = Cl.setdefault(int(c["label"]), np.zeros((), vm.COL_DTYPE))
            if out["frames"] == 0:
                out["label"], out["first_frame"], out["last_frame"] = c["label"], frame, frame
            out["first_frame"], out["last_frame"] = min(out["first_frame"], frame), max(out["last_frame"], frame)
            out["frames"] += 1
            out["volume"] += int(c["area"])
            out["uncovered"] += int(c["uncovered"])
        for p in pairs:
            key = (int(rows[p["row"]]["id"]), int(p["label"]))
            out = Pr.setdefault(key, np.zeros((), vm.PAIR_DTYPE))
            out["label"] = p["label"]
            out["frames"] += 1
            out["count"] += int(p["count"])
    ids, labs = sorted(R), sorted(Cl)
    rows = np.array([R[i] for i in ids], vm.ROW_DTYPE).reshape(-1)
    cols = np.array([Cl[l] for l in labs], vm.COL_DTYPE).reshape(-1)
    pairs = np.array([Pr[k] for k in sorted(Pr)], vm.PAIR_DTYPE).reshape(-1)
    rows["best_label"], cols["best_row"] = -1, -1
    for e, (g, l) in enumerate(sorted(Pr)):
        pairs[e]["row"], pairs[e]["col"] = ids.index(g), labs.index(l)
    for i in range(len(rows)):
        mine = np.flatnonzero(pairs["row"] == i)
        rows[i]["first_pair"] = int((pairs["row"] < i).sum())
        rows[i]["num_pairs"] = len(mine)
        if len(mine):
            best = max(mine, key=lambda e: (int(pairs[e]["count"]), -int(pairs[e]["label"])))
            rows[i]["best_label"], rows[i]["best_count"] = pairs[best]["label"], pairs[best]["count"]
    for j in range(len(cols)):
        mine = np.flatnonzero(pairs["col"] == j)
        cols[j]["num_pairs"] = len(mine)
        if len(mine):
            best = max(mine, key=lambda e: (int(pairs[e]["count"]), -int(pairs[e]["row"])))
            cols[j]["best_row"], cols[j]["best_count"] = pairs[best]["row"], pairs[best]["count"]
    return rows, cols, pairs


@pytest.mark.parametrize("s", [s for s in ALL if s.name != "widths"], ids=lambda s: s.name)
def test_model_equals_the_sum_of_the_per_frame_models(s):
    for upto in range(1, len(s.adds) + 1):
        adds = vcs.model_adds(s, upto)
        assert vm.same_tables(vm.volume(adds), summed(adds)), (s.name, upto)


@pytest.mark.parametrize("s", ALL, ids=lambda s: s.name)
def test_identities(s):
    rows, cols, pairs = vm.volume(vcs.model_adds(s))
    assert np.array_equal(np.sort(rows["id"]), rows["id"]) and len(np.unique(rows["id"])) == len(rows)
    assert np.array_equal(np.sort(cols["label"]), cols["label"]) and len(np.unique(cols["label"])) == len(cols)
    per_row = np.bincount(pairs["row"], weights=pairs["count"], minlength=len(rows)).astype(np.int64)
    per_col = np.bincount(pairs["col"], weights=pairs["count"], minlength=len(cols)).astype(np.int64)
    assert np.array_equal(rows["volume"] - rows["unlabelled"], per_row)
    assert np.array_equal(cols["volume"] - cols["uncovered"], per_col)
    assert np.array_equal(cols["label"][pairs["col"]], pairs["label"])
    key = pairs["row"].astype(np.int64) << 32 | pairs["label"]
    assert (np.diff(key) > 0).all()
    assert (rows["frames"] >= 1).all() and (rows["first_frame"] <= rows["last_frame"]).all()
    assert (pairs["frames"] <= rows["frames"][pairs["row"]]).all()
    assert (pairs["frames"] <= cols["frames"][pairs["col"]]).all()


def test_defaults_without_labels_and_without_colours():
    s = vcs.search_edges()
    adds = vcs.model_adds(s)
    full = vm.volume(adds)
    rows, cols, pairs = vm.volume(adds, colors=True, labels=False)
    assert len(cols) == 0 and len(pairs) == 0
    assert not rows["unlabelled"].any() and not rows["best_count"].any() and (rows["best_label"] == -1).all()
    assert not rows["first_pair"].any() and not rows["num_pairs"].any()
    for name in ("id", "volume", "sum_x", "sum_t", "sum", "sum_sq", "min", "max", "frames"):
        assert np.array_equal(rows[name], full[0][name]), name
    rows, cols, pairs = vm.volume(adds, colors=False, labels=True)
    for name in ("sum", "sum_sq", "min", "max"):
        assert not rows[name].any(), name
    assert vm.same_bits(cols, full[1]) and vm.same_bits(pairs, full[2])


def test_life_span_and_sum_t():
    gap, out_of_order, late = vcs.life_span()
    rows = vm.volume(vcs.model_adds(gap))[0]
    three = rows[rows["id"] == 3][0]
    assert (three["first_frame"], three["last_frame"], three["frames"]) == (0, 2, 2)
    rows = vm.volume(vcs.model_adds(out_of_order))[0]
    assert rows["id"].tolist() == [3, 5]
    assert rows["first_frame"].tolist() == [5, 2] and rows["last_frame"].tolist() == [9, 9]
    assert rows["frames"].tolist() == [2, 3]
    rows = vm.volume(vcs.model_adds(late))[0]
    five = rows[rows["id"] == 5][0]
    assert five["sum_t"] == 94 * 7 + 200 * vcs.MAX and five["sum_t"] > 1 << 32
    assert (five["first_frame"], five["last_frame"], five["frames"]) == (7, vcs.MAX, 3)


def test_stats_of_a_steady_sequence_and_of_new_keys():
    s = vcs.search_edges()
    st = [vm.stats_of(vcs.model_adds(s, k)) for k in range(1, 5)]
    assert [x["new_rows"] for x in st] == [3, 4, 0, 8]
    assert [x["new_cols"] for x in st] == [3, 4, 0, 8]
    assert st[2]["new_pairs"] == 0 and st[1]["new_pairs"] > 4 and st[3]["new_pairs"] == 8
    assert st[3]["frames"] == 4 and st[3]["covered"] == 4 * 32 and st[3]["labelled"] == 4 * 32


def test_scores_from_the_table_equal_scores_from_the_voxels():
    from video_segment_amd import render
    for s in SMALL:
        adds = vcs.model_adds(s)
        rows, cols, pairs = vm.volume(adds)
        got = render.volume_scores(rows, cols, pairs)
        n, ue_sum, duration = vm.scores_direct(adds)
        assert (got["n"], got["ue_sum"]) == (n, ue_sum), s.name
        assert got["mean_duration"] == duration and got["supervoxels"] == len(rows)
        assert got["ue_3d"] == (ue_sum / n if n else None)
        if got["sa_3d"] is not None:
            assert 0.0 < got["sa_3d"] <= 1.0
        if got["explained_variation"] is not None:
            assert -1e-9 <= got["explained_variation"] <= 1.0 + 1e-9
    # one supervoxel per label: nothing leaks, every label is recovered
    P = np.array([[1, 1, 2, 2]], np.int32)
    F = np.zeros((1, 4, 3), np.uint8)
    F[0, 2:] = 200
    got = render.volume_scores(*vm.volume([(0, P, F, P + 10), (1, P, F, P + 10)]))
    assert got["ue_3d"] == 0.0 and got["sa_3d"] == 1.0 and got["mean_duration"] == 2.0
    assert abs(got["explained_variation"] - 1.0) < 1e-12
