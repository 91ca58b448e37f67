"""The cases of render_edge_cases.py do what tests/test_gpu_render_edges.py relies on, checked on the model
alone: every seam is there and decides a pixel by itself, the sizes pair every width and height as stated, the
blend has ties of both kinds, the fill cases have the interval lengths and counts they are there for -- and the
byte comparison can fail: five deliberately wrong variants of the model differ from it where they should."""
import numpy as np
import pytest

import render_edge_cases as rc
import render_model as rm

SEAMS = rc.cases_of("seams")
OPTIONS = rc.option_sets()


def case_id(c):
    return c.name


# ---- sizes ---------------------------------------------------------------------------------------------
def test_sizes_pair_every_width_and_height_with_every_residue():
    assert len(OPTIONS) == 21
    assert {w for w, _ in rc.SIZES} == set(rc.WIDTHS) and {h for _, h in rc.SIZES} == set(rc.HEIGHTS)
    for w in rc.WIDTHS:
        assert {h % 4 for (ww, h) in rc.SIZES if ww == w} == {0, 1, 2, 3}, w
    for h in rc.HEIGHTS:
        assert {w % 4 for (w, hh) in rc.SIZES if hh == h} == {0, 1, 2, 3}, h
    assert {(c.W, c.H) for c in SEAMS} == set(rc.SIZES)
    assert {(c.W, c.H) for c in rc.CASES} == set(rc.SIZES)
    print("%d sizes, %d descriptors" % (len(rc.SIZES), len(rc.CASES)))
    for c in rc.CASES:
        assert c.ids.shape == (c.H, c.W) and c.ids.dtype == np.int32
        m, seg = rc.desc(c.name)
        assert (m.frame_width, m.frame_height) == (c.W, c.H) and len(m.hierarchy) == 0
        assert np.array_equal(rc.model_id_image(c.name), c.ids)


def test_seam_lists_are_the_kernels_seams():
    assert (rc.PX, rc.ROWS, rc.GROUP_COLS, rc.GROUP_ROWS) == (4, 4, 64 * 4, 4 * 4)
    cols, rows = rc.column_seams(513), rc.row_seams(18)
    # x-1|x: 4k+2|4k+3, 4k-1|4k, 4k|4k+1, at the first thread's edge and at the workgroup's; the last two columns
    assert [x % 4 for x in cols[:6]] == [3, 0, 1, 3, 0, 1] and rc.GROUP_COLS in cols and cols[-1] == 512
    assert [y % 4 for y in rows[:4]] == [0, 1, 0, 1] and rc.GROUP_ROWS in rows and rows[-1] == 17
    assert rc.column_seams(1) == [] and rc.column_seams(2) == [1] and rc.column_seams(5) == [3, 4]
    assert rc.row_seams(1) == [] and rc.row_seams(3) == [2] and rc.row_seams(17) == [4, 5, 16]


# ---- seams ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SEAMS, ids=case_id)
def test_every_seam_is_there_and_alone(case):
    W, H = case.W, case.H
    ids, cols, rows = rc.seams(W, H)
    assert ids is case.ids
    assert sorted(cols) == sorted(rc.column_seams(W)) and sorted(rows) == sorted(rc.row_seams(H))
    assert rc.hidden(W, H) == []
    plain, marked = rc.filled(case.name), rc.highlighted(case.name)
    assert plain.all(axis=2).any()          # some pixel has no zero byte: blackening is visible in all three
    for x, y in cols.items():
        assert ids[y, x - 1] != ids[y, x]
        assert rc.column_seam_is_alone(ids, y, x)
        assert (plain[y, x - 1] != plain[y, x]).any()
        assert plain[y, x - 1].any() and not marked[y, x - 1].any(), ("col", x, y)
    for y, x in rows.items():
        assert ids[y - 1, x] != ids[y, x]
        assert rc.row_seam_is_alone(ids, y, x)
        assert (plain[y - 1, x] != plain[y, x]).any()
        assert plain[y - 1, x].any() and not marked[y - 1, x].any(), ("row", y, x)
    # without the mark the pixel is no edge pixel: the seam is its only reason
    flat_marked = rm.highlight_edges(rm.fill_colors(rc.lc.desc_from_ids(rc.flat(W, H)), W, H, 0, []))
    assert flat_marked.any(axis=2).all()
    # the seams of a kind sit in different rows (columns) where the frame has twice as many
    if H >= 2 * len(cols):
        assert len(set(cols.values())) == len(cols)
    if W >= 2 * len(rows):
        assert len(set(rows.values())) == len(rows)
    # one region per mark, one for the rest
    assert len(np.unique(ids)) == 1 + len(cols) + len(rows)


def test_last_columns_and_rows_have_a_seam():
    for c in SEAMS:
        ids, cols, rows = rc.seams(c.W, c.H)
        if c.W >= 2:
            assert c.W - 1 in cols and ids[cols[c.W - 1], c.W - 2] != ids[cols[c.W - 1], c.W - 1]
        if c.H >= 2:
            assert c.H - 1 in rows and ids[c.H - 2, rows[c.H - 1]] != ids[c.H - 1, rows[c.H - 1]]
    big = rc.seams(257, 17)
    assert set(big[1]) == {3, 4, 5, 255, 256} and set(big[2]) == {4, 5, 16}
    assert set(rc.seams(513, 18)[1]) == {3, 4, 5, 255, 256, 257, 512} and set(rc.seams(513, 18)[2]) == {4, 5, 16, 17}


# ---- the other families --------------------------------------------------------------------------------
def test_pixels_are_edges_everywhere_but_at_the_last_pixel():
    for c in rc.cases_of("pixels"):
        assert len(np.unique(c.ids)) == c.W * c.H
        plain, marked = rc.filled(c.name), rc.highlighted(c.name)
        black = ~marked.any(axis=2)
        assert not black[-1, -1] and np.array_equal(marked[-1, -1], plain[-1, -1])
        black[-1, -1] = True
        assert black.all(), c.name
    for c in rc.cases_of("checker"):
        assert len(np.unique(c.ids)) == min(2, c.W * c.H)
        black = ~rc.highlighted(c.name).any(axis=2)
        assert black.sum() == c.W * c.H - 1 and not black[-1, -1]


def test_flat_cases_blacken_nothing():
    assert {(c.W % 4, c.H % 4) for c in rc.cases_of("flat")} >= {(1, 1), (1, 3), (1, 2)}
    for c in rc.cases_of("flat"):
        plain = rc.filled(c.name)
        assert plain.all() and np.array_equal(rc.highlighted(c.name), plain)


def test_uncovered_pixels_read_as_colour_0():
    for c in rc.cases_of("uncovered"):
        ids = c.ids
        assert c.W >= 3 and c.H >= 3
        assert ids[0, 0] == -1 and ids[-1, -1] == -1
        assert (ids[:, -1] == -1).all() and (ids[-1, :] == -1).all() and (ids[c.H // 2, :] == -1).all()
        assert (ids[0, 1:-1] != -1).all()
        plain = rc.filled(c.name)
        assert not plain[ids == -1].any() and plain[ids != -1].any(axis=1).all()
        # a covered pixel next to an uncovered one is an edge pixel, an uncovered one next to another is none
        marked = rc.highlighted(c.name)
        assert not marked[c.H // 2 - 1, :-1].any() and not marked[:-1, -2].any()
        assert np.array_equal(rc.model_id_image(c.name), ids)


def test_big_ids_lie_next_to_each_other():
    for c in rc.cases_of("ids"):
        assert set(np.unique(c.ids).tolist()) == set(rc.BIG_IDS)
        pairs = set(zip(c.ids[:, :-1].ravel().tolist(), c.ids[:, 1:].ravel().tolist()))
        assert {(0, 1), (1, (1 << 30) + 7), ((1 << 30) + 7, (1 << 31) - 1), ((1 << 31) - 1, 0)} <= pairs
    colours = [rm.color_of(i) for i in rc.BIG_IDS]
    assert colours[0] == colours[1] and len(set(colours)) == 3      # srand(0) is srand(1)


def test_runs_case_has_the_stated_lengths_and_counts():
    name = "runs_%dx%d" % rc.RUNS_SIZE
    ids = rc.BY_NAME[name].ids
    W = rc.RUNS_SIZE[0]
    assert rc.RUN_LENGTHS == (1, 15, 16, 17, 63, 64, 65, 129) and rc.LONG_INTERVAL == 16
    for r, L in enumerate(rc.RUN_LENGTHS):
        cuts = np.flatnonzero(ids[r, 1:] != ids[r, :-1]) + 1
        lengths = np.diff(np.concatenate([[0], cuts, [W]]))
        assert (lengths[:-1] == L).all() and len(lengths) == -(-W // L), (r, L)
    assert len(np.unique(ids)) == sum(len(np.unique(row)) for row in ids)       # every run a region of its own
    lengths = rc.interval_lengths(name)
    n = len(lengths)
    print("runs: %d intervals" % n)
    assert n % rc.WAVE != 0 and n % rc.FILL_BLOCK != 0 and n > 3 * rc.FILL_BLOCK
    # more than 64 runs of exactly 16 pixels, and whole wavefront batches of them
    assert lengths.count(16) > 64
    assert set(lengths[:2 * rc.WAVE]) == {16}
    # both sides of kLongInterval and of the wavefront in one batch as well
    batches = [set(lengths[k:k + rc.WAVE]) for k in range(0, n, rc.WAVE)]
    assert any(min(b) < 16 <= max(b) for b in batches)
    assert {15, 16, 17, 63, 64, 65, 129, 513} <= set(lengths)


def test_stride_trip_case_needs_a_second_trip():
    c = rc.stride_trip_case()
    assert (c.W, c.H) == (1040, 512) and len(np.unique(c.ids)) == 2
    n = len(rc.interval_lengths(c.name))
    assert n == c.W * c.H == rc.STRIDE_TRIP_INTERVALS == 532480
    assert n > rc.FILL_GRID * rc.FILL_BLOCK == 524288
    assert n % rc.FILL_BLOCK == 0 and (n - rc.FILL_GRID * rc.FILL_BLOCK) // rc.FILL_BLOCK == 32


# ---- the model, from the cached planes ------------------------------------------------------------------
@pytest.mark.parametrize("o", OPTIONS, ids=rc.option_id)
def test_model_render_is_the_render_model(o):
    for c in rc.CASES:
        model = rm.RenderModel(c.W, c.H, **o)
        want = model.render(rc.desc(c.name)[0], rc.frame(c.W, c.H))
        got = rc.model_render(c.name, **o)
        assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), c.name


def test_literal_highlight_loop_agrees_on_every_case():
    for c in rc.CASES:
        plain = rc.filled(c.name)
        assert np.array_equal(rm.highlight_edges_literal(plain), rc.highlighted(c.name)), c.name


def test_blend_has_ties_of_both_kinds():
    """alpha = 0.5: source + colour odd means a tie; round half to even goes down where the floor is even and
    up where it is odd, round half up goes up in both."""
    name = "seams_257x17"
    s = rc.frame(257, 17).astype(np.int32)
    r = rc.highlighted(name).astype(np.int32)
    odd = (s + r) % 2 == 1
    floor = (s + r) // 2
    even_floor = int((odd & (floor % 2 == 0)).sum())
    odd_floor = int((odd & (floor % 2 == 1)).sum())
    print("ties: %d with an even floor, %d with an odd floor of %d bytes" % (even_floor, odd_floor, s.size))
    # 13 107 bytes of seeded noise: a quarter each is expected, 3 277 with a standard deviation of 50
    assert even_floor > 2500 and odd_floor > 2500
    got = rc.model_render(name)
    assert np.array_equal(got[odd & (floor % 2 == 0)], floor[odd & (floor % 2 == 0)])
    assert np.array_equal(got[odd & (floor % 2 == 1)], floor[odd & (floor % 2 == 1)] + 1)
    # 0.25 has ties at a quarter of the sums, 1/3 none that are exact in f32
    for alpha in (0.25, 1.0 / 3.0):
        a = rm.add_weighted(rc.frame(257, 17), rc.highlighted(name), alpha)
        assert not np.array_equal(a, got)


# ---- sensitivity: wrong models differ where they should ---------------------------------------------------
def _edges(plane, last_column_vs_0=False, last_row_vs_0=False, skip_right_of_3=False, skip_below_of_3=False):
    h, w = plane.shape[:2]
    right = np.zeros((h, w), bool)
    right[:, :w - 1] = (plane[:, :w - 1] != plane[:, 1:]).any(axis=2)
    below = np.zeros((h, w), bool)
    below[:h - 1] = (plane[:h - 1] != plane[1:]).any(axis=2)
    if last_column_vs_0:
        right[:, w - 1] = plane[:, w - 1].any(axis=1)
    if last_row_vs_0:
        below[h - 1] = plane[h - 1].any(axis=1)
    if skip_right_of_3:
        right[:, 3::4] = False
    if skip_below_of_3:
        below[3::4] = False
    out = plane.copy()
    out[right | below] = 0
    return out


def _half_up(frame, render, alpha):
    b = np.float32(alpha)
    a = np.float32(1.0) - b
    t = frame.astype(np.float32) * a + render.astype(np.float32) * b
    return np.clip(np.floor(t + np.float32(0.5)), 0, 255).astype(np.uint8)


def wrong_render(variant, name, **o):
    """model_render with one rule broken."""
    c = rc.BY_NAME[name]
    plane = rc.filled(name)
    if o.get("highlight_edges", True):
        plane = _edges(plane, **({variant: True} if variant != "half_up" else {}))
    bgr = rc.frame(c.W, c.H)
    if variant == "half_up" and o.get("has_video", True) and not o.get("concat_with_source", False):
        return _half_up(bgr, plane, o.get("blend_alpha", 0.5))
    return rc.compose(plane, bgr, **o)


def shows_plane(o):
    """Whether anything of the render plane reaches the picture: a blend with alpha 0 is the source frame."""
    return not (o["has_video"] and not o["concat_with_source"] and o["blend_alpha"] == 0.0)


def differs(variant, name, **o):
    return not np.array_equal(wrong_render(variant, name, **o), rc.model_render(name, **o))


def test_the_unbroken_variant_is_the_model():
    for c in rc.CASES:
        assert np.array_equal(_edges(rc.filled(c.name)), rc.highlighted(c.name))
        for o in OPTIONS:
            assert not differs("half_up", c.name, **dict(o, blend_alpha=1.0))      # integers: nothing to round


@pytest.mark.parametrize("variant", ["last_column_vs_0", "last_row_vs_0"])
def test_last_column_or_row_compared_with_colour_0_is_seen(variant):
    hit = 0
    for c in rc.cases_of("flat") + SEAMS:
        for o in OPTIONS:
            want = o["highlight_edges"] and shows_plane(o)         # a covered last pixel turns black
            assert differs(variant, c.name, **o) == want, (c.name, o)
            hit += want
    assert hit >= 11 * (len(SEAMS) + 4)
    # an uncovered last column or row is colour 0 itself
    for c in rc.cases_of("uncovered"):
        assert not differs(variant, c.name)


def test_ignored_right_neighbour_of_column_4k_plus_3_is_seen():
    for c in SEAMS:
        has = any(x % 4 == 0 for x in rc.column_seams(c.W))       # a seam 4k-1|4k
        for o in OPTIONS:
            assert differs("skip_right_of_3", c.name, **o) == (has and o["highlight_edges"] and shows_plane(o)), (c.name, o)
        if has:       # the pixels left of those seams come out unblackened, and only pixels of columns 4k+3 do
            got, want = wrong_render("skip_right_of_3", c.name, has_video=False), rc.model_render(c.name, has_video=False)
            ys, xs = np.nonzero((got != want).any(axis=2))
            cols = rc.seams(c.W, c.H)[1]
            assert {(x - 1, y) for x, y in cols.items() if x % 4 == 0} <= set(zip(xs.tolist(), ys.tolist()))
            assert (xs % 4 == 3).all()
    assert sum(any(x % 4 == 0 for x in rc.column_seams(c.W)) for c in SEAMS) >= 28
    assert differs("skip_right_of_3", "seams_257x17") and differs("skip_right_of_3", "seams_5x3")
    for c in rc.cases_of("flat"):
        for o in OPTIONS:
            assert not differs("skip_right_of_3", c.name, **o)


def test_ignored_row_under_row_4k_plus_3_is_seen():
    for c in SEAMS:
        has = any(y % 4 == 0 for y in rc.row_seams(c.H))
        for o in OPTIONS:
            assert differs("skip_below_of_3", c.name, **o) == (has and o["highlight_edges"] and shows_plane(o)), (c.name, o)
        if has:
            got, want = wrong_render("skip_below_of_3", c.name, has_video=False), rc.model_render(c.name, has_video=False)
            ys, xs = np.nonzero((got != want).any(axis=2))
            rows = rc.seams(c.W, c.H)[2]
            assert {(y - 1, x) for y, x in rows.items() if y % 4 == 0} <= set(zip(ys.tolist(), xs.tolist()))
            assert (ys % 4 == 3).all()
    assert sum(any(y % 4 == 0 for y in rc.row_seams(c.H)) for c in SEAMS) >= 28
    assert differs("skip_below_of_3", "seams_257x17")
    for c in rc.cases_of("flat"):
        for o in OPTIONS:
            assert not differs("skip_below_of_3", c.name, **o)


def test_blend_rounded_half_up_is_seen():
    for c in rc.CASES:
        big = c.W * c.H >= 64       # 192 bytes and more: a quarter are ties that go the other way
        for o in OPTIONS:
            blends = o["has_video"] and not o["concat_with_source"]
            if not blends or o["blend_alpha"] in (1.0, 0.0):
                assert not differs("half_up", c.name, **o), (c.name, o)
            elif o["blend_alpha"] == 0.5 and big:
                assert differs("half_up", c.name, **o), (c.name, o)
    for c in rc.cases_of("flat"):
        assert not differs("half_up", c.name, has_video=False, highlight_edges=True)
        assert not differs("half_up", c.name, concat_with_source=True)
    assert differs("half_up", "flat_257x17") and differs("half_up", "seams_257x17")
