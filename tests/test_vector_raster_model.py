"""The numpy model of the reference's polygon scan conversion (vector_raster_model.py) on hand-made
descs whose intervals can be worked out with pencil and paper, and the round trip through the
product's own vectorization where the boundary simplification changes nothing."""
import numpy as np
import pytest

import vector_cases as vc
import vector_raster_model as vm

F = np.float32


def rows_of(msg, W=None, H=None):
    rows, unspecified = vm.rasterize_desc(msg, W, H)
    assert unspecified == 0
    return [tuple(int(v) for v in r) for r in rows]


def test_rectangle_gives_its_exact_rows():
    m = vc.make_desc(12, 9, [(5, [vc.rect(2, 3, 7, 6)])])
    assert rows_of(m) == [(3, 2, 6, 5), (4, 2, 6, 5), (5, 2, 6, 5)]
    # the other orientation has its left and right edges swapped in name only
    m = vc.make_desc(12, 9, [(5, [vc.rect(2, 3, 7, 6)[::-1]])])
    assert rows_of(m) == [(3, 2, 6, 5), (4, 2, 6, 5), (5, 2, 6, 5)]


def test_triangle_with_an_integer_apex_has_an_empty_first_interval():
    m = vc.make_desc(10, 8, [(1, [[(5, 2), (8, 6), (2, 6), (5, 2)]])])
    got = rows_of(m)
    assert got[0] == (2, 5, 4, 1)                   # left_x = right_x + 1: emitted, paints nothing
    # rows below: x = 5 -+ 0.75 k, left end rounded up, right end rounded down
    assert got[1:] == [(3, 5, 5, 1), (4, 4, 6, 1), (5, 3, 7, 1)]
    assert (vm.id_plane(np.asarray(got), 10, 8) == 1).sum() == 1 + 3 + 5


def test_polygon_with_a_hole():
    m = vc.make_desc(10, 9, [(2, [vc.rect(1, 1, 9, 8), vc.rect(3, 3, 6, 5)[::-1]])])
    m.region[0].vectorization.polygon[1].hole = True
    got = rows_of(m)
    want = []
    for y in range(1, 8):
        want += [(y, 1, 2, 2), (y, 6, 8, 2)] if y in (3, 4) else [(y, 1, 8, 2)]
    assert got == want


def test_region_without_polygons_has_no_intervals():
    m = vc.make_desc(8, 8, [(1, []), (2, [vc.rect(0, 0, 3, 2)]), (3, [])])
    assert rows_of(m) == [(0, 0, 2, 2), (1, 0, 2, 2)]


def test_right_edge_on_an_integer_is_exclusive_and_the_frame_edge_gives_w_minus_1():
    W, H = 7, 3
    assert rows_of(vc.make_desc(W, H, [(1, [vc.rect(0, 0, 4, 3)])])) == [(y, 0, 3, 1) for y in range(3)]
    assert rows_of(vc.make_desc(W, H, [(1, [vc.rect(0, 0, W, H)])])) == [(y, 0, W - 1, 1) for y in range(3)]
    # a right edge a hair past the integer includes that pixel column's left neighbour only
    assert rows_of(vc.make_desc(W, H, [(1, [vc.rect(0, 0, 4.5, 1)])])) == [(0, 0, 4, 1)]
    # an apex on the right frame edge: the empty interval there does not leave the row
    got, unspecified = vm.rasterize_desc(vc.make_desc(W, H, [(1, [[(W, 0), (W, 3), (W - 3, 3), (W, 0)]])]))
    assert unspecified == 0 and tuple(got[0]) == (0, W, W - 1, 1)


def test_pinch_vertex():
    assert rows_of(vc.hourglass()) == [(2, 2, 7, 3), (3, 3, 6, 3), (4, 4, 5, 3), (5, 5, 4, 3), (6, 4, 5, 3),
                                       (7, 3, 6, 3)]


def test_comb_with_40_teeth_has_80_crossings_in_a_row_in_order():
    got = rows_of(vc.comb(40))
    want = [(y, 2 * k, 2 * k, 7) for y in (0, 1) for k in range(40)] + [(2, 0, 78, 7)]
    assert got == want
    assert sum(1 for r in got if r[0] == 0) * 2 == 80


@pytest.mark.parametrize("size", [(96, 72), (100, 75)])
def test_scaling_matches_the_literal_loop(size):
    W, H = size
    rng = np.random.default_rng(3)
    coord = rng.integers(0, 49, 41).astype(F)      # odd length: the parity counter, not the index pairs
    coord[::2] = rng.integers(0, 65, 21)
    got = vm.scale_vectorization(coord, 64, 48, W, H)
    sx = F(W) * (F(1) / F(64))
    sy = F(H) * (F(1) / F(48))
    want = coord.copy()
    want[0::2] = np.minimum(F(W), coord[0::2] * sx)
    want[1::2] = np.minimum(F(H), coord[1::2] * sy)
    assert got.dtype == F and np.array_equal(got, want)
    assert got[0::2].max() <= W and got[1::2].max() <= H
    # a rectangle through the scaling: fractional y truncates to the row of insertion, x keeps p1.x
    m = vc.make_desc(64, 48, [(1, [vc.rect(2, 3, 7, 6)])])
    fx, fy = W / 64.0, H / 48.0
    y0, y1 = int(3 * fy), int(np.floor(6 * fy))
    lx, rx = int(np.ceil(2 * fx)), int(np.floor(7 * fx))
    if rx == 7 * fx:
        rx -= 1
    assert rows_of(m, W, H) == [(y, lx, rx, 1) for y in range(y0, y1)]


def test_bow_tie_with_three_crossings_inside_eps_is_unspecified():
    m = vc.bow_tie()
    rows, unspecified = vm.rasterize_desc(m)
    assert unspecified == 1
    # without the sliver the two diagonals tie at (5, 2) and the row is defined: left before right
    tie_only = vc.make_desc(10, 4, [(1, [[(4, 0), (6, 0), (4, 4), (6, 4), (4, 0)]])])
    assert vm.rasterize_desc(tie_only)[1] == 0


def test_other_rows_the_reference_does_not_define():
    # odd active count: an open polyline
    m = vc.make_desc(8, 8, [(1, [[(2, 1), (2, 5), (6, 5)]])])
    assert vm.rasterize_desc(m)[1] == 4
    # an interval that leaves the row
    m = vc.make_desc(8, 8, [(1, [vc.rect(2, 1, 9, 3)])])
    assert vm.rasterize_desc(m)[1] == 2
    # two crossings the comparator cannot tell apart at different x
    m = vc.make_desc(8, 2, [(1, [[(2, 0), (2, 2)], [(2.0005, 0), (2.0005, 2)]])])
    assert vm.rasterize_desc(m)[1] == 2


@pytest.fixture(scope="module")
def product():
    from video_segment_amd import _lib
    try:
        _lib.lib()
    except (OSError, RuntimeError) as e:    # the shared library is missing or cannot be loaded
        pytest.skip("libvsg_hip.so cannot be loaded: %s" % e)
    return vc


@pytest.mark.parametrize("case", ["blocks0", "blocks1", "hole", "nested", "four_corner", "diagonal_touch"])
def test_round_trip_through_the_products_vectorization(product, case):
    """Axis-aligned boundaries: simplification changes nothing, so rasterizing the vectorization of
    an id image gives the id image back exactly."""
    from test_boundary import CASES
    ids = vc.block_partition(int(case[-1]), 37, 23) if case.startswith("blocks") else CASES[case]
    H, W = ids.shape
    m = vc.vector_only(ids)
    assert all(len(r.raster.scan_inter) == 0 for r in m.region) and m.rasterization_removed
    rows, unspecified = vm.rasterize_desc(m)
    assert unspecified == 0
    assert np.array_equal(vm.id_plane(rows, W, H), ids)
