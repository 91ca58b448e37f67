"""edge_list_cases.py on the CPU: the expected list equals the definition (a plain loop), a tiled
counting sort built the right way equals it too, built in each of the wrong ways it does not, and every
input does what tests/test_gpu_edge_lists.py has it for."""
import numpy as np
import pytest

import edge_list_cases as lc

BY_NAME = {c[0]: c for c in lc.CASES}
SMALL_CASES = [c for c in lc.CASES if c[1] * c[2] <= 4096]


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_case_names_are_unique():
    assert len(BY_NAME) == len(lc.CASES)


@pytest.mark.parametrize("case", SMALL_CASES, ids=lc.case_id)
def test_expected_list_equals_the_loop(case):
    for index, planes in lc.oracle_planes(case).items():
        want = lc.loop_list(planes)
        got = lc.expected_lists(case)[index]
        assert got[0].dtype == np.uint32 and got[1].dtype == np.int32 and got[1].size == lc.NUM_OFFSETS
        assert _same(got, want), "list %d" % index
        assert got[1][-1] == got[0].size == int((planes != lc.ABSENT).sum())
        assert lc.slot_keys(planes)[got[0]].tolist() == sorted(lc.slot_keys(planes)[got[0]].tolist())


@pytest.mark.parametrize("name", ["3x683-l2-flow", "flat", "ramp", "alternating", "virtual-flow", "second-frame"])
def test_tiled_sort_equals_the_expected_list(name):
    case = BY_NAME[name]
    for index, planes in lc.oracle_planes(case).items():
        assert _same(lc.tiled_list(planes), lc.expected_lists(case)[index]), "list %d" % index


def test_broken_models_differ():
    case = BY_NAME["second-frame"]          # 2310 pixels of noise: two spatial tiles, three temporal ones
    for index in (0, 1):
        planes = lc.oracle_planes(case)[index]
        want = lc.expected_lists(case)[index]
        keys = lc.slot_keys(planes)
        # stable inside a tile only: the offsets are right, the order inside a bucket is not
        got = lc.tiled_list(planes, tile_order="descending")
        assert np.array_equal(got[1], want[1]) and not np.array_equal(got[0], want[0])
        assert np.array_equal(np.sort(got[0]), np.sort(want[0]))
        # a tile boundary shifted by one slot: the slot that changes tile takes the place of the next
        # one with its key in the tile it left (two buckets: there always is one)
        dense = lc.oracle_planes(BY_NAME["alternating"])[index]
        got = lc.tiled_list(dense, scatter_shift=1)
        want_dense = lc.expected_lists(BY_NAME["alternating"])[index]
        assert np.array_equal(got[1], want_dense[1]) and not np.array_equal(got[0], want_dense[0])
        # an edge that does not exist listed
        assert (keys == lc.ABSENT).any()
        got = lc.tiled_list(planes, list_absent=True)
        assert got[0].size == keys.size > want[0].size and got[1][-1] != want[1][-1]
        # two buckets exchanged (both in use, of different sizes)
        used = np.nonzero(np.diff(want[1]))[0]
        a, b = int(used[0]), int(used[-1])
        assert a != b
        got = lc.tiled_list(planes, swap_bins=(a, b))
        assert not np.array_equal(got[0], want[0])


def test_single_tile_cases_cannot_show_the_tile_faults():
    planes = lc.oracle_planes(BY_NAME["2x512-l2-flow"])[0]       # 1024 pixels: one tile
    assert _same(lc.tiled_list(planes, tile_order="descending"), lc.expected_list(planes))


def test_sizes_cover_the_tile_edges():
    px = {c[1] * c[2] for c in lc.CASES}
    assert {1024, 1025, 2048, 2049} <= px
    assert any(c[1] == 2 for c in lc.CASES) and any(c[2] == 1 for c in lc.CASES)
    W, H = lc.BIG
    assert (W * H + lc.TILE_PX[9] - 1) // lc.TILE_PX[9] > 768
    W, H = lc.SMALL
    assert W * H > lc.TILE_PX[4] and (W * H) % lc.TILE_PX[9] and (W * H) % 64


def test_flat_case_has_one_bucket():
    for index, (slots, offsets) in lc.expected_lists(BY_NAME["flat"]).items():
        assert offsets[1] == slots.size > 0, "list %d" % index


def test_ramp_case_has_64_distinct_keys_in_a_step():
    planes = lc.oracle_planes(BY_NAME["ramp"])[1]
    keys = lc.slot_keys(planes)
    steps = keys[:keys.size // 64 * 64].reshape(-1, 64)
    distinct = np.array([np.unique(s).size for s in steps])
    full = np.array([(s != lc.ABSENT).all() for s in steps])
    assert full.sum() > steps.shape[0] // 2
    assert (distinct[full] == 64).all()


def test_alternating_case_has_two_buckets_that_alternate():
    planes = lc.oracle_planes(BY_NAME["alternating"])[0]
    keys = lc.slot_keys(planes)
    present = np.unique(keys[keys != lc.ABSENT])
    assert present.size == 2 and present[0] == 0
    W, H = lc.SMALL
    inner = keys.reshape(H, W, 4)[1:-1, 1:-1]
    assert (inner[..., 0] == present[1]).all() and (inner[..., 1] == present[1]).all()
    assert (inner[..., 2] == 0).all() and (inner[..., 3] == 0).all()


@pytest.mark.parametrize("name", ["virtual-flow", "virtual-flow-two-tiles"])
def test_virtual_case_is_all_2048_with_absent_slots_among_them(name):
    planes = lc.oracle_planes(BY_NAME[name])[1]
    assert set(np.unique(planes).tolist()) == {lc.VIRTUAL_BUCKET, lc.ABSENT}
    slots, offsets = lc.expected_lists(BY_NAME[name])[1]
    assert offsets[lc.VIRTUAL_BUCKET] == 0 and offsets[lc.VIRTUAL_BUCKET + 1] == slots.size
    assert (np.diff(slots.astype(np.int64)) > 1).any()       # absent slots between listed ones


def test_border_flows_leave_absent_slots_among_existing_ones():
    planes = lc.oracle_planes(BY_NAME["5x205-l2-flow"])[1]
    keys = lc.slot_keys(planes).reshape(-1, 9)
    mixed = ((keys == lc.ABSENT).any(axis=1) & (keys != lc.ABSENT).any(axis=1))
    assert mixed.sum() > 10


def test_second_frame_differs_from_the_first():
    lists = lc.expected_lists(BY_NAME["second-frame"])
    assert set(lists) == {0, 1, 2, 3, 4}
    assert not np.array_equal(lists[2][1], lists[4][1]) and not np.array_equal(lists[1][1], lists[3][1])
