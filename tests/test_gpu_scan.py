"""The fused device-wide scan of the merge path (csrc/scan_device.h: FusedScan, ExclusiveSum,
RunsOfSortedKeys) against numpy in int64, through the test hooks vsg_debug_exclusive_sum (a FusedScan
whose finish() stores the total) and vsg_debug_runs_of_sorted_keys.  Everything is an integer: the
comparison is array_equal.

Sizes from the kernels' constants: 64 lanes, 256 threads x 8 items = 2048 elements per sub-tile, the
second trip of the sum over the tile sums from 256 tiles on, and `chunks` sub-tiles per workgroup once
there are more than 2048 tiles -- above 2048 * 2048 elements, which no suite-sized frame reaches in a
stage: 2048 * 2048 + 1 is the first chunks = 2 launch (its last workgroup holds one element and breaks
at its second sub-tile), 2 * 2048 * 2048 + 1 the first with chunks = 4."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import vsg  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

SUB = 2048                 # kScanSub: 256 threads x 8 items
FULL = SUB * 2048          # the largest launch with one sub-tile per workgroup
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, SUB - 1, SUB, SUB + 1, 2 * SUB, 2 * SUB + 1,
         SUB * 256 - 1, SUB * 256, SUB * 256 + 1, FULL - 1, FULL, FULL + 1, 2 * FULL + 1]
FILL = -0x5A5A5A5B


def chunks_of(n):
    """The launcher's choice (FusedScan): sub-tiles per workgroup."""
    tiles = (n + SUB - 1) // SUB
    chunks = 1
    while (tiles + chunks - 1) // chunks > 2048:
        chunks *= 2
    return chunks


def test_sizes_cover_the_launcher_paths():
    assert [chunks_of(n) for n in (FULL - 1, FULL, FULL + 1, 2 * FULL, 2 * FULL + 1)] == [1, 1, 2, 2, 4]
    assert max(SIZES) * 200 < 2 ** 31   # random values in [0, 200] keep every prefix inside int32


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def exclusive_sum(vsg, a, in_place=False):  # noqa: F811
    from video_segment_amd._lib import check, lib
    a = np.ascontiguousarray(a, np.int32)
    src = a.copy()
    out = src if in_place else np.full(len(a), FILL, np.int32)
    total = C.c_int64(FILL)
    check(lib().vsg_debug_exclusive_sum(ptr(src), len(a), ptr(out), C.byref(total)))
    if not in_place:
        assert np.array_equal(src, a), "the input was written"
    return out, total.value


def check_sum(vsg, a, what, in_place=False):  # noqa: F811
    a = np.ascontiguousarray(a, np.int32)
    incl = np.cumsum(a, dtype=np.int64)
    ref = incl - a                      # the inclusive sums shifted by one element
    assert incl[-1] < 2 ** 31, "the reference has to stay inside int32"
    out, total = exclusive_sum(vsg, a, in_place)
    bad = np.flatnonzero(out.astype(np.int64) != ref)
    assert bad.size == 0, "%s, n=%d%s: %d prefixes differ, first at %d (sub-tile %d, element %d of it): %d != %d" % (
        what, len(a), " in place" if in_place else "", bad.size, bad[0], bad[0] // SUB, bad[0] % SUB, out[bad[0]],
        ref[bad[0]])
    assert total == incl[-1], "%s, n=%d: finish() got %d, the sum is %d" % (what, len(a), total, incl[-1])


def single(n, at):
    a = np.zeros(n, np.int32)
    a[at] = 7
    return a


@pytest.mark.parametrize("n", SIZES)
def test_exclusive_sum(vsg, n):  # noqa: F811
    rng = np.random.default_rng([n, 1])
    last_sub = (n - 1) // SUB * SUB                      # first element of the last sub-tile
    last_tile = (n - 1) // (SUB * chunks_of(n)) * (SUB * chunks_of(n))   # ... of the last workgroup's tile
    check_sum(vsg, np.zeros(n, np.int32), "all zero")
    check_sum(vsg, np.ones(n, np.int32), "all one")
    check_sum(vsg, rng.random(n) < 0.5, "flags, density 1/2")
    check_sum(vsg, rng.random(n) < 1.0 / 4096, "flags, density 1/4096")
    values = rng.integers(0, 201, n, dtype=np.int32)
    check_sum(vsg, values, "values in [0, 200]")
    check_sum(vsg, values, "values in [0, 200]", in_place=True)
    check_sum(vsg, single(n, 0), "one non-zero, the first")
    check_sum(vsg, single(n, n - 1), "one non-zero, the last")
    check_sum(vsg, single(n, last_sub), "one non-zero, first of the last sub-tile")
    check_sum(vsg, single(n, last_tile), "one non-zero, first of the last tile")


def test_exclusive_sum_of_nothing_launches_nothing(vsg):  # noqa: F811
    from video_segment_amd._lib import check, lib
    src = np.array([5, 6], np.int32)
    out = np.full(4, FILL, np.int32)
    total = C.c_int64(FILL)
    check(lib().vsg_debug_exclusive_sum(ptr(src), 0, ptr(out), C.byref(total)))
    assert (out == FILL).all() and total.value == FILL
    assert lib().vsg_debug_exclusive_sum(ptr(src), -1, ptr(out), C.byref(total)) == -1   # VSG_ERR_INVALID


def check_runs(vsg, keys, what):  # noqa: F811
    from video_segment_amd._lib import check, lib
    keys = np.ascontiguousarray(keys, np.uint32)
    n = len(keys)
    assert (np.diff(keys.astype(np.int64)) >= 0).all(), "the test's keys have to be sorted"
    heads = np.concatenate(([0], np.flatnonzero(np.diff(keys.astype(np.int64))) + 1)).astype(np.int64)
    counts = np.diff(np.concatenate((heads, [n])))
    src = keys.copy()
    seg_off = np.full(n, FILL, np.int32)
    seg_cnt = np.full(n, FILL, np.int32)
    num = C.c_int32(FILL)
    check(lib().vsg_debug_runs_of_sorted_keys(ptr(src), n, ptr(seg_off), ptr(seg_cnt), C.byref(num)))
    assert np.array_equal(src, keys), "the keys were written"
    r = len(heads)
    assert num.value == r, "%s, n=%d: %d runs, expected %d" % (what, n, num.value, r)
    bad = np.flatnonzero(seg_off[:r].astype(np.int64) != heads)
    assert bad.size == 0, "%s, n=%d: %d run starts differ, first run %d: %d != %d" % (
        what, n, bad.size, bad[0], seg_off[bad[0]], heads[bad[0]])
    assert np.array_equal(seg_cnt[:r].astype(np.int64), counts), "%s, n=%d: run lengths differ" % (what, n)
    assert int(seg_cnt[:r].astype(np.int64).sum()) == n
    assert (seg_off[r:] == FILL).all() and (seg_cnt[r:] == FILL).all(), \
        "%s, n=%d: slots past the last run were written" % (what, n)


def keys_with_heads(n, heads):
    """Sorted keys whose runs start at `heads` (and at 0); the upper half of the runs has bit 31 set."""
    flags = np.zeros(n, np.int64)
    hs = np.unique(np.asarray(heads, np.int64))
    hs = hs[(hs > 0) & (hs < n)]
    flags[hs] = 1
    run = np.cumsum(flags)
    base = 2 ** 31 - 3 * ((len(hs) + 1) // 2)
    keys = base + 3 * run
    assert keys[-1] < 2 ** 32 and keys[0] >= 0
    return keys.astype(np.uint32)


@pytest.mark.parametrize("n", SIZES)
def test_runs_of_sorted_keys(vsg, n):  # noqa: F811
    rng = np.random.default_rng([n, 2])
    tile = SUB * chunks_of(n)
    check_runs(vsg, np.full(n, 0x80000005, np.uint32), "one run")
    check_runs(vsg, (np.arange(n, dtype=np.int64) + (2 ** 31 - n // 2)).astype(np.uint32), "n runs")
    # heads on the first and the last element of a sub-tile, of a workgroup's tile (chunks sub-tiles), of
    # the last ones, and on the last element
    edges = []
    for unit in (SUB, tile, 4 * SUB):
        last = (n - 1) // unit * unit
        for start in (unit, 3 * unit, last):
            edges += [start - 1, start, start + unit - 1]
    edges += [1, 63, 64, 255, 256, n - 1]
    check_runs(vsg, keys_with_heads(n, edges), "heads at sub-tile and tile edges")
    # runs that span whole sub-tiles / tiles: from the last element of one to the second of the one after next
    span = []
    for unit in (SUB, tile):
        span += [unit - 1, 2 * unit + 1, 4 * unit - 1, 7 * unit + 1]
    check_runs(vsg, keys_with_heads(n, span), "runs across whole tiles")
    check_runs(vsg, keys_with_heads(n, np.flatnonzero(rng.random(n) < 0.3)), "random runs, mean length 3")
    check_runs(vsg, keys_with_heads(n, np.flatnonzero(rng.random(n) < 1.0 / 4096)), "random long runs")


def test_runs_of_nothing_launches_nothing(vsg):  # noqa: F811
    from video_segment_amd._lib import check, lib
    keys = np.array([1, 2], np.uint32)
    seg_off = np.full(4, FILL, np.int32)
    seg_cnt = np.full(4, FILL, np.int32)
    num = C.c_int32(FILL)
    check(lib().vsg_debug_runs_of_sorted_keys(ptr(keys), 0, ptr(seg_off), ptr(seg_cnt), C.byref(num)))
    assert (seg_off == FILL).all() and (seg_cnt == FILL).all() and num.value == FILL
