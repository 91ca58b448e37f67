"""The edge lists of a graph as edge_sort.hip has to build them, and the inputs of
tests/test_gpu_edge_lists.py.

A list is the stable counting sort of a frame's edge slots (slot = pix * 4 + k for the spatial list,
pix * 9 + k for the temporal one) by their bucket: `slots` holds the ids of the existing edges, in
ascending order inside every bucket, `offsets[b]` (2050 entries) the start of bucket b --
offsets[2048] the virtual edges, offsets[2049] the end of the list.  The expected list is derived from
the oracle's bucket planes (oracle_lib.spatial_buckets / temporal_buckets: [k][y][x], 0xFFFF where the
edge does not exist).  test_edge_list_cases.py checks the model and the cases on the CPU."""
import functools

import numpy as np

import edge_shape_cases as ec
import oracle_lib as ol

ABSENT = 0xFFFF
NUM_OFFSETS = 2050
VIRTUAL_BUCKET = 2048
TILE_PX = {4: 2048, 9: 1024}     # pixels per workgroup of the key and scatter kernels


def slot_keys(planes):
    """[k][y][x] bucket planes -> the key of every slot, in slot order."""
    k = planes.shape[0]
    return np.ascontiguousarray(planes.reshape(k, -1).T).ravel()


def expected_list(planes):
    """(slots u32, offsets i32[2050]) of a list with these bucket planes."""
    keys = slot_keys(planes)
    exists = np.nonzero(keys != ABSENT)[0]
    order = np.argsort(keys[exists], kind="stable")
    counts = np.bincount(keys[exists], minlength=NUM_OFFSETS - 1)
    assert counts.size == NUM_OFFSETS - 1, "a bucket above 2048"
    offsets = np.zeros(NUM_OFFSETS, np.int32)
    offsets[1:] = np.cumsum(counts)
    return exists[order].astype(np.uint32), offsets


def loop_list(planes):
    """The same by the definition: every slot appended to the vector of its bucket, in slot order."""
    keys = slot_keys(planes)
    buckets = [[] for _ in range(NUM_OFFSETS - 1)]
    for slot, key in enumerate(keys.tolist()):
        if key != ABSENT:
            buckets[key].append(slot)
    slots, offsets = [], [0]
    for b in buckets:
        slots += b
        offsets.append(len(slots))
    return np.array(slots, np.uint32), np.array(offsets, np.int32)


def tiled_list(planes, tile_order="ascending", scatter_shift=0, list_absent=False, swap_bins=None):
    """The list as a tiled counting sort builds it: a histogram per tile of TILE_PX pixels, the
    exclusive scan over (bucket, tile), every tile's slots scattered from its scanned starts.  With the
    defaults it equals expected_list; the other arguments are the ways it can go wrong:
      tile_order="descending"  the tiles of a bucket in the wrong order (stable inside a tile only)
      scatter_shift=1          the scatter's tiles begin one slot later than the histogram's
      list_absent=True         slots of edges that do not exist listed (in the virtual bucket)
      swap_bins=(a, b)         the starts of two buckets exchanged"""
    per_px = planes.shape[0]
    keys = slot_keys(planes).astype(np.int64)
    if list_absent:
        keys[keys == ABSENT] = VIRTUAL_BUCKET
    tile_slots = TILE_PX[per_px] * per_px
    num_tiles = (keys.size + tile_slots - 1) // tile_slots
    hist = np.zeros((NUM_OFFSETS - 1, num_tiles), np.int64)
    for t in range(num_tiles):
        k = keys[t * tile_slots:(t + 1) * tile_slots]
        hist[:, t] = np.bincount(k[k != ABSENT], minlength=NUM_OFFSETS - 1)
    per_bucket = hist.sum(axis=1)
    offsets = np.zeros(NUM_OFFSETS, np.int64)
    offsets[1:] = np.cumsum(per_bucket)
    in_bucket = hist if tile_order == "ascending" else hist[:, ::-1]
    before = np.cumsum(in_bucket, axis=1) - in_bucket
    if tile_order != "ascending":
        before = before[:, ::-1]
    starts = offsets[:-1, None] + before
    if swap_bins:
        a, b = swap_bins
        starts[[a, b]] = starts[[b, a]]
    slots = np.full(int(offsets[-1]), 0xFFFFFFFF, np.uint32)
    for t in range(num_tiles):
        lo = min(keys.size, t * tile_slots + (scatter_shift if t else 0))
        hi = min(keys.size, (t + 1) * tile_slots + scatter_shift)
        k = keys[lo:hi]
        ids = np.arange(lo, hi)[k != ABSENT]
        k = k[k != ABSENT]
        order = np.argsort(k, kind="stable")
        k, ids = k[order], ids[order]
        rank = np.arange(k.size) - np.searchsorted(k, k, side="left")
        pos = starts[k, t] + rank
        ok = pos < slots.size
        slots[pos[ok]] = ids[ok]
    return slots, offsets.astype(np.int32)


# ---- inputs -----------------------------------------------------------------------------------------
def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def _gray(plane):
    return _frozen(np.repeat(plane[:, :, None].astype(np.float32), 3, axis=2))


@functools.lru_cache(maxsize=None)
def flat_frame(W, H):
    """Every existing edge in bucket 0: the longest run of equal keys a step can see."""
    return _gray(np.full((H, W), 0.25, np.float32))


RAMP_STEP = 1.0 / 256      # 8 buckets apart: no rounding brings two of the 72 differences together


@functools.lru_cache(maxsize=None)
def ramp_frames(W, H):
    """(prev, cur), W a multiple of 8: the temporal keys of pixel p towards neighbour q are
    |0.5 + (9 (x_p mod 8) - j_q) RAMP_STEP| with j_q = x_q mod 3 + 3 (y_q mod 3) -- 72 different
    buckets over any eight consecutive pixels, so 64 consecutive slots of existing edges never
    hold a bucket twice."""
    assert W % 8 == 0
    x, y = np.arange(W)[None, :], np.arange(H)[:, None]
    prev = ((x % 3) + 3 * (y % 3)) * RAMP_STEP
    cur = 0.5 + 9 * (x % 8) * RAMP_STEP + 0 * y
    return _gray(prev), _gray(cur)


@functools.lru_cache(maxsize=None)
def alternating_frame(W, H, t):
    """Two colours on a checkerboard: right / bottom edges in one bucket, the diagonals in bucket 0."""
    return ec.features("checker", W, H, t)


# A case: (name, W, H, l1, frames, temporal) -- frames: names of the frame builders below; temporal:
# per frame after the first (flow or None, is_virtual).
def _frames_of(case):
    name, W, H, l1, kind = case
    f0, f1, flow, _ = ec.key_inputs(W, H)
    if kind == "noise-flow":
        return [f0, f1], [(flow, False)]
    if kind == "noise-noflow":
        return [f0, f1], [(None, False)]
    if kind == "flat":
        return [flat_frame(W, H), flat_frame(W, H)], [(None, False)]
    if kind == "ramp":
        prev, cur = ramp_frames(W, H)
        return [prev, cur], [(None, False)]
    if kind == "alternating":
        return [alternating_frame(W, H, 0), alternating_frame(W, H, 1)], [(None, False)]
    if kind == "virtual":
        return [f0, f1], [(flow, True)]
    if kind == "second-frame":      # a full noise frame, then a flat one on the same handle
        return [f0, f1, flat_frame(W, H)], [(flow, False), (None, False)]
    raise ValueError(kind)


SMALL = (70, 33)      # 2310 pixels: two spatial tiles, three temporal ones, the last of each partial
RAMP_SIZE = (72, 33)
BIG = (1024, 770)     # 770 temporal tiles: more than the 768 workgroups a launch has resident
CASES = (
    [("%dx%d-l2-flow" % s, s[0], s[1], False, "noise-flow") for s in ec.KEY_SIZES] +
    [("%dx%d-l1-noflow" % s, s[0], s[1], True, "noise-noflow") for s in ((2, 1), (3, 683), (2049, 1))] +
    [("big-l2-flow", BIG[0], BIG[1], False, "noise-flow"),
     ("flat", SMALL[0], SMALL[1], False, "flat"),
     ("ramp", RAMP_SIZE[0], RAMP_SIZE[1], False, "ramp"),
     ("alternating", SMALL[0], SMALL[1], False, "alternating"),
     ("virtual-flow", SMALL[0], SMALL[1], False, "virtual"),
     ("virtual-flow-two-tiles", 3, 683, True, "virtual"),
     ("second-frame", SMALL[0], SMALL[1], False, "second-frame")])


def case_id(case):
    return case[0]


def inputs(case):
    """(frames, temporal): the H x W x 3 feature frames and, per frame after the first, (flow, is_virtual)."""
    return _frames_of(case)


@functools.lru_cache(maxsize=None)
def oracle_planes(case):
    """{list index: bucket planes}: list 2 t the spatial list of frame t, 2 t - 1 the temporal list
    between frames t - 1 and t (a virtual list: bucket 2048 wherever the edge exists)."""
    _, W, H, l1, _ = case
    frames, temporal = _frames_of(case)
    out = {}
    for t, f in enumerate(frames):
        out[2 * t] = ol.spatial_buckets(f, l1)
        if t:
            flow, is_virtual = temporal[t - 1]
            planes, _ = ol.temporal_buckets(f, frames[t - 1], flow, l1)
            if is_virtual:
                planes = np.where(planes == ABSENT, ABSENT, VIRTUAL_BUCKET).astype(np.uint16)
            out[2 * t - 1] = planes
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected_lists(case):
    """{list index: (slots, offsets)} of a case (only read it)."""
    out = {}
    for index, planes in oracle_planes(case).items():
        slots, offsets = expected_list(planes)
        slots.setflags(write=False)
        offsets.setflags(write=False)
        out[index] = (slots, offsets)
    return out
