"""Sequences of id planes, frames and label planes for the volume session tests (not collected by pytest).  A
sequence is (name, W, H, level, adds); an add is (frame, msg, P, F, B): the caller's frame index, the
SegmentationDesc message (level_boundaries_cases.case of the id plane, so a raster per id), the id plane P at
the sequence's level, the H x W x 3 uint8 frame and the H x W int32 label plane.  `model_adds` gives what
volume_model takes."""
import collections
import copy
import zlib

import numpy as np

import level_adjacency_cases as ac
import level_boundaries_cases as bc
import level_colors_cases as kc
import level_overlap_cases as oc
import level_regions_cases as lc

Add = collections.namedtuple("Add", "frame msg P F B")
Seq = collections.namedtuple("Seq", "name W H level adds")

MAX = (1 << 31) - 1
MANY = ac.STAR_LEAVES      # 300: more than a wavefront (64) and more than a block (256)
GROWN = 5000               # keys of the frame that takes the tables past what 300 keys reserved


def seq(name, frames, planes, labels, level=0):
    """One add per entry of `planes` (id planes of equal shape); labels[k] is B of add k; F is noise from a seed
    that name and k fix."""
    planes = [np.asarray(p, np.int32) for p in planes]
    H, W = planes[0].shape
    adds = []
    for k, (frame, ids, B) in enumerate(zip(frames, planes, labels)):
        F = kc.frame(W, H, zlib.crc32(("%s/%d" % (name, k)).encode()))
        adds.append(Add(int(frame), bc.case("%s_%d" % (name, k), ids).msg, ids, F, np.ascontiguousarray(B, np.int32)))
    return Seq(name, W, H, level, adds)


def model_adds(s, upto=None):
    return [(a.frame, a.P, a.F, a.B) for a in s.adds[:upto]]


def _two(W, H, other):
    """Id 5 everywhere but for a 3 x 2 corner of id `other` (none for a negative one)."""
    ids = np.full((H, W), 5, np.int32)
    if other >= 0:
        ids[1:3, 2:5] = other
    return ids


def life_span():
    """Id 3 lives in frames 0 and 2 and not in frame 1; the same with the indices 5, 2, 9 given out of order; and
    a 10 x 10 region (area 100) in frame 2^31 - 1, twice: sum_t = 200 (2^31 - 1) needs 64 bits."""
    W, H = 10, 10
    B = oc.stripes(W, H)
    planes = [_two(W, H, 3), _two(W, H, -1), _two(W, H, 3)]
    return [seq("gap", (0, 1, 2), planes, [B] * 3),
            seq("out_of_order", (5, 2, 9), planes, [B, B + 1, B]),
            seq("late", (7, MAX, MAX), [_two(W, H, 3), _two(W, H, -1), _two(W, H, -1)], [B] * 3)]


def search_edges():
    """First add into an empty table; then ids, labels and pairs below all known keys, above all of them and
    between them; then an add without a new key; then one with new keys only."""
    W, H = 8, 4
    x = np.arange(W)
    base = np.tile((10 + 10 * (x * 3 // W)).astype(np.int32), (H, 1))            # 10, 20, 30
    more = np.tile(np.array([5, 5, 15, 15, 25, 25, 40, 40], np.int32), (H, 1))  # below, between, between, above
    more[H - 1] = base[0]                                                        # and the known ones again
    fresh = np.tile((100 + x).astype(np.int32), (H, 1))
    labels = [base + 1, more + 1, base + 1, fresh + 1]
    labels[1] = labels[1].copy()
    labels[1][0, :] = 11                   # known label under new ids: new pairs between known ones
    return seq("search_edges", (0, 1, 2, 3), [base, more, base, fresh], labels)


def widths():
    """100 x 50.  300 ids under one label; one id under 300 labels; then 5 000 ids under 5 000 labels, which
    takes every table past the room the first two adds reserved."""
    W, H = 100, 50
    leaves = np.full(W * H, -1, np.int32)
    leaves[:MANY] = 100 + np.arange(MANY)
    leaves = leaves.reshape(H, W)
    many = (1000 + 3 * np.arange(W * H, dtype=np.int32)).reshape(H, W)
    assert many.size == GROWN
    return seq("widths", (0, 1, 2), [leaves, np.full((H, W), 7, np.int32), many],
               [np.full((H, W), 9, np.int32), np.where(leaves >= 0, leaves + 50, -1), many[::-1, ::-1] + 1])


def empty_sides():
    """A frame with no covered pixel between two ordinary ones, and a frame whose B is all void, of several
    negative values."""
    W, H = 12, 6
    yy, xx = np.mgrid[0:H, 0:W]
    ids = (2 + (xx // 4) + 3 * (yy // 3)).astype(np.int32)
    B = ((xx + yy) % 4 - 1).astype(np.int32)
    void = (-1 - (xx + yy) % 3 * 1000).astype(np.int32)
    return seq("empty_sides", (0, 1, 2, 3), [ids, np.full((H, W), -1, np.int32), ids, ids + 1], [B, B, void, B])


def extremes():
    """Ids 0 and 2^31 - 1 with labels 0 and 2^31 - 1 on the same pixels, twice."""
    c = oc.max_values()
    P = lc.id_image(c.case.msg)
    return seq("extremes", (MAX, MAX - 1), [P, P], [c.B, c.B])


def three_levels(level):
    """level_regions_cases.three_levels at `level`: frame 0 carries the hierarchy, the later frames are the same
    desc without one."""
    c = lc.three_levels()
    bare = copy.deepcopy(c.msg)
    del bare.hierarchy[:]
    P = lc.id_image(c.msg, level)
    B = oc.stripes(c.W, c.H)
    adds = [Add(k, c.msg if k == 0 else bare, P, kc.frame(c.W, c.H, 40 + k), np.roll(B, 5 * k, axis=1))
            for k in range(3)]
    return Seq("three_levels_%d" % level, c.W, c.H, level, adds)


def geometry(W, H):
    """level_regions_cases.boundary_ids as a single-frame session."""
    return seq("geometry_%dx%d" % (W, H), (3,), [lc.boundary_ids(W, H)], [oc.stripes(W, H)])


def steady(n):
    """The same plane n times: no add after the first brings a key."""
    W, H = 16, 8
    P = _two(W, H, 3)
    return seq("steady", range(n), [P] * n, [oc.stripes(W, H)] * n)


def small():
    """The sequences small enough for the voxel loop."""
    return life_span() + [search_edges(), empty_sides(), extremes(), geometry(63, 3), steady(3)]


def all_sequences():
    return small() + [widths()] + [three_levels(level) for level in (0, 1, 2)]
