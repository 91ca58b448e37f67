"""Pairs of an id image and a label plane for the level overlap tests (not collected by pytest).  A case is
(name, case, B): `case` a level_regions_cases.Case (name, message, W, H, levels to ask for) that gives P at
its level 0, and B the H x W int32 plane of labels.  Negative pixels of either have no group / no label."""
import collections

import numpy as np

import level_adjacency_cases as ac
import level_boundaries_cases as bc
import level_regions_cases as lc

OCase = collections.namedtuple("OCase", "name case B")

MAX = (1 << 31) - 1
MANY = ac.STAR_LEAVES      # 300: more than a wavefront (64) and more than a block (256)


def ocase(name, ids, B):
    ids, B = np.asarray(ids, np.int32), np.ascontiguousarray(B, np.int32)
    assert ids.shape == B.shape
    return OCase(name, bc.case(name, ids), B)


def stripes(W, H):
    """Labels -1 .. 4 in stripes 37 wide that move 11 columns to the left with every row, so that their ends
    fall inside, at and across the multiples of 64 and 256 somewhere; row 1 is one label throughout."""
    yy, xx = np.mgrid[0:H, 0:W]
    B = ((xx + 11 * yy) // 37) % 6 - 1
    if H > 1:
        B[1] = 4
    return B.astype(np.int32)


def widths():
    """P: level_regions_cases.boundary_ids, whose runs start and end on and around the multiples of 64 and
    256 and whose row 1 is one run: with B's row 1 that is one run across every step of the kernel."""
    return [ocase("width_%dx%d" % (W, H), lc.boundary_ids(W, H), stripes(W, H)) for W in bc.WIDTHS for H in bc.HEIGHTS]


def wraps():
    """One group under one label: the last pixel of a row and the first of the next carry the same pair.
    That is H runs and one pair."""
    return [ocase("wrap_%dx%d" % (W, H), np.full((H, W), 5, np.int32), np.full((H, W), 2, np.int32))
            for W, H in ((1, 4), (64, 3), (257, 3), (600, 2))]


def diagonal():
    """B == P: the table is diagonal.  With holes, and with ids up to 2^30 + 7."""
    hole, three = ac.hole().msg, lc.three_levels().msg
    return [ocase("same_hole", lc.id_image(hole), lc.id_image(hole)),
            ocase("same_three_levels", lc.id_image(three, 2), lc.id_image(three, 2))]


def void():
    """A B without a label, of several negative values."""
    ids = lc.id_image(ac.hole().msg)
    yy, xx = np.mgrid[0:ids.shape[0], 0:ids.shape[1]]
    return ocase("void", ids, -1 - (xx + yy) % 3 * 1000)


def uncovered_frame():
    c = {k.name: k for k in lc.uncovered()}["uncovered_frame"]
    B = np.full((c.H, c.W), -1, np.int32)
    B[:, 2:5] = 8
    B[1:3, 6:] = 3
    return OCase("uncovered_frame", c, B)


def checker():
    """Both planes a one-pixel checker, B's one column further: every pixel is a run of its own, W * H of
    them, the most a frame can have."""
    yy, xx = np.mgrid[0:8, 0:64]
    return ocase("checker_offset", np.where((xx + yy) % 2 == 0, 4, 6), 20 + (xx + 1 + yy) % 3)


def stars():
    """One region under 300 labels (and some void), and one label over 300 regions (and a region without a
    label), each also transposed so that every pair is in a row of its own."""
    one = np.full((2, MANY), 7, np.int32)
    leaves = np.stack([np.full(MANY, -1), 100 + np.arange(MANY)]).astype(np.int32)
    hub = np.stack([np.full(MANY, 7), 100 + np.arange(MANY)]).astype(np.int32)
    label = np.stack([np.full(MANY, -1), np.full(MANY, 9)]).astype(np.int32)
    return [ocase("labels_300x2", one, leaves), ocase("labels_2x300", one.T, leaves.T),
            ocase("regions_300x2", hub, label), ocase("regions_2x300", hub.T, label.T)]


def max_values():
    """Id 2^31 - 1 and label 2^31 - 1 on the same pixels, next to id 0, label 0, no group and no label."""
    ids = np.array([[0, 0, MAX, MAX, -1, MAX], [MAX, 0, -1, MAX, MAX, 0]], np.int32)
    B = np.array([[0, MAX, MAX, MAX, MAX, -7], [MAX, -1, 0, MAX, 0, 0]], np.int32)
    return ocase("max_values", ids, B)


def small():
    """The cases small enough for the brute-force double loop."""
    return [c for c in all_cases() if c.case.W * c.case.H <= 1500]


def all_cases():
    return widths() + wraps() + diagonal() + [void(), uncovered_frame(), checker()] + stars() + [max_values()]
