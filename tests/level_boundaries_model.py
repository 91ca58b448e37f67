"""Plain numpy / Python model of the boundary point lists of a hierarchy level (not collected by pytest;
the level boundary tests compare the product against it byte for byte).  Two definitions:

  get_boundary_literal  the reference's GetBoundary (segment_util/segmentation_boundary.cpp:78-179)
                        restated loop for loop -- the three-row byte buffer of 3 * (frame_width + 2), the
                        row pointers and their rotation, the `ranges` queue, the short-circuit tests --
                        for one rasterization.  The buffer has one zero guard byte before and one behind
                        it; a read of either is counted.
  boundaries            the set form, from an int32 plane, for all of its groups at once

The set form.  P is a plane of W x H, -1 where nothing covers a pixel; positions outside the frame count
as -1.  inner(g): positions with P = g and one of the four neighbours != g.  outer(g): positions of
[-1, W] x [-1, H] with P != g and one of the four neighbours = g.  Within a group points are ordered by y,
then x; groups by ascending value.

The literal form's inner result is inner(g) exactly.  Its outer result is outer(g) with every x one too
large: its pointers start at min_range - shift, its x at min_range (:148-154).  Its outer mode also reads
the byte before its buffer (the left neighbour of position -1 of whichever row lies first) and the byte
behind a buffer of the advertised size; both are zero here, which is the set form's "not in the region"."""
import numpy as np

BOUNDARY_DTYPE = np.dtype([("id", np.int32), ("component", np.int32), ("first_point", np.int32),
                           ("num_points", np.int32)])


def get_boundary_literal(runs, W, inner):
    """runs: [(y, left_x, right_x)] of one rasterization in (y, left_x) order.  Returns (points, guard
    reads): points as [(x, y)] in the order the reference pushes them."""
    if not runs:
        return [], 0
    rad = 1
    width_step = W + 2 * rad
    size = 3 * width_step
    buf = [0] * (size + 2)                  # byte i of the reference's buffer is buf[i + 1]
    guard_reads = [0]

    def rd(i):
        if i < 0 or i >= size:
            assert i in (-1, size), i        # never further out than the guard bytes
            guard_reads[0] += 1
        return buf[i + 1]

    def render_scanlines(y, ptr):
        lo, hi = 10 ** 6, -10 ** 6
        for sy, lx, rx in runs:
            if sy == y:
                for x in range(lx, rx + 1):
                    buf[ptr + x + 1] = 1
                lo, hi = min(lo, lx), max(hi, rx)
        return lo, hi

    prev_ptr, curr_ptr, next_ptr = rad, rad + width_step, rad + 2 * width_step
    min_y, max_y = runs[0][0], runs[-1][0]
    ranges = [render_scanlines(min_y, curr_ptr if inner else next_ptr)]
    shift = 0 if inner else 1
    range_size = 1 if inner else 3
    out = []
    for y in range(min_y - shift, max_y + shift + 1):
        for x in range(W):
            buf[next_ptr + x + 1] = 0
        if y < max_y:
            ranges.append(render_scanlines(y + 1, next_ptr))
        min_range = min([10 ** 7] + [r[0] for r in ranges])
        max_range = max([-10 ** 7] + [r[1] for r in ranges])
        if min_range <= max_range:
            off = min_range - shift
            for x in range(min_range, max_range + 2 * shift + 1):
                p, c, n = prev_ptr + off, curr_ptr + off, next_ptr + off
                if inner:
                    if rd(c) and (not rd(c - 1) or not rd(c + 1) or not rd(p) or not rd(n)):
                        out.append((x, y))
                else:
                    if not rd(c) and (rd(c - 1) or rd(c + 1) or rd(p) or rd(n)):
                        out.append((x, y))
                off += 1
        prev_ptr, curr_ptr, next_ptr = curr_ptr, next_ptr, prev_ptr
        if len(ranges) >= range_size:
            ranges.pop(0)
    return out, guard_reads[0]


def runs_of_mask(mask):
    """[(y, left_x, right_x)] of a boolean image, in (y, left_x) order."""
    out = []
    for y, row in enumerate(np.asarray(mask, bool)):
        x, W = 0, len(row)
        while x < W:
            if row[x]:
                a = x
                while x + 1 < W and row[x + 1]:
                    x += 1
                out.append((y, a, x))
            x += 1
    return out


def boundaries(plane, outer, components=None):
    """(records, points) of every group of the plane: records a BOUNDARY_DTYPE array by ascending group,
    points (n, 2) int32 {x, y}.  id = group and component = -1, or, with the component list of
    level_components_model the plane is the label image of, that component's id and component."""
    plane = np.asarray(plane, np.int32)
    H, W = plane.shape
    R = np.full((H + 4, W + 4), -1, np.int64)
    R[2:-2, 2:-2] = plane
    c = R[1:-1, 1:-1]                        # the padded grid: entry [py, px] is position (px - 1, py - 1)
    around = (R[:-2, 1:-1], R[2:, 1:-1], R[1:-1, :-2], R[1:-1, 2:])
    triples = []
    if outer:
        for nb in around:
            py, px = np.nonzero((nb >= 0) & (nb != c))
            triples.append(np.stack([nb[py, px], py - 1, px - 1], axis=1))
    else:
        differs = np.zeros(c.shape, bool)
        for nb in around:
            differs |= nb != c
        py, px = np.nonzero((c >= 0) & differs)
        triples.append(np.stack([c[py, px], py - 1, px - 1], axis=1))
    t = np.concatenate(triples).reshape(-1, 3)
    t = np.unique(t, axis=0)                 # once per group, in (group, y, x) order
    groups, first, count = np.unique(t[:, 0], return_index=True, return_counts=True)
    records = np.zeros(len(groups), BOUNDARY_DTYPE)
    records["first_point"], records["num_points"] = first, count
    if components is None:
        records["id"], records["component"] = groups, -1
    else:
        records["id"], records["component"] = components["id"][groups], components["component"][groups]
    points = np.ascontiguousarray(t[:, [2, 1]].astype(np.int32)).reshape(-1, 2)
    return records, points


def of_mask(mask, outer):
    """[(x, y)] of one boolean image's boundary, the set form."""
    _, points = boundaries(np.where(np.asarray(mask, bool), 0, -1), outer)
    return [tuple(p) for p in points.tolist()]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
