"""Plain numpy-f32 / Python model of the reference's polygon scan conversion, restated from reading it
(not collected by pytest; the vector raster tests compare the product against it entry for entry).

  ScaleVectorization                      segment_util/segmentation_util.cpp:1248-1267
  EdgeEntry and its comparator            segmentation_util.cpp:1107-1136
  RasterVectorization                     segmentation_util.cpp:1140-1236
  ReplaceRasterizationFromVectorization   segmentation_util.cpp:1238-1246
  RemoveRasterization                     segmentation_util.cpp:1269-1275

Every float of the reference is a C++ `float`; every one here is an np.float32 and every operation is
one rounded f32 operation.  In particular an edge's x advances by `curr_x += dx` once per row
(:1113, :1232-1234): the accumulated rounding is part of the definition and is not replaced by
p1.x + k * dx.

Three things the reference leaves open and this model states:

* EMPTY INTERVALS.  Two edges that start at one vertex have the same curr_x in their first row, so
  x_start = ceil(x - 1e-6f) and x_end = floor(x), decremented (:1217-1224), give left_x = right_x + 1
  at an integer x.  Every apex and every pinch does that.  The reference emits the interval
  (add_scan_inter at :1226 is unconditional); so does the model.  Painting it paints nothing.

* ROWS THE REFERENCE DOES NOT DEFINE.  A row is `unspecified` when
    - the comparator (:1115-1135) is not a strict weak order on the row's active edges, which is when
      std::sort's result is not a function of the row: a pair whose two eps tests disagree
      (a < b - eps against b > a + eps, after f32 rounding), crossings chained within eps whose ends
      are not within eps, or two crossings that the comparator cannot tell apart (within eps, same
      side, same dx) but whose curr_x differ;
    - the active count is odd (:1214 only DCHECKs; :1218 then reads aet[size]);
    - an interval leaves the row: left_x outside [0, W] or right_x outside [-1, W - 1].  (This admits
      exactly the empty intervals at the frame's two borders, left_x = 0 / right_x = -1 and
      left_x = W / right_x = W - 1.)
    - an edge starts above row 0 or ends below row H (:1186-1187 only DCHECK; the reference's
      edge_list has H + 1 entries), which counts once per such edge.
  The product answers all of these with VSG_ERR_INVALID.

* A REGION WITHOUT POLYGONS (an erased hole, :1155) has no intervals.

Messages are parsed SegmentationDesc objects of test_proto_wire.build_schema().
"""
import numpy as np

F = np.float32
EPS = F(1e-3)        # EdgeEntry::operator< (:1116), and the horizontal-edge test (:1168)
TINY = F(1e-6)       # :1217, :1222


def scale_vectorization(coord, frame_width, frame_height, width, height):
    """ScaleVectorization(width, height, desc) on the mesh's coord list: the literal loop with its
    parity counter.  Returns a new f32 array."""
    scale_x = F(width) * (F(1.0) / F(frame_width))      # :1253
    scale_y = F(height) * (F(1.0) / F(frame_height))    # :1254
    out = np.empty(len(coord), F)
    parity = 0
    for k, c in enumerate(coord):
        c = F(c)
        if parity % 2 == 0:
            out[k] = min(F(width), c * scale_x)         # :1261
        else:
            out[k] = min(F(height), c * scale_y)        # :1263
        parity += 1
    return out


class _Edge:
    __slots__ = ("curr_x", "y_max", "dx", "is_left")


def _x_less(a, b):
    return a < b - EPS          # :1118, one f32 subtraction


def _x_greater(a, b):
    return a > b + EPS          # :1120


def sort_active_edges(aet):
    """std::sort(aet) where the comparator makes its result a function of the row.  Returns
    (sorted list, well_defined)."""
    order = sorted(aet, key=lambda e: float(e.curr_x))
    ok = True
    out = []
    k = 0
    n = len(order)
    while k < n:
        # a run of crossings whose neighbours are not separated by the eps tests
        j = k
        while j + 1 < n:
            a, b = order[j].curr_x, order[j + 1].curr_x
            lt, gt = _x_less(a, b), _x_greater(b, a)
            if lt != gt:
                ok = False          # comp(a, b) and comp(b, a) look at different roundings
            if lt and gt:
                break
            j += 1
        run = order[k:j + 1]
        first, last = run[0].curr_x, run[-1].curr_x
        if _x_less(first, last) or _x_greater(last, first):
            ok = False              # chained within eps, ends apart: equivalence is not transitive
        # inside a run x counts as equal: left before right (:1126-1130), then the smaller dx (:1134)
        run.sort(key=lambda e: (0 if e.is_left else 1, float(e.dx)))
        for a, b in zip(run, run[1:]):
            if a.is_left == b.is_left and a.dx == b.dx and a.curr_x != b.curr_x:
                ok = False          # indistinguishable to the comparator, distinguishable in the output
        out += run
        k = j + 1
    return out, ok


def raster_vectorization(polygons, coord, frame_width, frame_height):
    """RasterVectorization(vec, mesh, frame_height, raster).  polygons: list of coord_idx lists;
    coord: the mesh's floats.  Returns ([(y, left_x, right_x)], number of unspecified rows)."""
    H, W = frame_height, frame_width
    intervals = []
    unspecified = 0
    if len(polygons) == 0:      # :1155
        return intervals, 0
    edge_list = [[] for _ in range(H + 1)]      # :1149
    start_y, end_y = H, 0
    for poly in polygons:
        assert len(poly) > 0                    # :1160
        for c in range(1, len(poly)):
            i1, i2 = poly[c - 1], poly[c]
            if min(i1, i2) < 0 or max(i1, i2) + 1 >= len(coord):
                raise ValueError("coord_idx outside the vector mesh")
            p1 = (F(coord[i1]), F(coord[i1 + 1]))
            p2 = (F(coord[i2]), F(coord[i2 + 1]))
            if abs(p1[1] - p2[1]) < EPS:        # :1168
                continue
            e = _Edge()
            e.is_left = True
            if p2[1] < p1[1]:                   # :1174-1177
                p1, p2 = p2, p1
                e.is_left = False
            if not (p1[1] >= 0 and p2[1] <= H):     # :1186-1187 DCHECKs, the size of edge_list
                unspecified += 1
                continue
            start_y = min(int(np.floor(p1[1])), start_y)    # :1180
            end_y = max(int(np.ceil(p2[1])), end_y)         # :1181
            e.curr_x = p1[0]
            e.y_max = p2[1]
            e.dx = (p2[0] - p1[0]) / (p2[1] - p1[1])        # :1185, f32
            edge_list[int(p1[1])].append(e)                 # :1188, float -> index truncates
    if start_y > end_y:
        return intervals, unspecified
    aet = []
    for y in range(start_y, end_y + 1):
        aet += edge_list[y]                                 # :1200-1202
        aet = [e for e in aet if not (e.y_max < F(y + 1))]  # :1205-1211, int y + 1 -> float
        aet, ok = sort_active_edges(aet)                    # :1213
        if len(aet) % 2:                                    # :1214
            ok = False
        for k in range(0, len(aet) - 1, 2):
            x_start = int(np.ceil(aet[k].curr_x - TINY))    # :1217
            frac_x = aet[k + 1].curr_x
            x_end = int(np.floor(frac_x))
            if abs(frac_x - F(x_end)) < TINY:               # :1222
                x_end -= 1
            if x_start < 0 or x_start > W or x_end < -1 or x_end > W - 1:
                ok = False
            intervals.append((y, x_start, x_end))
        if not ok:
            unspecified += 1
        for e in aet:
            e.curr_x = e.curr_x + e.dx                      # :1232-1234, one rounded f32 addition
    return intervals, unspecified


def rasterize_desc(msg, width=None, height=None):
    """ScaleVectorization to width x height where that differs from the desc's frame size, then
    ReplaceRasterizationFromVectorization.  Returns ((n, 4) int32 rows {y, left_x, right_x,
    region id} in the reference's order: region order, row, left to right; unspecified rows)."""
    fw, fh = msg.frame_width, msg.frame_height
    W = fw if width is None else width
    H = fh if height is None else height
    coord = np.asarray(msg.vector_mesh.coord, F)
    if fw and fh and (fw != W or fh != H):      # segmentation_unit.cpp:380-384
        coord = scale_vectorization(coord, fw, fh, W, H)
    rows = []
    unspecified = 0
    for r in msg.region:
        polys = [list(p.coord_idx) for p in r.vectorization.polygon]
        iv, u = raster_vectorization(polys, coord, W, H)
        unspecified += u
        rows += [(y, lx, rx, r.id) for y, lx, rx in iv]
    return np.asarray(rows, np.int32).reshape(-1, 4), unspecified


def remove_rasterization(msg):
    """RemoveRasterization on a copy of the message."""
    out = type(msg)()
    out.CopyFrom(msg)
    for r in out.region:
        r.ClearField("raster")
    out.rasterization_removed = True
    return out


def with_intervals(msg, rows, width, height):
    """A copy of a vector-only desc with the model's intervals as rasters and the frame size set:
    what render_model.RenderModel is fed with."""
    out = type(msg)()
    out.CopyFrom(msg)
    out.frame_width, out.frame_height = width, height
    out.rasterization_removed = False
    by_id = {}
    for r in out.region:
        r.ClearField("raster")
        by_id.setdefault(r.id, r)
    for y, lx, rx, rid in rows:
        s = by_id[int(rid)].raster.scan_inter.add()
        s.y, s.left_x, s.right_x = int(y), int(lx), int(rx)
    return out


def id_plane(rows, width, height):
    """The intervals painted in order into an H x W int32 plane of region ids, -1 where none paints."""
    out = np.full((height, width), -1, np.int32)
    for y, lx, rx, rid in rows:
        out[y, lx:rx + 1] = rid
    return out
