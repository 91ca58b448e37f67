"""Hand-made and generated vector-only SegmentationDesc messages shared by the vector raster tests
(not collected by pytest).  Messages are of test_proto_wire.build_schema()."""
import ctypes as C

import numpy as np

from test_proto_wire import build_schema

Msg = build_schema()


def make_desc(width, height, regions, removed=True):
    """regions: [(id, [polygon, ...])], a polygon a list of (x, y) corner points, closed (first point
    repeated).  Every polygon gets mesh entries of its own."""
    m = Msg()
    m.frame_width, m.frame_height = width, height
    m.rasterization_removed = removed
    m.vector_mesh.SetInParent()
    for rid, polys in regions:
        r = m.region.add()
        r.id = rid
        r.vectorization.SetInParent()
        for pts in polys:
            p = r.vectorization.polygon.add()
            for x, y in pts:
                p.coord_idx.append(len(m.vector_mesh.coord))
                m.vector_mesh.coord.extend([float(x), float(y)])
    return m


def rect(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1), (x0, y0)]


def comb(teeth=40):
    """Teeth of width 1 at x = 2k .. 2k + 1 over rows 0 and 1, a base over row 2: 2 * teeth
    crossings in rows 0 and 1 of a 2 * teeth x 3 frame."""
    pts = [(0, 3), (0, 0)]
    for k in range(teeth):
        pts += [(2 * k + 1, 0)]
        if k + 1 < teeth:
            pts += [(2 * k + 1, 2), (2 * k + 2, 2), (2 * k + 2, 0)]
    pts += [(2 * teeth - 1, 3), (0, 3)]
    return make_desc(2 * teeth, 3, [(7, [pts])])


def hourglass():
    """Two triangles that meet in the vertex (5, 5) of one polygon: a pinch."""
    return make_desc(10, 10, [(3, [[(2, 2), (8, 2), (5, 5), (8, 8), (2, 8), (5, 5), (2, 2)]])])


def bow_tie(width=10, height=4):
    """A self-crossing quadrilateral whose two diagonals meet at exactly (5, 2), and a sliver with
    edges at x = 5.0008 and 5.0016: in row 2 the crossings 5, 5, 5.0008, 5.0016 are chained within
    the comparator's eps of 1e-3 while the outer two are 1.6e-3 apart."""
    tie = [(4, 0), (6, 0), (4, 4), (6, 4), (4, 0)]
    return make_desc(width, height, [(1, [tie, rect(5.0008, 0, 5.0016, 4)])])


def two_line_regions(n=300):
    """n regions of two lines each (a 1 x 2 box; its horizontal lines are dropped), laid out in a
    grid of 40 columns: more than one block of lines, more groups than a wavefront has lanes."""
    cols = 40
    regions = []
    for k in range(n):
        x, y = 2 * (k % cols), 3 * (k // cols)
        regions.append((1000 + k, [rect(x, y, x + 1, y + 2)]))
    return make_desc(2 * cols, 3 * ((n + cols - 1) // cols), regions)


def l1_voronoi(seed, W, H, k):
    """Every pixel to its nearest of k seeded points in the L1 metric (a chamfer pass, so a
    full-size frame takes a fraction of a second), then every N4-connected component a region of
    its own."""
    from scipy import ndimage
    rng = np.random.default_rng(seed)
    sx, sy = rng.integers(0, W, k), rng.integers(0, H, k)
    far = np.ones((H, W), bool)
    far[sy, sx] = False
    _, (iy, ix) = ndimage.distance_transform_cdt(far, metric="taxicab", return_indices=True)
    lab = (iy.astype(np.int64) * W + ix).astype(np.int64)
    _, lab = np.unique(lab, return_inverse=True)
    lab = lab.reshape(H, W).astype(np.int32)
    out = np.zeros((H, W), np.int32)
    nxt = 0
    for v, box in enumerate(ndimage.find_objects(lab + 1)):
        if box is None:
            continue
        comp, n = ndimage.label(lab[box] == v)      # 4-connectivity
        for c in range(1, n + 1):
            out[box][comp == c] = nxt
            nxt += 1
    return out


def block_partition(seed, W, H):
    """Axis-aligned blocks, every block a region of its own: boundaries on which the boundary
    simplification changes nothing."""
    rng = np.random.default_rng(seed)
    xs = np.unique(np.concatenate([[0, W], rng.integers(1, W, 5)]))
    ys = np.unique(np.concatenate([[0, H], rng.integers(1, H, 4)]))
    ids = np.zeros((H, W), np.int32)
    n = 0
    for j in range(len(ys) - 1):
        for i in range(len(xs) - 1):
            ids[ys[j]:ys[j + 1], xs[i]:xs[i + 1]] = n
            n += 1
    return ids


def vectorize(ids):
    """vsg_vectorize_id_image: the parsed desc (rasters and vectorizations) of an id image."""
    from video_segment_amd import _lib
    ids = np.ascontiguousarray(ids, np.int32)
    p, n = C.c_void_p(), C.c_size_t()
    _lib.check(_lib.lib().vsg_vectorize_id_image(ids.ctypes.data_as(C.c_void_p), ids.shape[1], ids.shape[0],
                                                 C.byref(p), C.byref(n)))
    m = Msg()
    m.ParseFromString(C.string_at(p, n.value))
    return m


def vector_only(ids):
    """The desc of an id image as the reference's writer leaves it: rasters cleared,
    rasterization_removed set, frame size present."""
    import vector_raster_model as vm
    m = vm.remove_rasterization(vectorize(ids))
    m.frame_width, m.frame_height = ids.shape[1], ids.shape[0]
    return m
