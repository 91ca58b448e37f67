"""Id images for the mesh simplification tests (not collected by pytest): level_mesh_cases.small() plus the
smallest planes at which a stage of the simplification can go wrong.  No plane is larger than 640 x 360 but the
ones level_mesh_cases brings along.  A case is level_regions_cases.Case."""
import numpy as np

import level_mesh_cases as mc

Case = mc.Case
case = mc.case

# what the device stages hold per segment: a wavefront's path up to WAVE_POINTS points, the workgroup's LDS
# path up to LDS_POINTS points, a block of the handle beyond (kSimplifyWavePoints, kSimplifyLdsPoints)
WAVE_POINTS = 256
LDS_POINTS = 2048

PARAMS = ((0.0, 0), (0.5, 0), (1.0, 4), (1.5, 3), (3.5, 9))
ERRORS = (0.0, 0.5, 1.0, 1.5, 2.0, 3.5)


def discs():
    """Two nested discs and an ellipse: closed segments of about 700 cracks with general slopes."""
    W, H = 200, 150
    y, x = np.mgrid[:H, :W]
    ids = np.full((H, W), 1, np.int32)
    ids[(x - 70) ** 2 + (y - 75) ** 2 <= 60 ** 2] = 2
    ids[(x - 70) ** 2 + (y - 75) ** 2 <= 31 ** 2] = 3
    ids[((x - 165) / 28.0) ** 2 + ((y - 60) / 47.0) ** 2 <= 1.0] = 4
    return case("discs_200x150", ids)


def euclidean_voronoi():
    """25 seeds with weights: borders of general slopes that meet in junctions of three."""
    W, H = 200, 150
    rng = np.random.default_rng(5)
    sx, sy = rng.integers(0, W, 25), rng.integers(0, H, 25)
    wt = rng.uniform(0.7, 1.4, 25)
    y, x = np.mgrid[:H, :W]
    d = ((x[..., None] - sx) ** 2 + (y[..., None] - sy) ** 2) * wt
    return case("euclidean_voronoi_200x150", np.argmin(d, axis=2).astype(np.int32))


def staircase(step):
    """A border that goes `step` right and `step` down, over and over: 0.71 * step from its chord."""
    W, H = 48, 40
    y, x = np.mgrid[:H, :W]
    ids = np.where(x // step >= y // step + 2, 2, 1).astype(np.int32)
    return case("staircase_%d" % step, ids)


def oblique_joint():
    """A border of slope 1:3 that goes on with slope 1:4: the joint lies 2.6 from the chord of the whole border,
    so it is kept up to max_error 2 and goes at 3.5, while the stairs of either part (0.95 and 0.97 from their
    chords) go from max_error 1 on."""
    W, H = 120, 40
    ids = np.full((H, W), 1, np.int32)
    edge = 2
    for y in range(H):
        edge += 3 if y < 16 else 4
        ids[y, :min(edge, W)] = 2
    return case("oblique_joint", ids)


def oblique_island():
    """The same two slopes on the outline of an island: a closed segment with oblique joints."""
    W, H = 150, 60
    ids = np.full((H, W), 1, np.int32)
    for y in range(4, 56):
        k = y - 4
        lo = 5 + (3 * k if k < 14 else 42 + 4 * (k - 14)) // 2
        hi = lo + 20 + (k if k < 26 else 52 - k)
        ids[y, lo:min(hi, W - 2)] = 6
    return case("oblique_island", ids)


def tilted_ellipse():
    """An ellipse island at an angle: the sweeps choose another start than vertex 0, and at max_error 1.5 and 2
    the joint pass drops points of the closed list."""
    W, H = 64, 48
    rng = np.random.default_rng(43)
    y, x = np.mgrid[:H, :W]
    ids = np.full((H, W), 1, np.int32)
    th = rng.uniform(0, np.pi)
    a, b = rng.uniform(12, 24), rng.uniform(5, 12)
    cx, cy = W / 2 + rng.uniform(-3, 3), H / 2 + rng.uniform(-3, 3)
    u = (x - cx) * np.cos(th) + (y - cy) * np.sin(th)
    v = -(x - cx) * np.sin(th) + (y - cy) * np.cos(th)
    ids[(u / a) ** 2 + (v / b) ** 2 <= 1] = 2
    return case("tilted_ellipse", ids)


def sector(half_deg, bulge):
    """A tilted pie slice whose apex is the farthest point from vertex 0: the sweeps start the list in the middle
    of the arc, the recursion keeps the arc's two ends next to it, and the joint pass drops the start.  Its last
    read then wraps around to the slot the first write changed."""
    W, H = 64, 56
    y, x = np.mgrid[:H, :W]
    dx, dy = x - 12.5, (H - 4.5) - y
    th = np.degrees(np.arctan2(dy, dx)) - 30.0
    lim = 30.0 + bulge * np.cos(np.radians(th * 90.0 / half_deg))
    ids = np.full((H, W), 1, np.int32)
    ids[(np.abs(th) <= half_deg) & (np.hypot(dx, dy) <= lim)] = 2
    return case("sector_%d" % half_deg, ids)


def plus_island():
    """A plus: four corners equally far from the sweep's start, and equally far from a chord."""
    ids = np.full((13, 13), 1, np.int32)
    ids[2:11, 5:8] = 4
    ids[5:8, 2:11] = 4
    return case("plus_island", ids)


def tiny_islands():
    """A 1 x 1 and a 2 x 2 island: closed segments that come back as one vertex at max_error 2 and 3.5."""
    ids = np.full((8, 12), 1, np.int32)
    ids[3, 3] = 2
    ids[3:5, 7:9] = 3
    return case("tiny_islands", ids)


def growing_zigzag():
    """A border of 70 teeth, each higher than the one before: every round keeps one tooth."""
    W, H = 290, 80
    ids = np.full((H, W), 1, np.int32)
    ids[76:] = 2
    for k in range(70):
        ids[75 - k:76, 4 + 4 * k:6 + 4 * k] = 2
    return case("growing_zigzag_70", ids)


def long_zigzag():
    """One-pixel teeth across 640 columns: an open segment of more than 1024 corners, longer than a wavefront's
    path and a workgroup, whose first-index ties make the recursion as deep as the segment is long."""
    W, H = 640, 6
    ids = np.full((H, W), 1, np.int32)
    ids[3:] = 2
    ids[2, 1::2] = 2
    return case("long_zigzag_640", ids)


def band_zigzag():
    """A band with teeth on both sides, attached to the left frame edge: its border with the region around it is
    one open segment of more than LDS_POINTS = 2048 corners, which the workgroup keeps in a block of the handle
    instead of LDS."""
    W, H = 640, 12
    ids = np.full((H, W), 1, np.int32)
    ids[4:8, :630] = 2
    ids[3, 1:629:2] = 2
    ids[8, 1:629:2] = 2
    return case("band_zigzag_640", ids)


def own():
    return [discs(), euclidean_voronoi(), staircase(1), staircase(2), oblique_joint(), oblique_island(),
            tilted_ellipse(), sector(15, 1.5), sector(20, 0.0), plus_island(), tiny_islands(), growing_zigzag(),
            long_zigzag(), band_zigzag()]


def all_cases():
    return own() + mc.small()
