"""SegmentationDesc messages and ground-truth label planes for the boundary distance tests (not collected by
pytest).  A case is level_regions_cases.Case: (name, message, W, H, levels).  Every case of persistence_cases is
reused (the widths around tile and block edges, the ladders, the narrow frames); the planted frames are larger
than one block of columns (256), one chunk of rows (32) and one tile of the disc scan (64 x 32) in both
directions, and most have a closed form."""
import numpy as np

import level_regions_cases as lc
import persistence_cases as pc

Case = lc.Case
TOLERANCES = (0, 1, 2, 4, 24, 25, 4096)
PW, PH = 300, 200          # the planted frames


def _two_levels(name, ids):
    """The plane with a second level that merges everything into one region."""
    ids = np.asarray(ids, np.int32)
    present = [int(r) for r in np.unique(ids[ids >= 0])]
    return pc.case(name, ids, [{r: 9000 for r in present}] if present else [])


def uniform():
    return _two_levels("uniform", np.full((PH, PW), 4, np.int32))


def uncovered_frame():
    return Case("uncovered_300x200", lc.desc_from_ids(np.full((PH, PW), -1, np.int32)), PW, PH, (0,))


def every_pixel():
    """Every pixel its own id, 260 x 70: more than one block of columns and two chunks of rows.  Level 1 has
    vertical stripes 5 wide, level 2 is one region."""
    W, H = 260, 70
    ids = np.arange(W * H, dtype=np.int32).reshape(H, W)
    stripes = {int(k): 100000 + (int(k) % W) // 5 for k in range(W * H)}
    return pc.case("every_pixel", ids, [stripes, {v: 200000 for v in set(stripes.values())}])


def first_column():
    """Column 0 differs: E is column 0, D = x^2, the row pass searches across every block of the row."""
    ids = np.full((PH, PW), 1, np.int32)
    ids[:, 0] = 0
    return _two_levels("first_column", ids)


def first_row():
    """Row 0 differs: E is row 0, D = y^2, the column pass looks across every chunk above."""
    ids = np.full((PH, PW), 1, np.int32)
    ids[0, :] = 0
    return _two_levels("first_row", ids)


def corner():
    """Only the last pixel differs: E = {(W - 2, H - 1), (W - 1, H - 2)}."""
    ids = np.full((PH, PW), 1, np.int32)
    ids[PH - 1, PW - 1] = 0
    return _two_levels("corner", ids)


def blobs():
    """An L1 Voronoi partition of 300 x 200 with three levels: curved boundaries at every distance."""
    rs = np.random.RandomState(5)
    n = 40
    sx, sy = rs.randint(0, PW, n), rs.randint(0, PH, n)
    yy, xx = np.mgrid[0:PH, 0:PW]
    ids = (np.abs(xx[:, :, None] - sx) + np.abs(yy[:, :, None] - sy)).argmin(axis=2).astype(np.int32)
    ids[150:160, 100:140] = -1                      # an uncovered hole
    return pc.case("blobs", ids, [{k: 500 + k % 7 for k in range(n)}, {500 + k: 900 + k // 4 for k in range(7)}])


def thin():
    """Frames of 1 x 1, 1 x N and N x 1, with and without an edge."""
    out = [pc.case("thin_1x1", [[3]])]
    row = (np.arange(290) // 97).astype(np.int32)
    out.append(pc.case("thin_290x1", row[None, :], [{0: 7, 1: 7, 2: 8}]))
    out.append(pc.case("thin_1x290", row[:, None], [{0: 7, 1: 7, 2: 8}]))
    out.append(pc.case("thin_uniform_290x1", np.full((1, 290), 2, np.int32)))
    return out


def planted():
    return [uniform(), uncovered_frame(), every_pixel(), first_column(), first_row(), corner(), blobs()] + thin()


def all_cases():
    return pc.all_cases() + planted()


# ---- ground-truth planes -----------------------------------------------------------------------------------

def shifted(ids0, dx=3, dy=4):
    """The level-0 ids moved by (dx, dy), the border filled by repeating the first row and column: an
    anti-diagonal boundary of the case then has its image's nearest pixels (3, 4) and (4, 3) away, unmatched at
    T = 24 and matched at T = 25; a vertical one lies 3 away, a horizontal one 4."""
    ids0 = np.asarray(ids0, np.int32)
    H, W = ids0.shape
    ys = np.clip(np.arange(H) - dy, 0, H - 1)
    xs = np.clip(np.arange(W) - dx, 0, W - 1)
    return np.ascontiguousarray(ids0[ys][:, xs])


def random_labels(W, H, seed):
    """Blocks of 7 x 5 with labels in [-3, 5]: negatives of several values, which are one void label."""
    rs = np.random.RandomState(seed)
    small = rs.randint(-3, 6, ((H + 4) // 5, (W + 6) // 7)).astype(np.int32)
    return np.ascontiguousarray(np.kron(small, np.ones((5, 7), np.int32))[:H, :W])


def all_void(W, H):
    return np.full((H, W), -1, np.int32) - (np.arange(W, dtype=np.int32)[None, :] % 3)


def pitched(plane, extra=5):
    """The same values as a view of rows W + extra apart; the gaps hold a value that would be an edge."""
    H, W = plane.shape
    buf = np.full((H, W + extra), 77777, np.int32)
    buf[:, :W] = plane
    return buf[:, :W]


def others(case, ids0):
    """[(name, H x W int32 plane)]: the ground truths a case is scored against."""
    W, H = case.W, case.H
    return [("shifted", shifted(ids0)), ("random", random_labels(W, H, W * 31 + H)), ("void", all_void(W, H)),
            ("pitched", pitched(random_labels(W, H, W * 17 + H + 1)))]
