"""The inputs of tests/test_gpu_render_edges.py: id images at the sizes and with the edges at which
k_render_fill and k_render_compose (video_segment_amd/render/render.hip) change path, their descriptors
(level_regions_cases.desc_from_ids; -1: no region), a source frame each, and the results of render_model.py,
computed once and shared (only read them).  Not collected by pytest; test_render_edge_cases.py checks on the
CPU that every case does what it is here for.

The constants the cases come from: a thread of k_render_compose decides 4 x 4 pixels, a workgroup 256 columns x
16 rows; k_render_fill paints an interval of kLongInterval = 16 pixels and more with a whole wavefront, takes 64
intervals per wavefront and 256 per workgroup, and 2048 x 256 intervals per trip of its grid."""
import collections
import functools

import numpy as np

import level_regions_cases as lc
import render_model as rm

PX, ROWS = 4, 4                      # pixels and rows per thread of k_render_compose
GROUP_COLS, GROUP_ROWS = 256, 16     # columns and rows per workgroup
LONG_INTERVAL = 16                   # kLongInterval
WAVE, FILL_BLOCK, FILL_GRID = 64, 256, 2048

WIDTHS = (1, 2, 3, 4, 5, 7, 8, 255, 256, 257, 259, 513)
HEIGHTS = (1, 2, 3, 4, 5, 15, 16, 17, 18)


# Every width with four heights, one per value of H % 4, and every height with a width of every value of W % 4.
# 2 is the only width with W % 4 == 2, so it meets all the heights: 53 sizes is the least the pairing allows.
HEIGHTS_OF = {
    1: (1, 4, 15, 18), 2: HEIGHTS, 3: (2, 5, 15, 16), 4: (1, 3, 4, 18), 5: (2, 3, 16, 17), 7: (4, 5, 15, 18),
    8: (3, 16, 17, 18), 255: (3, 4, 17, 18), 256: (2, 5, 15, 16), 257: (2, 4, 15, 17), 259: (1, 3, 16, 18),
    513: (4, 5, 15, 18),
}
SIZES = sorted((w, h) for w in WIDTHS for h in HEIGHTS_OF[w])

Case = collections.namedtuple("Case", "name family W H ids")

FLAT_ID, FIRST_MARK_ID = 11, 20


# ---- seams ---------------------------------------------------------------------------------------------
def column_seams(W):
    """x of every column seam x-1|x that the width has: 2|3 (4k+2|4k+3), 3|4 (4k-1|4k) and 4|5 (4k|4k+1) at
    the first thread's edge, the same three at the workgroup's edge 255|256, and the last two columns."""
    want = [3, 4, 5, 255, 256, 257, W - 1]
    out = []
    for x in want:
        if 1 <= x <= W - 1 and x not in out:
            out.append(x)
    return out


def row_seams(H):
    """y of every row seam y-1|y that the height has: 3|4 (4k-1|4k) and 4|5 (4k|4k+1) at the first thread's
    edge, the same two at the workgroup's edge 15|16, and the last two rows."""
    want = [4, 5, 16, 17, H - 1]
    out = []
    for y in want:
        if 1 <= y <= H - 1 and y not in out:
            out.append(y)
    return out


def column_seam_is_alone(ids, y, x):
    """Pixel (y, x-1) differs from its right neighbour and from nothing else the edge rule reads."""
    H = ids.shape[0]
    return ids[y, x - 1] != ids[y, x] and (y == H - 1 or ids[y + 1, x - 1] == ids[y, x - 1])


def row_seam_is_alone(ids, y, x):
    """Pixel (y-1, x) differs from the pixel below and from nothing else the edge rule reads."""
    W = ids.shape[1]
    return ids[y - 1, x] != ids[y, x] and (x == W - 1 or ids[y - 1, x + 1] == ids[y - 1, x])


@functools.lru_cache(maxsize=None)
def seams(W, H):
    """(ids, column marks {x: y}, row marks {y: x}).  One region fills the frame; every seam has a one-pixel
    region of its own on its right (lower) side, so that the pixel on its left (upper) side is an edge pixel
    because of that one neighbour alone.  Marks are placed first fit, rows and columns tried in turn from a
    start that moves on with every mark, those that no seam of the kind has yet first, so they spread over the
    frame; a place is taken only if every seam placed so far stays alone.  hidden() names the seams for which
    no such place was found (none at the sizes used here: test_render_edge_cases.py asserts it)."""
    ids = np.full((H, W), FLAT_ID, np.int32)
    cols, rows = {}, {}
    next_id = [FIRST_MARK_ID]

    def all_alone():
        return (all(column_seam_is_alone(ids, y, x) for x, y in cols.items())
                and all(row_seam_is_alone(ids, y, x) for y, x in rows.items()))

    def place(seam, is_column, strict):
        n = H if is_column else W
        start = (3 * len(cols) + 5 * len(rows) + 1) % n
        used = set((cols if is_column else rows).values())
        turn = [(start + k) % n for k in range(n)]
        for other in [v for v in turn if v not in used] + [v for v in turn if v in used]:
            y, x = (other, seam) if is_column else (seam, other)
            if ids[y, x] != FLAT_ID:
                continue
            ids[y, x] = next_id[0]
            (cols if is_column else rows)[seam] = other
            if not strict or all_alone():
                next_id[0] += 1
                return True
            ids[y, x] = FLAT_ID
            del (cols if is_column else rows)[seam]
        return False

    for strict in (True, False):      # second pass: a seam that cannot be alone is there all the same
        for x in column_seams(W):
            if x not in cols:
                place(x, True, strict)
        for y in row_seams(H):
            if y not in rows:
                place(y, False, strict)
    ids.setflags(write=False)
    return ids, dict(cols), dict(rows)


def hidden(W, H):
    """The seams of seams(W, H) whose left (upper) pixel is an edge pixel for a second reason as well."""
    ids, cols, rows = seams(W, H)
    return ([("col", x) for x, y in cols.items() if not column_seam_is_alone(ids, y, x)]
            + [("row", y) for y, x in rows.items() if not row_seam_is_alone(ids, y, x)])


# ---- the other families --------------------------------------------------------------------------------
def pixels(W, H):
    return np.arange(W * H, dtype=np.int32).reshape(H, W) + 1


def checker(W, H, a=5, b=9):
    y, x = np.divmod(np.arange(W * H), W)
    return np.where((x + y) % 2 == 0, a, b).astype(np.int32).reshape(H, W)


def flat(W, H):
    return np.full((H, W), FLAT_ID, np.int32)


def uncovered(W, H):
    """Columns of three ids, four pixels wide; no region at (0, 0), at the last pixel, in a whole row, in the
    last column and in the last row (what the size has room for)."""
    ids = (3 + (np.arange(W) // 4) % 3)[None, :].repeat(H, axis=0).astype(np.int32)
    ids[0, 0] = -1
    ids[H - 1, W - 1] = -1
    if H >= 3:
        ids[H // 2, :] = -1
        ids[H - 1, :] = -1
    if W >= 3:
        ids[:, W - 1] = -1
    return ids


BIG_IDS = (0, 1, (1 << 30) + 7, (1 << 31) - 1)


def big_ids(W, H):
    """Regions 0, 1, 2^30 + 7 and 2^31 - 1 as columns next to each other, shifted by one column per row.
    srand(0) is srand(1), so regions 0 and 1 have one colour and no edge between them, in the model too."""
    y, x = np.divmod(np.arange(W * H), W)
    return np.asarray(BIG_IDS, np.int64)[(x + y) % 4].astype(np.int32).reshape(H, W)


RUN_LENGTHS = (1, 15, 16, 17, 63, 64, 65, 129)
RUNS_SIZE = (513, 18)
LONG_ROWS = (8, 9, 10, 11)     # runs of exactly 16 pixels, with the lowest ids of the frame


def runs():
    """513 x 18.  Row r < 8 is made of runs of RUN_LENGTHS[r] pixels, each a region of its own.  A row of 513
    pixels holds 32 runs of 16 pixels, not 64, so rows 8-11 are four more rows of them: their 128 runs have the
    lowest ids, that is they come first in the interval list, and the first two wavefronts' batches take the long
    path throughout.  Row 12 is one run, rows 13-17 repeat rows 1-5 with other ids.  The remainders at the rows'
    ends are regions too."""
    W, H = RUNS_SIZE
    ids = np.zeros((H, W), np.int32)
    x = np.arange(W)
    next_id = 1000
    for r in LONG_ROWS:
        full = W // 16 * 16
        ids[r, :full] = 1 + (r - LONG_ROWS[0]) * (W // 16) + x[:full] // 16
        ids[r, full:] = next_id
        next_id += 1
    for r in list(range(8)) + [12] + list(range(13, 18)):
        L = W if r == 12 else RUN_LENGTHS[r if r < 8 else r - 12]
        ids[r] = next_id + x // L
        next_id += W // L + 1
    return ids


STRIDE_TRIP_SIZE = (1040, 512)
STRIDE_TRIP_INTERVALS = 532480


# ---- the list ----------------------------------------------------------------------------------------------
def _cases():
    out = [Case("seams_%dx%d" % (w, h), "seams", w, h, seams(w, h)[0]) for (w, h) in SIZES]
    extra = {
        "pixels": ((3, 5), (257, 17), (259, 18)),
        "checker": ((1, 15), (8, 16), (513, 18)),
        "flat": ((1, 1), (5, 3), (257, 17), (513, 18)),
        "uncovered": ((5, 3), (7, 5), (257, 17)),
        "ids": ((5, 3), (257, 17)),
    }
    make = {"pixels": pixels, "checker": checker, "flat": flat, "uncovered": uncovered, "ids": big_ids}
    for family, sizes in extra.items():
        for (w, h) in sizes:
            assert (w, h) in SIZES, (family, w, h)
            out.append(Case("%s_%dx%d" % (family, w, h), family, w, h, make[family](w, h)))
    assert RUNS_SIZE in SIZES
    out.append(Case("runs_%dx%d" % RUNS_SIZE, "runs", RUNS_SIZE[0], RUNS_SIZE[1], runs()))
    for c in out:
        c.ids.setflags(write=False)
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def cases_of(family):
    return [c for c in CASES if c.family == family]


def cases_at(W, H):
    return [c for c in CASES if (c.W, c.H) == (W, H)]


def stride_trip_case():
    W, H = STRIDE_TRIP_SIZE
    return Case("stride_trip_%dx%d" % (W, H), "stride_trip", W, H, checker(W, H))


# ---- descriptors, frames, model results (cached; only read them) -----------------------------------------
def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _stride_trip_desc():
    m = lc.desc_from_ids(stride_trip_case().ids)
    return m, m.SerializeToString()


@functools.lru_cache(maxsize=None)
def desc(name):
    """(parsed message, serialized bytes)."""
    if name not in BY_NAME:
        return _stride_trip_desc()
    m = lc.desc_from_ids(BY_NAME[name].ids)
    return m, m.SerializeToString()


@functools.lru_cache(maxsize=None)
def frame(W, H):
    """The source frame of every case of a size: seeded noise, H x W x 3 uint8."""
    return _frozen(np.random.default_rng(1000 * W + H).integers(0, 256, (H, W, 3), dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def filled(name):
    """The model's render buffer after the fill."""
    c = BY_NAME[name] if name in BY_NAME else stride_trip_case()
    return _frozen(rm.fill_colors(desc(name)[0], c.W, c.H, 0, []))


@functools.lru_cache(maxsize=None)
def highlighted(name):
    return _frozen(rm.highlight_edges(filled(name)))


def compose(plane, bgr, blend_alpha=0.5, concat_with_source=False, has_video=True, **_):
    """What RenderModel.render does with the plane it has filled and highlighted."""
    if concat_with_source:
        return np.concatenate([plane, bgr], axis=0)
    if has_video:
        return rm.add_weighted(bgr, plane, float(blend_alpha))
    return plane


def model_render(name, **options):
    """RenderModel(W, H, **options).render(desc, frame) from the cached planes (test_render_edge_cases.py
    holds it against the class itself)."""
    c = BY_NAME[name] if name in BY_NAME else stride_trip_case()
    plane = highlighted(name) if options.get("highlight_edges", True) else filled(name)
    return compose(plane, frame(c.W, c.H), **options)


@functools.lru_cache(maxsize=None)
def model_id_image(name):
    c = BY_NAME[name] if name in BY_NAME else stride_trip_case()
    return _frozen(rm.RenderModel(c.W, c.H).id_image(desc(name)[0], 0))


def interval_lengths(name):
    """The lengths of a case's intervals in the order of the list the fill kernel gets."""
    return [s.right_x - s.left_x + 1 for r in desc(name)[0].region for s in r.raster.scan_inter]


def option_sets():
    """The 18 combinations of test_gpu_render.option_combinations(), then blends whose weights are 0 and 1, exact
    in f32 with ties of another kind (0.25), and inexact in f32 (1/3)."""
    from test_gpu_render import option_combinations
    out = list(option_combinations())
    for alpha in (0.0, 0.25, 1.0 / 3.0):
        out.append(dict(highlight_edges=True, blend_alpha=alpha, has_video=True, concat_with_source=False))
    return out


def option_id(o):
    return "%s-a%.3f-%s" % ("hl" if o["highlight_edges"] else "nohl", o["blend_alpha"],
                            "concat" if o["concat_with_source"] else "blend" if o["has_video"] else "render")
