"""The cases of edge_shape_cases.py do what the GPU tests rely on, checked on the oracle alone: the N4
pass really moves pixels, the wide cases really yield many regions, every border flow really ends on
a border with an absent edge, the extreme bytes really sit at a row's ends."""
import numpy as np
import pytest

import edge_shape_cases as ec
import oracle_lib as ol

ABSENT = 0xFFFF      # key of a temporal edge whose end point lies outside the frame


def moved_pixels(a, b):
    """Pixels that differ between two partitions under the best mapping of a's labels onto b's (a: the
    partition before the N4 pass, b: after it -- a pixel the pass moves leaves its label's image)."""
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    _, ai = np.unique(a, return_inverse=True)
    _, bi = np.unique(b, return_inverse=True)
    nb = int(bi.max()) + 1
    pairs, counts = np.unique(ai.astype(np.int64) * nb + bi, return_counts=True)
    best = np.zeros(int(ai.max()) + 1, np.int64)
    np.maximum.at(best, pairs // nb, counts)
    return int(a.size - best.sum())


def _partition(og, F):
    return np.stack([og.index_image(t) for t in range(F)])


@pytest.mark.parametrize("case", ec.READOUT_CASES, ids=ec.readout_id)
def test_readout_case_moves_pixels(case):
    F = case[3]
    with_n4 = _partition(ec.oracle_readout(case), F)
    without = _partition(ec.oracle_readout(case, enforce_n4=False), F)
    moved = moved_pixels(without, with_n4)
    print("%s: N4 pass moves %d pixels" % (ec.readout_id(case), moved))
    if case in ec.N4_IDLE_CASES:
        assert moved == 0
    else:
        assert moved > 0


def test_idle_cases_are_listed_cases():
    assert ec.N4_IDLE_CASES <= set(ec.READOUT_CASES)
    assert set(ec.FLAG_CASES + ec.FLOW_CASES + ec.UNHASHED_CASES) <= set(ec.READOUT_CASES)


@pytest.mark.parametrize("pattern", ["diag3", "anti3"])
def test_wide_cases_have_many_regions(pattern):
    n = ec.oracle_readout((pattern, 1030, 5, 1, 0)).num_regions()
    print("%s 1030x5: %d regions" % (pattern, n))
    assert n >= 1000


def test_wide_case_moves_pixels():
    F = ec.WIDE_CASE[3]
    moved = moved_pixels(_partition(ec.oracle_readout(ec.WIDE_CASE, enforce_n4=False), F),
                         _partition(ec.oracle_readout(ec.WIDE_CASE), F))
    assert moved > 0


# ---- edge keys --------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", ec.KEY_SIZES)
def test_border_flows_end_on_the_border(W, H):
    _, _, flow, placed = ec.key_inputs(W, H)
    _, _, tb, pidx = ec.oracle_keys(W, H, False, True)
    px, py = ec.model_prev_xy(W, H, flow)
    assert np.array_equal(pidx, py * W + px)     # the oracle against the plain statement of the rule
    for (y, x), k in placed.items():
        fx, fy, side = ec.BORDER_SET[k]
        assert (tb[:, y, x] == ABSENT).any(), (k, y, x)
        on_x = px[y, x] in (0, W - 1)
        on_y = py[y, x] in (0, H - 1)
        if fx is not None:
            assert on_x, (k, y, x)
        if fy is not None:
            assert on_y, (k, y, x)
        # a flow of less than a pixel, or of a pixel that the clamp takes back, stays where it is
        if fx is not None and abs(fx) <= 1.5:
            assert px[y, x] == x
        if fy is not None and abs(fy) <= 1.5:
            assert py[y, x] == y


def test_every_border_row_is_placed_somewhere():
    seen = set()
    for (W, H) in ec.KEY_SIZES:
        seen |= set(ec.key_inputs(W, H)[3].values())
    assert seen == set(range(len(ec.BORDER_SET)))
    # the special values reach both parts of the flow
    for part in (0, 1):
        vals = [r[part] for r in ec.BORDER_SET if r[part] is not None]
        assert any(np.isnan(v) for v in vals) and np.inf in vals and -np.inf in vals
        assert 1e12 in vals and -1e12 in vals and ec.BELOW_2_31 in vals
    assert np.float32(ec.BELOW_2_31) == ec.BELOW_2_31 < 2.0 ** 31
    assert np.nextafter(np.float32(ec.BELOW_2_31), np.float32(np.inf)) == 2.0 ** 31


@pytest.mark.parametrize("W,H", ec.TWO_TILE_SIZES)
@pytest.mark.parametrize("l1", [False, True])
def test_tile_edge_cases_fill_several_buckets(W, H, l1):
    assert W * H in (2048, 2049)
    s0, s1, tb, _ = ec.oracle_keys(W, H, l1, True)
    for keys in (s0, s1, tb):
        real = np.unique(keys[keys != ABSENT])
        assert len(real) > 1


def test_key_sizes_sit_on_the_tile_edges():
    assert sorted({W * H for (W, H) in ec.TILE_EDGE_SIZES}) == [1024, 1025, 2048, 2049]
    assert any(H == 1 for (_, H) in ec.KEY_SIZES) and any(W == 2 for (W, _) in ec.KEY_SIZES)


# ---- min / max ----------------------------------------------------------------------------------------
EXTREME_CASES = [c for c in ec.BILATERAL_CASES if c[2] == "extremes"]


@pytest.mark.parametrize("case", EXTREME_CASES, ids=ec.bilateral_id)
def test_extremes_sit_at_row_ends(case):
    W, H, kind, pad, _ = case
    view, buf = ec.padded_frame(W, H, kind, pad)
    rows = buf[:, :3 * W]
    assert rows.min() == ec.EXTREME_MIN and rows.max() == ec.EXTREME_MAX
    lo = np.argwhere(rows == ec.EXTREME_MIN)
    hi = np.argwhere(rows == ec.EXTREME_MAX)
    assert len(lo) == 1 and lo[0][1] == 0
    assert len(hi) == 1 and hi[0][1] == 3 * W - 1
    assert H == 1 or lo[0][0] != hi[0][0]
    if pad:     # the padding is more extreme than the frame, on both sides
        assert buf[:, 3 * W:].min() == 0 < ec.EXTREME_MIN
        assert buf.max() == 255
        assert pad == 1 and H == 1 or set(np.unique(buf[:, 3 * W:])) == {0, 255}


def test_extremes_reach_head_and_tail_bytes():
    """With rows from a 16-byte aligned start: in some case the minimum is an unaligned row's first
    byte and in some case the maximum the last byte of a row that ends unaligned."""
    head = tail = 0
    for (W, H, kind, pad, _) in EXTREME_CASES:
        lo, hi = ec.extreme_rows(W, H, pad)
        stride = 3 * W + pad
        head += (lo * stride) % 16 != 0
        tail += (hi * stride + 3 * W) % 16 != 0
    assert head >= 5 and tail >= 5


@pytest.mark.parametrize("case", [c for c in ec.BILATERAL_CASES if (c[0], c[1]) != ec.BIG_SIZE],
                         ids=ec.bilateral_id)
def test_oracle_ignores_the_padding(case):
    W, H, kind, pad, pre = case
    view, _ = ec.padded_frame(W, H, kind, pad)
    packed = np.empty((H, W, 3), np.uint8)
    packed[...] = view
    assert packed.strides == (3 * W, 3, 1)
    a, b = ec.oracle_smoothed(*case), ol.preprocess(packed, pre)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_bilateral_cases_follow_the_pruning_rules():
    cases = ec.BILATERAL_CASES
    assert 50 <= len(cases) <= 65 and len(set(cases)) == len(cases)
    for size in ec.FRAME_SIZES:
        assert any((c[0], c[1]) == size and c[4] == 2 for c in cases)
    assert {c[3] for c in cases if c[2] == "extremes"} == set(ec.PADS)
    assert sorted(c[4] for c in cases if (c[0], c[1]) == ec.BIG_SIZE) == [0, 1, 2]
    assert {c[2] for c in cases} == set(ec.FRAME_KINDS) and {c[4] for c in cases} == {0, 1, 2}
    W, H = ec.BIG_SIZE
    assert -(-W // 64) * -(-H // 64) > 256 and W % 64 == 1 and H % 64 == 1
    assert (1400 * 3 // 16 + 255) // 256 == 2      # two blocks along a row in k_minmax_u8


# ---- the width limit -----------------------------------------------------------------------------------
def test_frame_wider_than_the_limit_is_rejected_before_the_device():
    """vsg_graph_create / vsg_stream_create check the frame size first: one pixel past the stated
    limit fails with VSG_ERR_INVALID and a message that names it, with or without a device."""
    import ctypes as C
    import video_segment_amd as vsg
    from video_segment_amd import _lib
    lib = _lib.lib()
    limit = 10224
    h = C.c_void_p()
    assert lib.vsg_graph_create(limit + 1, 3, 1, 0, -1, C.byref(h)) == _lib.VSG_ERR_INVALID
    assert str(limit) in lib.vsg_last_error().decode() and not h
    opts = vsg.default_options()
    assert lib.vsg_stream_create(C.byref(opts), limit + 1, 3, C.byref(h)) == _lib.VSG_ERR_INVALID
    assert str(limit) in lib.vsg_last_error().decode() and not h
