"""CPU checks of the renderer: the colour generator against the process's own libc, the numpy model
(render_model.py) on hand-made SegmentationDescs whose expected pictures are written out here, and the
library's refusal to run without a device."""
import ctypes as C

import numpy as np
import pytest

import render_model as rm
from test_proto_wire import build_schema


@pytest.fixture(scope="module")
def render():
    from video_segment_amd import render as r
    r.build()
    return r


Msg = build_schema()


def make_desc(width, height, regions, hierarchy=()):
    """regions: {id: [(y, left_x, right_x), ...]}; hierarchy: per level {id: parent_id or None}."""
    m = Msg()
    m.frame_width, m.frame_height = width, height
    for rid in sorted(regions):
        r = m.region.add()
        r.id = rid
        for y, lx, rx in regions[rid]:
            s = r.raster.scan_inter.add()
            s.y, s.left_x, s.right_x = y, lx, rx
    for level in hierarchy:
        hl = m.hierarchy.add()
        for rid in sorted(level):
            c = hl.region.add()
            c.id, c.size = rid, 1
            if level[rid] is not None:
                c.parent_id = level[rid]
    return m


def libc_color(region_id):
    libc = C.CDLL(None)
    libc.srand(C.c_uint(region_id & 0xFFFFFFFF))
    return tuple(libc.rand() % 255 for _ in range(3))


def test_color_is_glibc_srand_rand(render):
    """vsg_render_color and the model against srand(id); rand() % 255 of the real libc."""
    rng = np.random.RandomState(7)
    ids = list(range(4096)) + [2 ** 31 - 1, -1, -2 ** 31] + [int(v) for v in rng.randint(-2 ** 31, 2 ** 31, 300)]
    for rid in ids:
        want = libc_color(rid)
        assert render.render_color(rid) == want, rid
        assert rm.color_of(rid) == want, rid


def test_color_leaves_the_process_generator_alone(render):
    libc = C.CDLL(None)
    libc.srand(99)
    first = libc.rand()
    libc.srand(99)
    render.render_color(1234)
    assert libc.rand() == first


def test_no_device_is_an_error(render):
    from video_segment_amd import _lib
    L = render.lib()
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("a GPU is present")
    except ImportError:
        pass
    h = C.c_void_p()
    assert L.vsg_render_create(None, 64, 48, C.byref(h)) == _lib.VSG_ERR_DEVICE
    assert b"no usable HIP device" in L.vsg_render_last_error()
    with pytest.raises(_lib.VsgError) as e:
        render.SegmentationRenderer(64, 48)
    assert e.value.code == _lib.VSG_ERR_DEVICE


def test_default_options_and_stride(render):
    o = render.default_render_options()
    assert (o.blend_alpha, o.hierarchy_level, o.highlight_edges, o.concat_with_source, o.has_video, o.device) == \
        (0.5, 0.0, 1, 0, 1, -1)
    L = render.lib()
    assert [L.vsg_render_default_stride(w) for w in (320, 322, 1, 2)] == [960, 968, 4, 8]
    assert [render.default_stride(w) for w in (320, 322, 1, 2)] == [960, 968, 4, 8]
    import video_segment_amd as v
    assert v.SegmentationRenderer is render.SegmentationRenderer and v.render_color is render.render_color


# ---- the model on hand-made descs ----------------------------------------------------------------
def test_gap_stays_black_and_minus_one():
    # 4 x 3; region 5 covers the left two columns, nobody the rest
    d = make_desc(4, 3, {5: [(0, 0, 1), (1, 0, 1), (2, 0, 1)]})
    m = rm.RenderModel(4, 3, highlight_edges=False, has_video=False)
    out = m.render(d)
    c = libc_color(5)
    assert (out[:, :2] == c).all() and (out[:, 2:] == 0).all()
    ids = m.id_image(d, 0)
    assert (ids[:, :2] == 5).all() and (ids[:, 2:] == -1).all()


def test_highlight_last_row_last_column_and_corner():
    # 3 x 3, four regions: A = top-left 2x2, B = right column rows 0-1, C = bottom row cols 0-1,
    # D = the corner pixel
    A, B, Cc, D = 1, 2, 3, 4
    d = make_desc(3, 3, {A: [(0, 0, 1), (1, 0, 1)], B: [(0, 2, 2), (1, 2, 2)], Cc: [(2, 0, 1)], D: [(2, 2, 2)]})
    m = rm.RenderModel(3, 3, has_video=False)
    out = m.render(d)
    a, b, c, dd = (np.array(libc_color(i), np.uint8) for i in (A, B, Cc, D))
    assert len({tuple(v) for v in (a, b, c, dd)}) == 4 and all(v.any() for v in (a, b, c, dd))
    z = np.zeros(3, np.uint8)
    want = np.array([[a, z, b],     # (0,1): right differs; (0,2) last column: below is B, same
                     [z, z, z],     # (1,0),(1,1): below differs; (1,2) last column: below is D
                     [c, z, dd]])   # (2,0): right same; (2,1) last row: right differs; corner untouched
    assert (out == want).all()
    assert (rm.highlight_edges_literal(rm.fill_colors(d, 3, 3, 0, [])) == want).all()


def test_vectorised_highlight_equals_the_in_place_loop():
    rng = np.random.RandomState(3)
    for _ in range(30):
        h, w = rng.randint(1, 9), rng.randint(1, 9)
        plane = rng.randint(0, 3, (h, w, 1)).astype(np.uint8).repeat(3, axis=2) * 40
        assert (rm.highlight_edges(plane) == rm.highlight_edges_literal(plane)).all()


def hier_desc():
    # 4 x 2: regions 1 | 2 | 3 side by side (columns 0, 1, 2-3); level 1: {1, 2} -> 10, {3} -> 11;
    # level 2: both -> 20.  (Ids 0 and 1 would share a colour: srand takes seed 0 as 1.)
    regions = {1: [(0, 0, 0), (1, 0, 0)], 2: [(0, 1, 1), (1, 1, 1)], 3: [(0, 2, 3), (1, 2, 3)]}
    hierarchy = [{1: 10, 2: 10, 3: 11}, {10: 20, 11: 20}, {20: None}]
    return make_desc(4, 2, regions, hierarchy)


def test_same_parent_has_no_edge_at_level_1_but_one_at_level_0():
    d = hier_desc()
    out0 = rm.RenderModel(4, 2, hierarchy_level=0, has_video=False).render(d)
    out1 = rm.RenderModel(4, 2, hierarchy_level=1, has_video=False).render(d)
    c10, c11 = libc_color(10), libc_color(11)
    assert libc_color(1) != libc_color(2) != libc_color(3) and c10 != c11
    assert (out0[0, 0] == 0).all() and (out0[0, 1] == 0).all()   # edges 1|2 and 2|3
    assert (out0[1, 0] == 0).all()                                # last row: right differs
    assert (out0[:, 2:] == libc_color(3)).all()
    assert (out1[:, 0] == c10).all()                              # 1|2 share parent 10: no edge
    assert (out1[:, 1] == 0).all() and (out1[:, 2:] == c11).all()
    m = rm.RenderModel(4, 2, has_video=False)
    assert (m.id_image(d, 1) == [[10, 10, 11, 11]] * 2).all()
    assert (m.id_image(d, 2) == 20).all()
    with pytest.raises(ValueError):
        m.id_image(d, 3)


def test_fractional_level_and_both_clamps():
    d = hier_desc()                          # three levels
    for level, want in ((0.1, 0), (0.4, 1), (0.75, 2), (0.99, 2), (2.0, 2), (7.0, 2), (1.0, 1)):
        m = rm.RenderModel(4, 2, hierarchy_level=level, has_video=False)
        m.render(d)
        assert m.level == want, level
    # second clamp: a later, lower hierarchy replaces the kept one (segmentation_render.cpp:46-48)
    m = rm.RenderModel(4, 2, hierarchy_level=2, has_video=False, highlight_edges=False)
    m.render(d)
    low = make_desc(4, 2, {5: [(0, 0, 3), (1, 0, 3)]}, [{5: 10}, {10: None}])
    assert m.level == 2 and (m.render(low) == libc_color(10)).all()
    # a desc without hierarchy keeps the last one
    plain = make_desc(4, 2, {7: [(0, 0, 3), (1, 0, 3)]})
    with pytest.raises(AssertionError):
        m.render(plain)                      # region 7 is not in the kept hierarchy's level 0
    # an over-segmentation first: min(level, -1), painted by region id
    m = rm.RenderModel(4, 2, hierarchy_level=0.4, has_video=False, highlight_edges=False)
    assert (m.render(plain) == libc_color(7)).all() and m.level == -1


def test_blend_bytes():
    f32 = np.float32
    s = np.array([[[0, 10, 255], [1, 3, 200], [100, 101, 7]]], np.uint8)
    r = np.array([[[0, 20, 255], [0, 0, 100], [101, 100, 2]]], np.uint8)
    # alpha 0.5: a = b = 0.5, every product and the sum are exact
    #   (0,0)->0  (10,20)->15  (255,255)->255  (1,0)->0.5->0 (even)  (3,0)->1.5->2 (even)
    #   (200,100)->150  (100,101)->100.5->100 (even)  (101,100)->100.5->100  (7,2)->4.5->4 (even)
    assert rm.add_weighted(s, r, 0.5).tolist() == [[[0, 15, 255], [0, 2, 150], [100, 100, 4]]]
    # alpha 0.9: b = f32(0.9), a = 1.0f - b = 0.100000024 (exactly 1 - b in f32)
    b = f32(0.9)
    a = f32(1.0) - b
    assert float(a) == 0.10000002384185791
    want = [[int(np.rint(f32(f32(int(x)) * a) + f32(f32(int(y)) * b))) for x, y in zip(px_s, px_r)]
            for px_s, px_r in zip(s[0], r[0])]
    assert rm.add_weighted(s, r, 0.9).tolist() == [want]
    assert want == [[0, 19, 255], [0, 0, 110], [101, 100, 2]]   # 1+18, 20+90, 10+90.9, 10.1+90, .7+1.8
    # alpha 1: the render itself
    assert (rm.add_weighted(s, r, 1.0) == r).all()


def test_concat_and_no_video():
    d = make_desc(2, 1, {3: [(0, 0, 1)]})
    src = np.array([[[1, 2, 3], [4, 5, 6]]], np.uint8)
    out = rm.RenderModel(2, 1, concat_with_source=True).render(d, src)
    assert out.shape == (2, 2, 3) and (out[0] == libc_color(3)).all() and (out[1] == src[0]).all()
    assert (rm.RenderModel(2, 1, has_video=False, blend_alpha=0.3).render(d) == libc_color(3)).all()
