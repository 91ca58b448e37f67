"""Plain numpy / Python model of the reference's segmentation renderer, restated from reading it (not
collected by pytest; the render tests compare the product against it byte for byte).

  hierarchy state      SegmentationRenderUnit::ProcessFrame, segmentation/segmentation_unit.cpp:567-591
  level clamps         HierarchyColorGenerator, segment_util/segmentation_render.cpp:40-50
  GetParentId          segment_util/segmentation_util.cpp:166-185 (binary search in id-sorted levels)
  colour               srand(id); rand() % 255 three times, segmentation_render.cpp:66-69 (glibc's
                       generator restated below; test_render_model.py pins it to the real libc)
  fill                 RenderRegions, segment_util/segmentation_render.h:136-156, output set to 0 (:205)
  edge highlight       segmentation_render.h:159-182
  compose              segmentation_unit.cpp:612-634; cv::addWeighted on 8-bit data as DESIGN.md section 8
                       states it (OpenCV itself is not available: that one rule is unpinned)
  id image             SegmentationDescToIdImage, segmentation_util.cpp:741-770

Messages are parsed SegmentationDesc objects of test_proto_wire.build_schema().
"""
import bisect

import numpy as np


def glibc_rand3(seed):
    """srand(seed) followed by three rand() calls of glibc (stdlib/random_r.c, TYPE_3: degree 31,
    separation 3; seed 0 is taken as 1; the first 310 outputs are discarded)."""
    seed &= 0xFFFFFFFF                       # srand(unsigned int)
    if seed == 0:
        seed = 1
    word = seed - (1 << 32) if seed >= (1 << 31) else seed   # int32_t word = seed
    state = [word & 0xFFFFFFFF]
    for _ in range(30):
        # C division truncates towards zero
        hi = abs(word) // 127773 * (1 if word >= 0 else -1)
        lo = word - hi * 127773
        word = 16807 * lo - 2836 * hi
        if word < 0:
            word += 2147483647
        state.append(word & 0xFFFFFFFF)
    f, r = 3, 0
    out = []
    for k in range(313):
        state[f] = (state[f] + state[r]) & 0xFFFFFFFF
        val = state[f] >> 1
        f += 1
        if f >= 31:
            f = 0
            r += 1
        else:
            r += 1
            if r >= 31:
                r = 0
        if k >= 310:
            out.append(val)
    return out


_COLORS = {}


def color_of(region_id):
    c = _COLORS.get(region_id)
    if c is None:
        c = _COLORS[region_id] = tuple(v % 255 for v in glibc_rand3(region_id))
    return c


def hierarchy_of(msg):
    """[(sorted ids, parent ids)] per level."""
    return [([c.id for c in lvl.region], [c.parent_id for c in lvl.region]) for lvl in msg.hierarchy]


def get_parent_id(region_id, level, hierarchy):
    """GetParentId(region_id, 0, level, hierarchy)."""
    rid = region_id
    for l in range(level):
        ids, parents = hierarchy[l]
        k = bisect.bisect_left(ids, rid)
        assert k < len(ids) and ids[k] == rid, "region %d is not in level %d" % (rid, l)
        rid = parents[k]
    return rid


def fill_colors(msg, width, height, level, hierarchy):
    """The render buffer after RenderRegions' fill: H x W x 3 uint8, 0 where no region paints."""
    plane = np.zeros((height, width, 3), np.uint8)
    for r in msg.region:
        mapped = get_parent_id(r.id, level, hierarchy) if level > 0 else r.id
        c = color_of(mapped)
        for s in r.raster.scan_inter:
            plane[s.y, s.left_x:s.right_x + 1] = c
    return plane


def highlight_edges_literal(plane):
    """The reference's in-place loop, statement for statement (slow; small inputs only)."""
    out = plane.copy()
    h, w = out.shape[:2]

    def diff(a, b):
        return int(np.abs(a.astype(np.int32) - b.astype(np.int32)).sum())

    for i in range(h - 1):
        for j in range(w - 1):
            if diff(out[i, j], out[i, j + 1]) != 0 or diff(out[i, j], out[i + 1, j]) != 0:
                out[i, j] = 0
        if diff(out[i, w - 1], out[i + 1, w - 1]) != 0:
            out[i, w - 1] = 0
    for j in range(w - 1):
        if diff(out[h - 1, j], out[h - 1, j + 1]) != 0:
            out[h - 1, j] = 0
    return out


def highlight_edges(plane):
    """The same rule for all pixels at once.  The in-place loop compares a pixel with its right and
    its lower neighbour, both of which it decides later, so every comparison reads filled values and
    the result is a function of the filled plane (test_render_model.py checks this against the
    literal loop)."""
    h, w = plane.shape[:2]
    edge = np.zeros((h, w), bool)
    edge[:, :w - 1] |= (plane[:, :w - 1] != plane[:, 1:]).any(axis=2)
    edge[:h - 1, :] |= (plane[:h - 1] != plane[1:]).any(axis=2)
    out = plane.copy()
    out[edge] = 0
    return out


def add_weighted(frame, render, alpha):
    """cv::addWeighted(frame, 1.0f - alpha, render, alpha, 0) on 8-bit data: f32 products and sum,
    each rounded on its own, round half to even, saturated."""
    b = np.float32(alpha)
    a = np.float32(1.0) - b
    t = frame.astype(np.float32) * a + render.astype(np.float32) * b
    assert t.dtype == np.float32
    return np.clip(np.rint(t), 0, 255).astype(np.uint8)


class RenderModel:
    """SegmentationRenderUnit without its streams; same options and state as the product's handle."""

    def __init__(self, width, height, blend_alpha=0.5, hierarchy_level=0.0, highlight_edges=True,
                 concat_with_source=False, has_video=True):
        assert not (concat_with_source and not has_video)
        self.W, self.H = width, height
        self.blend_alpha = float(blend_alpha) if has_video else 1.0
        self.hierarchy_level = np.float32(hierarchy_level)
        self.highlight = bool(highlight_edges)
        self.concat = bool(concat_with_source)
        self.has_video = bool(has_video)
        self.level = None       # resolved on the first frame
        self.kept = []          # seg_hier_'s hierarchy

    def _ingest(self, msg):
        if len(msg.hierarchy) > 0:
            self.kept = hierarchy_of(msg)
        return self.kept

    def render(self, msg, bgr=None):
        hier = self._ingest(msg)
        if self.level is None:
            size = len(msg.hierarchy)
            lvl = self.hierarchy_level
            if lvl != np.floor(lvl):
                lvl = np.float32(int(lvl * np.float32(size)))
            self.level = min(int(lvl), size - 1)
        level = self.level
        if level > 0 and not hier:
            level = 0
        if hier and level >= len(hier):
            level = len(hier) - 1
        plane = fill_colors(msg, self.W, self.H, level, hier)
        if self.highlight:
            plane = highlight_edges(plane)
        if self.concat:
            return np.concatenate([plane, np.asarray(bgr)], axis=0)
        if self.has_video:
            return add_weighted(np.asarray(bgr), plane, self.blend_alpha)
        return plane

    def id_image(self, msg, level=0):
        hier = self._ingest(msg)
        if level < 0 or (level > 0 and level >= len(hier)):
            raise ValueError("level %d is not in the hierarchy" % level)
        out = np.full((self.H, self.W), -1, np.int32)
        for r in msg.region:
            mapped = get_parent_id(r.id, level, hier) if level > 0 else r.id
            for s in r.raster.scan_inter:
                out[s.y, s.left_x:s.right_x + 1] = mapped
        return out


def fnv1a32(arrays):
    """FNV-1a-32 over the bytes of a sequence of arrays (what seg_tree_synth prints as render_fnv1a32)."""
    h = 2166136261
    for a in arrays:
        for b in np.ascontiguousarray(a).tobytes():
            h = ((h ^ b) * 16777619) & 0xFFFFFFFF
    return h
