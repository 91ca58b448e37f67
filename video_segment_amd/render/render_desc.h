// render_desc.h -- what the renderer reads of a serialized SegmentationDesc, on the host alone: the region
// colours, the proto reader, the hierarchy lookup and the polygon lines of a vector-only desc.  No HIP call:
// the reader parses bytes it does not trust and is built and run on its own by tests/test_desc_reader.py.
// Like ../common/capi_support.h a part of one translation unit.  Include it after the public header
// (VSG_ERR_*), after ../common/capi_support.h (Throw) and after render.h (Interval, VecLine).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

namespace {

using vsg_render_impl::Interval;
using vsg_render_impl::VecLine;

// ---- glibc rand() ---------------------------------------------------------------------------
// srand(seed) + three rand() calls of glibc's default generator (stdlib/random_r.c: TYPE_3, an
// additive feedback generator of degree 31 and separation 3, seeded by a Lehmer sequence, its first
// 310 outputs discarded), on a private state.
void GlibcColor(int region_id, uint8_t c[3]) {
  uint32_t seed = (uint32_t)region_id;   // srand takes an unsigned int
  if (seed == 0) seed = 1;
  uint32_t state[31];
  int32_t word = (int32_t)seed;
  state[0] = (uint32_t)word;
  for (int i = 1; i < 31; ++i) {
    const int64_t hi = word / 127773, lo = word % 127773;
    int64_t w = 16807 * lo - 2836 * hi;
    if (w < 0) w += 2147483647;
    word = (int32_t)w;
    state[i] = (uint32_t)word;
  }
  int f = 3, r = 0;
  auto next = [&]() {
    const uint32_t val = (state[f] += state[r]);
    if (++f >= 31) {
      f = 0;
      ++r;
    } else if (++r >= 31) {
      r = 0;
    }
    return (int32_t)(val >> 1);
  };
  for (int i = 0; i < 310; ++i) next();
  for (int k = 0; k < 3; ++k) c[k] = (uint8_t)(next() % 255);
}

// ---- minimal proto2 reader --------------------------------------------------------------------
struct Cursor {
  const uint8_t* p;
  const uint8_t* end;
  bool ok = true;
  uint64_t Varint() {
    uint64_t v = 0;
    int shift = 0;
    while (p < end) {
      const uint8_t b = *p++;
      v |= (uint64_t)(b & 0x7f) << shift;
      if (!(b & 0x80)) return v;
      shift += 7;
      if (shift > 63) break;
    }
    ok = false;
    return 0;
  }
  // Next field: number and wire type; a varint's value, or a length-delimited payload in *sub.
  bool Next(int* field, int* wt, Cursor* sub, uint64_t* value) {
    if (p >= end || !ok) return false;
    const uint64_t tag = Varint();
    *field = (int)(tag >> 3);
    *wt = (int)(tag & 7);
    if (*wt == 0) {
      *value = Varint();
    } else if (*wt == 2) {
      const uint64_t n = Varint();
      if (!ok || n > (uint64_t)(end - p)) return ok = false;
      sub->p = p;
      sub->end = p + n;
      sub->ok = true;
      p += n;
    } else if (*wt == 5) {
      if (end - p < 4) return ok = false;
      p += 4;
    } else if (*wt == 1) {
      if (end - p < 8) return ok = false;
      p += 8;
    } else {
      return ok = false;
    }
    return ok;
  }
};

struct CompoundRef {
  int32_t id, parent_id;
};
typedef std::vector<std::vector<CompoundRef>> Hierarchy;   // [level], sorted by id

// What a render needs of a SegmentationDesc: per Region2D its id and where its intervals start in
// `intervals` (value still unset), and the hierarchy.
struct ParsedDesc {
  std::vector<int32_t> region_ids;
  std::vector<size_t> region_begin;   // region_ids.size() + 1 entries
  Hierarchy hierarchy;
  // the vector form: Region2D.vectorization.polygon.coord_idx of all regions back to back,
  // vector_mesh.coord, rasterization_removed
  int frame_w = 0, frame_h = 0;
  bool has_mesh = false, rasterization_removed = false;
  std::vector<float> mesh;
  std::vector<int32_t> coord_idx;
  std::vector<size_t> poly_begin;          // polygons + 1 entries into coord_idx
  std::vector<size_t> region_poly_begin;   // region_ids.size() + 1 entries into poly_begin
};

// repeated int32, packed or not
void ReadInt32s(int wt, Cursor sub, uint64_t v, std::vector<int32_t>* out) {
  if (wt == 0) {
    out->push_back((int32_t)(int64_t)v);
  } else if (wt == 2) {
    while (sub.p < sub.end && sub.ok) out->push_back((int32_t)(int64_t)sub.Varint());
    if (!sub.ok) Throw(VSG_ERR_INVALID, "malformed packed int32");
  }
}

// Region2D.vectorization: polygon{coord_idx = 1, hole = 2}.  A hole is a polygon like any other to
// the scan conversion (its lines run the other way round), so the flag is read past.
void ParseVectorization(Cursor vec, ParsedDesc* d) {
  int f, wt;
  uint64_t v;
  Cursor poly{nullptr, nullptr}, sub{nullptr, nullptr};
  while (vec.Next(&f, &wt, &poly, &v)) {
    if (f != 1 || wt != 2) continue;   // Vectorization.polygon
    while (poly.Next(&f, &wt, &sub, &v)) {
      if (f == 1) ReadInt32s(wt, sub, v, &d->coord_idx);   // Polygon.coord_idx
    }
    if (!poly.ok) Throw(VSG_ERR_INVALID, "malformed Polygon");
    d->poly_begin.push_back(d->coord_idx.size());
  }
  if (!vec.ok) Throw(VSG_ERR_INVALID, "malformed Vectorization");
}

// VectorMesh.coord: repeated float, packed or not.
void ParseMesh(Cursor mesh, std::vector<float>* out) {
  while (mesh.p < mesh.end) {
    const uint64_t tag = mesh.Varint();
    if (!mesh.ok) break;
    const int f = (int)(tag >> 3), wt = (int)(tag & 7);
    const uint8_t* from = nullptr;
    size_t count = 0;
    if (wt == 5) {
      if (mesh.end - mesh.p < 4) Throw(VSG_ERR_INVALID, "malformed VectorMesh");
      from = mesh.p;
      count = 1;
      mesh.p += 4;
    } else if (wt == 2) {
      const uint64_t n = mesh.Varint();
      if (!mesh.ok || n > (uint64_t)(mesh.end - mesh.p)) Throw(VSG_ERR_INVALID, "malformed VectorMesh");
      if (f == 1 && n % 4) Throw(VSG_ERR_INVALID, "packed VectorMesh.coord is not a whole number of floats");
      from = mesh.p;
      count = n / 4;
      mesh.p += n;
    } else if (wt == 0) {
      (void)mesh.Varint();
    } else if (wt == 1) {
      if (mesh.end - mesh.p < 8) Throw(VSG_ERR_INVALID, "malformed VectorMesh");
      mesh.p += 8;
    } else {
      Throw(VSG_ERR_INVALID, "malformed VectorMesh");
    }
    if (f == 1 && count) {   // an empty packed field adds nothing: no memcpy to the null data() of an empty vector
      const size_t at = out->size();
      out->resize(at + count);
      std::memcpy(out->data() + at, from, count * 4);   // little-endian IEEE floats on the wire
    }
  }
  if (!mesh.ok) Throw(VSG_ERR_INVALID, "malformed VectorMesh");
}

// Whether the desc is rendered from its vectorization: rasterization_removed (13) is set and there
// is a vector_mesh (11).  Looks at top-level fields only.
bool IsVectorOnly(const uint8_t* seg, size_t len) {
  Cursor top{seg, seg + len};
  int f, wt;
  uint64_t v;
  Cursor sub{nullptr, nullptr};
  bool removed = false, mesh = false;
  while (top.Next(&f, &wt, &sub, &v)) {
    if (f == 13 && wt == 0) removed = v != 0;
    if (f == 11 && wt == 2) mesh = true;
  }
  return removed && mesh;
}

// vector: read the vectorizations and the mesh instead of the rasters; the desc's frame size may
// then differ from W x H (the caller scales the mesh).
void ParseDesc(const uint8_t* seg, size_t len, int W, int H, bool vector, ParsedDesc* d,
               std::vector<Interval>* intervals) {
  d->region_ids.clear();
  d->region_begin.clear();
  d->hierarchy.clear();
  d->has_mesh = d->rasterization_removed = false;
  d->mesh.clear();
  d->coord_idx.clear();
  d->poly_begin.assign(1, 0);
  d->region_poly_begin.clear();
  intervals->clear();
  Cursor top{seg, seg + len};
  int f, wt;
  uint64_t v;
  Cursor sub{nullptr, nullptr};
  int frame_w = 0, frame_h = 0;
  while (top.Next(&f, &wt, &sub, &v)) {
    if (f == 4 && wt == 0) frame_w = (int)(int64_t)v;
    if (f == 5 && wt == 0) frame_h = (int)(int64_t)v;
    if (f == 13 && wt == 0) d->rasterization_removed = v != 0;
    if (f == 11 && wt == 2) {   // SegmentationDesc.vector_mesh
      d->has_mesh = true;
      if (vector) ParseMesh(sub, &d->mesh);
    }
    if (f == 2 && wt == 2) {   // SegmentationDesc.region
      int id = -1;
      Cursor region = sub, raster{nullptr, nullptr}, rsub{nullptr, nullptr};
      bool has_raster = false;
      d->region_poly_begin.push_back(d->poly_begin.size() - 1);
      while (region.Next(&f, &wt, &rsub, &v)) {
        if (f == 1 && wt == 0) id = (int)(int64_t)v;                      // Region2D.id
        if (f == 3 && wt == 2) { raster = rsub; has_raster = true; }      // Region2D.raster
        if (f == 6 && wt == 2 && vector) ParseVectorization(rsub, d);     // Region2D.vectorization
      }
      if (!region.ok) Throw(VSG_ERR_INVALID, "malformed Region2D");
      d->region_ids.push_back(id);
      d->region_begin.push_back(intervals->size());
      if (!has_raster || vector) continue;
      Cursor scan{nullptr, nullptr}, none{nullptr, nullptr};
      while (raster.Next(&f, &wt, &scan, &v)) {
        if (f != 1 || wt != 2) continue;   // Rasterization.scan_inter
        int y = 0, lx = 0, rx = -1;
        while (scan.Next(&f, &wt, &none, &v)) {
          if (wt != 0) continue;
          if (f == 1) y = (int)(int64_t)v;
          if (f == 2) lx = (int)(int64_t)v;
          if (f == 3) rx = (int)(int64_t)v;
        }
        if (!scan.ok) Throw(VSG_ERR_INVALID, "malformed ScanInterval");
        if (rx < lx) continue;   // paints nothing in the reference's loop either
        // the kernel trusts these bounds
        if (y < 0 || y >= H || lx < 0 || rx >= W) Throw(VSG_ERR_INVALID, "scan interval outside the frame");
        intervals->push_back(Interval{y, lx, rx, 0u});
      }
      if (!raster.ok) Throw(VSG_ERR_INVALID, "malformed Rasterization");
    }
    if (f == 3 && wt == 2) {   // SegmentationDesc.hierarchy
      d->hierarchy.emplace_back();
      std::vector<CompoundRef>& level = d->hierarchy.back();
      Cursor hl = sub, cr{nullptr, nullptr}, none{nullptr, nullptr};
      while (hl.Next(&f, &wt, &cr, &v)) {
        if (f != 2 || wt != 2) continue;   // HierarchyLevel.region
        CompoundRef c{-1, -1};             // parent_id defaults to -1
        while (cr.Next(&f, &wt, &none, &v)) {
          if (f == 1 && wt == 0) c.id = (int)(int64_t)v;
          if (f == 4 && wt == 0) c.parent_id = (int)(int64_t)v;
        }
        if (!cr.ok) Throw(VSG_ERR_INVALID, "malformed CompoundRegion");
        level.push_back(c);
      }
      if (!hl.ok) Throw(VSG_ERR_INVALID, "malformed HierarchyLevel");
      // GetCompoundRegionFromId is a binary search (segmentation_util.cpp:123-136)
      if (!std::is_sorted(level.begin(), level.end(),
                          [](const CompoundRef& a, const CompoundRef& b) { return a.id < b.id; })) {
        Throw(VSG_ERR_INVALID, "hierarchy level is not sorted by region id");
      }
    }
  }
  if (!top.ok) Throw(VSG_ERR_INVALID, "malformed SegmentationDesc");
  d->region_begin.push_back(intervals->size());
  d->region_poly_begin.push_back(d->poly_begin.size() - 1);
  d->frame_w = frame_w;
  d->frame_h = frame_h;
  if (vector) return;
  if ((frame_w && frame_w != W) || (frame_h && frame_h != H)) {
    Throw(VSG_ERR_INVALID, "SegmentationDesc is " + std::to_string(frame_w) + "x" + std::to_string(frame_h) +
                               ", the handle " + std::to_string(W) + "x" + std::to_string(H));
  }
}

// GetParentId(region_id, 0, level, hierarchy), segmentation_util.cpp:166-185.
int ParentId(int region_id, int level, const Hierarchy& hier) {
  int id = region_id;
  for (int l = 0; l < level; ++l) {
    const std::vector<CompoundRef>& regions = hier[l];
    auto it = std::lower_bound(regions.begin(), regions.end(), id,
                               [](const CompoundRef& c, int key) { return c.id < key; });
    if (it == regions.end() || it->id != id) {
      Throw(VSG_ERR_INVALID, "region " + std::to_string(id) + " is not in hierarchy level " + std::to_string(l));
    }
    id = it->parent_id;
  }
  return id;
}

// ---- vector path ----
// Scales the mesh where the desc's frame size is not W x H (ScaleVectorization,
// segmentation_util.cpp:1248-1267; *scaled_mesh is the scratch for it), then one VecLine per kept polygon
// line (:1159-1189) with its crossing count and the prefix sum.  Returns the number of crossings.
int64_t BuildLines(const ParsedDesc& d, int W, int H, std::vector<float>* scaled_mesh, std::vector<VecLine>* lines) {
  const float* coord = d.mesh.data();
  const size_t n_coord = d.mesh.size();
  if (d.frame_w > 0 && d.frame_h > 0 && (d.frame_w != W || d.frame_h != H)) {
    const float scale_x = (float)W * (1.0f / (float)d.frame_w);
    const float scale_y = (float)H * (1.0f / (float)d.frame_h);
    scaled_mesh->resize(n_coord);
    for (size_t k = 0; k < n_coord; ++k) {
      (*scaled_mesh)[k] = k % 2 == 0 ? std::min<float>((float)W, d.mesh[k] * scale_x)
                                     : std::min<float>((float)H, d.mesh[k] * scale_y);
    }
    coord = scaled_mesh->data();
  }
  lines->clear();
  uint64_t total = 0;
  for (size_t r = 0; r < d.region_ids.size(); ++r) {
    for (size_t p = d.region_poly_begin[r]; p < d.region_poly_begin[r + 1]; ++p) {
      for (size_t c = d.poly_begin[p] + 1; c < d.poly_begin[p + 1]; ++c) {
        const int32_t i1 = d.coord_idx[c - 1], i2 = d.coord_idx[c];
        if (i1 < 0 || i2 < 0 || (size_t)i1 + 1 >= n_coord || (size_t)i2 + 1 >= n_coord) {
          Throw(VSG_ERR_INVALID, "coord_idx outside the vector mesh");
        }
        float x1 = coord[i1], y1 = coord[i1 + 1], x2 = coord[i2], y2 = coord[i2 + 1];
        // bounds the accumulated x of every row far inside f32's range
        if (!(std::fabs(x1) <= 16777216.0f && std::fabs(x2) <= 16777216.0f && std::isfinite(y1) &&
              std::isfinite(y2))) {
          Throw(VSG_ERR_INVALID, "vector mesh coordinate is not a usable number");
        }
        if (std::fabs(y1 - y2) < 1e-3f) continue;   // horizontal, :1168
        VecLine l;
        l.is_left = 1;
        if (y2 < y1) {
          std::swap(x1, x2);
          std::swap(y1, y2);
          l.is_left = 0;
        }
        // the reference DCHECKs 0 <= p1.y <= frame_height; its edge_list has frame_height + 1 rows
        if (!(y1 >= 0.0f && y2 <= (float)H)) Throw(VSG_ERR_INVALID, "polygon line outside the frame's rows");
        l.region = (int32_t)r;
        l.y0 = (int)y1;
        l.x = x1;
        l.y_max = y2;
        l.dx = (x2 - x1) / (y2 - y1);
        // active in rows y0, y0 + 1, ... while !(y_max < y + 1): that is floor(y_max) - y0 rows
        const int rows = (int)std::floor(y2) - l.y0;
        l.count = (uint32_t)std::max(rows, 0);
        l.offset = (uint32_t)total;
        total += l.count;
        if (total > (1ull << 31)) Throw(VSG_ERR_INVALID, "more than 2^31 edge crossings in one frame");
        lines->push_back(l);
      }
    }
  }
  if (lines->size() > (1u << 30) || d.region_ids.size() > (1u << 30)) {
    Throw(VSG_ERR_INVALID, "too many polygon lines or regions");
  }
  // an odd total has an odd row somewhere: the reference reads past its active edge list there
  if (total & 1) Throw(VSG_ERR_INVALID, "odd number of edge crossings: a polygon is not closed");
  return (int64_t)total;
}

}  // namespace
