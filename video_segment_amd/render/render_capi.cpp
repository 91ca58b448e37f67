// render_capi.cpp -- extern "C" entry points declared in include/vsg_render.h: the proto reader, the
// hierarchy state of the reference's SegmentationRenderUnit, the colour table and the device buffers
// around the two kernels of render.hip.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/vsg_render.h"
#include "render.h"
#include "persistence_table.h"
#include "../common/capi_support.h"

namespace {

using vsg_render_impl::AdjStatus;
using vsg_render_impl::BoundStatus;
using vsg_render_impl::ColorStatus;
using vsg_render_impl::CompStatus;
using vsg_render_impl::ContourStatus;
using vsg_render_impl::DistStatus;
using vsg_render_impl::Interval;
using vsg_render_impl::LevelStatus;
using vsg_render_impl::OvlStatus;
using vsg_render_impl::PersStatus;
using vsg_render_impl::VecLine;
using vsg_render_impl::VecStatus;

enum Stage { STAGE_CLEAR = 0, STAGE_FILL, STAGE_COMPOSE, STAGE_COUNT };
enum VecStage { VEC_WALK = 0, VEC_SORT, VEC_PAIRS, VEC_COUNT };
enum LevelStage { LVL_RUNS = 0, LVL_SORT, LVL_TABLE, LVL_MOMENTS, LVL_COUNT };
// CMP_WAIT: the stream idles while the host reads the number of components; reported with no stage
enum CompStage { CMP_LINK = 0, CMP_ORDER, CMP_MOMENTS, CMP_LABEL, CMP_WAIT, CMP_COUNT };
enum BoundStage { BND_COUNT = 0, BND_EMIT, BND_SORT, BND_TABLE, BND_STAGES };
enum AdjStage { ADJ_COUNT = 0, ADJ_EMIT, ADJ_SORT, ADJ_TABLE, ADJ_STAGES };
enum OvlStage { OVL_UPLOAD = 0, OVL_COUNT, OVL_EMIT, OVL_SORT, OVL_TABLE, OVL_STAGES };
// PRS_WAIT: the source frame's upload between the two kernels of a picture; reported with no stage
enum PersStage { PRS_PERSIST = 0, PRS_COMPOSE, PRS_WAIT, PRS_STAGES };
enum ColorStage { CLR_UPLOAD = 0, CLR_SUMS, CLR_TABLE, CLR_PAINT, CLR_STAGES };
enum ContourStage { CNT_CLASSIFY = 0, CNT_TRACE, CNT_TABLE, CNT_STAGES };
enum MeshStage { MSH_SPLIT = 0, MSH_TABLE, MSH_STAGES };
// DST_PLANE: the upload of a host label plane
enum DistStage { DST_PLANE = 0, DST_CLASSIFY, DST_COLUMNS, DST_ROWS, DST_MATCH, DST_STAGES };

double NowMs() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch())
      .count();
}

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
    if (f == 1 && from) {
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

}  // namespace

struct vsg_render {
  vsg_render_options opt;
  int device = 0, W = 0, H = 0, pitch = 0;
  hipStream_t stream = nullptr;
  // clear, fill, compose; the vector path's walk, sort, pairs; the level stages; the component stages
  StageClock clock, vclock, lclock, cclock, bclock, aclock, oclock, pclock, kclock, tclock, dclock, mclock;
  // SegmentationRenderUnit's state
  bool level_resolved = false;
  int level = 0;
  Hierarchy kept;
  // scratch of a call
  ParsedDesc desc;
  std::vector<Interval> intervals;
  std::unordered_map<int32_t, uint32_t> colors;   // mapped id -> packed colour (a pure function)
  Block d_intervals, h_intervals, d_plane, d_src, d_out, d_ids;
  // the vector path: lines and per-region values (host, then one upload), crossings (two key and two
  // value arrays for the sort), the sort's work space, the status words
  std::vector<VecLine> lines;
  std::vector<uint32_t> region_value;
  std::vector<float> scaled_mesh;
  Block d_vec_in, d_cross, d_sort_temp, d_status, h_status;
  // level regions: unsorted runs (keys, right ends), sorted runs with their ranks, the two lists,
  // the status words, and the pinned block the status and host outputs come back through
  Block d_runs, d_sorted, d_level_regions, d_level_intervals, d_level_status, h_level;
  // level components: the union-find's parents, labels and indices with their sorted copies and the
  // components' ranks; the component table; the ordered intervals; the same with component indices
  // for the label fill; every region's first component; the label plane of a host output; the status
  // words and the pinned block they come back through
  Block d_comp_work, d_comp_table, d_comp_intervals, d_comp_fill, d_comp_first, d_labels, d_comp_status, h_comp;
  // level boundaries: unsorted and sorted keys; their groups' ranks; the points; the records; the
  // status words and the pinned block the status and host outputs come back through
  Block d_bound_keys, d_bound_rank, d_bound_points, d_bound_records, d_bound_status, h_bound;
  // level adjacency: unsorted and sorted keys; their node and edge heads' counts; the nodes; the edges;
  // the status words and the pinned block the status and host outputs come back through
  Block d_adj_keys, d_adj_heads, d_adj_nodes, d_adj_edges, d_adj_status, h_adj;
  // level overlap: a host B on the device and the pinned block it goes through; the count pass's words of
  // every frame row; unsorted and sorted runs
  // (keys, lengths), the unsorted halves taken again for the column sort's operands; the two scans, taken
  // again for the sorted column operands and their ranks; the distinct keys (key, rank, start) and the
  // columns' first keys; rows, columns, pairs; the status words and the pinned block the status and host
  // outputs come back through
  Block d_other, h_other, d_ovl_totals, d_ovl_runs, d_ovl_heads, d_ovl_keys, d_ovl_rows, d_ovl_cols, d_ovl_pairs,
      d_ovl_status, h_ovl;
  // boundary persistence: the region ids the ancestor table's columns stand for and the table (host, then
  // one upload through the pinned block into d_anc: ids, then rows); the persistence plane of a picture or
  // of a host output; the edges' persistences, the histogram and the levels' sides; the status words
  std::vector<int32_t> pers_ids, pers_table;
  Block d_anc, d_pq, d_pers_out, d_pers_status, h_pers;
  // level colours: the intervals' partials; what the records gather; the records of a host output or of a
  // picture; the interval list with the means as values; the status words and the pinned block the status,
  // the number of records and a host table come back through
  Block d_color_partials, d_color_acc, d_color_records, d_color_intervals, d_color_status, h_color;
  // level contours: the pixels' crack masks and offsets; what there is per crack (the two doubling states,
  // key, successor, leader, place, the vertices' owners; the vertices take the doubling state that is free
  // at the end); what there is per contour slot (unsorted and sorted keys, group ranks, vertex counts and
  // offsets); the records; the status words and the pinned block the status and host outputs come back
  // through
  Block d_cont_mask, d_cont_offset, d_cont_cracks, d_cont_slots, d_cont_records, d_cont_status, h_cont;
  // level mesh: what there is per crack and per contour (the third doubling's two states, the unsorted owner
  // keys, half, head and last crack of a half, a half's segment, the contours' junction marks, ref counts and
  // offsets, the cracks' sides); what there is per segment, vertex, loop and ref (sorted keys, vertex counts
  // and offsets, the four lists, the vertices' segments); the status words and the pinned block the status
  // and host outputs come back through
  Block d_mesh_cracks, d_mesh_lists, d_mesh_status, h_mesh;
  // boundary distance: the edge set's words; the columns' squared distances; D of a host output or of the
  // other plane's edge set; the three histograms; the records of a host output; the status words and the
  // pinned block they come back through
  Block d_dist_words, d_dist_gsq, d_dist_out, d_dist_hist, d_dist_scores, d_dist_status, h_dist;
  int64_t allocations = 0;
  vsg_render_stats stats;
  vsg_render_vector_stats vstats;
  vsg_render_level_stats lstats;
  vsg_render_component_stats cstats;
  vsg_render_boundary_stats bstats;
  vsg_render_adjacency_stats astats;
  vsg_render_overlap_stats ostats;
  vsg_render_persistence_stats pstats;
  vsg_render_color_stats kstats;
  vsg_render_contour_stats tstats;
  vsg_render_distance_stats dstats;
  vsg_render_mesh_stats mstats;

  ~vsg_render() {
    if (!stream) return;
    (void)hipStreamSynchronize(stream);
    (void)hipStreamDestroy(stream);
  }

  // Interval list to the device through the pinned block (rewritten only after the stream drained:
  // every call ends with a synchronisation).
  void UploadIntervals() {
    const size_t bytes = intervals.size() * sizeof(Interval);
    if (!bytes) return;
    h_intervals.Reserve(bytes, &allocations);
    d_intervals.Reserve(bytes, &allocations);
    std::memcpy(h_intervals.p, intervals.data(), bytes);
    VSG_HIP(hipMemcpyAsync(d_intervals.p, h_intervals.p, bytes, hipMemcpyHostToDevice, stream));
    ++stats.launches;
  }

  void FinishStats() {
    VSG_HIP(hipStreamSynchronize(stream));
    float us[STAGE_COUNT];
    clock.Read(us, STAGE_COUNT);
    stats.clear_us = us[STAGE_CLEAR];
    stats.fill_us = us[STAGE_FILL];
    stats.compose_us = us[STAGE_COMPOSE];
    stats.device_allocations = allocations;
  }

  // ---- vector path ----
  // Scales the mesh where the desc's frame size is not the handle's (ScaleVectorization,
  // segmentation_util.cpp:1248-1267), then one VecLine per kept polygon line (:1159-1189) with its
  // crossing count and the prefix sum.  Returns the number of crossings.
  int64_t BuildLines() {
    const ParsedDesc& d = desc;
    const float* coord = d.mesh.data();
    const size_t n_coord = d.mesh.size();
    if (d.frame_w > 0 && d.frame_h > 0 && (d.frame_w != W || d.frame_h != H)) {
      const float scale_x = (float)W * (1.0f / (float)d.frame_w);
      const float scale_y = (float)H * (1.0f / (float)d.frame_h);
      scaled_mesh.resize(n_coord);
      for (size_t k = 0; k < n_coord; ++k) {
        scaled_mesh[k] = k % 2 == 0 ? std::min<float>((float)W, d.mesh[k] * scale_x)
                                    : std::min<float>((float)H, d.mesh[k] * scale_y);
      }
      coord = scaled_mesh.data();
    }
    lines.clear();
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
          lines.push_back(l);
        }
      }
    }
    if (lines.size() > (1u << 30) || d.region_ids.size() > (1u << 30)) {
      Throw(VSG_ERR_INVALID, "too many polygon lines or regions");
    }
    // an odd total has an odd row somewhere: the reference reads past its active edge list there
    if (total & 1) Throw(VSG_ERR_INVALID, "odd number of edge crossings: a polygon is not closed");
    return (int64_t)total;
  }

  // Uploads lines and region values, then walk -> sort -> pairs on the stream.  Leaves n_cross / 2
  // intervals in d_intervals.  CheckVector has to be called after the stream has drained.
  void RunVector(int64_t n_cross) {
    using namespace vsg_render_impl;
    std::memset(&vstats, 0, sizeof(vstats));
    vstats.lines = (int64_t)lines.size();
    vstats.crossings = n_cross;
    if (n_cross == 0) return;
    const size_t n = (size_t)n_cross;
    const size_t lines_bytes = lines.size() * sizeof(VecLine);
    const size_t values_bytes = region_value.size() * sizeof(uint32_t);
    int region_bits = 1;
    while (region_bits < 31 && (region_value.size() >> region_bits)) ++region_bits;
    const int end_bit = kVecRowBits + region_bits;
    const size_t temp_bytes = std::max<size_t>(VecSortTempBytes(n_cross, end_bit), 16);
    h_intervals.Reserve(lines_bytes + values_bytes, &allocations);
    d_vec_in.Reserve(lines_bytes + values_bytes, &allocations);
    d_cross.Reserve(4 * n * sizeof(unsigned long long), &allocations);
    d_sort_temp.Reserve(temp_bytes, &allocations);
    d_intervals.Reserve(n / 2 * sizeof(Interval), &allocations);
    d_status.Reserve(sizeof(VecStatus), &allocations);
    h_status.Reserve(sizeof(VecStatus), &allocations);
    std::memcpy(h_intervals.p, lines.data(), lines_bytes);
    std::memcpy(static_cast<char*>(h_intervals.p) + lines_bytes, region_value.data(), values_bytes);
    VSG_HIP(hipMemcpyAsync(d_vec_in.p, h_intervals.p, lines_bytes + values_bytes, hipMemcpyHostToDevice, stream));
    const VecLine* d_lines = static_cast<const VecLine*>(d_vec_in.p);
    const uint32_t* d_values = reinterpret_cast<const uint32_t*>(static_cast<const char*>(d_vec_in.p) + lines_bytes);
    unsigned long long* keys = static_cast<unsigned long long*>(d_cross.p);
    unsigned long long* vals = keys + n;
    unsigned long long* keys_sorted = keys + 2 * n;
    unsigned long long* vals_sorted = keys + 3 * n;
    VecStatus* status = static_cast<VecStatus*>(d_status.p);
    VSG_HIP(hipMemsetAsync(status, 0, sizeof(VecStatus), stream));
    // every entry of the list is in the frame whatever the pairs stage leaves unwritten on bad input
    VSG_HIP(hipMemsetAsync(d_intervals.p, 0, n / 2 * sizeof(Interval), stream));
    vclock.Begin(stream);
    LaunchVecWalk(d_lines, (int)lines.size(), keys, vals, status, stream);
    vclock.Mark(VEC_WALK);
    VSG_HIP(VecSort(d_sort_temp.p, temp_bytes, keys, keys_sorted, vals, vals_sorted, n_cross, end_bit, stream));
    vclock.Mark(VEC_SORT);
    LaunchVecPairs(keys_sorted, vals_sorted, d_lines, (uint32_t)lines.size(), d_values,
                   (uint32_t)region_value.size(), n_cross, W, H, static_cast<Interval*>(d_intervals.p), status, stream);
    VSG_HIP(hipGetLastError());
    vclock.Mark(VEC_PAIRS);
    VSG_HIP(hipMemcpyAsync(h_status.p, status, sizeof(VecStatus), hipMemcpyDeviceToHost, stream));
    vstats.launches = 7;   // upload, two clears, walk, the sort counted as one, pairs, status
    stats.launches += vstats.launches;
  }

  // After the call's one synchronisation: stage times, group statistics, the device flag.
  void CheckVector() {
    if (vstats.crossings == 0) return;
    float us[VEC_COUNT];
    vclock.Read(us, VEC_COUNT);
    vstats.walk_us = us[VEC_WALK];
    vstats.sort_us = us[VEC_SORT];
    vstats.pairs_us = us[VEC_PAIRS];
    const VecStatus* st = static_cast<const VecStatus*>(h_status.p);
    vstats.groups = (int64_t)st->groups;
    vstats.largest_group = (int64_t)st->largest_group;
    if (st->flags & vsg_render_impl::VEC_FLAG_INTERNAL) Throw(VSG_ERR_INTERNAL, "the edge walk and the host's row counts disagree");
    if (st->flags & vsg_render_impl::VEC_FLAG_UNSPECIFIED) {
      Throw(VSG_ERR_INVALID,
            "the vectorization has a row the reference does not define: an odd number of active edges, edges "
            "it cannot order, or an interval outside the frame");
    }
  }
};

namespace {

// Parses the desc, applies the hierarchy bookkeeping both entry points share (a desc that carries a
// hierarchy replaces the kept one) and returns the hierarchy to map ids with.
const Hierarchy& Ingest(vsg_render* h, const uint8_t* seg, size_t seg_len, bool* vector) {
  if (!seg && seg_len) Throw(VSG_ERR_INVALID, "seg is null");
  *vector = IsVectorOnly(seg, seg_len);
  ParseDesc(seg, seg_len, h->W, h->H, *vector, &h->desc, &h->intervals);
  if (!h->desc.hierarchy.empty()) h->kept = h->desc.hierarchy;
  return h->kept;
}

// Sets every interval's value to value_of(mapped id of its region); returns the distinct mapped ids.
template <class ValueOf>
int64_t AssignValues(vsg_render* h, int level, const Hierarchy& hier, ValueOf value_of) {
  std::unordered_map<int32_t, uint32_t> seen;   // one lookup and one colour per distinct id and frame
  const ParsedDesc& d = h->desc;
  for (size_t r = 0; r < d.region_ids.size(); ++r) {
    if (d.region_begin[r] == d.region_begin[r + 1]) continue;
    const int mapped = level > 0 ? ParentId(d.region_ids[r], level, hier) : d.region_ids[r];
    auto it = seen.find(mapped);
    if (it == seen.end()) it = seen.emplace(mapped, value_of(mapped)).first;
    for (size_t k = d.region_begin[r]; k < d.region_begin[r + 1]; ++k) h->intervals[k].value = it->second;
  }
  return (int64_t)seen.size();
}

// The same for a vector-only desc: one value per region that has a polygon, in h->region_value.
template <class ValueOf>
int64_t AssignRegionValues(vsg_render* h, int level, const Hierarchy& hier, ValueOf value_of) {
  std::unordered_map<int32_t, uint32_t> seen;
  const ParsedDesc& d = h->desc;
  h->region_value.assign(d.region_ids.size(), 0u);
  for (size_t r = 0; r < d.region_ids.size(); ++r) {
    if (d.region_poly_begin[r] == d.region_poly_begin[r + 1]) continue;
    const int mapped = level > 0 ? ParentId(d.region_ids[r], level, hier) : d.region_ids[r];
    auto it = seen.find(mapped);
    if (it == seen.end()) it = seen.emplace(mapped, value_of(mapped)).first;
    h->region_value[r] = it->second;
  }
  return (int64_t)seen.size();
}

// The front half of vsg_render_id_image: ingests the desc, checks the level, maps every region to
// value_of(its id at `level`) and paints the W-pitched plane `ids` (device memory; -1 where no region
// is).  Leaves clock between STAGE_FILL and the next mark, and the vector path's status in flight:
// the caller calls CheckVector after its synchronisation when the desc was vector-only (returned).
// The plane's rows are `pitch` values apart, all of them cleared; ready() is called once every region has
// its value, before any device work.
template <class ValueOf, class Ready>
bool PaintIdsAt(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, uint32_t* ids, int pitch,
                ValueOf value_of, Ready ready) {
  const int H = h->H;
  std::memset(&h->stats, 0, sizeof(h->stats));
  std::memset(&h->vstats, 0, sizeof(h->vstats));
  const double t0 = NowMs();
  bool vector = false;
  const Hierarchy& hier = Ingest(h, seg, seg_len, &vector);
  if (level < 0 || (level > 0 && level >= (int)hier.size())) {
    Throw(VSG_ERR_INVALID, "level " + std::to_string(level) + " is not in the hierarchy (" +
                               std::to_string(hier.size()) + " levels)");
  }
  int64_t n_cross = 0;
  if (vector) {
    h->stats.distinct_ids = AssignRegionValues(h, level, hier, value_of);
    n_cross = h->BuildLines();
  } else {
    h->stats.distinct_ids = AssignValues(h, level, hier, value_of);
  }
  const int64_t n_intervals = vector ? n_cross / 2 : (int64_t)h->intervals.size();
  h->stats.intervals = n_intervals;
  ready();
  const double t1 = NowMs();
  h->stats.decode_ms = t1 - t0;
  if (vector) h->RunVector(n_cross);
  else h->UploadIntervals();
  const size_t bytes = (size_t)pitch * H * sizeof(int32_t);
  h->stats.upload_ms = NowMs() - t1;
  h->clock.Begin(h->stream);
  VSG_HIP(hipMemsetAsync(ids, 0xff, bytes, h->stream));   // -1: no region
  h->clock.Mark(STAGE_CLEAR);
  vsg_render_impl::LaunchFill(static_cast<const Interval*>(h->d_intervals.p), n_intervals, ids, pitch, h->stream);
  VSG_HIP(hipGetLastError());
  h->clock.Mark(STAGE_FILL);
  h->stats.launches += 1 + (n_intervals == 0 ? 0 : 1);
  return vector;
}

// The W-pitched plane of vsg_render_id_image and the level calls.
template <class ValueOf>
bool PaintIds(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, uint32_t* ids, ValueOf value_of) {
  return PaintIdsAt(h, seg, seg_len, level, ids, h->W, value_of, [] {});
}

// What the front half of the level calls leaves behind: n runs, unsorted (keys, rights) and, after
// SortLevelRuns, sorted with their regions' ranks, as intervals, and with id and first interval of every
// region in `regions`.
struct LevelFront {
  bool vector = false;
  uint32_t n = 0, cap_runs = 0, cap_regions = 0;
  int32_t max_id = 0;
  unsigned long long* keys = nullptr;
  uint32_t* rights = nullptr;
  LevelStatus* status = nullptr;
  unsigned long long* keys_sorted = nullptr;
  uint32_t* rights_sorted = nullptr;
  uint32_t* rank = nullptr;
  int32_t* regions = nullptr;
  Interval* intervals = nullptr;
};

// The id plane of the level calls in h->d_ids, as vsg_render_id_image paints it, with their rule for
// ids; *max_id receives the largest id.  Returns whether the desc was vector-only; the rest as PaintIds.
bool PaintLevelPlane(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int32_t* max_id) {
  h->d_ids.Reserve((size_t)h->W * h->H * sizeof(int32_t), &h->allocations);
  *max_id = 0;
  return PaintIds(h, seg, seg_len, level, h->d_ids.As<uint32_t>(), [&](int mapped) {
    // -1 is the plane's "no region"; the sort key takes the id as an unsigned number
    if (mapped < 0) Throw(VSG_ERR_INVALID, "region id " + std::to_string(mapped) + " is negative");
    *max_id = std::max(*max_id, mapped);
    return (uint32_t)mapped;
  });
}

// Paints the id plane as vsg_render_id_image does, finds its runs and waits for their number, which
// sizes everything after it.  Fills the run fields of *ls.
LevelFront PaintLevelRuns(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, vsg_render_level_stats* ls) {
  using namespace vsg_render_impl;
  const int W = h->W, H = h->H;
  LevelFront f;
  // ---- the id plane, as vsg_render_id_image paints it ----
  f.vector = PaintLevelPlane(h, seg, seg_len, level, &f.max_id);

  // ---- runs ----
  // Intervals that do not overlap give at most one run each; every end of an interval that lies
  // on another one can add a run.  The kernel drops what has no slot and says so.
  const uint64_t painted = (uint64_t)h->stats.intervals;
  const uint32_t cap_runs = (uint32_t)std::min<uint64_t>(2 * painted + 1, (uint64_t)W * H);
  h->d_runs.Reserve((size_t)cap_runs * 12, &h->allocations);
  h->d_level_status.Reserve(sizeof(LevelStatus), &h->allocations);
  h->h_level.Reserve(2 * sizeof(LevelStatus), &h->allocations);
  f.cap_runs = cap_runs;
  f.keys = h->d_runs.As<unsigned long long>();
  f.rights = reinterpret_cast<uint32_t*>(f.keys + cap_runs);
  f.status = h->d_level_status.As<LevelStatus>();
  LevelStatus* seen = h->h_level.As<LevelStatus>();   // [0] after the runs, [1] at the end
  VSG_HIP(hipMemsetAsync(f.status, 0, sizeof(LevelStatus), h->stream));
  h->lclock.Begin(h->stream);
  LaunchLevelRuns(h->d_ids.As<int32_t>(), W, W, H, cap_runs, f.keys, f.rights, f.status, h->stream);
  VSG_HIP(hipGetLastError());
  h->lclock.Mark(LVL_RUNS);
  VSG_HIP(hipMemcpyAsync(&seen[0], f.status, sizeof(LevelStatus), hipMemcpyDeviceToHost, h->stream));
  ls->launches = 3;
  VSG_HIP(hipStreamSynchronize(h->stream));   // the run count sizes everything below
  {
    float us[STAGE_COUNT], lus[LVL_COUNT];
    h->clock.Read(us, STAGE_COUNT);
    h->stats.clear_us = us[STAGE_CLEAR];
    h->stats.fill_us = us[STAGE_FILL];
    h->lclock.Read(lus, LVL_COUNT);
    ls->runs_us = lus[LVL_RUNS];
  }
  if (f.vector) h->CheckVector();
  if (seen[0].overflow || seen[0].runs > cap_runs) Throw(VSG_ERR_INTERNAL, "more runs than the intervals allow");
  f.n = seen[0].runs;
  ls->runs = f.n;
  // every region has a run, and every id of the plane is one of the host's distinct mapped ids
  f.cap_regions = (uint32_t)std::min<uint64_t>(f.n, (uint64_t)h->stats.distinct_ids);
  return f;
}

// The n > 0 runs into (id, y, left_x) order, their regions' ranks, the interval list and the heads of
// the region table; restarts lclock and leaves it after LVL_TABLE.
void SortLevelRuns(vsg_render* h, LevelFront* f, vsg_render_level_stats* ls) {
  using namespace vsg_render_impl;
  const uint32_t n = f->n;
  int id_bits = 1;
  while (id_bits < 31 && (f->max_id >> id_bits)) ++id_bits;
  const int end_bit = 32 + id_bits;
  const size_t temp_bytes = std::max<size_t>(LevelTempBytes(n, end_bit), 16);
  h->d_sort_temp.Reserve(temp_bytes, &h->allocations);
  h->d_sorted.Reserve((size_t)n * 16, &h->allocations);
  h->d_level_regions.Reserve((size_t)f->cap_regions * sizeof(vsg_render_level_region), &h->allocations);
  h->d_level_intervals.Reserve((size_t)n * sizeof(Interval), &h->allocations);
  f->keys_sorted = h->d_sorted.As<unsigned long long>();
  f->rights_sorted = reinterpret_cast<uint32_t*>(f->keys_sorted + n);
  f->rank = f->rights_sorted + n;
  f->regions = h->d_level_regions.As<int32_t>();
  f->intervals = h->d_level_intervals.As<Interval>();
  h->lclock.Begin(h->stream);
  VSG_HIP(LevelSort(h->d_sort_temp.p, temp_bytes, f->keys, f->keys_sorted, f->rights, f->rights_sorted, n, end_bit,
                    h->stream));
  h->lclock.Mark(LVL_SORT);
  VSG_HIP(LevelRank(h->d_sort_temp.p, temp_bytes, f->keys_sorted, f->rank, n, h->stream));
  LaunchLevelTable(f->keys_sorted, f->rights_sorted, f->rank, n, h->W, f->cap_regions, f->intervals, f->regions,
                   f->status, h->stream);
  VSG_HIP(hipGetLastError());
  h->lclock.Mark(LVL_TABLE);
  ls->launches += 3;   // the sort and the scan count as one each
}

// vsg_render_level_components behind its argument checks.  labels_only: the call is made for
// vsg_render_level_boundaries, which needs the label image in h->d_labels and id and component of every
// entry of h->d_comp_table and nothing else: no output is looked at, no capacity is checked, the moments
// are not computed and nothing is delivered but the two counts.
void LevelComponents(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness,
                     vsg_render_level_component* components, size_t capacity_components, size_t* num_components,
                     int32_t* intervals, size_t capacity_intervals, size_t* num_intervals, int32_t* label_image,
                     int mem_out, bool labels_only) {
  using namespace vsg_render_impl;
  CheckMem(mem_out, "outputs");
  const bool count_only = !labels_only && !components && !intervals && !label_image && capacity_components == 0 &&
                          capacity_intervals == 0;
  const bool paint_labels = labels_only || label_image;
  const int W = h->W, H = h->H;
  if ((uint64_t)W * (uint64_t)H >= (1ull << 32)) Throw(VSG_ERR_INVALID, "the frame has 2^32 pixels or more");
  DeviceGuard guard(h->device);
  vsg_render_component_stats& cs = h->cstats;
  std::memset(&cs, 0, sizeof(cs));
  vsg_render_level_stats ls;   // of the shared front half; the last level_regions call's stay
  std::memset(&ls, 0, sizeof(ls));

  LevelFront f = PaintLevelRuns(h, seg, seg_len, level, &ls);
  const uint32_t n = f.n;
  *num_intervals = n;
  cs.runs = n;
  cs.runs_us = ls.runs_us;
  if (!count_only && !labels_only && n && n <= capacity_intervals && (!components || !intervals)) {
    Throw(VSG_ERR_INVALID, "an output is null");
  }
  h->d_comp_status.Reserve(sizeof(CompStatus), &h->allocations);
  h->h_comp.Reserve(2 * sizeof(CompStatus) + sizeof(LevelStatus), &h->allocations);
  CompStatus* status = h->d_comp_status.As<CompStatus>();
  CompStatus* seen = h->h_comp.As<CompStatus>();   // [0] once the table is made, [1] at the end
  LevelStatus* seen_level = reinterpret_cast<LevelStatus*>(seen + 2);
  std::memset(seen, 0, 2 * sizeof(CompStatus) + sizeof(LevelStatus));
  Interval* ordered = nullptr;
  Interval* fill = nullptr;
  int32_t* table = nullptr;
  int launches = 0;
  if (!n) h->cclock.Begin(h->stream);   // an empty frame still clears the label image
  if (n) {
    // ---- the runs sorted by (id, y, left_x), as vsg_render_level_regions has them ----
    int label_bits = 1;
    while (label_bits < 32 && ((uint64_t)(n - 1) >> label_bits)) ++label_bits;
    const size_t temp_bytes = std::max<size_t>(CompTempBytes(n, label_bits), 16);
    h->d_sort_temp.Reserve(temp_bytes, &h->allocations);   // before anything that uses the block is enqueued
    SortLevelRuns(h, &f, &ls);

    // ---- union-find, order, table ----
    h->d_comp_work.Reserve((size_t)n * 6 * sizeof(uint32_t), &h->allocations);
    h->d_comp_table.Reserve((size_t)n * sizeof(vsg_render_level_component), &h->allocations);
    h->d_comp_intervals.Reserve((size_t)n * sizeof(Interval), &h->allocations);
    h->d_comp_first.Reserve((size_t)f.cap_regions * sizeof(uint32_t), &h->allocations);
    if (paint_labels) h->d_comp_fill.Reserve((size_t)n * sizeof(Interval), &h->allocations);
    uint32_t* parent = h->d_comp_work.As<uint32_t>();
    uint32_t* label = parent + n;
    uint32_t* index = label + n;
    uint32_t* label_sorted = index + n;
    uint32_t* order = label_sorted + n;
    uint32_t* comp_rank = order + n;
    ordered = h->d_comp_intervals.As<Interval>();
    fill = paint_labels ? h->d_comp_fill.As<Interval>() : nullptr;
    table = h->d_comp_table.As<int32_t>();
    VSG_HIP(hipMemsetAsync(status, 0, sizeof(CompStatus), h->stream));
    h->cclock.Begin(h->stream);
    LaunchCompLink(f.keys_sorted, f.rights_sorted, n, W, connectedness == VSG_RENDER_CONNECT_N8 ? 1 : 0, parent,
                   label, index, status, h->stream);
    VSG_HIP(hipGetLastError());
    h->cclock.Mark(CMP_LINK);
    VSG_HIP(CompSort(h->d_sort_temp.p, temp_bytes, label, label_sorted, index, order, n, label_bits, h->stream));
    VSG_HIP(CompRank(h->d_sort_temp.p, temp_bytes, label_sorted, comp_rank, n, h->stream));
    // a run has at most one component: n slots hold them all
    LaunchCompTable(label_sorted, order, comp_rank, f.rank, f.intervals, n, n, f.cap_regions, ordered, fill, table,
                    h->d_comp_first.As<uint32_t>(), f.status, status, h->stream);
    VSG_HIP(hipGetLastError());
    h->cclock.Mark(CMP_ORDER);
    VSG_HIP(hipMemcpyAsync(&seen[0], status, sizeof(CompStatus), hipMemcpyDeviceToHost, h->stream));
    VSG_HIP(hipMemcpyAsync(seen_level, f.status, sizeof(LevelStatus), hipMemcpyDeviceToHost, h->stream));
    launches += 11;   // the clear, five kernels, two copies; the sorts and the scans count as one each
    VSG_HIP(hipStreamSynchronize(h->stream));   // the number of components decides what is delivered
    if (seen_level->regions == 0 || seen_level->regions > f.cap_regions) {
      Throw(VSG_ERR_INTERNAL, "the plane has more regions than the desc has ids");
    }
    if (seen[0].flags & COMP_FLAG_BOUND) Throw(VSG_ERR_INTERNAL, "the union-find did not end within its bound");
    if ((seen[0].flags & COMP_FLAG_DROPPED) || seen[0].components == 0 || seen[0].components > n) {
      Throw(VSG_ERR_INTERNAL, "a component had no slot");
    }
  }
  const uint32_t n_components = seen[0].components;
  *num_components = n_components;
  cs.regions = seen_level->regions;
  cs.components = n_components;
  cs.links = (int64_t)seen[0].links;
  auto finish = [&] {
    float us[CMP_COUNT], lus[LVL_COUNT];
    h->cclock.Read(us, CMP_COUNT);
    cs.link_us = us[CMP_LINK];
    cs.order_us = us[CMP_ORDER];
    cs.moments_us = us[CMP_MOMENTS];
    cs.label_us = us[CMP_LABEL];
    if (n) {
      h->lclock.Read(lus, LVL_COUNT);
      cs.sort_us = lus[LVL_SORT] + lus[LVL_TABLE];
    }
    cs.launches = ls.launches + launches;
    h->stats.launches += cs.launches;
    h->stats.device_allocations = h->allocations;
  };
  if (count_only) {
    finish();
    return;
  }
  if (!labels_only && (n > capacity_intervals || n_components > capacity_components)) {
    finish();
    Throw(VSG_ERR_INVALID, "the level has " + std::to_string(n_components) + " components and " +
                               std::to_string(n) + " intervals, the capacities are " +
                               std::to_string(capacity_components) + " and " + std::to_string(capacity_intervals));
  }

  // ---- moments, label image, outputs ----
  if (n) h->cclock.Mark(CMP_WAIT);
  const hipMemcpyKind kind = mem_out == VSG_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  if (n && !labels_only) {
    LaunchComponentMoments(ordered, n, n_components, table, status, h->stream);
    VSG_HIP(hipGetLastError());
    h->cclock.Mark(CMP_MOMENTS);
    ++launches;
  }
  if (paint_labels) {
    const size_t bytes = (size_t)W * H * sizeof(int32_t);
    uint32_t* plane = reinterpret_cast<uint32_t*>(label_image);   // device output: painted in place
    if (labels_only || mem_out == VSG_MEM_HOST) {
      h->d_labels.Reserve(bytes, &h->allocations);
      plane = h->d_labels.As<uint32_t>();
    }
    VSG_HIP(hipMemsetAsync(plane, 0xff, bytes, h->stream));   // -1: no component
    LaunchFill(fill, n, plane, W, h->stream);
    VSG_HIP(hipGetLastError());
    h->cclock.Mark(CMP_LABEL);
    launches += 1 + (n ? 1 : 0);
    if (!labels_only && mem_out == VSG_MEM_HOST) {
      VSG_HIP(hipMemcpyAsync(label_image, plane, bytes, hipMemcpyDeviceToHost, h->stream));
      ++launches;
    }
  }
  if (n && !labels_only) {
    VSG_HIP(hipMemcpyAsync(components, table, (size_t)n_components * sizeof(vsg_render_level_component), kind,
                           h->stream));
    VSG_HIP(hipMemcpyAsync(intervals, ordered, (size_t)n * sizeof(Interval), kind, h->stream));
    VSG_HIP(hipMemcpyAsync(&seen[1], status, sizeof(CompStatus), hipMemcpyDeviceToHost, h->stream));
    launches += 3;
  }
  VSG_HIP(hipStreamSynchronize(h->stream));
  cs.largest_component_intervals = seen[1].largest;
  finish();
}

}  // namespace

extern "C" {

const char* vsg_render_last_error(void) { return g_last_error.c_str(); }

void vsg_render_default_options(vsg_render_options* o) {
  if (!o) return;
  o->blend_alpha = 0.5f;
  o->hierarchy_level = 0.0f;
  o->highlight_edges = 1;
  o->concat_with_source = 0;
  o->has_video = 1;
  o->device = -1;
}

size_t vsg_render_default_stride(int width) {
  size_t step = (size_t)width * 3;
  if (step % 4) step += 4 - step % 4;
  return step;
}

void vsg_render_color(int region_id, uint8_t c[3]) { GlibcColor(region_id, c); }

int vsg_render_create(const vsg_render_options* o, int width, int height, vsg_render** out) {
  return Guard([&] {
    if (!out) Throw(VSG_ERR_INVALID, "handle pointer is null");
    *out = nullptr;
    vsg_render_options opt;
    vsg_render_default_options(&opt);
    if (o) opt = *o;
    if (width <= 0 || height <= 0 || width > (1 << 15) || height > (1 << 15)) Throw(VSG_ERR_INVALID, "bad frame size");
    if (!(opt.hierarchy_level >= 0.0f && opt.hierarchy_level <= 1e6f)) Throw(VSG_ERR_INVALID, "bad hierarchy_level");
    if (!std::isfinite(opt.blend_alpha)) Throw(VSG_ERR_INVALID, "bad blend_alpha");
    if (opt.concat_with_source && !opt.has_video) {
      Throw(VSG_ERR_INVALID, "Request concatenation with source but no video stream present.");
    }
    if (!opt.has_video) opt.blend_alpha = 1.0f;   // segmentation_unit.cpp:486-490
    std::unique_ptr<vsg_render> h(new vsg_render);
    h->device = SelectDevice(opt.device, "libvsg_render");
    h->opt = opt;
    h->W = width;
    h->H = height;
    h->pitch = vsg_render_impl::PlanePitch(width);
    std::memset(&h->stats, 0, sizeof(h->stats));
    h->h_intervals.pinned = true;
    h->h_status.pinned = true;
    std::memset(&h->vstats, 0, sizeof(h->vstats));
    h->h_level.pinned = true;
    std::memset(&h->lstats, 0, sizeof(h->lstats));
    DeviceGuard guard(h->device);
    VSG_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    h->clock.Create(STAGE_COUNT + 1);
    h->vclock.Create(VEC_COUNT + 1);
    h->lclock.Create(LVL_COUNT + 1);
    h->cclock.Create(CMP_COUNT + 1);
    h->h_comp.pinned = true;
    std::memset(&h->cstats, 0, sizeof(h->cstats));
    h->bclock.Create(BND_STAGES + 1);
    h->h_bound.pinned = true;
    std::memset(&h->bstats, 0, sizeof(h->bstats));
    h->aclock.Create(ADJ_STAGES + 1);
    h->h_adj.pinned = true;
    std::memset(&h->astats, 0, sizeof(h->astats));
    h->oclock.Create(OVL_STAGES + 1);
    h->h_other.pinned = true;
    h->h_ovl.pinned = true;
    std::memset(&h->ostats, 0, sizeof(h->ostats));
    h->pclock.Create(PRS_STAGES + 1);
    h->h_pers.pinned = true;
    std::memset(&h->pstats, 0, sizeof(h->pstats));
    h->kclock.Create(CLR_STAGES + 1);
    h->h_color.pinned = true;
    std::memset(&h->kstats, 0, sizeof(h->kstats));
    h->tclock.Create(CNT_STAGES + 1);
    h->h_cont.pinned = true;
    std::memset(&h->tstats, 0, sizeof(h->tstats));
    h->dclock.Create(DST_STAGES + 1);
    h->h_dist.pinned = true;
    std::memset(&h->dstats, 0, sizeof(h->dstats));
    h->mclock.Create(MSH_STAGES + 1);
    h->h_mesh.pinned = true;
    std::memset(&h->mstats, 0, sizeof(h->mstats));
    h->d_plane.Reserve((size_t)h->pitch * height * sizeof(uint32_t), &h->allocations);
    *out = h.release();
  });
}

void vsg_render_destroy(vsg_render* h) { DestroyOnDevice(h); }

int vsg_render_frame(vsg_render* h, const uint8_t* seg, size_t seg_len, const uint8_t* bgr, size_t stride,
                     int mem_in, uint8_t* out, size_t out_stride, int mem_out) {
  return Guard([&] {
    if (!h) Throw(VSG_ERR_INVALID, "handle is null");
    if (!out) Throw(VSG_ERR_INVALID, "out is null");
    CheckMem(mem_in, "bgr");
    CheckMem(mem_out, "out");
    const int W = h->W, H = h->H;
    const size_t row_bytes = (size_t)W * 3;
    const bool video = h->opt.has_video != 0;
    if (video && !bgr) Throw(VSG_ERR_INVALID, "the handle was created with has_video: bgr is null");
    if (video && stride < row_bytes) Throw(VSG_ERR_INVALID, "stride is smaller than 3 * width");
    if (out_stride == 0) out_stride = vsg_render_default_stride(W);
    if (out_stride < row_bytes) Throw(VSG_ERR_INVALID, "out_stride is smaller than 3 * width");
    const int out_rows = h->opt.concat_with_source ? 2 * H : H;
    DeviceGuard guard(h->device);
    std::memset(&h->stats, 0, sizeof(h->stats));
    std::memset(&h->vstats, 0, sizeof(h->vstats));

    // ---- host: decode, hierarchy state (segmentation_unit.cpp:567-591), colour table ----
    const double t0 = NowMs();
    bool vector = false;
    const Hierarchy& hier = Ingest(h, seg, seg_len, &vector);
    if (!h->level_resolved) {
      const int size = (int)h->desc.hierarchy.size();   // the first frame's own hierarchy
      float lvl = h->opt.hierarchy_level;
      if (lvl != std::floor(lvl)) lvl = (float)(int)(lvl * size);
      h->level = std::min<int>((int)lvl, size - 1);
      h->level_resolved = true;
    }
    // HierarchyColorGenerator's own clamps (segmentation_render.cpp:40-50)
    int level = h->level;
    if (level > 0 && hier.empty()) level = 0;
    if (!hier.empty() && level >= (int)hier.size()) level = (int)hier.size() - 1;
    if (h->colors.size() > (1u << 20)) h->colors.clear();
    auto color_of = [&](int mapped) {
      auto it = h->colors.find(mapped);
      if (it == h->colors.end()) {
        uint8_t c[3];
        GlibcColor(mapped, c);
        it = h->colors.emplace(mapped, (uint32_t)c[0] | (uint32_t)c[1] << 8 | (uint32_t)c[2] << 16).first;
      }
      return it->second;
    };
    int64_t n_cross = 0;
    if (vector) {
      h->stats.distinct_ids = AssignRegionValues(h, level, hier, color_of);
      n_cross = h->BuildLines();
    } else {
      h->stats.distinct_ids = AssignValues(h, level, hier, color_of);
    }
    const int64_t n_intervals = vector ? n_cross / 2 : (int64_t)h->intervals.size();
    h->stats.intervals = n_intervals;
    const double t1 = NowMs();
    h->stats.decode_ms = t1 - t0;

    // ---- uploads (and, for a vector-only desc, the scan conversion that makes the list) ----
    if (vector) h->RunVector(n_cross);
    else h->UploadIntervals();
    const uint8_t* src = nullptr;
    size_t src_stride = 0;
    if (video) {
      if (mem_in == VSG_MEM_DEVICE) {
        src = bgr;
        src_stride = stride;
      } else {
        src_stride = vsg_render_default_stride(W);
        h->d_src.Reserve(src_stride * H, &h->allocations);
        VSG_HIP(hipMemcpy2DAsync(h->d_src.p, src_stride, bgr, stride, row_bytes, H, hipMemcpyHostToDevice,
                                 h->stream));
        ++h->stats.launches;
        src = static_cast<const uint8_t*>(h->d_src.p);
      }
    }
    uint8_t* dst = out;
    size_t dst_stride = out_stride;
    if (mem_out == VSG_MEM_HOST) {
      dst_stride = vsg_render_default_stride(W);
      h->d_out.Reserve(dst_stride * out_rows, &h->allocations);
      dst = static_cast<uint8_t*>(h->d_out.p);
    }
    h->stats.upload_ms = NowMs() - t1;

    // ---- device: clear, fill, compose ----
    uint32_t* plane = static_cast<uint32_t*>(h->d_plane.p);
    h->clock.Begin(h->stream);
    VSG_HIP(hipMemsetAsync(plane, 0, (size_t)h->pitch * H * sizeof(uint32_t), h->stream));
    h->clock.Mark(STAGE_CLEAR);
    vsg_render_impl::LaunchFill(static_cast<const Interval*>(h->d_intervals.p), n_intervals, plane, h->pitch,
                                h->stream);
    h->clock.Mark(STAGE_FILL);
    const int mode = h->opt.concat_with_source ? vsg_render_impl::COMPOSE_CONCAT
                     : video                   ? vsg_render_impl::COMPOSE_BLEND
                                               : vsg_render_impl::COMPOSE_RENDER;
    vsg_render_impl::LaunchCompose(plane, h->pitch, W, H, src, src_stride, dst, dst_stride, h->opt.highlight_edges,
                                   mode, h->opt.blend_alpha, h->stream);
    VSG_HIP(hipGetLastError());
    h->clock.Mark(STAGE_COMPOSE);
    h->stats.launches += 2 + (n_intervals == 0 ? 0 : 1);
    if (mem_out == VSG_MEM_HOST) {
      VSG_HIP(hipMemcpy2DAsync(out, out_stride, dst, dst_stride, row_bytes, out_rows, hipMemcpyDeviceToHost,
                               h->stream));
      ++h->stats.launches;
    }
    h->FinishStats();
    if (vector) h->CheckVector();
  });
}

int vsg_render_id_image(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int32_t* out, int mem_out) {
  return Guard([&] {
    if (!h) Throw(VSG_ERR_INVALID, "handle is null");
    if (!out) Throw(VSG_ERR_INVALID, "out is null");
    CheckMem(mem_out, "out");
    const size_t bytes = (size_t)h->W * h->H * sizeof(int32_t);
    DeviceGuard guard(h->device);
    uint32_t* ids = reinterpret_cast<uint32_t*>(out);   // device output: painted in place
    if (mem_out == VSG_MEM_HOST) {
      h->d_ids.Reserve(bytes, &h->allocations);
      ids = static_cast<uint32_t*>(h->d_ids.p);
    }
    const bool vector = PaintIds(h, seg, seg_len, level, ids, [](int mapped) { return (uint32_t)mapped; });
    h->clock.Mark(STAGE_COMPOSE);   // nothing is composed: the two marks are back to back
    if (mem_out == VSG_MEM_HOST) {
      VSG_HIP(hipMemcpyAsync(out, ids, bytes, hipMemcpyDeviceToHost, h->stream));
      ++h->stats.launches;
    }
    h->FinishStats();
    if (vector) h->CheckVector();
  });
}

int vsg_render_level_regions(vsg_render* h, const uint8_t* seg, size_t seg_len, int level,
                             vsg_render_level_region* regions, size_t capacity_regions, size_t* num_regions,
                             int32_t* intervals, size_t capacity_intervals, size_t* num_intervals, int mem_out) {
  return Guard([&] {
    using namespace vsg_render_impl;
    static_assert(sizeof(vsg_render_level_region) == kLevelRegionWords * sizeof(int32_t), "moved as int32 words");
    if (!h) Throw(VSG_ERR_INVALID, "handle is null");
    if (!num_regions || !num_intervals) Throw(VSG_ERR_INVALID, "a count pointer is null");
    *num_regions = *num_intervals = 0;
    CheckMem(mem_out, "outputs");
    const bool count_only = !regions && !intervals && capacity_regions == 0 && capacity_intervals == 0;
    const int W = h->W, H = h->H;
    if ((uint64_t)W * (uint64_t)H >= (1ull << 32)) Throw(VSG_ERR_INVALID, "the frame has 2^32 pixels or more");
    DeviceGuard guard(h->device);
    std::memset(&h->lstats, 0, sizeof(h->lstats));

    LevelFront f = PaintLevelRuns(h, seg, seg_len, level, &h->lstats);
    const uint32_t n = f.n;
    *num_intervals = n;

    // ---- sort, table, moments, outputs ----
    const uint32_t cap_regions = f.cap_regions;
    const bool intervals_fit = n <= capacity_intervals;
    const bool deliver = !count_only && intervals_fit;
    const size_t region_bytes = (size_t)cap_regions * sizeof(vsg_render_level_region);
    const size_t interval_bytes = (size_t)n * sizeof(Interval);
    if (deliver && n && (!regions || !intervals)) Throw(VSG_ERR_INVALID, "an output is null");
    if (n) {
      SortLevelRuns(h, &f, &h->lstats);
      LevelStatus* status = f.status;
      LevelStatus* seen = h->h_level.As<LevelStatus>();
      int32_t* d_regions = f.regions;
      Interval* d_intervals = f.intervals;
      if (!count_only) {
        LaunchLevelMoments(d_intervals, n, cap_regions, d_regions, status, h->stream);
        VSG_HIP(hipGetLastError());
        h->lclock.Mark(LVL_MOMENTS);
        ++h->lstats.launches;
      }
      if (deliver && mem_out == VSG_MEM_DEVICE) {
        // the number of regions is on the device: the copy decides there whether they fit
        LaunchLevelCopy(d_regions, d_intervals, n, (uint32_t)std::min<size_t>(capacity_regions, cap_regions),
                        reinterpret_cast<int32_t*>(regions), intervals, status, h->stream);
        VSG_HIP(hipGetLastError());
        ++h->lstats.launches;
      } else if (deliver) {
        // through the pinned block; handed to the caller once the number of regions is known
        h->h_level.Reserve(2 * sizeof(LevelStatus) + region_bytes + interval_bytes, &h->allocations);
        seen = h->h_level.As<LevelStatus>();
        char* stage = reinterpret_cast<char*>(seen + 2);
        VSG_HIP(hipMemcpyAsync(stage, d_regions, region_bytes, hipMemcpyDeviceToHost, h->stream));
        VSG_HIP(hipMemcpyAsync(stage + region_bytes, d_intervals, interval_bytes, hipMemcpyDeviceToHost, h->stream));
        h->lstats.launches += 2;
      }
      VSG_HIP(hipMemcpyAsync(&seen[1], status, sizeof(LevelStatus), hipMemcpyDeviceToHost, h->stream));
      ++h->lstats.launches;
      VSG_HIP(hipStreamSynchronize(h->stream));
      if (seen[1].regions == 0 || seen[1].regions > cap_regions) {
        Throw(VSG_ERR_INTERNAL, "the plane has more regions than the desc has ids");
      }
      float us[LVL_COUNT];
      h->lclock.Read(us, LVL_COUNT);
      h->lstats.sort_us = us[LVL_SORT];
      h->lstats.table_us = us[LVL_TABLE];
      h->lstats.moments_us = us[LVL_MOMENTS];
      h->lstats.regions = seen[1].regions;
      h->lstats.largest_region_intervals = seen[1].largest;
    }
    h->stats.launches += h->lstats.launches;
    h->stats.device_allocations = h->allocations;
    const size_t n_regions = (size_t)h->lstats.regions;
    *num_regions = n_regions;
    if (count_only) return;
    if (!intervals_fit || n_regions > capacity_regions) {
      Throw(VSG_ERR_INVALID, "the level has " + std::to_string(n_regions) + " regions and " + std::to_string(n) +
                                 " intervals, the capacities are " + std::to_string(capacity_regions) + " and " +
                                 std::to_string(capacity_intervals));
    }
    if (n && mem_out == VSG_MEM_HOST) {
      const char* stage = reinterpret_cast<const char*>(h->h_level.As<LevelStatus>() + 2);
      std::memcpy(regions, stage, n_regions * sizeof(vsg_render_level_region));
      std::memcpy(intervals, stage + region_bytes, interval_bytes);
    }
  });
}

int vsg_render_last_level_stats(vsg_render* h, vsg_render_level_stats* s) {
  return Guard([&] {
    if (!h || !s) Throw(VSG_ERR_INVALID, "null argument");
    *s = h->lstats;
  });
}

int vsg_render_level_components(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness,
                                vsg_render_level_component* components, size_t capacity_components,
                                size_t* num_components, int32_t* intervals, size_t capacity_intervals,
                                size_t* num_intervals, int32_t* label_image, int mem_out) {
  return Guard([&] {
    using namespace vsg_render_impl;
    static_assert(sizeof(vsg_render_level_component) == kLevelComponentWords * sizeof(int32_t), "moved as int32 words");
    if (connectedness != VSG_RENDER_CONNECT_N4 && connectedness != VSG_RENDER_CONNECT_N8) {
      Throw(VSG_ERR_INVALID, "connectedness is neither VSG_RENDER_CONNECT_N4 nor VSG_RENDER_CONNECT_N8");
    }
    if (!h) Throw(VSG_ERR_INVALID, "handle is null");
    if (!num_components || !num_intervals) Throw(VSG_ERR_INVALID, "a count pointer is null");
    *num_components = *num_intervals = 0;
    LevelComponents(h, seg, seg_len, level, connectedness, components, capacity_components, num_components, intervals,
                    capacity_intervals, num_intervals, label_image, mem_out, false);
  });
}

int vsg_render_last_component_stats(vsg_render* h, vsg_render_component_stats* s) {
  return Guard([&] {
    if (!h || !s) Throw(VSG_ERR_INVALID, "null argument");
    *s = h->cstats;
  });
}

int vsg_render_level_boundaries(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness,
                                int which, vsg_render_level_boundary* boundaries, size_t capacity_boundaries,
                                size_t* num_boundaries, int32_t* points, size_t capacity_points, size_t* num_points,
                                int mem_out) {
  return Guard([&] {
    using namespace vsg_render_impl;
    static_assert(sizeof(vsg_render_level_boundary) == kLevelBoundaryWords * sizeof(int32_t), "moved as int32 words");
    if (connectedness != 0 && connectedness != VSG_RENDER_CONNECT_N4 && connectedness != VSG_RENDER_CONNECT_N8) {
      Throw(VSG_ERR_INVALID, "connectedness is neither 0, VSG_RENDER_CONNECT_N4 nor VSG_RENDER_CONNECT_N8");
    }
    if (which != VSG_RENDER_BOUNDARY_INNER && which != VSG_RENDER_BOUNDARY_OUTER) {
      Throw(VSG_ERR_INVALID, "which is neither VSG_RENDER_BOUNDARY_INNER nor VSG_RENDER_BOUNDARY_OUTER");
    }
    if (!h) Throw(VSG_ERR_INVALID, "handle is null");
    if (!num_boundaries || !num_points) Throw(VSG_ERR_INVALID, "a count pointer is null");
    *num_boundaries = *num_points = 0;
    CheckMem(mem_out, "outputs");
    const bool count_only = !boundaries && !points && capacity_boundaries == 0 && capacity_points == 0;
    const bool outer = which == VSG_RENDER_BOUNDARY_OUTER;
    const int W = h->W, H = h->H;
    if ((uint64_t)W * (uint64_t)H >= (1ull << 32)) Throw(VSG_ERR_INVALID, "the frame has 2^32 pixels or more");
    DeviceGuard guard(h->device);
    vsg_render_boundary_stats& bs = h->bstats;
    std::memset(&bs, 0, sizeof(bs));

    // ---- the plane: the level's ids, or the indices of its regions' components ----
    const int32_t* plane = nullptr;
    const int32_t* comp_table = nullptr;
    uint32_t max_group = 0;
    uint64_t groups_bound = 0;   // no more groups than this
    bool vector = false;
    if (connectedness == 0) {
      int32_t max_id = 0;
      vector = PaintLevelPlane(h, seg, seg_len, level, &max_id);
      plane = h->d_ids.As<int32_t>();
      max_group = (uint32_t)max_id;
      groups_bound = (uint64_t)h->stats.distinct_ids;
      bs.launches = h->stats.launches;
    } else {
      size_t n_components = 0, n_intervals = 0;
      LevelComponents(h, seg, seg_len, level, connectedness, nullptr, 0, &n_components, nullptr, 0, &n_intervals,
                      nullptr, VSG_MEM_DEVICE, true);
      plane = h->d_labels.As<int32_t>();
      comp_table = h->d_comp_table.As<int32_t>();
      max_group = n_components ? (uint32_t)(n_components - 1) : 0u;
      groups_bound = n_components;
      const vsg_render_component_stats& cs = h->cstats;
      bs.plane_us = h->stats.clear_us + h->stats.fill_us + cs.runs_us + cs.sort_us + cs.link_us + cs.order_us +
                    cs.label_us;
      bs.launches = h->stats.launches;
    }

    // ---- count: the number of points sizes everything below ----
    h->d_bound_status.Reserve(sizeof(BoundStatus), &h->allocations);
    h->h_bound.Reserve(2 * sizeof(BoundStatus), &h->allocations);
    BoundStatus* status = h->d_bound_status.As<BoundStatus>();
    BoundStatus* seen = h->h_bound.As<BoundStatus>();   // [0] after the count, [1] at the end
    std::memset(seen, 0, 2 * sizeof(BoundStatus));
    VSG_HIP(hipMemsetAsync(status, 0, sizeof(BoundStatus), h->stream));
    h->bclock.Begin(h->stream);
    LaunchBoundClassify(plane, W, H, outer, false, 0, nullptr, status, h->stream);
    VSG_HIP(hipGetLastError());
    h->bclock.Mark(BND_COUNT);
    VSG_HIP(hipMemcpyAsync(&seen[0], status, sizeof(BoundStatus), hipMemcpyDeviceToHost, h->stream));
    int launches = 3;
    VSG_HIP(hipStreamSynchronize(h->stream));
    {
      float us[BND_STAGES];
      h->bclock.Read(us, BND_STAGES);
      bs.count_us = us[BND_COUNT];
    }
    if (connectedness == 0) {
      float us[STAGE_COUNT];
      h->clock.Read(us, STAGE_COUNT);
      h->stats.clear_us = us[STAGE_CLEAR];
      h->stats.fill_us = us[STAGE_FILL];
      bs.plane_us = us[STAGE_CLEAR] + us[STAGE_FILL];
      if (vector) h->CheckVector();
    }
    auto finish = [&] {
      bs.launches += launches;
      h->stats.launches += launches;
      h->stats.device_allocations = h->allocations;
    };
    if (seen[0].points > 0x7fffffffull) {
      finish();
      Throw(VSG_ERR_INVALID, "the level has more than 2^31 - 1 boundary points");
    }
    const uint32_t n = (uint32_t)seen[0].points;
    *num_points = n;
    bs.points = n;
    if (n == 0) return finish();   // no group at all: both lists are empty

    // ---- emit, sort, table ----
    const uint32_t cap_records = (uint32_t)std::min<uint64_t>(groups_bound, n);   // every group has a point
    if (cap_records == 0) Throw(VSG_ERR_INTERNAL, "the plane has groups the desc has no ids for");
    const bool points_fit = n <= capacity_points;
    const bool deliver = !count_only && points_fit;
    if (deliver && (!boundaries || !points)) Throw(VSG_ERR_INVALID, "an output is null");
    int group_bits = 1;
    while (group_bits < 32 && (max_group >> group_bits)) ++group_bits;
    const int end_bit = 32 + group_bits;
    const size_t temp_bytes = std::max<size_t>(BoundTempBytes(n, end_bit), 16);
    const size_t record_bytes = (size_t)cap_records * sizeof(vsg_render_level_boundary);
    const size_t point_bytes = (size_t)n * 2 * sizeof(int32_t);
    h->d_sort_temp.Reserve(temp_bytes, &h->allocations);
    h->d_bound_keys.Reserve((size_t)n * 2 * sizeof(unsigned long long), &h->allocations);
    h->d_bound_rank.Reserve((size_t)n * sizeof(uint32_t), &h->allocations);
    h->d_bound_points.Reserve(point_bytes, &h->allocations);
    h->d_bound_records.Reserve(record_bytes, &h->allocations);
    unsigned long long* keys = h->d_bound_keys.As<unsigned long long>();
    unsigned long long* keys_sorted = keys + n;
    uint32_t* rank = h->d_bound_rank.As<uint32_t>();
    int32_t* d_points = h->d_bound_points.As<int32_t>();
    int32_t* d_records = h->d_bound_records.As<int32_t>();
    h->bclock.Begin(h->stream);
    LaunchBoundClassify(plane, W, H, outer, true, n, keys, status, h->stream);
    VSG_HIP(hipGetLastError());
    h->bclock.Mark(BND_EMIT);
    VSG_HIP(BoundSort(h->d_sort_temp.p, temp_bytes, keys, keys_sorted, n, end_bit, h->stream));
    h->bclock.Mark(BND_SORT);
    VSG_HIP(LevelRank(h->d_sort_temp.p, temp_bytes, keys_sorted, rank, n, h->stream));
    LaunchBoundTable(keys_sorted, rank, n, W, H, max_group, cap_records, comp_table, d_points, d_records, status,
                     h->stream);
    VSG_HIP(hipGetLastError());
    h->bclock.Mark(BND_TABLE);
    launches += 5;   // emit, the sort and the scan counted as one each, table, finish
    if (deliver && mem_out == VSG_MEM_DEVICE) {
      // the number of boundaries is on the device: the copy decides there whether they fit
      LaunchBoundCopy(d_records, d_points, n, (uint32_t)std::min<size_t>(capacity_boundaries, cap_records),
                      reinterpret_cast<int32_t*>(boundaries), points, status, h->stream);
      VSG_HIP(hipGetLastError());
      ++launches;
    } else if (deliver) {
      // through the pinned block; handed to the caller once the number of boundaries is known
      h->h_bound.Reserve(2 * sizeof(BoundStatus) + record_bytes + point_bytes, &h->allocations);
      seen = h->h_bound.As<BoundStatus>();
      char* stage = reinterpret_cast<char*>(seen + 2);
      VSG_HIP(hipMemcpyAsync(stage, d_records, record_bytes, hipMemcpyDeviceToHost, h->stream));
      VSG_HIP(hipMemcpyAsync(stage + record_bytes, d_points, point_bytes, hipMemcpyDeviceToHost, h->stream));
      launches += 2;
    }
    VSG_HIP(hipMemcpyAsync(&seen[1], status, sizeof(BoundStatus), hipMemcpyDeviceToHost, h->stream));
    ++launches;
    VSG_HIP(hipStreamSynchronize(h->stream));
    {
      float us[BND_STAGES];
      h->bclock.Read(us, BND_STAGES);
      bs.emit_us = us[BND_EMIT];
      bs.sort_us = us[BND_SORT];
      bs.table_us = us[BND_TABLE];
    }
    finish();
    if ((seen[1].flags & BOUND_FLAG_OVERFLOW) || seen[1].emitted != n) {
      Throw(VSG_ERR_INTERNAL, "the emit pass found other boundary points than the count pass");
    }
    if ((seen[1].flags & BOUND_FLAG_RANGE) || seen[1].boundaries == 0 || seen[1].boundaries > cap_records ||
        (comp_table && seen[1].boundaries != groups_bound)) {
      Throw(VSG_ERR_INTERNAL, "a sorted boundary key or a boundary record is out of range");
    }
    const size_t n_boundaries = seen[1].boundaries;
    *num_boundaries = n_boundaries;
    bs.boundaries = (int64_t)n_boundaries;
    bs.largest_boundary_points = seen[1].largest;
    if (count_only) return;
    if (!points_fit || n_boundaries > capacity_boundaries) {
      Throw(VSG_ERR_INVALID, "the level has " + std::to_string(n_boundaries) + " boundaries and " + std::to_string(n) +
                                 " points, the capacities are " + std::to_string(capacity_boundaries) + " and " +
                                 std::to_string(capacity_points));
    }
    if (mem_out == VSG_MEM_HOST) {
      const char* stage = reinterpret_cast<const char*>(h->h_bound.As<BoundStatus>() + 2);
      std::memcpy(boundaries, stage, n_boundaries * sizeof(vsg_render_level_boundary));
      std::memcpy(points, stage + record_bytes, point_bytes);
    }
  });
}

int vsg_render_last_boundary_stats(vsg_render* h, vsg_render_boundary_stats* s) {
  return Guard([&] {
    if (!h || !s) Throw(VSG_ERR_INVALID, "null argument");
    *s = h->bstats;
  });
}

}  // extern "C"

namespace {

// The body of vsg_render_level_adjacency; vsg_render_persistence_graph runs it for the counts alone and
// takes the lists from h->d_adj_nodes and h->d_adj_edges.
void LevelAdjacency(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness,
                    int neighbourhood, vsg_render_level_node* nodes, size_t capacity_nodes, size_t* num_nodes,
                    vsg_render_level_edge* edges, size_t capacity_edges, size_t* num_edges, int mem_out) {
  using namespace vsg_render_impl;
  static_assert(sizeof(vsg_render_level_node) == kLevelNodeWords * sizeof(int32_t), "moved as int32 words");
  static_assert(sizeof(vsg_render_level_edge) == kLevelEdgeWords * sizeof(int32_t), "moved as int32 words");
  if (connectedness != 0 && connectedness != VSG_RENDER_CONNECT_N4 && connectedness != VSG_RENDER_CONNECT_N8) {
    Throw(VSG_ERR_INVALID, "connectedness is neither 0, VSG_RENDER_CONNECT_N4 nor VSG_RENDER_CONNECT_N8");
  }
  if (neighbourhood != VSG_RENDER_ADJACENT_N4 && neighbourhood != VSG_RENDER_ADJACENT_N8) {
    Throw(VSG_ERR_INVALID, "neighbourhood is neither VSG_RENDER_ADJACENT_N4 nor VSG_RENDER_ADJACENT_N8");
  }
  if (!h) Throw(VSG_ERR_INVALID, "handle is null");
  if (!num_nodes || !num_edges) Throw(VSG_ERR_INVALID, "a count pointer is null");
  *num_nodes = *num_edges = 0;
  CheckMem(mem_out, "outputs");
  const bool count_only = !nodes && !edges && capacity_nodes == 0 && capacity_edges == 0;
  const bool diagonal = neighbourhood == VSG_RENDER_ADJACENT_N8;
  const int W = h->W, H = h->H;
  if ((uint64_t)W * (uint64_t)H >= (1ull << 32)) Throw(VSG_ERR_INVALID, "the frame has 2^32 pixels or more");
  DeviceGuard guard(h->device);
  vsg_render_adjacency_stats& as = h->astats;
  std::memset(&as, 0, sizeof(as));

  // ---- the plane: the level's ids, or the indices of its regions' components ----
  const int32_t* plane = nullptr;
  const int32_t* comp_table = nullptr;
  uint32_t max_group = 0;
  uint64_t groups_bound = 0;   // no more groups than this
  bool vector = false;
  if (connectedness == 0) {
    int32_t max_id = 0;
    vector = PaintLevelPlane(h, seg, seg_len, level, &max_id);
    plane = h->d_ids.As<int32_t>();
    max_group = (uint32_t)max_id;
    groups_bound = (uint64_t)h->stats.distinct_ids;
    as.launches = h->stats.launches;
  } else {
    size_t n_components = 0, n_intervals = 0;
    LevelComponents(h, seg, seg_len, level, connectedness, nullptr, 0, &n_components, nullptr, 0, &n_intervals,
                    nullptr, VSG_MEM_DEVICE, true);
    plane = h->d_labels.As<int32_t>();
    comp_table = h->d_comp_table.As<int32_t>();
    max_group = n_components ? (uint32_t)(n_components - 1) : 0u;
    groups_bound = n_components;
    const vsg_render_component_stats& cs = h->cstats;
    as.plane_us = h->stats.clear_us + h->stats.fill_us + cs.runs_us + cs.sort_us + cs.link_us + cs.order_us +
                  cs.label_us;
    as.launches = h->stats.launches;
  }
  int group_bits = 1;
  while (group_bits < 31 && (max_group >> group_bits)) ++group_bits;

  // ---- count: the number of keys sizes everything below ----
  h->d_adj_status.Reserve(sizeof(AdjStatus), &h->allocations);
  h->h_adj.Reserve(2 * sizeof(AdjStatus), &h->allocations);
  AdjStatus* status = h->d_adj_status.As<AdjStatus>();
  AdjStatus* seen = h->h_adj.As<AdjStatus>();   // [0] after the count, [1] at the end
  std::memset(seen, 0, 2 * sizeof(AdjStatus));
  VSG_HIP(hipMemsetAsync(status, 0, sizeof(AdjStatus), h->stream));
  h->aclock.Begin(h->stream);
  LaunchAdjClassify(plane, W, H, group_bits, diagonal, false, 0, nullptr, status, h->stream);
  VSG_HIP(hipGetLastError());
  h->aclock.Mark(ADJ_COUNT);
  VSG_HIP(hipMemcpyAsync(&seen[0], status, sizeof(AdjStatus), hipMemcpyDeviceToHost, h->stream));
  int launches = 3;
  VSG_HIP(hipStreamSynchronize(h->stream));
  {
    float us[ADJ_STAGES];
    h->aclock.Read(us, ADJ_STAGES);
    as.count_us = us[ADJ_COUNT];
  }
  if (connectedness == 0) {
    float us[STAGE_COUNT];
    h->clock.Read(us, STAGE_COUNT);
    h->stats.clear_us = us[STAGE_CLEAR];
    h->stats.fill_us = us[STAGE_FILL];
    as.plane_us = us[STAGE_CLEAR] + us[STAGE_FILL];
    if (vector) h->CheckVector();
  }
  auto finish = [&] {
    as.launches += launches;
    h->stats.launches += launches;
    h->stats.device_allocations = h->allocations;
  };
  if (seen[0].keys > 0x7fffffffull) {
    finish();
    Throw(VSG_ERR_INVALID, "the level has more than 2^31 - 1 bordering sides and diagonal contacts");
  }
  const uint32_t n = (uint32_t)seen[0].keys;
  as.sides = as.keys = n;
  if (n == 0) return finish();   // no covered pixel: both lists are empty

  // ---- emit, sort, table ----
  const uint32_t cap_nodes = (uint32_t)std::min<uint64_t>(groups_bound, n);   // every group has a key
  if (cap_nodes == 0) Throw(VSG_ERR_INTERNAL, "the plane has groups the desc has no ids for");
  const uint32_t cap_edges = n;                                               // every edge has a key
  const int end_bit = 2 * group_bits + 2;
  const size_t temp_bytes = std::max<size_t>(AdjTempBytes(n, end_bit), 16);
  const size_t node_bytes = (size_t)cap_nodes * sizeof(vsg_render_level_node);
  const size_t edge_bytes = (size_t)cap_edges * sizeof(vsg_render_level_edge);
  h->d_sort_temp.Reserve(temp_bytes, &h->allocations);
  h->d_adj_keys.Reserve((size_t)n * 2 * sizeof(unsigned long long), &h->allocations);
  h->d_adj_heads.Reserve((size_t)n * sizeof(unsigned long long), &h->allocations);
  h->d_adj_nodes.Reserve(node_bytes, &h->allocations);
  h->d_adj_edges.Reserve(edge_bytes, &h->allocations);
  unsigned long long* keys = h->d_adj_keys.As<unsigned long long>();
  unsigned long long* keys_sorted = keys + n;
  unsigned long long* heads = h->d_adj_heads.As<unsigned long long>();
  int32_t* d_nodes = h->d_adj_nodes.As<int32_t>();
  int32_t* d_edges = h->d_adj_edges.As<int32_t>();
  h->aclock.Begin(h->stream);
  LaunchAdjClassify(plane, W, H, group_bits, diagonal, true, n, keys, status, h->stream);
  VSG_HIP(hipGetLastError());
  h->aclock.Mark(ADJ_EMIT);
  VSG_HIP(AdjSort(h->d_sort_temp.p, temp_bytes, keys, keys_sorted, n, end_bit, h->stream));
  h->aclock.Mark(ADJ_SORT);
  VSG_HIP(hipMemsetAsync(d_nodes, 0, node_bytes, h->stream));   // the counts are summed into them
  VSG_HIP(hipMemsetAsync(d_edges, 0, edge_bytes, h->stream));
  VSG_HIP(AdjRank(h->d_sort_temp.p, temp_bytes, keys_sorted, group_bits, heads, n, h->stream));
  LaunchAdjTable(keys_sorted, heads, n, group_bits, max_group, cap_nodes, cap_edges, comp_table, d_nodes, d_edges,
                 status, h->stream);
  VSG_HIP(hipGetLastError());
  h->aclock.Mark(ADJ_TABLE);
  // emit, the sort and the scan counted as one each, two clears, table, finish, resolve
  launches += 7 + (comp_table ? 0 : 1);
  const bool to_device = !count_only && mem_out == VSG_MEM_DEVICE && nodes && edges;
  if (to_device) {
    // the lengths of both lists are on the device: the copy decides there whether they fit
    LaunchAdjCopy(d_nodes, d_edges, (uint32_t)std::min<size_t>(capacity_nodes, cap_nodes),
                  (uint32_t)std::min<size_t>(capacity_edges, cap_edges), reinterpret_cast<int32_t*>(nodes),
                  reinterpret_cast<int32_t*>(edges), status, h->stream);
    VSG_HIP(hipGetLastError());
    ++launches;
  }
  VSG_HIP(hipMemcpyAsync(&seen[1], status, sizeof(AdjStatus), hipMemcpyDeviceToHost, h->stream));
  ++launches;
  VSG_HIP(hipStreamSynchronize(h->stream));
  {
    float us[ADJ_STAGES];
    h->aclock.Read(us, ADJ_STAGES);
    as.emit_us = us[ADJ_EMIT];
    as.sort_us = us[ADJ_SORT];
    as.table_us = us[ADJ_TABLE];
  }
  if ((seen[1].flags & ADJ_FLAG_OVERFLOW) || seen[1].emitted != n) {
    finish();
    Throw(VSG_ERR_INTERNAL, "the emit pass found other adjacency keys than the count pass");
  }
  if ((seen[1].flags & ADJ_FLAG_RANGE) || seen[1].nodes == 0 || seen[1].nodes > cap_nodes ||
      seen[1].edges > cap_edges || (comp_table && seen[1].nodes != groups_bound)) {
    finish();
    Throw(VSG_ERR_INTERNAL, "a sorted adjacency key, a node or an edge is out of range");
  }
  const size_t n_nodes = seen[1].nodes, n_edges = seen[1].edges;
  *num_nodes = n_nodes;
  *num_edges = n_edges;
  as.nodes = (int64_t)n_nodes;
  as.edges = (int64_t)n_edges;
  as.largest_node_edges = seen[1].largest;
  if (count_only) return finish();
  if (n_nodes > capacity_nodes || n_edges > capacity_edges) {
    finish();
    Throw(VSG_ERR_INVALID, "the level has " + std::to_string(n_nodes) + " nodes and " + std::to_string(n_edges) +
                               " edges, the capacities are " + std::to_string(capacity_nodes) + " and " +
                               std::to_string(capacity_edges));
  }
  if (!nodes || (n_edges && !edges)) {
    finish();
    Throw(VSG_ERR_INVALID, "an output is null");
  }
  if (mem_out == VSG_MEM_HOST) {
    // through the pinned block, now that the lengths are known
    const size_t nb = n_nodes * sizeof(vsg_render_level_node), eb = n_edges * sizeof(vsg_render_level_edge);
    h->h_adj.Reserve(2 * sizeof(AdjStatus) + nb + eb, &h->allocations);
    char* stage = reinterpret_cast<char*>(h->h_adj.As<AdjStatus>() + 2);
    VSG_HIP(hipMemcpyAsync(stage, d_nodes, nb, hipMemcpyDeviceToHost, h->stream));
    ++launches;
    if (eb) {
      VSG_HIP(hipMemcpyAsync(stage + nb, d_edges, eb, hipMemcpyDeviceToHost, h->stream));
      ++launches;
    }
    VSG_HIP(hipStreamSynchronize(h->stream));
    std::memcpy(nodes, stage, nb);
    if (eb) std::memcpy(edges, stage + nb, eb);
  } else if (!to_device) {
    // edges was null with no edge to deliver: the copy kernel was not launched
    VSG_HIP(hipMemcpyAsync(nodes, d_nodes, n_nodes * sizeof(vsg_render_level_node), hipMemcpyDeviceToDevice,
                           h->stream));
    ++launches;
    VSG_HIP(hipStreamSynchronize(h->stream));
  }
  finish();
}

}  // namespace

extern "C" {

int vsg_render_level_adjacency(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness,
                               int neighbourhood, vsg_render_level_node* nodes, size_t capacity_nodes,
                               size_t* num_nodes, vsg_render_level_edge* edges, size_t capacity_edges,
                               size_t* num_edges, int mem_out) {
  return Guard([&] {
    LevelAdjacency(h, seg, seg_len, level, connectedness, neighbourhood, nodes, capacity_nodes, num_nodes, edges,
                   capacity_edges, num_edges, mem_out);
  });
}

int vsg_render_last_adjacency_stats(vsg_render* h, vsg_render_adjacency_stats* s) {
  return Guard([&] {
    if (!h || !s) Throw(VSG_ERR_INVALID, "null argument");
    *s = h->astats;
  });
}

int vsg_render_level_overlap(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness,
                             const int32_t* other, size_t other_pitch, int mem_other,
                             vsg_render_overlap_row* rows, size_t capacity_rows, size_t* num_rows,
                             vsg_render_overlap_col* cols, size_t capacity_cols, size_t* num_cols,
                             vsg_render_overlap_pair* pairs, size_t capacity_pairs, size_t* num_pairs,
                             int mem_out) {
  return Guard([&] {
    using namespace vsg_render_impl;
    static_assert(sizeof(vsg_render_overlap_row) == kOverlapRowWords * sizeof(int32_t), "moved as int32 words");
    static_assert(sizeof(vsg_render_overlap_col) == kOverlapColWords * sizeof(int32_t), "moved as int32 words");
    static_assert(sizeof(vsg_render_overlap_pair) == kOverlapPairWords * sizeof(int32_t), "moved as int32 words");
    if (!h) Throw(VSG_ERR_INVALID, "handle is null");
    if (!num_rows || !num_cols || !num_pairs) Throw(VSG_ERR_INVALID, "a count pointer is null");
    *num_rows = *num_cols = *num_pairs = 0;
    if (!other) Throw(VSG_ERR_INVALID, "other is null");
    if (mem_other != VSG_MEM_HOST && mem_other != VSG_MEM_DEVICE) {
      Throw(VSG_ERR_INVALID, "mem_other is neither VSG_MEM_HOST nor VSG_MEM_DEVICE");
    }
    if (connectedness != 0 && connectedness != VSG_RENDER_CONNECT_N4 && connectedness != VSG_RENDER_CONNECT_N8) {
      Throw(VSG_ERR_INVALID, "connectedness is neither 0, VSG_RENDER_CONNECT_N4 nor VSG_RENDER_CONNECT_N8");
    }
    CheckMem(mem_out, "outputs");
    const int W = h->W, H = h->H;
    if (other_pitch != 0 && other_pitch < (size_t)W) {
      Throw(VSG_ERR_INVALID, "the pitch of other, " + std::to_string(other_pitch) + ", is below the width " +
                                 std::to_string(W));
    }
    const size_t pitch = other_pitch ? other_pitch : (size_t)W;
    const bool count_only =
        !rows && !cols && !pairs && capacity_rows == 0 && capacity_cols == 0 && capacity_pairs == 0;
    if ((uint64_t)W * (uint64_t)H >= (1ull << 32)) Throw(VSG_ERR_INVALID, "the frame has 2^32 pixels or more");
    DeviceGuard guard(h->device);
    vsg_render_overlap_stats& os = h->ostats;
    std::memset(&os, 0, sizeof(os));

    // ---- P: the level's ids, or the indices of its regions' components ----
    const int32_t* plane = nullptr;
    const int32_t* comp_table = nullptr;
    uint32_t max_group = 0;
    uint64_t groups_bound = 0;   // no more groups than this
    bool vector = false;
    if (connectedness == 0) {
      int32_t max_id = 0;
      vector = PaintLevelPlane(h, seg, seg_len, level, &max_id);
      plane = h->d_ids.As<int32_t>();
      max_group = (uint32_t)max_id;
      groups_bound = (uint64_t)h->stats.distinct_ids;
      os.launches = h->stats.launches;
    } else {
      size_t n_components = 0, n_intervals = 0;
      LevelComponents(h, seg, seg_len, level, connectedness, nullptr, 0, &n_components, nullptr, 0, &n_intervals,
                      nullptr, VSG_MEM_DEVICE, true);
      plane = h->d_labels.As<int32_t>();
      comp_table = h->d_comp_table.As<int32_t>();
      max_group = n_components ? (uint32_t)(n_components - 1) : 0u;
      groups_bound = n_components;
      const vsg_render_component_stats& cs = h->cstats;
      os.plane_us = h->stats.clear_us + h->stats.fill_us + cs.runs_us + cs.sort_us + cs.link_us + cs.order_us +
                    cs.label_us;
      os.launches = h->stats.launches;
    }
    int group_bits = 1;
    while (group_bits < 31 && (max_group >> group_bits)) ++group_bits;

    // ---- B: where it is, or through the pinned block to the device, rows packed ----
    h->d_ovl_status.Reserve(sizeof(OvlStatus), &h->allocations);
    h->h_ovl.Reserve(2 * sizeof(OvlStatus), &h->allocations);
    h->d_ovl_totals.Reserve((size_t)H * kOverlapRowTotals * sizeof(uint32_t), &h->allocations);
    OvlStatus* status = h->d_ovl_status.As<OvlStatus>();
    OvlStatus* seen = h->h_ovl.As<OvlStatus>();   // [0] after the count, [1] at the end
    std::memset(seen, 0, 2 * sizeof(OvlStatus));
    int launches = 0;
    const int32_t* label_plane = other;
    size_t label_pitch = pitch;
    h->oclock.Begin(h->stream);
    if (mem_other == VSG_MEM_HOST) {
      const size_t bytes = (size_t)W * H * sizeof(int32_t);
      h->h_other.Reserve(bytes, &h->allocations);
      h->d_other.Reserve(bytes, &h->allocations);
      for (int y = 0; y < H; ++y) {
        std::memcpy(h->h_other.As<int32_t>() + (size_t)y * W, other + (size_t)y * pitch, (size_t)W * sizeof(int32_t));
      }
      VSG_HIP(hipMemcpyAsync(h->d_other.p, h->h_other.p, bytes, hipMemcpyHostToDevice, h->stream));
      label_plane = h->d_other.As<int32_t>();
      label_pitch = (size_t)W;
      ++launches;
    }
    h->oclock.Mark(OVL_UPLOAD);

    // ---- count: the number of runs sizes everything below ----
    VSG_HIP(hipMemsetAsync(status, 0, sizeof(OvlStatus), h->stream));
    LaunchOverlapRuns(plane, label_plane, label_pitch, W, H, 1, 1, false, 0, nullptr, nullptr,
                      h->d_ovl_totals.As<uint32_t>(), status, h->stream);
    VSG_HIP(hipGetLastError());
    h->oclock.Mark(OVL_COUNT);
    VSG_HIP(hipMemcpyAsync(&seen[0], status, sizeof(OvlStatus), hipMemcpyDeviceToHost, h->stream));
    launches += 4;
    VSG_HIP(hipStreamSynchronize(h->stream));
    {
      float us[OVL_STAGES];
      h->oclock.Read(us, OVL_STAGES);
      os.count_us = us[OVL_COUNT];
      os.plane_us += us[OVL_UPLOAD];
    }
    if (connectedness == 0) {
      float us[STAGE_COUNT];
      h->clock.Read(us, STAGE_COUNT);
      h->stats.clear_us = us[STAGE_CLEAR];
      h->stats.fill_us = us[STAGE_FILL];
      os.plane_us += us[STAGE_CLEAR] + us[STAGE_FILL];
      if (vector) h->CheckVector();
    }
    auto finish = [&] {
      os.launches += launches;
      h->stats.launches += launches;
      h->stats.device_allocations = h->allocations;
    };
    os.covered = seen[0].covered;
    os.labelled = seen[0].labelled;
    os.both = seen[0].both;
    os.runs = seen[0].runs;
    if (seen[0].runs > 0x7fffffffu) {
      finish();
      Throw(VSG_ERR_INVALID, "the two planes have more than 2^31 - 1 runs");
    }
    const uint32_t n = seen[0].runs;
    if (n == 0) return finish();   // nothing covered and nothing labelled: all three lists are empty

    // ---- emit, sort, table ----
    const uint32_t max_label = seen[0].max_label;
    int label_bits = 1;
    while (label_bits < 31 && (max_label >> label_bits)) ++label_bits;
    const int end_bit = group_bits + label_bits + 2;
    // distinct keys: no more than runs, and no more than (groups or none) x (labels or none)
    const uint32_t m = (uint32_t)std::min<uint64_t>(n, (groups_bound + 1) * ((uint64_t)max_label + 2));
    const uint32_t cap_rows = (uint32_t)std::min<uint64_t>(groups_bound, n);   // every group has a run
    if (seen[0].covered && cap_rows == 0) Throw(VSG_ERR_INTERNAL, "the plane has groups the desc has no ids for");
    const size_t temp_bytes = std::max<size_t>(std::max(LevelTempBytes(n, end_bit), OverlapScanTempBytes(n)), 16);
    const size_t row_bytes = (size_t)cap_rows * sizeof(vsg_render_overlap_row);
    h->d_sort_temp.Reserve(temp_bytes, &h->allocations);
    h->d_ovl_runs.Reserve((size_t)n * 2 * 12, &h->allocations);
    h->d_ovl_heads.Reserve((size_t)n * 2 * sizeof(unsigned long long), &h->allocations);
    h->d_ovl_keys.Reserve((size_t)m * 24 + 8, &h->allocations);
    h->d_ovl_rows.Reserve(std::max<size_t>(row_bytes, 16), &h->allocations);
    h->d_ovl_cols.Reserve((size_t)m * sizeof(vsg_render_overlap_col), &h->allocations);
    h->d_ovl_pairs.Reserve((size_t)m * sizeof(vsg_render_overlap_pair), &h->allocations);
    // runs: keys, sorted keys, lengths, sorted lengths
    unsigned long long* keys = h->d_ovl_runs.As<unsigned long long>();
    unsigned long long* keys_sorted = keys + n;
    uint32_t* lengths = reinterpret_cast<uint32_t*>(keys + 2 * (size_t)n);
    uint32_t* lengths_sorted = lengths + n;
    unsigned long long* row_heads = h->d_ovl_heads.As<unsigned long long>();
    unsigned long long* key_heads = row_heads + n;
    // distinct keys: key, rank, start (m + 1), the columns' first keys (m + 1)
    unsigned long long* dkey = h->d_ovl_keys.As<unsigned long long>();
    unsigned long long* drank = dkey + m;
    uint32_t* dstart = reinterpret_cast<uint32_t*>(dkey + 2 * (size_t)m);
    uint32_t* cfirst = dstart + m + 1;
    // the column sort: its operands where the unsorted runs were, its results and the labels' ranks where
    // the scans were; m <= n, and both are read for the last time before they are written again
    unsigned long long* ckeys = keys;
    uint32_t* cvals = lengths;
    unsigned long long* ckeys_sorted = row_heads;
    uint32_t* cvals_sorted = reinterpret_cast<uint32_t*>(key_heads);
    uint32_t* col_rank = cvals_sorted + n;
    int32_t* d_rows = h->d_ovl_rows.As<int32_t>();
    int32_t* d_cols = h->d_ovl_cols.As<int32_t>();
    int32_t* d_pairs = h->d_ovl_pairs.As<int32_t>();
    h->oclock.Begin(h->stream);
    LaunchOverlapRuns(plane, label_plane, label_pitch, W, H, group_bits, label_bits, true, n, keys, lengths, nullptr,
                      status, h->stream);
    VSG_HIP(hipGetLastError());
    h->oclock.Mark(OVL_EMIT);
    VSG_HIP(LevelSort(h->d_sort_temp.p, temp_bytes, keys, keys_sorted, lengths, lengths_sorted, n, end_bit,
                      h->stream));
    h->oclock.Mark(OVL_SORT);
    if (row_bytes) VSG_HIP(hipMemsetAsync(d_rows, 0, row_bytes, h->stream));   // `unlabelled` of a row without any
    VSG_HIP(OverlapRank(h->d_sort_temp.p, temp_bytes, keys_sorted, lengths_sorted, group_bits, label_bits, row_heads,
                        key_heads, n, h->stream));
    LaunchOverlapTable(keys_sorted, lengths_sorted, row_heads, key_heads, n, m, group_bits, label_bits, max_group,
                       cap_rows, comp_table, dkey, dstart, drank, d_rows, d_pairs, ckeys, cvals, status, h->stream);
    VSG_HIP(hipGetLastError());
    VSG_HIP(LevelSort(h->d_sort_temp.p, temp_bytes, ckeys, ckeys_sorted, cvals, cvals_sorted, m, end_bit, h->stream));
    VSG_HIP(OverlapColRank(h->d_sort_temp.p, temp_bytes, ckeys_sorted, group_bits, label_bits, col_rank, m,
                           h->stream));
    LaunchOverlapCols(ckeys_sorted, cvals_sorted, col_rank, dstart, drank, m, group_bits, label_bits, cfirst, d_cols,
                      d_pairs, status, h->stream);
    VSG_HIP(hipGetLastError());
    h->oclock.Mark(OVL_TABLE);
    // emit, a clear, table, pairs, rows, column heads, columns; two sorts and three scans counted as one each
    launches += 12;
    const bool to_device = !count_only && mem_out == VSG_MEM_DEVICE;
    if (to_device) {
      // the lengths of the lists are on the device: the copy decides there whether they fit
      LaunchOverlapCopy(d_rows, d_cols, d_pairs, rows ? (uint32_t)std::min<size_t>(capacity_rows, cap_rows) : 0u,
                        cols ? (uint32_t)std::min<size_t>(capacity_cols, m) : 0u,
                        pairs ? (uint32_t)std::min<size_t>(capacity_pairs, m) : 0u, reinterpret_cast<int32_t*>(rows),
                        reinterpret_cast<int32_t*>(cols), reinterpret_cast<int32_t*>(pairs), status, h->stream);
      VSG_HIP(hipGetLastError());
      ++launches;
    }
    VSG_HIP(hipMemcpyAsync(&seen[1], status, sizeof(OvlStatus), hipMemcpyDeviceToHost, h->stream));
    ++launches;
    VSG_HIP(hipStreamSynchronize(h->stream));
    {
      float us[OVL_STAGES];
      h->oclock.Read(us, OVL_STAGES);
      os.emit_us = us[OVL_EMIT];
      os.sort_us = us[OVL_SORT];
      os.table_us = us[OVL_TABLE];
    }
    if ((seen[1].flags & OVL_FLAG_OVERFLOW) || seen[1].emitted != n) {
      finish();
      Throw(VSG_ERR_INTERNAL, "the emit pass found other runs than the count pass");
    }
    if ((seen[1].flags & OVL_FLAG_RANGE) || seen[1].distinct == 0 || seen[1].distinct > m ||
        seen[1].rows > cap_rows || seen[1].pairs > m || seen[1].cols > m ||
        (comp_table && seen[1].rows != groups_bound)) {
      finish();
      Throw(VSG_ERR_INTERNAL, "a sorted overlap key, a row, a column or a pair is out of range");
    }
    const size_t n_rows = seen[1].rows, n_cols = seen[1].cols, n_pairs = seen[1].pairs;
    *num_rows = n_rows;
    *num_cols = n_cols;
    *num_pairs = n_pairs;
    os.rows = (int64_t)n_rows;
    os.cols = (int64_t)n_cols;
    os.pairs = (int64_t)n_pairs;
    os.largest_row_pairs = seen[1].largest;
    if (count_only) return finish();
    if (n_rows > capacity_rows || n_cols > capacity_cols || n_pairs > capacity_pairs) {
      finish();
      Throw(VSG_ERR_INVALID, "the table has " + std::to_string(n_rows) + " rows, " + std::to_string(n_cols) +
                                 " columns and " + std::to_string(n_pairs) + " pairs, the capacities are " +
                                 std::to_string(capacity_rows) + ", " + std::to_string(capacity_cols) + " and " +
                                 std::to_string(capacity_pairs));
    }
    if ((n_rows && !rows) || (n_cols && !cols) || (n_pairs && !pairs)) {
      finish();
      Throw(VSG_ERR_INVALID, "an output is null");
    }
    if (mem_out == VSG_MEM_HOST) {
      // through the pinned block, now that the lengths are known
      const size_t rb = n_rows * sizeof(vsg_render_overlap_row), cb = n_cols * sizeof(vsg_render_overlap_col);
      const size_t pb = n_pairs * sizeof(vsg_render_overlap_pair);
      h->h_ovl.Reserve(2 * sizeof(OvlStatus) + rb + cb + pb, &h->allocations);
      char* stage = reinterpret_cast<char*>(h->h_ovl.As<OvlStatus>() + 2);
      if (rb) VSG_HIP(hipMemcpyAsync(stage, d_rows, rb, hipMemcpyDeviceToHost, h->stream));
      if (cb) VSG_HIP(hipMemcpyAsync(stage + rb, d_cols, cb, hipMemcpyDeviceToHost, h->stream));
      if (pb) VSG_HIP(hipMemcpyAsync(stage + rb + cb, d_pairs, pb, hipMemcpyDeviceToHost, h->stream));
      launches += (rb ? 1 : 0) + (cb ? 1 : 0) + (pb ? 1 : 0);
      VSG_HIP(hipStreamSynchronize(h->stream));
      if (rb) std::memcpy(rows, stage, rb);
      if (cb) std::memcpy(cols, stage + rb, cb);
      if (pb) std::memcpy(pairs, stage + rb + cb, pb);
    }
    finish();
  });
}

int vsg_render_last_overlap_stats(vsg_render* h, vsg_render_overlap_stats* s) {
  return Guard([&] {
    if (!h || !s) Throw(VSG_ERR_INVALID, "null argument");
    *s = h->ostats;
  });
}

}  // extern "C"

namespace {

// The hierarchy's height and the ancestor table of h->pers_ids in h->pers_table, or the refusals of
// vsg_render_id_image at the top level.  Host work only.
int BuildPersistenceTable(vsg_render* h) {
  const size_t L = vsg_render_impl::PersistenceHeight(h->kept.size());
  if (L > 65535) Throw(VSG_ERR_INVALID, "the hierarchy has " + std::to_string(L) + " levels, more than 65535");
  if (h->pers_ids.size() > (1u << 30)) Throw(VSG_ERR_INVALID, "too many regions");
  int bad_level = 0;
  int32_t bad_id = 0;
  if (!vsg_render_impl::BuildAncestorTable(h->kept, h->pers_ids.data(), h->pers_ids.size(), &h->pers_table,
                                           &bad_level, &bad_id)) {
    Throw(VSG_ERR_INVALID,
          "region " + std::to_string(bad_id) + " is not in hierarchy level " + std::to_string(bad_level));
  }
  return (int)L;
}

// Region ids, then the table's rows, to h->d_anc in one copy on the stream; returns the table (null
// when there is none: one level, or no region).  The pinned block gets room for at least pinned_bytes, what
// the call reads back through it later: it must not grow while the copy is in flight.
const int32_t* UploadPersistenceTable(vsg_render* h, size_t pinned_bytes, int* launches) {
  const size_t n = h->pers_ids.size() + h->pers_table.size();
  h->d_anc.Reserve(std::max<size_t>(n, 1) * sizeof(int32_t), &h->allocations);
  h->h_pers.Reserve(std::max(n * sizeof(int32_t), pinned_bytes), &h->allocations);
  if (n == 0) return nullptr;
  int32_t* stage = h->h_pers.As<int32_t>();
  std::copy(h->pers_ids.begin(), h->pers_ids.end(), stage);
  std::copy(h->pers_table.begin(), h->pers_table.end(), stage + h->pers_ids.size());
  VSG_HIP(hipMemcpyAsync(h->d_anc.p, stage, n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  ++*launches;
  return h->pers_table.empty() ? nullptr : h->d_anc.As<int32_t>() + h->pers_ids.size();
}

// The front half of the image and the frame call: the level-0 plane in h->d_plane painted with a dense
// number per distinct region id (so that sparse ids cost nothing), the ancestor table on the device, and
// Q written to q.  Leaves pclock after PRS_PERSIST and the status in flight.  Returns whether the desc was
// vector-only; *levels = L.
bool PaintPersistence(vsg_render* h, const uint8_t* seg, size_t seg_len, int32_t* q, size_t q_pitch, int* levels,
                      int* launches) {
  const int W = h->W, H = h->H;
  vsg_render_persistence_stats& ps = h->pstats;
  h->pers_ids.clear();
  int L = 1;
  uint32_t* plane = h->d_plane.As<uint32_t>();
  const bool vector = PaintIdsAt(
      h, seg, seg_len, 0, plane, h->pitch,
      [&](int mapped) {
        if (mapped < 0) Throw(VSG_ERR_INVALID, "region id " + std::to_string(mapped) + " is negative");
        h->pers_ids.push_back(mapped);
        return (uint32_t)(h->pers_ids.size() - 1);
      },
      [&] { L = BuildPersistenceTable(h); });
  *levels = L;
  ps.levels = L;
  ps.regions = (int64_t)h->pers_ids.size();
  const int32_t* table = UploadPersistenceTable(h, sizeof(PersStatus), launches);
  h->d_pers_status.Reserve(sizeof(PersStatus), &h->allocations);
  PersStatus* status = h->d_pers_status.As<PersStatus>();
  VSG_HIP(hipMemsetAsync(status, 0, sizeof(PersStatus), h->stream));
  h->pclock.Begin(h->stream);
  vsg_render_impl::LaunchPersistPlane(reinterpret_cast<const int32_t*>(plane), h->pitch, W, H, table,
                                      (uint32_t)h->pers_ids.size(), L, q, q_pitch, status, h->stream);
  VSG_HIP(hipGetLastError());
  h->pclock.Mark(PRS_PERSIST);
  *launches += 2;
  return vector;
}

// The back half: the status back, the one synchronisation, the stats, the device's flag.
void FinishPersistence(vsg_render* h, bool vector, int launches) {
  vsg_render_persistence_stats& ps = h->pstats;
  // the table went through the pinned block before the plane kernel ran; the status may follow it
  PersStatus* seen = h->h_pers.As<PersStatus>();
  VSG_HIP(hipMemcpyAsync(seen, h->d_pers_status.p, sizeof(PersStatus), hipMemcpyDeviceToHost, h->stream));
  ++launches;
  h->FinishStats();
  float us[PRS_STAGES];
  h->pclock.Read(us, PRS_STAGES);
  ps.plane_us = h->stats.clear_us + h->stats.fill_us;
  ps.persist_us = us[PRS_PERSIST];
  ps.compose_us = us[PRS_COMPOSE];
  h->stats.launches += launches;
  ps.launches = h->stats.launches;
  if (vector) h->CheckVector();
  if (seen->flags) Throw(VSG_ERR_INTERNAL, "the plane holds a region number the host did not give out");
  ps.edge_pixels = (int64_t)seen->edge_pixels;
  ps.top_pixels = (int64_t)seen->top_pixels;
}

}  // namespace

extern "C" {

int vsg_render_persistence_image(vsg_render* h, const uint8_t* seg, size_t seg_len, int32_t* out, int* num_levels,
                                 int mem_out) {
  return Guard([&] {
    if (!h) Throw(VSG_ERR_INVALID, "handle is null");
    if (!out) Throw(VSG_ERR_INVALID, "out is null");
    if (!num_levels) Throw(VSG_ERR_INVALID, "the count pointer is null");
    CheckMem(mem_out, "out");
    *num_levels = 0;
    const int W = h->W, H = h->H;
    const size_t bytes = (size_t)W * H * sizeof(int32_t);
    DeviceGuard guard(h->device);
    std::memset(&h->pstats, 0, sizeof(h->pstats));
    int32_t* q = out;   // device output: written in place
    if (mem_out == VSG_MEM_HOST) {
      h->d_pq.Reserve(bytes, &h->allocations);
      q = h->d_pq.As<int32_t>();
    }
    int launches = 0, levels = 0;
    const bool vector = PaintPersistence(h, seg, seg_len, q, (size_t)W, &levels, &launches);
    if (mem_out == VSG_MEM_HOST) {
      VSG_HIP(hipMemcpyAsync(out, q, bytes, hipMemcpyDeviceToHost, h->stream));
      ++launches;
    }
    FinishPersistence(h, vector, launches);
    *num_levels = levels;
  });
}

int vsg_render_persistence_frame(vsg_render* h, const uint8_t* seg, size_t seg_len, const uint8_t* bgr, size_t stride,
                                 int mem_in, uint8_t* out, size_t out_stride, int mem_out, int* num_levels) {
  return Guard([&] {
    if (!h) Throw(VSG_ERR_INVALID, "handle is null");
    if (!out) Throw(VSG_ERR_INVALID, "out is null");
    if (!num_levels) Throw(VSG_ERR_INVALID, "the count pointer is null");
    CheckMem(mem_in, "bgr");
    CheckMem(mem_out, "out");
    *num_levels = 0;
    const int W = h->W, H = h->H;
    const size_t row_bytes = (size_t)W * 3;
    const bool video = h->opt.has_video != 0;
    if (video && !bgr) Throw(VSG_ERR_INVALID, "the handle was created with has_video: bgr is null");
    if (video && stride < row_bytes) Throw(VSG_ERR_INVALID, "stride is smaller than 3 * width");
    if (out_stride == 0) out_stride = vsg_render_default_stride(W);
    if (out_stride < row_bytes) Throw(VSG_ERR_INVALID, "out_stride is smaller than 3 * width");
    DeviceGuard guard(h->device);
    std::memset(&h->pstats, 0, sizeof(h->pstats));
    // Q has the plane's pitch: every tile row of it is 16-byte aligned
    h->d_pq.Reserve((size_t)h->pitch * H * sizeof(int32_t), &h->allocations);
    int32_t* q = h->d_pq.As<int32_t>();
    int launches = 0, levels = 0;
    const bool vector = PaintPersistence(h, seg, seg_len, q, (size_t)h->pitch, &levels, &launches);
    const uint8_t* src = nullptr;
    size_t src_stride = 0;
    if (video) {
      if (mem_in == VSG_MEM_DEVICE) {
        src = bgr;
        src_stride = stride;
      } else {
        src_stride = vsg_render_default_stride(W);
        h->d_src.Reserve(src_stride * H, &h->allocations);
        VSG_HIP(hipMemcpy2DAsync(h->d_src.p, src_stride, bgr, stride, row_bytes, H, hipMemcpyHostToDevice,
                                 h->stream));
        ++launches;
        src = static_cast<const uint8_t*>(h->d_src.p);
      }
    }
    uint8_t* dst = out;
    size_t dst_stride = out_stride;
    if (mem_out == VSG_MEM_HOST) {
      dst_stride = vsg_render_default_stride(W);
      h->d_out.Reserve(dst_stride * H, &h->allocations);
      dst = static_cast<uint8_t*>(h->d_out.p);
    }
    h->pclock.Mark(PRS_WAIT);
    vsg_render_impl::LaunchPersistCompose(q, (size_t)h->pitch, W, H, levels, src, src_stride, dst, dst_stride,
                                          h->stream);
    VSG_HIP(hipGetLastError());
    h->pclock.Mark(PRS_COMPOSE);
    ++launches;
    if (mem_out == VSG_MEM_HOST) {
      VSG_HIP(hipMemcpy2DAsync(out, out_stride, dst, dst_stride, row_bytes, H, hipMemcpyDeviceToHost, h->stream));
      ++launches;
    }
    FinishPersistence(h, vector, launches);
    *num_levels = levels;
  });
}

int vsg_render_persistence_graph(vsg_render* h, const uint8_t* seg, size_t seg_len, int neighbourhood,
                                 vsg_render_level_node* nodes, size_t capacity_nodes, size_t* num_nodes,
                                 vsg_render_level_edge* edges, size_t capacity_edges, size_t* num_edges,
                                 int32_t* persistence, int64_t* level_sides, size_t capacity_levels,
                                 size_t* num_levels, int mem_out) {
  return Guard([&] {
    using namespace vsg_render_impl;
    if (neighbourhood != VSG_RENDER_ADJACENT_N4 && neighbourhood != VSG_RENDER_ADJACENT_N8) {
      Throw(VSG_ERR_INVALID, "neighbourhood is neither VSG_RENDER_ADJACENT_N4 nor VSG_RENDER_ADJACENT_N8");
    }
    if (!h) Throw(VSG_ERR_INVALID, "handle is null");
    if (!num_nodes || !num_edges || !num_levels) Throw(VSG_ERR_INVALID, "a count pointer is null");
    *num_nodes = *num_edges = *num_levels = 0;
    CheckMem(mem_out, "outputs");
    const bool count_only = !nodes && !edges && !persistence && !level_sides && capacity_nodes == 0 &&
                            capacity_edges == 0 && capacity_levels == 0;
    DeviceGuard guard(h->device);
    vsg_render_persistence_stats& ps = h->pstats;
    std::memset(&ps, 0, sizeof(ps));

    // ---- the level-0 graph, left on the device ----
    size_t n_nodes = 0, n_edges = 0;
    LevelAdjacency(h, seg, seg_len, 0, 0, neighbourhood, nullptr, 0, &n_nodes, nullptr, 0, &n_edges, VSG_MEM_DEVICE);
    const vsg_render_adjacency_stats& as = h->astats;
    ps.nodes = (int64_t)n_nodes;
    ps.edges = (int64_t)n_edges;
    ps.plane_us = as.plane_us;
    ps.graph_us = as.count_us + as.emit_us + as.sort_us + as.table_us;
    int launches = 0;
    auto finish = [&] {
      h->stats.launches += launches;
      ps.launches = h->stats.launches;
      h->stats.device_allocations = h->allocations;
    };

    // ---- the ancestors of every region that paints, by ascending id ----
    const ParsedDesc& d = h->desc;
    const bool vector = d.rasterization_removed && d.has_mesh;
    h->pers_ids.clear();
    for (size_t r = 0; r < d.region_ids.size(); ++r) {
      const bool paints = vector ? d.region_poly_begin[r] != d.region_poly_begin[r + 1]
                                 : d.region_begin[r] != d.region_begin[r + 1];
      if (paints) h->pers_ids.push_back(d.region_ids[r]);   // none is negative: the adjacency call refused those
    }
    std::sort(h->pers_ids.begin(), h->pers_ids.end());
    h->pers_ids.erase(std::unique(h->pers_ids.begin(), h->pers_ids.end()), h->pers_ids.end());
    int L = 1;
    try {
      L = BuildPersistenceTable(h);
    } catch (...) {
      finish();
      throw;
    }
    ps.levels = L;
    ps.regions = (int64_t)h->pers_ids.size();
    *num_nodes = n_nodes;
    *num_edges = n_edges;
    *num_levels = (size_t)L;

    // ---- one thread per edge, then the levels' sums ----
    const size_t hist_bytes = ((size_t)L + 1) * sizeof(unsigned long long);
    const size_t sides_bytes = (size_t)L * sizeof(int64_t);
    const size_t pers_bytes = n_edges * sizeof(int32_t);
    h->d_pers_out.Reserve(hist_bytes + sides_bytes + pers_bytes, &h->allocations);
    h->d_pers_status.Reserve(sizeof(PersStatus), &h->allocations);
    unsigned long long* hist = h->d_pers_out.As<unsigned long long>();
    long long* d_sides = reinterpret_cast<long long*>(hist + L + 1);
    int32_t* d_pers = reinterpret_cast<int32_t*>(d_sides + L);
    PersStatus* status = h->d_pers_status.As<PersStatus>();
    // the table has left the pinned block by the time the status and the lists arrive in it
    const size_t nb = n_nodes * sizeof(vsg_render_level_node), eb = n_edges * sizeof(vsg_render_level_edge);
    const bool fits = n_nodes <= capacity_nodes && n_edges <= capacity_edges && (size_t)L <= capacity_levels;
    const bool have = (n_nodes == 0 || nodes) && level_sides && (n_edges == 0 || (edges && persistence));
    const bool to_host = !count_only && fits && have && mem_out == VSG_MEM_HOST;
    const int32_t* table = UploadPersistenceTable(
        h, sizeof(PersStatus) + (to_host ? sides_bytes + nb + eb + pers_bytes : 0), &launches);
    VSG_HIP(hipMemsetAsync(status, 0, sizeof(PersStatus), h->stream));
    VSG_HIP(hipMemsetAsync(hist, 0, hist_bytes, h->stream));
    h->pclock.Begin(h->stream);
    LaunchPersistEdges(h->d_adj_nodes.As<int32_t>(), (uint32_t)n_nodes, h->d_adj_edges.As<int32_t>(),
                       (uint32_t)n_edges, h->d_anc.As<int32_t>(), (uint32_t)h->pers_ids.size(), table, L, d_pers, hist,
                       status, h->stream);
    LaunchPersistSides(hist, L, d_sides, h->stream);
    VSG_HIP(hipGetLastError());
    h->pclock.Mark(PRS_PERSIST);
    launches += 3 + (n_edges ? 1 : 0);
    char* stage = h->h_pers.As<char>();
    VSG_HIP(hipMemcpyAsync(stage, status, sizeof(PersStatus), hipMemcpyDeviceToHost, h->stream));
    ++launches;
    VSG_HIP(hipStreamSynchronize(h->stream));
    {
      float us[PRS_STAGES];
      h->pclock.Read(us, PRS_STAGES);
      ps.persist_us = us[PRS_PERSIST];
    }
    if (reinterpret_cast<const PersStatus*>(stage)->flags) {
      finish();
      Throw(VSG_ERR_INTERNAL, "an edge of the level-0 graph, its node or a region id is out of range");
    }
    if (count_only) return finish();
    if (!fits) {
      finish();
      Throw(VSG_ERR_INVALID, "the graph has " + std::to_string(n_nodes) + " nodes and " + std::to_string(n_edges) +
                                 " edges, the hierarchy " + std::to_string(L) + " levels; the capacities are " +
                                 std::to_string(capacity_nodes) + ", " + std::to_string(capacity_edges) + " and " +
                                 std::to_string(capacity_levels));
    }
    if (!have) {
      finish();
      Throw(VSG_ERR_INVALID, "an output is null");
    }
    // the lengths are known: four copies, through the pinned block for host outputs
    struct Part {
      void* to;
      const void* from;
      size_t bytes;
    };
    const Part parts[4] = {{level_sides, d_sides, sides_bytes},
                           {nodes, h->d_adj_nodes.p, nb},
                           {edges, h->d_adj_edges.p, eb},
                           {persistence, d_pers, pers_bytes}};
    char* at = stage + sizeof(PersStatus);
    for (const Part& part : parts) {
      if (!part.bytes) continue;
      if (to_host) VSG_HIP(hipMemcpyAsync(at, part.from, part.bytes, hipMemcpyDeviceToHost, h->stream));
      else VSG_HIP(hipMemcpyAsync(part.to, part.from, part.bytes, hipMemcpyDeviceToDevice, h->stream));
      at += part.bytes;
      ++launches;
    }
    VSG_HIP(hipStreamSynchronize(h->stream));
    if (to_host) {
      at = stage + sizeof(PersStatus);
      for (const Part& part : parts) {
        if (part.bytes) std::memcpy(part.to, at, part.bytes);
        at += part.bytes;
      }
    }
    finish();
  });
}

int vsg_render_last_persistence_stats(vsg_render* h, vsg_render_persistence_stats* s) {
  return Guard([&] {
    if (!h || !s) Throw(VSG_ERR_INVALID, "null argument");
    *s = h->pstats;
  });
}

}  // extern "C"

namespace {

// vsg_render_level_colors (picture == nullptr) and vsg_render_mean_frame (colors == nullptr) behind their
// argument checks that need no handle.
void LevelColors(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness, const uint8_t* bgr,
                 size_t stride, int mem_in, vsg_render_level_color* colors, size_t capacity_colors, size_t* num_colors,
                 uint8_t* picture, size_t out_stride, int mem_out) {
  using namespace vsg_render_impl;
  static_assert(sizeof(vsg_render_level_color) == kLevelColorWords * sizeof(int32_t), "moved as int32 words");
  static_assert(sizeof(vsg_render_color_stats) == 56, "as the header says");
  const int W = h->W, H = h->H;
  const size_t row_bytes = (size_t)W * 3;
  if (stride < row_bytes) Throw(VSG_ERR_INVALID, "stride is smaller than 3 * width");
  if (picture) {
    if (out_stride == 0) out_stride = vsg_render_default_stride(W);
    if (out_stride < row_bytes) Throw(VSG_ERR_INVALID, "out_stride is smaller than 3 * width");
  }
  const bool count_only = !picture && !colors && capacity_colors == 0;
  if (!picture && !colors && capacity_colors) Throw(VSG_ERR_INVALID, "colors is null");
  if ((uint64_t)W * (uint64_t)H >= (1ull << 32)) Throw(VSG_ERR_INVALID, "the frame has 2^32 pixels or more");
  DeviceGuard guard(h->device);
  vsg_render_color_stats& ks = h->kstats;
  std::memset(&ks, 0, sizeof(ks));

  // ---- the interval list grouped by record, every interval's record, id and component of every record ----
  const Interval* list = nullptr;
  const uint32_t* rank = nullptr;
  const int32_t* table = nullptr;
  const uint32_t* d_count = nullptr;
  int table_words = 0;
  uint32_t n = 0, cap_records = 0;
  vsg_render_level_stats ls;   // of the shared front half; the last level_regions call's stay
  std::memset(&ls, 0, sizeof(ls));
  if (connectedness == 0) {
    LevelFront f = PaintLevelRuns(h, seg, seg_len, level, &ls);
    n = f.n;
    if (n) SortLevelRuns(h, &f, &ls);
    list = f.intervals;
    rank = f.rank;
    table = f.regions;
    table_words = kLevelRegionWords;
    d_count = &f.status->regions;
    cap_records = f.cap_regions;
    ks.plane_us = h->stats.clear_us + h->stats.fill_us + ls.runs_us;
    h->stats.launches += ls.launches;
  } else {
    size_t n_components = 0, n_intervals = 0;
    LevelComponents(h, seg, seg_len, level, connectedness, nullptr, 0, &n_components, nullptr, 0, &n_intervals, nullptr,
                    VSG_MEM_DEVICE, true);
    n = (uint32_t)n_intervals;
    list = h->d_comp_intervals.As<Interval>();
    rank = h->d_comp_work.As<uint32_t>() + (size_t)5 * n;   // LevelComponents' comp_rank
    table = h->d_comp_table.As<int32_t>();
    table_words = kLevelComponentWords;
    d_count = &h->d_comp_status.As<CompStatus>()->components;
    cap_records = (uint32_t)n_components;
    const vsg_render_component_stats& cs = h->cstats;
    ks.plane_us = h->stats.clear_us + h->stats.fill_us + cs.runs_us + cs.sort_us + cs.link_us + cs.order_us +
                  cs.label_us;
  }
  ks.launches = h->stats.launches;
  ks.intervals = n;
  if (n && cap_records == 0) Throw(VSG_ERR_INTERNAL, "the plane has groups the desc has no ids for");

  // ---- blocks, all before anything that uses them is enqueued ----
  struct Seen {
    ColorStatus status;
    uint32_t records, pad[3];
  };
  const size_t record_bytes = (size_t)cap_records * sizeof(vsg_render_level_color);
  const bool host_table = colors && mem_out == VSG_MEM_HOST;
  h->d_color_status.Reserve(sizeof(ColorStatus), &h->allocations);
  h->h_color.Reserve(sizeof(Seen) + (host_table ? record_bytes : 0), &h->allocations);
  h->d_color_partials.Reserve((size_t)n * kColorPartialWords * sizeof(uint32_t), &h->allocations);
  h->d_color_acc.Reserve((size_t)cap_records * kColorAccBytes, &h->allocations);
  if (host_table || picture) h->d_color_records.Reserve(record_bytes, &h->allocations);
  if (picture) h->d_color_intervals.Reserve((size_t)n * sizeof(Interval), &h->allocations);
  ColorStatus* status = h->d_color_status.As<ColorStatus>();
  Seen* seen = h->h_color.As<Seen>();
  std::memset(seen, 0, sizeof(Seen));
  int launches = 0;

  // ---- F: where it is, or to the device with the default stride ----
  const uint8_t* src = bgr;
  size_t src_stride = stride;
  h->kclock.Begin(h->stream);
  if (mem_in == VSG_MEM_HOST) {
    src_stride = vsg_render_default_stride(W);
    h->d_src.Reserve(src_stride * H, &h->allocations);
    VSG_HIP(hipMemcpy2DAsync(h->d_src.p, src_stride, bgr, stride, row_bytes, H, hipMemcpyHostToDevice, h->stream));
    ++launches;
    src = h->d_src.As<uint8_t>();
  }
  uint8_t* dst = picture;
  size_t dst_stride = out_stride;
  const int out_rows = h->opt.concat_with_source ? 2 * H : H;
  if (picture && mem_out == VSG_MEM_HOST) {
    dst_stride = vsg_render_default_stride(W);
    h->d_out.Reserve(dst_stride * out_rows, &h->allocations);
    dst = h->d_out.As<uint8_t>();
  }
  h->kclock.Mark(CLR_UPLOAD);

  // ---- partials, table ----
  uint32_t* partials = h->d_color_partials.As<uint32_t>();
  LaunchColorRuns(list, n, W, H, src, src_stride, partials, h->stream);
  VSG_HIP(hipGetLastError());
  h->kclock.Mark(CLR_SUMS);
  // where the records go: the caller's device memory (the kernel decides there whether they fit), or the
  // handle's block; nowhere in a count-only call
  int32_t* records = nullptr;
  uint32_t capacity = 0;
  if (picture || host_table) {
    records = h->d_color_records.As<int32_t>();
    capacity = cap_records;
  } else if (colors) {
    records = reinterpret_cast<int32_t*>(colors);
    capacity = (uint32_t)std::min<size_t>(capacity_colors, cap_records);
  }
  VSG_HIP(hipMemsetAsync(status, 0, sizeof(ColorStatus), h->stream));
  ++launches;
  if (n) {
    VSG_HIP(hipMemsetAsync(h->d_color_acc.p, 0, (size_t)cap_records * kColorAccBytes, h->stream));
    LaunchColorTable(list, rank, partials, n, cap_records, h->d_color_acc.p, table, table_words, connectedness != 0,
                     d_count, capacity, records, status, h->stream);
    VSG_HIP(hipGetLastError());
    VSG_HIP(hipMemcpyAsync(&seen->records, d_count, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    launches += 5;   // k_color_runs, the clear, k_color_table, k_color_finish, the count
  }
  h->kclock.Mark(CLR_TABLE);

  // ---- the picture: vsg_render_frame's clear, fill and compose on the intervals with the means ----
  if (picture) {
    const bool video = h->opt.has_video != 0;
    Interval* painted = h->d_color_intervals.As<Interval>();
    uint32_t* plane = h->d_plane.As<uint32_t>();
    LaunchColorIntervals(list, rank, n, records, capacity, painted, h->stream);
    VSG_HIP(hipMemsetAsync(plane, 0, (size_t)h->pitch * H * sizeof(uint32_t), h->stream));
    LaunchFill(painted, n, plane, h->pitch, h->stream);
    const int mode = h->opt.concat_with_source ? COMPOSE_CONCAT : video ? COMPOSE_BLEND : COMPOSE_RENDER;
    LaunchCompose(plane, h->pitch, W, H, src, src_stride, dst, dst_stride, h->opt.highlight_edges, mode,
                  h->opt.blend_alpha, h->stream);
    VSG_HIP(hipGetLastError());
    launches += 2 + (n ? 2 : 0);
    h->kclock.Mark(CLR_PAINT);
    if (mem_out == VSG_MEM_HOST) {
      VSG_HIP(hipMemcpy2DAsync(picture, out_stride, dst, dst_stride, row_bytes, out_rows, hipMemcpyDeviceToHost,
                               h->stream));
      ++launches;
    }
  }
  if (host_table && n) {
    VSG_HIP(hipMemcpyAsync(seen + 1, records, record_bytes, hipMemcpyDeviceToHost, h->stream));
    ++launches;
  }
  VSG_HIP(hipMemcpyAsync(&seen->status, status, sizeof(ColorStatus), hipMemcpyDeviceToHost, h->stream));
  ++launches;
  VSG_HIP(hipStreamSynchronize(h->stream));
  {
    float us[CLR_STAGES];
    h->kclock.Read(us, CLR_STAGES);
    ks.plane_us += us[CLR_UPLOAD];
    ks.sums_us = us[CLR_SUMS];
    ks.table_us = us[CLR_TABLE];
    ks.paint_us = us[CLR_PAINT];
    if (n && connectedness == 0) {
      float lus[LVL_COUNT];
      h->lclock.Read(lus, LVL_COUNT);
      ks.plane_us += lus[LVL_SORT] + lus[LVL_TABLE];
    }
  }
  ks.launches += launches;
  h->stats.launches += launches;
  h->stats.device_allocations = h->allocations;
  const uint32_t n_records = seen->records;
  if ((n == 0) != (n_records == 0) || n_records > cap_records || (connectedness != 0 && n_records != cap_records)) {
    Throw(VSG_ERR_INTERNAL, "the level has other groups than the desc has ids for");
  }
  if ((seen->status.flags & COLOR_FLAG_RANGE) || seen->status.largest > n) {
    Throw(VSG_ERR_INTERNAL, "an interval's record is out of range");
  }
  ks.groups = n_records;
  ks.covered = (int64_t)seen->status.covered;
  ks.largest_group_intervals = seen->status.largest;
  if (num_colors) *num_colors = n_records;
  if (picture || count_only) return;
  if (n_records > capacity_colors) {
    Throw(VSG_ERR_INVALID, "the level has " + std::to_string(n_records) + " groups, the capacity is " +
                               std::to_string(capacity_colors));
  }
  if (host_table && n_records) std::memcpy(colors, seen + 1, (size_t)n_records * sizeof(vsg_render_level_color));
}

// The refusals of both calls that are answered before the handle is dereferenced.
void CheckColorArguments(const vsg_render* h, int connectedness, const uint8_t* bgr, int mem_in, int mem_out) {
  if (!h) Throw(VSG_ERR_INVALID, "handle is null");
  if (!bgr) Throw(VSG_ERR_INVALID, "bgr is null");
  if (mem_in != VSG_MEM_HOST && mem_in != VSG_MEM_DEVICE) {
    Throw(VSG_ERR_INVALID, "mem_in is neither VSG_MEM_HOST nor VSG_MEM_DEVICE");
  }
  if (mem_out != VSG_MEM_HOST && mem_out != VSG_MEM_DEVICE) {
    Throw(VSG_ERR_INVALID, "mem_out is neither VSG_MEM_HOST nor VSG_MEM_DEVICE");
  }
  if (connectedness != 0 && connectedness != VSG_RENDER_CONNECT_N4 && connectedness != VSG_RENDER_CONNECT_N8) {
    Throw(VSG_ERR_INVALID, "connectedness is neither 0, VSG_RENDER_CONNECT_N4 nor VSG_RENDER_CONNECT_N8");
  }
}

}  // namespace

extern "C" {

int vsg_render_level_colors(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness,
                            const uint8_t* bgr, size_t stride, int mem_in, vsg_render_level_color* colors,
                            size_t capacity_colors, size_t* num_colors, int mem_out) {
  return Guard([&] {
    if (!num_colors) Throw(VSG_ERR_INVALID, "the count pointer is null");
    *num_colors = 0;
    CheckColorArguments(h, connectedness, bgr, mem_in, mem_out);
    LevelColors(h, seg, seg_len, level, connectedness, bgr, stride, mem_in, colors, capacity_colors, num_colors,
                nullptr, 0, mem_out);
  });
}

int vsg_render_mean_frame(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness,
                          const uint8_t* bgr, size_t stride, int mem_in, uint8_t* out, size_t out_stride,
                          int mem_out) {
  return Guard([&] {
    if (!out) Throw(VSG_ERR_INVALID, "out is null");
    CheckColorArguments(h, connectedness, bgr, mem_in, mem_out);
    LevelColors(h, seg, seg_len, level, connectedness, bgr, stride, mem_in, nullptr, 0, nullptr, out, out_stride,
                mem_out);
  });
}

int vsg_render_last_color_stats(vsg_render* h, vsg_render_color_stats* s) {
  return Guard([&] {
    if (!h || !s) Throw(VSG_ERR_INVALID, "null argument");
    *s = h->kstats;
  });
}

}  // extern "C"

namespace {

// What a vsg_render_level_contours call left on the device for vsg_render_level_mesh; in.n == 0: no crack.
struct ContourRun {
  vsg_render_impl::MeshInput in;
  const unsigned long long* ckeys_sorted;
  uint32_t max_group;
  int rounds;
};

// vsg_render_level_contours; run: null, or what the mesh call goes on with.
void LevelContours(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness,
                   vsg_render_level_contour* contours, size_t capacity_contours, size_t* num_contours,
                   int32_t* vertices, size_t capacity_vertices, size_t* num_vertices, int mem_out, ContourRun* run) {
  {
    using namespace vsg_render_impl;
    if (run) std::memset(run, 0, sizeof(*run));
    static_assert(sizeof(vsg_render_level_contour) == kLevelContourWords * sizeof(int32_t), "moved as int32 words");
    static_assert(sizeof(vsg_render_contour_stats) == 64, "documented size");
    if (connectedness != 0 && connectedness != VSG_RENDER_CONNECT_N4 && connectedness != VSG_RENDER_CONNECT_N8) {
      Throw(VSG_ERR_INVALID, "connectedness is neither 0, VSG_RENDER_CONNECT_N4 nor VSG_RENDER_CONNECT_N8");
    }
    if (!h) Throw(VSG_ERR_INVALID, "handle is null");
    if (!num_contours || !num_vertices) Throw(VSG_ERR_INVALID, "a count pointer is null");
    *num_contours = *num_vertices = 0;
    CheckMem(mem_out, "mem_out");
    const bool count_only = !contours && !vertices && capacity_contours == 0 && capacity_vertices == 0;
    const int W = h->W, H = h->H;
    if ((uint64_t)W * (uint64_t)H * 4 > (1ull << 31)) {
      Throw(VSG_ERR_INVALID, "the frame has more than 2^31 pixel sides: crack keys do not fit 32 bits");
    }
    const uint32_t pixels = (uint32_t)W * (uint32_t)H;
    DeviceGuard guard(h->device);
    vsg_render_contour_stats& ts = h->tstats;
    std::memset(&ts, 0, sizeof(ts));
    // the offsets' scan runs before the first synchronisation: its work space before anything is enqueued
    const size_t scan_bytes = std::max<size_t>(ContourTempBytes(pixels, 1, 64), 16);
    h->d_sort_temp.Reserve(scan_bytes, &h->allocations);

    // ---- the plane: the level's ids, or the indices of its regions' components ----
    const int32_t* plane = nullptr;
    const int32_t* comp_table = nullptr;
    uint32_t max_group = 0;
    bool vector = false;
    if (connectedness == 0) {
      int32_t max_id = 0;
      vector = PaintLevelPlane(h, seg, seg_len, level, &max_id);
      plane = h->d_ids.As<int32_t>();
      max_group = (uint32_t)max_id;
      ts.launches = h->stats.launches;
    } else {
      size_t n_components = 0, n_intervals = 0;
      LevelComponents(h, seg, seg_len, level, connectedness, nullptr, 0, &n_components, nullptr, 0, &n_intervals,
                      nullptr, VSG_MEM_DEVICE, true);
      plane = h->d_labels.As<int32_t>();
      comp_table = h->d_comp_table.As<int32_t>();
      max_group = n_components ? (uint32_t)(n_components - 1) : 0u;
      const vsg_render_component_stats& cs = h->cstats;
      ts.plane_us = h->stats.clear_us + h->stats.fill_us + cs.runs_us + cs.sort_us + cs.link_us + cs.order_us +
                    cs.label_us;
      ts.launches = h->stats.launches;
    }

    // ---- count: the number of cracks sizes everything below ----
    h->d_cont_status.Reserve(sizeof(ContourStatus), &h->allocations);
    h->h_cont.Reserve(2 * sizeof(ContourStatus), &h->allocations);
    h->d_cont_mask.Reserve(pixels, &h->allocations);
    h->d_cont_offset.Reserve((size_t)pixels * sizeof(uint32_t), &h->allocations);
    ContourStatus* status = h->d_cont_status.As<ContourStatus>();
    ContourStatus* seen = h->h_cont.As<ContourStatus>();   // [0] after the count, [1] at the end
    std::memset(seen, 0, 2 * sizeof(ContourStatus));
    uint8_t* mask = h->d_cont_mask.As<uint8_t>();
    uint32_t* offset = h->d_cont_offset.As<uint32_t>();
    VSG_HIP(hipMemsetAsync(status, 0, sizeof(ContourStatus), h->stream));
    h->tclock.Begin(h->stream);
    VSG_HIP(ContourClassify(h->d_sort_temp.p, h->d_sort_temp.cap, plane, W, H, mask, offset, status, h->stream));
    VSG_HIP(hipGetLastError());
    h->tclock.Mark(CNT_CLASSIFY);
    VSG_HIP(hipMemcpyAsync(&seen[0], status, sizeof(ContourStatus), hipMemcpyDeviceToHost, h->stream));
    int launches = 4;   // the clear, the masks, the scan counted as one, the status
    VSG_HIP(hipStreamSynchronize(h->stream));
    {
      float us[CNT_STAGES];
      h->tclock.Read(us, CNT_STAGES);
      ts.classify_us = us[CNT_CLASSIFY];
    }
    if (connectedness == 0) {
      float us[STAGE_COUNT];
      h->clock.Read(us, STAGE_COUNT);
      h->stats.clear_us = us[STAGE_CLEAR];
      h->stats.fill_us = us[STAGE_FILL];
      ts.plane_us = us[STAGE_CLEAR] + us[STAGE_FILL];
      if (vector) h->CheckVector();
    }
    auto finish = [&] {
      ts.launches += launches;
      h->stats.launches += launches;
      h->stats.device_allocations = h->allocations;
    };
    if (seen[0].cracks > 4ull * pixels) {
      finish();
      Throw(VSG_ERR_INTERNAL, "more cracks than pixel sides");
    }
    const uint32_t n = (uint32_t)seen[0].cracks;
    ts.cracks = n;
    if (n == 0) return finish();   // no covered pixel: both lists are empty
    if (n < 4) {
      finish();
      Throw(VSG_ERR_INTERNAL, "fewer cracks than one pixel has");
    }

    // ---- emit, trace, table ----
    const int rounds = ContourRounds(n);
    const uint32_t cap = n / 4;   // a contour has four cracks or more
    int group_bits = 1;
    while (group_bits < 32 && (max_group >> group_bits)) ++group_bits;
    const int end_bit = 32 + group_bits;
    const size_t temp_bytes = std::max<size_t>(ContourTempBytes(pixels, cap, end_bit), 16);
    h->d_sort_temp.Reserve(temp_bytes, &h->allocations);
    h->d_cont_cracks.Reserve((size_t)n * 36, &h->allocations);
    h->d_cont_slots.Reserve((size_t)cap * 28, &h->allocations);
    h->d_cont_records.Reserve((size_t)cap * sizeof(vsg_render_level_contour), &h->allocations);
    uint2* state_a = h->d_cont_cracks.As<uint2>();
    uint2* state_b = state_a + n;
    uint32_t* key = reinterpret_cast<uint32_t*>(state_b + n);
    uint32_t* succ = key + n;
    uint32_t* leader = succ + n;
    uint32_t* place = leader + n;
    uint32_t* owner = place + n;
    unsigned long long* ckeys = h->d_cont_slots.As<unsigned long long>();
    unsigned long long* ckeys_sorted = ckeys + cap;
    uint32_t* crank = reinterpret_cast<uint32_t*>(ckeys_sorted + cap);
    uint32_t* count = crank + cap;
    uint32_t* first = count + cap;
    int32_t* d_records = h->d_cont_records.As<int32_t>();
    h->tclock.Begin(h->stream);
    LaunchContourEmit(plane, W, H, mask, offset, n, key, succ, state_a, status, h->stream);
    VSG_HIP(hipGetLastError());
    h->tclock.Mark(CNT_CLASSIFY);
    const uint2* ranked = LaunchContourTrace(key, succ, n, rounds, state_a, state_b, leader, status, h->stream);
    // the doubling state that is not the result holds the vertices: n pairs at the most
    int32_t* d_vertices = reinterpret_cast<int32_t*>(ranked == state_a ? state_b : state_a);
    VSG_HIP(hipMemsetAsync(ckeys, 0xff, (size_t)cap * sizeof(unsigned long long), h->stream));   // unused: last
    LaunchContourLeaders(leader, key, plane, n, cap, ckeys, status, h->stream);
    VSG_HIP(hipGetLastError());
    VSG_HIP(ContourSort(h->d_sort_temp.p, temp_bytes, ckeys, ckeys_sorted, cap, end_bit, h->stream));
    VSG_HIP(LevelRank(h->d_sort_temp.p, temp_bytes, ckeys_sorted, crank, cap, h->stream));
    VSG_HIP(ContourVertices(h->d_sort_temp.p, temp_bytes, ckeys_sorted, key, succ, leader, ranked, n, cap, W, place,
                            count, first, d_vertices, owner, status, h->stream));
    VSG_HIP(hipGetLastError());
    h->tclock.Mark(CNT_TRACE);
    LaunchContourTable(ckeys_sorted, crank, count, first, d_vertices, owner, n, cap, max_group, comp_table, d_records,
                       status, h->stream);
    VSG_HIP(hipGetLastError());
    ts.rounds = 2 * rounds;
    // emit, the rounds (two a launch) and the cut between them, the clear, leaders, the sort and the scan
    // counted as one each, heads, the scan, vertices, table, measure, finish
    launches += rounds + 12;
    const bool to_device = !count_only && mem_out == VSG_MEM_DEVICE && contours && vertices;
    if (to_device) {
      // the lengths of both lists are on the device: the copy decides there whether they fit
      LaunchContourCopy(d_records, d_vertices, cap, n, (uint32_t)std::min<size_t>(capacity_contours, cap),
                        (uint32_t)std::min<size_t>(capacity_vertices, n), reinterpret_cast<int32_t*>(contours),
                        vertices, status, h->stream);
      VSG_HIP(hipGetLastError());
      ++launches;
    }
    h->tclock.Mark(CNT_TABLE);
    VSG_HIP(hipMemcpyAsync(&seen[1], status, sizeof(ContourStatus), hipMemcpyDeviceToHost, h->stream));
    ++launches;
    if (!count_only && mem_out == VSG_MEM_HOST) launches += 2;   // counted whether or not the lists fit
    VSG_HIP(hipStreamSynchronize(h->stream));
    {
      float us[CNT_STAGES];
      h->tclock.Read(us, CNT_STAGES);
      ts.classify_us += us[CNT_CLASSIFY];
      ts.trace_us = us[CNT_TRACE];
      ts.table_us = us[CNT_TABLE];
    }
    finish();
    if (seen[1].flags & CONTOUR_FLAG_OVERFLOW) Throw(VSG_ERR_INTERNAL, "more contours than a quarter of the cracks");
    if ((seen[1].flags & CONTOUR_FLAG_RANGE) || seen[1].contours == 0 || seen[1].contours > cap ||
        seen[1].vertices > n || (uint64_t)seen[1].vertices < 4ull * seen[1].contours) {
      Throw(VSG_ERR_INTERNAL, "a crack, a contour or a vertex is out of range");
    }
    const size_t n_contours = seen[1].contours, n_vertices = seen[1].vertices;
    *num_contours = n_contours;
    *num_vertices = n_vertices;
    ts.contours = (int64_t)n_contours;
    ts.vertices = (int64_t)n_vertices;
    ts.holes = seen[1].holes;
    ts.largest_contour_cracks = seen[1].largest;
    if (run) {
      MeshInput& in = run->in;
      in.plane = plane;
      in.width = W;
      in.height = H;
      in.mask = mask;
      in.offset = offset;
      in.n = n;
      in.key = key;
      in.succ = succ;
      in.leader = leader;
      in.place = place;
      in.ranked = ranked;
      in.contours = (uint32_t)n_contours;
      in.count = count;
      in.records = d_records;
      run->ckeys_sorted = ckeys_sorted;
      run->max_group = max_group;
      run->rounds = rounds;
    }
    if (count_only) return;
    if (n_contours > capacity_contours || n_vertices > capacity_vertices) {
      Throw(VSG_ERR_INVALID, "the level has " + std::to_string(n_contours) + " contours and " +
                                 std::to_string(n_vertices) + " vertices, the capacities are " +
                                 std::to_string(capacity_contours) + " and " + std::to_string(capacity_vertices));
    }
    if (!contours || !vertices) Throw(VSG_ERR_INVALID, "an output is null");
    if (mem_out == VSG_MEM_HOST) {
      // through the pinned block, now that the lengths are known
      const size_t cb = n_contours * sizeof(vsg_render_level_contour), vb = n_vertices * 2 * sizeof(int32_t);
      h->h_cont.Reserve(2 * sizeof(ContourStatus) + cb + vb, &h->allocations);
      h->stats.device_allocations = h->allocations;
      char* stage = reinterpret_cast<char*>(h->h_cont.As<ContourStatus>() + 2);
      VSG_HIP(hipMemcpyAsync(stage, d_records, cb, hipMemcpyDeviceToHost, h->stream));
      VSG_HIP(hipMemcpyAsync(stage + cb, d_vertices, vb, hipMemcpyDeviceToHost, h->stream));
      VSG_HIP(hipStreamSynchronize(h->stream));
      std::memcpy(contours, stage, cb);
      std::memcpy(vertices, stage + cb, vb);
    }
  }
}

}  // namespace

extern "C" {

int vsg_render_level_contours(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness,
                              vsg_render_level_contour* contours, size_t capacity_contours, size_t* num_contours,
                              int32_t* vertices, size_t capacity_vertices, size_t* num_vertices, int mem_out) {
  return Guard([&] {
    LevelContours(h, seg, seg_len, level, connectedness, contours, capacity_contours, num_contours, vertices,
                  capacity_vertices, num_vertices, mem_out, nullptr);
  });
}

int vsg_render_last_contour_stats(vsg_render* h, vsg_render_contour_stats* s) {
  return Guard([&] {
    if (!h || !s) Throw(VSG_ERR_INVALID, "null argument");
    *s = h->tstats;
  });
}

int vsg_render_level_mesh(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness,
                          vsg_render_mesh_segment* segments, size_t capacity_segments, size_t* num_segments,
                          int32_t* vertices, size_t capacity_vertices, size_t* num_vertices,
                          vsg_render_mesh_loop* loops, size_t capacity_loops, size_t* num_loops, int32_t* refs,
                          size_t capacity_refs, size_t* num_refs, int mem_out) {
  return Guard([&] {
    using namespace vsg_render_impl;
    static_assert(sizeof(vsg_render_mesh_segment) == kMeshSegmentWords * sizeof(int32_t), "moved as int32 words");
    static_assert(sizeof(vsg_render_mesh_loop) == kMeshLoopWords * sizeof(int32_t), "moved as int32 words");
    static_assert(sizeof(vsg_render_mesh_stats) == 104, "documented size");
    if (connectedness != 0 && connectedness != VSG_RENDER_CONNECT_N4 && connectedness != VSG_RENDER_CONNECT_N8) {
      Throw(VSG_ERR_INVALID, "connectedness is neither 0, VSG_RENDER_CONNECT_N4 nor VSG_RENDER_CONNECT_N8");
    }
    if (!h) Throw(VSG_ERR_INVALID, "handle is null");
    if (!num_segments || !num_vertices || !num_loops || !num_refs) Throw(VSG_ERR_INVALID, "a count pointer is null");
    CheckMem(mem_out, "mem_out");
    *num_segments = *num_vertices = *num_loops = *num_refs = 0;
    const bool count_only = !segments && !vertices && !loops && !refs && capacity_segments == 0 &&
                            capacity_vertices == 0 && capacity_loops == 0 && capacity_refs == 0;
    vsg_render_mesh_stats& ms = h->mstats;
    std::memset(&ms, 0, sizeof(ms));

    // ---- the contour stages, as a count-only call ----
    ContourRun run;
    size_t n_contours = 0, n_contour_vertices = 0;
    struct ContourPart {
      vsg_render* h;
      ~ContourPart() {
        const vsg_render_contour_stats& ts = h->tstats;
        vsg_render_mesh_stats& ms = h->mstats;
        ms.cracks = ts.cracks;
        ms.plane_us = ts.plane_us;
        ms.classify_us = ts.classify_us;
        ms.trace_us = ts.trace_us + ts.table_us;
        ms.rounds = ts.rounds;
        ms.launches = ts.launches;
      }
    };
    {
      ContourPart part{h};
      LevelContours(h, seg, seg_len, level, connectedness, nullptr, 0, &n_contours, nullptr, 0, &n_contour_vertices,
                    VSG_MEM_HOST, &run);
    }
    const uint32_t n = run.in.n;
    if (n == 0) return;   // no covered pixel: all four lists are empty
    DeviceGuard guard(h->device);
    const uint32_t C = run.in.contours;
    int group_bits = 1;
    while (group_bits < 32 && (run.max_group >> group_bits)) ++group_bits;
    const int end_bit = 32 + group_bits;

    // ---- split: junctions, the third doubling, halves, owners ----
    // sized for every crack and for what is scanned here: the library's need is not promised to grow with the
    // number of items
    size_t temp_bytes = std::max<size_t>(std::max(MeshTempBytes(n, end_bit), MeshTempBytes(C, end_bit)), 16);
    h->d_sort_temp.Reserve(temp_bytes, &h->allocations);
    h->d_mesh_status.Reserve(sizeof(MeshStatus), &h->allocations);
    h->h_mesh.Reserve(2 * sizeof(MeshStatus), &h->allocations);
    h->d_mesh_cracks.Reserve((size_t)n * 40 + (size_t)C * 12 + n, &h->allocations);
    MeshStatus* status = h->d_mesh_status.As<MeshStatus>();
    MeshStatus* seen = h->h_mesh.As<MeshStatus>();   // [0] after the split, [1] at the end
    std::memset(seen, 0, 2 * sizeof(MeshStatus));
    MeshCrackSpace w;
    w.state_a = h->d_mesh_cracks.As<uint2>();
    w.state_b = w.state_a + n;
    w.skeys = reinterpret_cast<unsigned long long*>(w.state_b + n);
    w.half = reinterpret_cast<uint32_t*>(w.skeys + n);
    w.head_of = w.half + n;            // and last_of behind it
    w.seg_of = w.head_of + 2 * (size_t)n;
    w.hasj = w.seg_of + n;
    w.nrefs = w.hasj + C;
    w.first_ref = w.nrefs + C;
    w.sides = reinterpret_cast<uint8_t*>(w.first_ref + C);
    w.heads = nullptr;
    int launches = 0;
    auto finish = [&] {
      ms.launches += launches;
      h->stats.launches += launches;
      h->stats.device_allocations = h->allocations;
    };
    VSG_HIP(hipMemsetAsync(status, 0, sizeof(MeshStatus), h->stream));
    h->mclock.Begin(h->stream);
    VSG_HIP(MeshSplit(h->d_sort_temp.p, temp_bytes, run.in, run.ckeys_sorted, run.rounds, &w, status, h->stream));
    h->mclock.Mark(MSH_SPLIT);
    VSG_HIP(hipMemcpyAsync(&seen[0], status, sizeof(MeshStatus), hipMemcpyDeviceToHost, h->stream));
    // the clear, MeshSplit's 7 and a launch for two rounds, the status
    launches += 9 + run.rounds / 2;
    VSG_HIP(hipStreamSynchronize(h->stream));
    ms.rounds += run.rounds;
    ms.junctions = seen[0].junctions;
    const uint32_t S = seen[0].segments, R = seen[0].refs;
    if ((seen[0].flags & MESH_FLAG_RANGE) || S == 0 || S > n || R < C || R > n || S > R) {
      finish();
      Throw(VSG_ERR_INTERNAL, "a crack, a contour or a half is out of range");
    }

    // ---- tables: the segments' order, vertices, records, loops, refs, lengths ----
    if ((uint64_t)n + S > 0xffffffffull) {
      finish();
      Throw(VSG_ERR_INVALID, "the level has more than 2^32 - 1 cracks and segments");
    }
    const uint32_t slots = n + S;      // a vertex per crack of an owner half and an end corner per segment
    temp_bytes = std::max(temp_bytes, MeshTempBytes(S, end_bit));
    h->d_sort_temp.Reserve(temp_bytes, &h->allocations);
    const size_t seg_words = (size_t)S * kMeshSegmentWords, loop_words = (size_t)C * kMeshLoopWords;
    h->d_mesh_lists.Reserve((size_t)S * 16 + (seg_words + (size_t)slots * 3 + loop_words + R) * 4, &h->allocations);
    MeshSegmentSpace t;
    t.skeys_sorted = h->d_mesh_lists.As<unsigned long long>();
    t.scount = reinterpret_cast<uint32_t*>(t.skeys_sorted + S);
    t.sfirst = t.scount + S;
    t.segments = reinterpret_cast<int32_t*>(t.sfirst + S);
    t.vertex_slots = slots;
    t.vertices = t.segments + seg_words;
    t.vseg = reinterpret_cast<uint32_t*>(t.vertices + (size_t)slots * 2);
    t.loops = reinterpret_cast<int32_t*>(t.vseg + slots);
    t.refs = t.loops + loop_words;
    VSG_HIP(MeshTables(h->d_sort_temp.p, temp_bytes, run.in, w, t, S, R, end_bit, status, h->stream));
    launches += 11;
    const bool fits = S <= capacity_segments && C <= capacity_loops && R <= capacity_refs;
    const bool to_device = !count_only && mem_out == VSG_MEM_DEVICE && segments && vertices && loops && refs;
    if (to_device) {
      // the number of vertices is on the device: the copy decides there whether they fit.  Counted whether or
      // not the other three lists fit
      if (fits) {
        LaunchMeshCopy(t, S, C, R, (uint32_t)std::min<size_t>(capacity_vertices, slots),
                       reinterpret_cast<int32_t*>(segments), vertices, reinterpret_cast<int32_t*>(loops), refs, status,
                       h->stream);
        VSG_HIP(hipGetLastError());
      }
      ++launches;
    }
    h->mclock.Mark(MSH_TABLE);
    VSG_HIP(hipMemcpyAsync(&seen[1], status, sizeof(MeshStatus), hipMemcpyDeviceToHost, h->stream));
    ++launches;
    if (!count_only && mem_out == VSG_MEM_HOST) launches += 4;   // counted whether or not the lists fit
    VSG_HIP(hipStreamSynchronize(h->stream));
    {
      float us[MSH_STAGES];
      h->mclock.Read(us, MSH_STAGES);
      ms.split_us = us[MSH_SPLIT];
      ms.table_us = us[MSH_TABLE];
    }
    finish();
    const size_t V = seen[1].vertices;
    if ((seen[1].flags & MESH_FLAG_RANGE) || V > slots || V < 2ull * S) {
      Throw(VSG_ERR_INTERNAL, "a segment, a vertex or a ref is out of range");
    }
    *num_segments = S;
    *num_vertices = V;
    *num_loops = C;
    *num_refs = R;
    ms.segments = S;
    ms.closed_segments = seen[1].closed;
    ms.shared_segments = seen[1].shared;
    ms.vertices = (int64_t)V;
    ms.loops = C;
    ms.refs = R;
    ms.longest_segment_cracks = seen[1].longest;
    if (count_only) return;
    if (!fits || V > capacity_vertices) {
      Throw(VSG_ERR_INVALID, "the level has " + std::to_string(S) + " segments, " + std::to_string(V) + " vertices, " +
                                 std::to_string(C) + " loops and " + std::to_string(R) + " refs, the capacities are " +
                                 std::to_string(capacity_segments) + ", " + std::to_string(capacity_vertices) + ", " +
                                 std::to_string(capacity_loops) + " and " + std::to_string(capacity_refs));
    }
    if (!segments || !vertices || !loops || !refs) Throw(VSG_ERR_INVALID, "an output is null");
    if (mem_out == VSG_MEM_HOST) {
      // through the pinned block, now that the lengths are known
      const size_t sb = seg_words * 4, vb = V * 8, lb = loop_words * 4, rb = (size_t)R * 4;
      h->h_mesh.Reserve(2 * sizeof(MeshStatus) + sb + vb + lb + rb, &h->allocations);
      h->stats.device_allocations = h->allocations;
      char* stage = reinterpret_cast<char*>(h->h_mesh.As<MeshStatus>() + 2);
      VSG_HIP(hipMemcpyAsync(stage, t.segments, sb, hipMemcpyDeviceToHost, h->stream));
      VSG_HIP(hipMemcpyAsync(stage + sb, t.vertices, vb, hipMemcpyDeviceToHost, h->stream));
      VSG_HIP(hipMemcpyAsync(stage + sb + vb, t.loops, lb, hipMemcpyDeviceToHost, h->stream));
      VSG_HIP(hipMemcpyAsync(stage + sb + vb + lb, t.refs, rb, hipMemcpyDeviceToHost, h->stream));
      VSG_HIP(hipStreamSynchronize(h->stream));
      std::memcpy(segments, stage, sb);
      std::memcpy(vertices, stage + sb, vb);
      std::memcpy(loops, stage + sb + vb, lb);
      std::memcpy(refs, stage + sb + vb + lb, rb);
    }
  });
}

int vsg_render_last_mesh_stats(vsg_render* h, vsg_render_mesh_stats* s) {
  return Guard([&] {
    if (!h || !s) Throw(VSG_ERR_INVALID, "null argument");
    *s = h->mstats;
  });
}

int vsg_render_boundary_distance(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int32_t* out,
                                 int mem_out) {
  return Guard([&] {
    using namespace vsg_render_impl;
    static_assert(VSG_RENDER_DISTANCE_NONE == kDistanceNone, "the kernels' none is the header's");
    if (!h) Throw(VSG_ERR_INVALID, "handle is null");
    if (!out) Throw(VSG_ERR_INVALID, "out is null");
    CheckMem(mem_out, "out");
    const int W = h->W, H = h->H;
    const size_t n = (size_t)W * H, bytes = n * sizeof(int32_t);
    DeviceGuard guard(h->device);
    vsg_render_distance_stats& ds = h->dstats;
    std::memset(&ds, 0, sizeof(ds));

    // ---- P, as vsg_render_id_image paints it, and its edge set ----
    h->d_ids.Reserve(bytes, &h->allocations);
    const bool vector = PaintIds(h, seg, seg_len, level, h->d_ids.As<uint32_t>(),
                                 [](int mapped) { return (uint32_t)mapped; });
    h->d_dist_words.Reserve((size_t)DistChunks(H) * W * sizeof(uint32_t), &h->allocations);
    h->d_dist_status.Reserve(sizeof(DistStatus), &h->allocations);
    h->h_dist.Reserve(2 * sizeof(DistStatus), &h->allocations);
    uint32_t* words = h->d_dist_words.As<uint32_t>();
    DistStatus* status = h->d_dist_status.As<DistStatus>();
    DistStatus* seen = h->h_dist.As<DistStatus>();   // [0] after the classify pass, [1] at the end
    std::memset(seen, 0, 2 * sizeof(DistStatus));
    VSG_HIP(hipMemsetAsync(status, 0, sizeof(DistStatus), h->stream));
    h->dclock.Begin(h->stream);
    LaunchDistClassify(h->d_ids.As<int32_t>(), (size_t)W, W, H, false, words, status, h->stream);
    VSG_HIP(hipGetLastError());
    h->dclock.Mark(DST_CLASSIFY);
    VSG_HIP(hipMemcpyAsync(&seen[0], status, sizeof(DistStatus), hipMemcpyDeviceToHost, h->stream));
    int launches = 3;
    h->FinishStats();   // the number of edge pixels decides what runs below
    if (vector) h->CheckVector();
    float us[DST_STAGES];
    h->dclock.Read(us, DST_STAGES);
    ds.plane_us = h->stats.clear_us + h->stats.fill_us;
    ds.classify_us = us[DST_CLASSIFY];
    ds.edge_pixels = (int64_t)seen[0].edge_pixels;

    if (ds.edge_pixels == 0) {
      // ---- no edge: none everywhere ----
      if (mem_out == VSG_MEM_HOST) {
        std::fill(out, out + n, (int32_t)VSG_RENDER_DISTANCE_NONE);
      } else {
        VSG_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(out), VSG_RENDER_DISTANCE_NONE, n, h->stream));
        VSG_HIP(hipStreamSynchronize(h->stream));
        ++launches;
      }
    } else {
      // ---- columns, then rows ----
      h->d_dist_gsq.Reserve(bytes, &h->allocations);
      int32_t* d = out;   // device output: written in place
      if (mem_out == VSG_MEM_HOST) {
        h->d_dist_out.Reserve(bytes, &h->allocations);
        d = h->d_dist_out.As<int32_t>();
      }
      h->dclock.Begin(h->stream);
      LaunchDistColumns(words, W, H, h->d_dist_gsq.As<int32_t>(), h->stream);
      VSG_HIP(hipGetLastError());
      h->dclock.Mark(DST_COLUMNS);
      VSG_HIP(LaunchDistRows(h->d_dist_gsq.As<int32_t>(), W, H, d, status, h->stream));
      h->dclock.Mark(DST_ROWS);
      launches += 3;
      if (mem_out == VSG_MEM_HOST) {
        VSG_HIP(hipMemcpyAsync(out, d, bytes, hipMemcpyDeviceToHost, h->stream));
        ++launches;
      }
      VSG_HIP(hipMemcpyAsync(&seen[1], status, sizeof(DistStatus), hipMemcpyDeviceToHost, h->stream));
      VSG_HIP(hipStreamSynchronize(h->stream));
      h->dclock.Read(us, DST_STAGES);
      ds.columns_us = us[DST_COLUMNS];
      ds.rows_us = us[DST_ROWS];
      ds.max_distance = (int64_t)seen[1].max_distance;
    }
    h->stats.launches += launches;
    h->stats.device_allocations = h->allocations;
    ds.launches = h->stats.launches;
  });
}

int vsg_render_boundary_benchmark(vsg_render* h, const uint8_t* seg, size_t seg_len, const int32_t* other,
                                  size_t other_pitch, int mem_other, int tolerance_sq,
                                  vsg_render_boundary_score* scores, size_t capacity_levels, size_t* num_levels,
                                  int mem_out) {
  return Guard([&] {
    using namespace vsg_render_impl;
    static_assert(sizeof(vsg_render_boundary_score) == kBoundaryScoreWords * sizeof(int64_t), "moved as int64 words");
    if (!h) Throw(VSG_ERR_INVALID, "handle is null");
    if (!num_levels) Throw(VSG_ERR_INVALID, "the count pointer is null");
    if (!other) Throw(VSG_ERR_INVALID, "other is null");
    if (mem_other != VSG_MEM_HOST && mem_other != VSG_MEM_DEVICE) {
      Throw(VSG_ERR_INVALID, "mem_other is neither VSG_MEM_HOST nor VSG_MEM_DEVICE");
    }
    CheckMem(mem_out, "scores");
    if (tolerance_sq < 0 || tolerance_sq > VSG_RENDER_MAX_TOLERANCE_SQ) {
      Throw(VSG_ERR_INVALID, "tolerance_sq " + std::to_string(tolerance_sq) + " is outside [0, " +
                                 std::to_string(VSG_RENDER_MAX_TOLERANCE_SQ) + "]");
    }
    if (!scores && capacity_levels != 0) Throw(VSG_ERR_INVALID, "scores is null");
    const int W = h->W, H = h->H;
    if (other_pitch != 0 && other_pitch < (size_t)W) {
      Throw(VSG_ERR_INVALID, "the pitch of other, " + std::to_string(other_pitch) + ", is below the width " +
                                 std::to_string(W));
    }
    const size_t pitch = other_pitch ? other_pitch : (size_t)W;
    const size_t n = (size_t)W * H, bytes = n * sizeof(int32_t);
    DeviceGuard guard(h->device);
    vsg_render_distance_stats& ds = h->dstats;
    std::memset(&ds, 0, sizeof(ds));
    std::memset(&h->pstats, 0, sizeof(h->pstats));

    // ---- Q, as vsg_render_persistence_image makes it ----
    h->d_pq.Reserve(bytes, &h->allocations);
    const int32_t* q = h->d_pq.As<int32_t>();
    int launches = 0, levels = 0;
    const bool vector = PaintPersistence(h, seg, seg_len, h->d_pq.As<int32_t>(), (size_t)W, &levels, &launches);
    const size_t L = (size_t)levels, bins = L + 1;

    // ---- B: where it is, or through the pinned block to the device, rows packed; G ----
    h->d_dist_words.Reserve((size_t)DistChunks(H) * W * sizeof(uint32_t), &h->allocations);
    h->d_dist_status.Reserve(sizeof(DistStatus), &h->allocations);
    h->h_dist.Reserve(2 * sizeof(DistStatus), &h->allocations);
    h->d_dist_hist.Reserve(3 * bins * sizeof(uint32_t), &h->allocations);
    uint32_t* words = h->d_dist_words.As<uint32_t>();
    uint32_t* hist = h->d_dist_hist.As<uint32_t>();   // all, near, disc
    DistStatus* status = h->d_dist_status.As<DistStatus>();
    DistStatus* seen = h->h_dist.As<DistStatus>();   // [0] after the classify pass, [1] at the end
    std::memset(seen, 0, 2 * sizeof(DistStatus));
    const int32_t* label_plane = other;
    size_t label_pitch = pitch;
    h->dclock.Begin(h->stream);
    if (mem_other == VSG_MEM_HOST) {
      h->h_other.Reserve(bytes, &h->allocations);
      h->d_other.Reserve(bytes, &h->allocations);
      for (int y = 0; y < H; ++y) {
        std::memcpy(h->h_other.As<int32_t>() + (size_t)y * W, other + (size_t)y * pitch, (size_t)W * sizeof(int32_t));
      }
      VSG_HIP(hipMemcpyAsync(h->d_other.p, h->h_other.p, bytes, hipMemcpyHostToDevice, h->stream));
      label_plane = h->d_other.As<int32_t>();
      label_pitch = (size_t)W;
      ++launches;
    }
    h->dclock.Mark(DST_PLANE);
    VSG_HIP(hipMemsetAsync(status, 0, sizeof(DistStatus), h->stream));
    VSG_HIP(hipMemsetAsync(hist, 0, 3 * bins * sizeof(uint32_t), h->stream));
    LaunchDistClassify(label_plane, label_pitch, W, H, true, words, status, h->stream);
    VSG_HIP(hipGetLastError());
    h->dclock.Mark(DST_CLASSIFY);
    VSG_HIP(hipMemcpyAsync(&seen[0], status, sizeof(DistStatus), hipMemcpyDeviceToHost, h->stream));
    launches += 4;
    FinishPersistence(h, vector, launches);   // the size of G decides what runs below
    float us[DST_STAGES];
    h->dclock.Read(us, DST_STAGES);
    ds.plane_us = h->pstats.plane_us + h->pstats.persist_us + us[DST_PLANE];
    ds.classify_us = us[DST_CLASSIFY];
    ds.levels = (int64_t)L;
    ds.edge_pixels = h->pstats.edge_pixels;
    ds.other_edge_pixels = (int64_t)seen[0].edge_pixels;
    ds.launches = h->stats.launches;
    h->stats.device_allocations = h->allocations;
    *num_levels = L;
    if (!scores && capacity_levels == 0) return;   // the count only
    if (capacity_levels < L) {
      Throw(VSG_ERR_INVALID, "the hierarchy has " + std::to_string(L) + " levels, scores has room for " +
                                 std::to_string(capacity_levels));
    }

    // ---- D_G where G has a pixel; the histograms; the records ----
    const bool any = seen[0].edge_pixels != 0;
    const int32_t* dist = nullptr;
    long long* records = reinterpret_cast<long long*>(scores);   // device output: written in place
    if (mem_out == VSG_MEM_HOST) {
      h->d_dist_scores.Reserve(L * sizeof(vsg_render_boundary_score), &h->allocations);
      records = h->d_dist_scores.As<long long>();
    }
    launches = 0;
    h->dclock.Begin(h->stream);
    if (any) {
      h->d_dist_gsq.Reserve(bytes, &h->allocations);
      h->d_dist_out.Reserve(bytes, &h->allocations);
      LaunchDistColumns(words, W, H, h->d_dist_gsq.As<int32_t>(), h->stream);
      VSG_HIP(hipGetLastError());
      h->dclock.Mark(DST_COLUMNS);
      VSG_HIP(LaunchDistRows(h->d_dist_gsq.As<int32_t>(), W, H, h->d_dist_out.As<int32_t>(), status, h->stream));
      h->dclock.Mark(DST_ROWS);
      dist = h->d_dist_out.As<int32_t>();
      launches += 2;
    }
    LaunchDistMatch(q, dist, W, H, levels, tolerance_sq, hist, hist + bins, status, h->stream);
    if (any) LaunchDistDisc(q, words, W, H, levels, tolerance_sq, hist + 2 * bins, status, h->stream);
    LaunchDistScores(hist, hist + bins, hist + 2 * bins, levels, status, records, h->stream);
    VSG_HIP(hipGetLastError());
    h->dclock.Mark(DST_MATCH);
    launches += any ? 3 : 2;
    if (mem_out == VSG_MEM_HOST) {
      VSG_HIP(hipMemcpyAsync(scores, records, L * sizeof(vsg_render_boundary_score), hipMemcpyDeviceToHost,
                             h->stream));
      ++launches;
    }
    VSG_HIP(hipMemcpyAsync(&seen[1], status, sizeof(DistStatus), hipMemcpyDeviceToHost, h->stream));
    ++launches;
    VSG_HIP(hipStreamSynchronize(h->stream));
    h->dclock.Read(us, DST_STAGES);
    ds.columns_us = us[DST_COLUMNS];
    ds.rows_us = us[DST_ROWS];
    ds.match_us = us[DST_MATCH];
    h->stats.launches += launches;
    h->stats.device_allocations = h->allocations;
    ds.launches = h->stats.launches;
    if (seen[1].flags) Throw(VSG_ERR_INTERNAL, "the persistence plane holds a value outside [0, L]");
  });
}

int vsg_render_last_distance_stats(vsg_render* h, vsg_render_distance_stats* s) {
  return Guard([&] {
    if (!h || !s) Throw(VSG_ERR_INVALID, "null argument");
    *s = h->dstats;
  });
}

int vsg_render_rasterize(vsg_render* h, const uint8_t* seg, size_t seg_len, int32_t* out, size_t capacity_intervals,
                         size_t* count, int mem_out) {
  return Guard([&] {
    if (!h) Throw(VSG_ERR_INVALID, "handle is null");
    if (!count) Throw(VSG_ERR_INVALID, "count is null");
    *count = 0;
    CheckMem(mem_out, "out");
    if (!seg && seg_len) Throw(VSG_ERR_INVALID, "seg is null");
    DeviceGuard guard(h->device);
    std::memset(&h->stats, 0, sizeof(h->stats));
    std::memset(&h->vstats, 0, sizeof(h->vstats));
    const double t0 = NowMs();
    // the handle's kept hierarchy is left alone: this call renders nothing
    ParseDesc(seg, seg_len, h->W, h->H, true, &h->desc, &h->intervals);
    if (!h->desc.has_mesh) Throw(VSG_ERR_INVALID, "the SegmentationDesc has no vector_mesh");
    h->region_value.assign(h->desc.region_ids.begin(), h->desc.region_ids.end());
    const int64_t n_cross = h->BuildLines();
    const size_t n = (size_t)(n_cross / 2);
    h->stats.intervals = (int64_t)n;
    h->stats.distinct_ids = (int64_t)h->desc.region_ids.size();
    *count = n;
    if (!out && capacity_intervals == 0) return;   // asked for the count only
    if (n > capacity_intervals) {
      Throw(VSG_ERR_INVALID, "capacity_intervals is " + std::to_string(capacity_intervals) + ", the frame has " +
                                 std::to_string(n) + " intervals");
    }
    if (n && !out) Throw(VSG_ERR_INVALID, "out is null");
    const double t1 = NowMs();
    h->stats.decode_ms = t1 - t0;
    h->RunVector(n_cross);
    h->stats.upload_ms = NowMs() - t1;
    if (n) {
      VSG_HIP(hipMemcpyAsync(out, h->d_intervals.p, n * sizeof(Interval),
                             mem_out == VSG_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, h->stream));
      ++h->stats.launches;
    }
    VSG_HIP(hipStreamSynchronize(h->stream));
    h->stats.device_allocations = h->allocations;
    h->CheckVector();
  });
}

int vsg_render_last_vector_stats(vsg_render* h, vsg_render_vector_stats* s) {
  return Guard([&] {
    if (!h || !s) Throw(VSG_ERR_INVALID, "null argument");
    *s = h->vstats;
  });
}

int vsg_render_level(vsg_render* h, int* level) {
  return Guard([&] {
    if (!h || !level) Throw(VSG_ERR_INVALID, "null argument");
    if (!h->level_resolved) Throw(VSG_ERR_STATE, "no frame has been rendered yet");
    *level = h->level;
  });
}

int vsg_render_last_stats(vsg_render* h, vsg_render_stats* s) {
  return Guard([&] {
    if (!h || !s) Throw(VSG_ERR_INVALID, "null argument");
    *s = h->stats;
  });
}

}  // extern "C"
