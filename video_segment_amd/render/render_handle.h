// render_handle.h -- struct vsg_render: the state of a renderer handle, one small struct per entry family, the
// stage enums of the families' clocks, and the helpers the families share: argument checks, the status pair,
// the upload of a host label plane, the delivery of host outputs.  A part of render_capi.cpp's translation
// unit: include it after ../common/capi_support.h and render_desc.h.
#pragma once

namespace {

using vsg_render_impl::AdjStatus;
using vsg_render_impl::BoundStatus;
using vsg_render_impl::ColorStatus;
using vsg_render_impl::CompStatus;
using vsg_render_impl::ContourStatus;
using vsg_render_impl::CutStatus;
using vsg_render_impl::DistStatus;
using vsg_render_impl::Interval;
using vsg_render_impl::LevelStatus;
using vsg_render_impl::MeshStatus;
using vsg_render_impl::OvlStatus;
using vsg_render_impl::PersStatus;
using vsg_render_impl::PoolStatus;
using vsg_render_impl::SimplifyStatus;
using vsg_render_impl::VecLine;
using vsg_render_impl::VecStatus;
using vsg_render_impl::VolumeStatus;

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
enum PoolStage { POOL_UPLOAD = 0, POOL_SUMS, POOL_TABLE, POOL_PAINT, POOL_STAGES };
enum ContourStage { CNT_CLASSIFY = 0, CNT_TRACE, CNT_TABLE, CNT_STAGES };
enum MeshStage { MSH_SPLIT = 0, MSH_TABLE, MSH_STAGES };
enum SimplifyStage { SMP_DP = 0, SMP_CLEAN, SMP_TABLE, SMP_STAGES };
// DST_PLANE: the upload of a host label plane
enum DistStage { DST_PLANE = 0, DST_CLASSIFY, DST_COLUMNS, DST_ROWS, DST_MATCH, DST_STAGES };
enum VolumeStage { VOL_GEOMETRY = 0, VOL_MERGE, VOL_SORT, VOL_TABLE, VOL_STAGES };
// CUT_WAIT: the stream idles while the host reads the number of nodes, then of records; reported with no stage
enum CutStage { CUT_LIFT = 0, CUT_DP, CUT_PAINT, CUT_WAIT, CUT_STAGES };

double NowMs() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch())
      .count();
}

// ---- the families' state ------------------------------------------------------------------------
// Every family has the clock of its stages, its blocks (`status`: the status words on the device; `seen`: the
// pinned block they, and host outputs, come back through) and the stats of its last call.  Init(), once the
// handle has its stream: the pinned block marked, an event for Begin and one per stage, the stats zeroed.
template <class Family>
void InitFamily(Family* f, int stages) {
  f->seen.pinned = true;
  f->clock.Create((size_t)stages + 1);
  std::memset(&f->stats, 0, sizeof(f->stats));
}

// the vector path: lines and per-region values (host, then one upload), crossings (two key and two value arrays
// for the sort), the status words
struct VectorState {
  StageClock clock;
  std::vector<VecLine> lines;
  std::vector<uint32_t> region_value;
  std::vector<float> scaled_mesh;
  Block in, cross, status, seen;
  vsg_render_vector_stats stats;
  void Init() { InitFamily(this, VEC_COUNT); }
};

// level regions: unsorted runs (keys, right ends), sorted runs with their ranks, the two lists, the status
// words, and the pinned block the status and host outputs come back through
struct LevelState {
  StageClock clock;
  Block runs, sorted, regions, intervals, status, seen;
  vsg_render_level_stats stats;
  void Init() { InitFamily(this, LVL_COUNT); }
};

// level components: the union-find's parents, labels and indices with their sorted copies and the components'
// ranks; the component table; the ordered intervals; the same with component indices for the label fill; every
// region's first component; the label plane of a host output; the status words and the pinned block they come
// back through
struct ComponentState {
  StageClock clock;
  Block work, table, intervals, fill, first, labels, status, seen;
  vsg_render_component_stats stats;
  void Init() { InitFamily(this, CMP_COUNT); }
};

// level boundaries: unsorted and sorted keys; their groups' ranks; the points; the records; the status words
// and the pinned block the status and host outputs come back through
struct BoundaryState {
  StageClock clock;
  Block keys, rank, points, records, status, seen;
  vsg_render_boundary_stats stats;
  void Init() { InitFamily(this, BND_STAGES); }
};

// level adjacency: unsorted and sorted keys; their node and edge heads' counts; the nodes; the edges; the
// status words and the pinned block the status and host outputs come back through
struct AdjacencyState {
  StageClock clock;
  Block keys, heads, nodes, edges, status, seen;
  vsg_render_adjacency_stats stats;
  void Init() { InitFamily(this, ADJ_STAGES); }
};

// level overlap: the count pass's words of every frame row; unsorted and sorted runs (keys, lengths), the
// unsorted halves taken again for the column sort's operands; the two scans, taken again for the sorted column
// operands and their ranks; the distinct keys (key, rank, start) and the columns' first keys; rows, columns,
// pairs; the status words and the pinned block the status and host outputs come back through
struct OverlapState {
  StageClock clock;
  Block totals, runs, heads, keys, rows, cols, pairs, status, seen;
  vsg_render_overlap_stats stats;
  void Init() { InitFamily(this, OVL_STAGES); }
};

// boundary persistence: the region ids the ancestor table's columns stand for and the table (host, then one
// upload through the pinned block into anc: ids, then rows); the persistence plane of a picture or of a host
// output; the edges' persistences, the histogram and the levels' sides; the status words
struct PersistenceState {
  StageClock clock;
  std::vector<int32_t> ids, table;
  Block anc, q, out, status, seen;
  vsg_render_persistence_stats stats;
  void Init() { InitFamily(this, PRS_STAGES); }
};

// level colours: the intervals' partials; what the records gather; the records of a host output or of a
// picture; the interval list with the means as values; the status words and the pinned block the status, the
// number of records and a host table come back through
struct ColorState {
  StageClock clock;
  Block partials, acc, records, intervals, status, seen;
  vsg_render_color_stats stats;
  void Init() { InitFamily(this, CLR_STAGES); }
};

// level pooling: a host feature map or a host output's span on the device; host values on the device; the parts
// of the records that span slices; area and interval count of every record; groups and matrices of a host
// output; the interval list with the records as values; the status words and the pinned block the status, the
// number of records and host outputs come back through
struct PoolState {
  StageClock clock;
  Block features, values, spill, acc, out, intervals, status, seen;
  vsg_render_pool_stats stats;
  void Init() { InitFamily(this, POOL_STAGES); }
};

// level contours: the pixels' crack masks and offsets; what there is per crack (the two doubling states, key,
// successor, leader, place, the vertices' owners; the vertices take the doubling state that is free at the
// end); what there is per contour slot (unsorted and sorted keys, group ranks, vertex counts and offsets); the
// records; the status words and the pinned block the status and host outputs come back through
struct ContourState {
  StageClock clock;
  Block mask, offset, cracks, slots, records, status, seen;
  vsg_render_contour_stats stats;
  void Init() { InitFamily(this, CNT_STAGES); }
};

// boundary distance: the edge set's words; the columns' squared distances; D of a host output or of the other
// plane's edge set; the three histograms; the records of a host output; the status words and the pinned block
// they come back through
struct DistanceState {
  StageClock clock;
  Block words, gsq, out, hist, scores, status, seen;
  vsg_render_distance_stats stats;
  void Init() { InitFamily(this, DST_STAGES); }
};

// level mesh: what there is per crack and per contour (the third doubling's two states, the unsorted owner
// keys, half, head and last crack of a half, a half's segment, the contours' junction marks, ref counts and
// offsets, the cracks' sides); what there is per segment, vertex, loop and ref (sorted keys, vertex counts and
// offsets, the four lists, the vertices' segments); the status words and the pinned block the status and host
// outputs come back through
struct MeshState {
  StageClock clock;
  Block cracks, lists, status, seen;
  vsg_render_mesh_stats stats;
  void Init() { InitFamily(this, MSH_STAGES); }
};

// mesh simplification: what there is per slot (the kept vertices and their segments, the state of the long
// segments' rounds) and per segment (kept and new counts, new offsets, rounds, the collapse marks, the list of
// long segments); the new records and vertices; the status words and the pinned block the status and host
// outputs come back through
struct SimplifyState {
  StageClock clock;
  Block work, lists, status, seen;
  vsg_render_simplify_stats stats;
  void Init() { InitFamily(this, SMP_STAGES); }
};

// volume session: what begin fixed; the three accumulated tables, each sorted keys and records in twin blocks
// (`at` says which twin holds the table; the other receives a re-sort); the number of entries and the largest
// key of each; the permutation of a re-sort (in, out); what the regions of a frame gather; the copies a table
// call fills in; the status words and the pinned block they and host outputs come back through.  The blocks
// are the family's own: no other call touches them.
struct VolumeState {
  StageClock clock;
  bool active = false, with_colors = false, with_labels = false;
  int level = 0;
  uint32_t n_rows = 0, n_cols = 0, n_pairs = 0;
  uint32_t max_id = 0, max_label = 0;
  int rows_at = 0, cols_at = 0, pairs_at = 0;
  Block row_keys[2], rows[2], col_keys[2], cols[2], pair_keys[2], pairs[2];
  Block perm, geo, out_rows, out_cols, out_pairs, status, seen;
  vsg_render_volume_stats stats;
  void Init() { InitFamily(this, VOL_STAGES); }
};

// tree cut: the threshold between the two DP paths; what there is per leaf (id, area, ancestor column, selected
// node); per (level, leaf) (unsorted and sorted keys and values, ranks, the map to nodes); per node (the table's
// fields, the best labels' words, marks and places); per (level, pair) (unsorted and sorted keys and counts,
// ranks, sums); the first node of every level and the pinned block it comes back through; a host gain table on
// the device; the records; the plane of a host output; the status words and the pinned block they and host
// outputs come back through
struct CutState {
  StageClock clock;
  int64_t block_nodes = 32768;
  Block leaves, lift, nodes, pairs, levels, levels_seen, gains, records, plane, status, seen;
  vsg_render_cut_stats stats;
  void Init() {
    levels_seen.pinned = true;
    seen.pinned = true;
    clock.Create(12);   // Begin, and the marks of the longest call
    std::memset(&stats, 0, sizeof(stats));
  }
};

// The number of bits of a sort key's field that holds values up to `value`: at least 1, at most `limit`.
int BitsFor(uint64_t value, int limit) {
  int bits = 1;
  while (bits < limit && (value >> bits)) ++bits;
  return bits;
}

// The work space that serves every library sort and scan of a call: the largest of their sizes, 16 at the least.
size_t MaxBytes(std::initializer_list<size_t> sizes) { return std::max<size_t>(std::max(sizes), 16); }

// The sort of a level's runs (64-bit key, 32-bit value) and the scan of their regions' ranks.
size_t LevelTempBytes(int64_t n, int end_bit) {
  using namespace vsg_render_impl;
  return MaxBytes({SortPairsU64U32TempBytes(n, end_bit), HeadScanTempBytes<HeadFlag>(n)});
}

}  // namespace

struct vsg_render {
  vsg_render_options opt;
  int device = 0, W = 0, H = 0, pitch = 0;
  hipStream_t stream = nullptr;
  StageClock clock;   // clear, fill, compose
  // SegmentationRenderUnit's state
  bool level_resolved = false;
  int level = 0;
  Hierarchy kept;
  // scratch of a call
  ParsedDesc desc;
  std::vector<Interval> intervals;
  std::unordered_map<int32_t, uint32_t> colors;   // mapped id -> packed colour (a pure function)
  Block d_intervals, h_intervals, d_plane, d_src, d_out, d_ids;
  // the work space of every family's sorts and scans; a host label plane (vsg_render_level_overlap's and
  // vsg_render_boundary_benchmark's B) on the device and the pinned block it goes through
  Block d_sort_temp, d_other, h_other;
  int64_t allocations = 0;
  vsg_render_stats stats;
  VectorState vec;
  LevelState lvl;
  ComponentState comp;
  BoundaryState bound;
  AdjacencyState adj;
  OverlapState ovl;
  PersistenceState pers;
  ColorState color;
  PoolState pool;
  ContourState cont;
  DistanceState dist;
  MeshState mesh;
  SimplifyState simp;
  VolumeState vol;
  CutState cut;

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
  // The polygon lines of the parsed desc, scaled to the handle's frame; returns the number of crossings.
  int64_t BuildLines() { return ::BuildLines(desc, W, H, &vec.scaled_mesh, &vec.lines); }

  // Uploads lines and region values, then walk -> sort -> pairs on the stream.  Leaves n_cross / 2
  // intervals in d_intervals.  CheckVector has to be called after the stream has drained.
  void RunVector(int64_t n_cross) {
    using namespace vsg_render_impl;
    const std::vector<VecLine>& lines = vec.lines;
    const std::vector<uint32_t>& region_value = vec.region_value;
    vsg_render_vector_stats& vstats = vec.stats;
    std::memset(&vstats, 0, sizeof(vstats));
    vstats.lines = (int64_t)lines.size();
    vstats.crossings = n_cross;
    if (n_cross == 0) return;
    const size_t n = (size_t)n_cross;
    const size_t lines_bytes = lines.size() * sizeof(VecLine);
    const size_t values_bytes = region_value.size() * sizeof(uint32_t);
    const int end_bit = kVecRowBits + BitsFor(region_value.size(), 31);
    const size_t temp_bytes = MaxBytes({SortPairsU64U64TempBytes(n_cross, end_bit)});
    h_intervals.Reserve(lines_bytes + values_bytes, &allocations);
    vec.in.Reserve(lines_bytes + values_bytes, &allocations);
    vec.cross.Reserve(4 * n * sizeof(unsigned long long), &allocations);
    d_sort_temp.Reserve(temp_bytes, &allocations);
    d_intervals.Reserve(n / 2 * sizeof(Interval), &allocations);
    vec.status.Reserve(sizeof(VecStatus), &allocations);
    vec.seen.Reserve(sizeof(VecStatus), &allocations);
    std::memcpy(h_intervals.p, lines.data(), lines_bytes);
    std::memcpy(static_cast<char*>(h_intervals.p) + lines_bytes, region_value.data(), values_bytes);
    VSG_HIP(hipMemcpyAsync(vec.in.p, h_intervals.p, lines_bytes + values_bytes, hipMemcpyHostToDevice, stream));
    const VecLine* d_lines = static_cast<const VecLine*>(vec.in.p);
    const uint32_t* d_values = reinterpret_cast<const uint32_t*>(static_cast<const char*>(vec.in.p) + lines_bytes);
    unsigned long long* keys = static_cast<unsigned long long*>(vec.cross.p);
    unsigned long long* vals = keys + n;
    unsigned long long* keys_sorted = keys + 2 * n;
    unsigned long long* vals_sorted = keys + 3 * n;
    VecStatus* status = static_cast<VecStatus*>(vec.status.p);
    VSG_HIP(hipMemsetAsync(status, 0, sizeof(VecStatus), stream));
    // every entry of the list is in the frame whatever the pairs stage leaves unwritten on bad input
    VSG_HIP(hipMemsetAsync(d_intervals.p, 0, n / 2 * sizeof(Interval), stream));
    vec.clock.Begin(stream);
    LaunchVecWalk(d_lines, (int)lines.size(), keys, vals, status, stream);
    vec.clock.Mark(VEC_WALK);
    VSG_HIP(SortPairsU64U64(d_sort_temp.p, temp_bytes, keys, keys_sorted, vals, vals_sorted, n_cross, end_bit, stream));
    vec.clock.Mark(VEC_SORT);
    LaunchVecPairs(keys_sorted, vals_sorted, d_lines, (uint32_t)lines.size(), d_values,
                   (uint32_t)region_value.size(), n_cross, W, H, static_cast<Interval*>(d_intervals.p), status, stream);
    VSG_HIP(hipGetLastError());
    vec.clock.Mark(VEC_PAIRS);
    VSG_HIP(hipMemcpyAsync(vec.seen.p, status, sizeof(VecStatus), hipMemcpyDeviceToHost, stream));
    vstats.launches = 7;   // upload, two clears, walk, the sort counted as one, pairs, status
    stats.launches += vstats.launches;
  }

  // After the call's one synchronisation: stage times, group statistics, the device flag.
  void CheckVector() {
    vsg_render_vector_stats& vstats = vec.stats;
    if (vstats.crossings == 0) return;
    float us[VEC_COUNT];
    vec.clock.Read(us, VEC_COUNT);
    vstats.walk_us = us[VEC_WALK];
    vstats.sort_us = us[VEC_SORT];
    vstats.pairs_us = us[VEC_PAIRS];
    const VecStatus* st = static_cast<const VecStatus*>(vec.seen.p);
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

// ---- argument checks ----------------------------------------------------------------------------
// zero_allowed: 0 asks for the level's regions themselves, not for their connected components.
void CheckConnectedness(int connectedness, bool zero_allowed) {
  if (connectedness == VSG_RENDER_CONNECT_N4 || connectedness == VSG_RENDER_CONNECT_N8) return;
  if (!zero_allowed) Throw(VSG_ERR_INVALID, "connectedness is neither VSG_RENDER_CONNECT_N4 nor VSG_RENDER_CONNECT_N8");
  if (connectedness != 0) {
    Throw(VSG_ERR_INVALID, "connectedness is neither 0, VSG_RENDER_CONNECT_N4 nor VSG_RENDER_CONNECT_N8");
  }
}

void CheckFrameBelow2Pow32(const vsg_render* h) {
  if ((uint64_t)h->W * (uint64_t)h->H >= (1ull << 32)) Throw(VSG_ERR_INVALID, "the frame has 2^32 pixels or more");
}

// What a family's call enqueued itself, added to its stats and to the handle's; the allocations so far.
void CountLaunches(vsg_render* h, int* family_launches, int launches) {
  *family_launches += launches;
  h->stats.launches += launches;
  h->stats.device_allocations = h->allocations;
}

// The body of every vsg_render_last_*_stats.
#define VSG_RENDER_LAST_STATS(entry, type, member)                 \
  int entry(vsg_render* h, type* s) {                              \
    return Guard([&] {                                             \
      if (!h || !s) Throw(VSG_ERR_INVALID, "null argument");       \
      *s = h->member;                                              \
    });                                                            \
  }

// ---- frames in, pictures out ------------------------------------------------------------------------
struct SourceFrame {
  const uint8_t* p;
  size_t stride;
};

// A BGR frame where the kernels read it: the caller's device memory, or the handle's block with the default stride.
SourceFrame UploadSource(vsg_render* h, const uint8_t* bgr, size_t stride, int mem_in, int* launches) {
  if (mem_in == VSG_MEM_DEVICE) return {bgr, stride};
  const size_t packed = vsg_render_default_stride(h->W);
  h->d_src.Reserve(packed * h->H, &h->allocations);
  VSG_HIP(hipMemcpy2DAsync(h->d_src.p, packed, bgr, stride, (size_t)h->W * 3, h->H, hipMemcpyHostToDevice, h->stream));
  ++*launches;
  return {h->d_src.As<uint8_t>(), packed};
}

struct PictureOut {
  uint8_t* p;
  size_t stride;
};

// Where the kernels write a picture of `rows` rows: the caller's device memory, or, for a host output, the
// handle's block with the default stride, which the caller copies out.
PictureOut StagePicture(vsg_render* h, uint8_t* out, size_t out_stride, int rows, int mem_out) {
  if (mem_out != VSG_MEM_HOST) return {out, out_stride};
  const size_t packed = vsg_render_default_stride(h->W);
  h->d_out.Reserve(packed * rows, &h->allocations);
  return {h->d_out.As<uint8_t>(), packed};
}

// ---- a label plane of the caller's (`other`) ------------------------------------------------------
void CheckOtherPlane(const int32_t* other, int mem_other) {
  if (!other) Throw(VSG_ERR_INVALID, "other is null");
  if (mem_other != VSG_MEM_HOST && mem_other != VSG_MEM_DEVICE) {
    Throw(VSG_ERR_INVALID, "mem_other is neither VSG_MEM_HOST nor VSG_MEM_DEVICE");
  }
}

// The distance between its rows, in values: other_pitch, or the width for 0.
size_t CheckOtherPitch(const vsg_render* h, size_t other_pitch) {
  if (other_pitch != 0 && other_pitch < (size_t)h->W) {
    Throw(VSG_ERR_INVALID, "the pitch of other, " + std::to_string(other_pitch) + ", is below the width " +
                               std::to_string(h->W));
  }
  return other_pitch ? other_pitch : (size_t)h->W;
}

struct OtherPlane {
  const int32_t* plane;
  size_t pitch;
};

// The plane where the kernels read it: where it is, or through the pinned block to the device, rows packed.
OtherPlane UploadOtherPlane(vsg_render* h, const int32_t* other, size_t pitch, int mem_other, int* launches) {
  if (mem_other != VSG_MEM_HOST) return {other, pitch};
  const int W = h->W, H = h->H;
  const size_t bytes = (size_t)W * H * sizeof(int32_t);
  h->h_other.Reserve(bytes, &h->allocations);
  h->d_other.Reserve(bytes, &h->allocations);
  for (int y = 0; y < H; ++y) {
    std::memcpy(h->h_other.As<int32_t>() + (size_t)y * W, other + (size_t)y * pitch, (size_t)W * sizeof(int32_t));
  }
  VSG_HIP(hipMemcpyAsync(h->d_other.p, h->h_other.p, bytes, hipMemcpyHostToDevice, h->stream));
  ++*launches;
  return {h->d_other.As<int32_t>(), (size_t)W};
}

// ---- status words and host outputs ----------------------------------------------------------------
template <class T>
struct StatusPair {
  T* status;   // on the device; the caller clears it on the stream where its sequence has the clear
  T* seen;     // pinned, zeroed: [0] read back in the middle of the call, [1] at the end
};

template <class T>
StatusPair<T> ReserveStatusPair(vsg_render* h, Block* device, Block* pinned) {
  device->Reserve(sizeof(T), &h->allocations);
  pinned->Reserve(2 * sizeof(T), &h->allocations);
  std::memset(pinned->p, 0, 2 * sizeof(T));
  return {device->As<T>(), pinned->As<T>()};
}

// One list of a host delivery: `bytes` of device memory for the caller's `to`.
struct Delivery {
  const void* from;
  size_t bytes;
  void* to;
};

// Lists to host outputs through a family's pinned block, now that their lengths are known: makes room for them
// behind the block's first status_bytes, enqueues a copy per non-empty list, waits for the stream and hands the
// lists to the caller.  The block may move: what was read of the status words is used before.  Returns the
// number of copies enqueued.
int DeliverToHost(vsg_render* h, Block* pinned, size_t status_bytes, std::initializer_list<Delivery> lists) {
  size_t bytes = status_bytes;
  for (const Delivery& l : lists) bytes += l.bytes;
  pinned->Reserve(bytes, &h->allocations);
  char* const stage = pinned->As<char>() + status_bytes;
  int copies = 0;
  char* at = stage;
  for (const Delivery& l : lists) {
    if (!l.bytes) continue;
    VSG_HIP(hipMemcpyAsync(at, l.from, l.bytes, hipMemcpyDeviceToHost, h->stream));
    at += l.bytes;
    ++copies;
  }
  VSG_HIP(hipStreamSynchronize(h->stream));
  at = stage;
  for (const Delivery& l : lists) {
    if (l.bytes) std::memcpy(l.to, at, l.bytes);
    at += l.bytes;
  }
  return copies;
}

}  // namespace
