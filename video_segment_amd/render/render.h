// render.h -- launchers of the render kernels, one section per .hip file (render, vector, lists, level,
// components, boundaries, adjacency, overlap, persistence, colors, pool, contours, mesh, simplify, distance,
// volume), called by the parts of render_capi.cpp (render_handle.h and the capi_*.inc files).  The library sorts,
// the plain scan and the copy of a call's lists to device memory are lists.hip's, shared by every family; the
// scans over segment heads are render_scan.h's; the device helpers the kernels share are render_device.h's.
#ifndef VSG_RENDER_RENDER_H_
#define VSG_RENDER_RENDER_H_

#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace vsg_render_impl {

// One scan interval to paint: pixels [left_x, right_x] of row y get `value` (a packed colour
// c0 | c1 << 8 | c2 << 16, or a region id).  The host has checked it against the frame.
struct Interval {
  int32_t y, left_x, right_x;
  uint32_t value;
};
static_assert(sizeof(Interval) == 16, "uploaded as int4");

enum ComposeMode { COMPOSE_RENDER = 0, COMPOSE_BLEND = 1, COMPOSE_CONCAT = 2 };

// Row pitch (in uint32) of the colour plane of a W-wide frame: a multiple of 4 with at least four
// spare columns, so that k_render_compose may load the uint4 of its last column group and that
// group's right neighbour without leaving the row.
inline int PlanePitch(int width) { return (width + 3) / 4 * 4 + 4; }

// plane[y * pitch + x] = value for every pixel of every interval.  No launch when n == 0.
void LaunchFill(const Interval* intervals, int64_t n, uint32_t* plane, int pitch, hipStream_t stream);

// Edge rule + blend / concatenation from the filled plane into BGR24 rows.  src may be null for
// COMPOSE_RENDER.  out has H rows (2 * H for COMPOSE_CONCAT) of out_stride bytes.
void LaunchCompose(const uint32_t* plane, int pitch, int width, int height, const uint8_t* src,
                   size_t src_stride, uint8_t* out, size_t out_stride, int highlight_edges, int mode,
                   float alpha, hipStream_t stream);

// ---- vector path (vector.hip): scan intervals from polygon lines ------------------------------------

// One kept polygon line (|dy| >= 1e-3f), points ordered by y: what the reference's EdgeEntry holds,
// the row it is inserted at, and where its crossings go.  Built and checked by the host: y0 >= 0,
// y_max <= H, and [offset, offset + count) is this line's own slice of the crossing arrays.
struct VecLine {
  int32_t region;    // index of the Region2D in the desc
  int32_t y0;        // (int)p1.y, the row of insertion
  float x;           // p1.x
  float y_max;       // p2.y
  float dx;          // (p2.x - p1.x) / (p2.y - p1.y)
  int32_t is_left;   // 0 when the points were swapped
  uint32_t offset;   // prefix sum of count
  uint32_t count;    // rows y0, y0 + 1, ... with !(y_max < y + 1)
};
static_assert(sizeof(VecLine) == 32, "uploaded as is");

constexpr int kVecRowBits = 16;   // sort key = region index << 16 | row; frames have at most 2^15 rows

enum VecFlag { VEC_FLAG_UNSPECIFIED = 1, VEC_FLAG_INTERNAL = 2 };

// Written by the vector kernels, read once by the host at the end of a call.
struct VecStatus {
  uint32_t flags, pad;
  unsigned long long groups, largest_group;
};

void LaunchVecWalk(const VecLine* lines, int n_lines, unsigned long long* keys, unsigned long long* vals,
                   VecStatus* status, hipStream_t stream);
// n sorted crossings (n even) -> n / 2 intervals, dense, in region / row / left-to-right order.
// `intervals` has to be cleared to zero before.  value = region_value[region index].
void LaunchVecPairs(const unsigned long long* keys, const unsigned long long* vals, const VecLine* lines,
                    uint32_t n_lines, const uint32_t* region_value, uint32_t n_regions, int64_t n, int width,
                    int height, Interval* intervals, VecStatus* status, hipStream_t stream);

// ---- lists (lists.hip): the library sorts and scan, the copy of a call's lists to device memory ------

// The library radix sort on bits [0, end_bit) of n keys (with their values), and its work space.  U64U32:
// 64-bit keys, 32-bit values.
size_t SortKeysU64TempBytes(int64_t n, int end_bit);
hipError_t SortKeysU64(void* temp, size_t temp_bytes, const unsigned long long* in, unsigned long long* out, int64_t n,
                       int end_bit, hipStream_t stream);
size_t SortPairsU64U32TempBytes(int64_t n, int end_bit);
hipError_t SortPairsU64U32(void* temp, size_t temp_bytes, const unsigned long long* keys_in,
                           unsigned long long* keys_out, const uint32_t* vals_in, uint32_t* vals_out, int64_t n,
                           int end_bit, hipStream_t stream);
size_t SortPairsU64U64TempBytes(int64_t n, int end_bit);
hipError_t SortPairsU64U64(void* temp, size_t temp_bytes, const unsigned long long* keys_in,
                           unsigned long long* keys_out, const unsigned long long* vals_in,
                           unsigned long long* vals_out, int64_t n, int end_bit, hipStream_t stream);
size_t SortPairsU32U32TempBytes(int64_t n, int end_bit);
hipError_t SortPairsU32U32(void* temp, size_t temp_bytes, const uint32_t* keys_in, uint32_t* keys_out,
                           const uint32_t* vals_in, uint32_t* vals_out, int64_t n, int end_bit, hipStream_t stream);
// out[i] = in[0] + ... + in[i - 1], i < n.
size_t ExclusiveSumU32TempBytes(int n);
hipError_t ExclusiveSumU32(void* temp, size_t temp_bytes, const uint32_t* in, uint32_t* out, int n,
                           hipStream_t stream);

// One list of a call: `words` int32 per entry, *count entries (device memory), or `fixed` of them when count is
// null.  limit: the most entries the list may have: the smaller of the caller's capacity and the slots of `from`.
struct CopyList {
  const int32_t* from;
  int32_t* to;
  uint32_t words;
  const uint32_t* count;
  uint32_t fixed, limit;
};
// The lists of a call, unused ones zero.  flags: null, or a word of device memory that has to be 0.
struct CopyLists {
  CopyList list[4];
  const uint32_t* flags;
};
// Copies every list to its `to` (device memory), or nothing at all when a list is longer than its limit or a
// flag is up.  No launch when every limit is 0.
void LaunchCopyLists(const CopyLists& lists, hipStream_t stream);

// ---- level regions (level.hip): runs, regions and moments from the filled id plane ------------------

constexpr int kLevelRegionWords = 14;   // vsg_render_level_region as int32 words

// Written by the level kernels; read by the host after k_level_runs and at the end of a call.
struct LevelStatus {
  uint32_t runs;       // maximal runs of the plane
  uint32_t overflow;   // a run had no slot: the host's bound on the runs was wrong
  uint32_t regions;    // distinct ids among the runs
  uint32_t largest;    // most intervals of one region
};

// Runs of the H x W id plane (-1: no run): keys[k] = id << 32 | (y * W + left_x), rights[k] = right_x,
// in no particular order, status->runs of them.  Slots at or beyond `capacity` are not written.
void LaunchLevelRuns(const int32_t* plane, int pitch, int width, int height, uint32_t capacity,
                     unsigned long long* keys, uint32_t* rights, LevelStatus* status, hipStream_t stream);
// n sorted runs -> n intervals, and id and first_interval of every region; status->regions.
// `regions` has room for capacity_regions entries of kLevelRegionWords words.
void LaunchLevelTable(const unsigned long long* keys_sorted, const uint32_t* rights_sorted, const uint32_t* rank,
                      uint32_t n, int width, uint32_t capacity_regions, Interval* intervals, int32_t* regions,
                      LevelStatus* status, hipStream_t stream);
// The remaining fields of every region; status->largest.
void LaunchLevelMoments(const Interval* intervals, uint32_t n, uint32_t capacity_regions, int32_t* regions,
                        LevelStatus* status, hipStream_t stream);

// ---- level components (components.hip): the connected components of every region of a level ---------

constexpr int kLevelComponentWords = 16;   // vsg_render_level_component as int32 words

enum CompFlag {
  COMP_FLAG_BOUND = 1,     // a find or hook loop ran out of its bound, or an index was out of range
  COMP_FLAG_DROPPED = 2,   // a component or a region had no slot
};

// Written by the component kernels; read by the host once the table is made and at the end of a call.
struct CompStatus {
  unsigned long long links;   // neighbour pairs found between adjacent rows
  uint32_t components;
  uint32_t largest;           // most intervals of one component
  uint32_t flags, pad;
};

// Union-find over the n sorted runs of the level (keys, right ends): runs of one id in adjacent rows
// are united when left_a <= right_b + slack and left_b <= right_a + slack (slack 0: N4, 1: N8).
// Leaves label[i] = the smallest run index of i's component and index[i] = i.  parent, label and index
// have n entries each.
void LaunchCompLink(const unsigned long long* keys_sorted, const uint32_t* rights_sorted, uint32_t n, int width,
                    int slack, uint32_t* parent, uint32_t* label, uint32_t* index, CompStatus* status,
                    hipStream_t stream);
// n ordered runs -> the ordered interval list, the same list with the component's index as its value
// (`fill`, may be null), and id, component, region_components and first_interval of every component;
// status->components.  region_rank and intervals are the scan of HeadFlag and LaunchLevelTable's, level_status
// holds the number of regions.  `components` has room for capacity_components entries of
// kLevelComponentWords words, region_first for capacity_regions words.
void LaunchCompTable(const uint32_t* label_sorted, const uint32_t* order, const uint32_t* comp_rank,
                     const uint32_t* region_rank, const Interval* intervals, uint32_t n,
                     uint32_t capacity_components, uint32_t capacity_regions, Interval* ordered, Interval* fill,
                     int32_t* components, uint32_t* region_first, const LevelStatus* level_status,
                     CompStatus* status, hipStream_t stream);
// The remaining fields of every component, by the kernel of LaunchLevelMoments; status->largest.
void LaunchComponentMoments(const Interval* intervals, uint32_t n, uint32_t capacity_components,
                            int32_t* components, CompStatus* status, hipStream_t stream);

// ---- level boundaries (boundaries.hip): the N4 boundary pixels of every group of an int32 plane -----

constexpr int kLevelBoundaryWords = 4;   // vsg_render_level_boundary as int32 words

enum BoundFlag {
  BOUND_FLAG_OVERFLOW = 1,   // a key had no slot: the emit pass found more keys than the count pass
  BOUND_FLAG_RANGE = 2,      // a sorted key, a rank or a record was out of range
};

// Written by the boundary kernels; read by the host after the count pass and at the end of a call.
struct BoundStatus {
  unsigned long long points;   // keys the count pass found
  uint32_t emitted;            // slots the emit pass reserved
  uint32_t boundaries;         // distinct groups among the keys
  uint32_t largest;            // most points of one boundary
  uint32_t flags;
};

// The boundary keys of the H x W plane (row pitch W; -1 and everything outside the frame: no group),
// group << 32 | (y + 1) * (W + 2) + (x + 1).  outer false: the pixels of a group with a 4-neighbour
// outside it; true: the positions of [-1, W] x [-1, H] outside a group with a 4-neighbour in it, once
// per group.  emit false: status->points += their number, keys is not looked at.  emit true: the keys,
// in no particular order, status->emitted of them; a slot at or beyond `capacity` is not written and
// raises BOUND_FLAG_OVERFLOW.
void LaunchBoundClassify(const int32_t* plane, int width, int height, bool outer, bool emit, uint32_t capacity,
                         unsigned long long* keys, BoundStatus* status, hipStream_t stream);
// n sorted keys with their ranks (the scan of HeadFlag) -> n points {x, y} and the records {id, component, first_point,
// num_points}; status->boundaries and status->largest.  comp_table: null (id = group, component = -1),
// or the table of LaunchCompTable the groups index.  `records` has room for capacity_records entries.
void LaunchBoundTable(const unsigned long long* keys_sorted, const uint32_t* rank, uint32_t n, int width, int height,
                      uint32_t max_group, uint32_t capacity_records, const int32_t* comp_table, int32_t* points,
                      int32_t* records, BoundStatus* status, hipStream_t stream);

// ---- level adjacency (adjacency.hip): the region adjacency graph of an int32 plane -------------------

constexpr int kLevelNodeWords = 7;   // vsg_render_level_node as int32 words
constexpr int kLevelEdgeWords = 4;   // vsg_render_level_edge as int32 words

enum AdjFlag {
  ADJ_FLAG_OVERFLOW = 1,   // a key had no slot: the emit pass found more keys than the count pass
  ADJ_FLAG_RANGE = 2,      // a sorted key, a rank, a node or an edge was out of range
};

// Written by the adjacency kernels; read by the host after the count pass and at the end of a call.
struct AdjStatus {
  unsigned long long keys;   // keys the count pass found
  uint32_t emitted;          // slots the emit pass reserved
  uint32_t nodes;            // distinct groups among the keys
  uint32_t edges;            // distinct (group, neighbouring group) among the keys
  uint32_t largest;          // most edges of one node
  uint32_t flags, pad;
};

// The adjacency keys of the H x W plane (row pitch W; negative: no group): for every covered position
// one key group << (group_bits + 2) | other << 1 | kind per pixel side that does not lead to its own
// group (kind 0; other = the group across, 1 << group_bits for the frame edge, 1 << group_bits | 1 for
// an uncovered pixel) and, with `diagonal`, one per diagonal neighbour of another group (kind 1).  Every
// group is below 1 << group_bits, group_bits in [1, 31].  emit false: status->keys += their number,
// keys is not looked at.  emit true: the keys, in no particular order, status->emitted of them; a slot
// at or beyond `capacity` is not written and raises ADJ_FLAG_OVERFLOW.
void LaunchAdjClassify(const int32_t* plane, int width, int height, int group_bits, bool diagonal, bool emit,
                       uint32_t capacity, unsigned long long* keys, AdjStatus* status, hipStream_t stream);
// n sorted keys with the scan of AdjHeads -> the nodes and the edges; status->nodes, ->edges and ->largest.
// `nodes` (capacity_nodes entries) and `edges` (capacity_edges entries) have to be cleared to zero
// before.  comp_table: null (id = group, component = -1, neighbour = the rank of the neighbour's id), or
// the table of LaunchCompTable the groups index (neighbour = the group across).
void LaunchAdjTable(const unsigned long long* keys_sorted, const unsigned long long* heads, uint32_t n, int group_bits,
                    uint32_t max_group, uint32_t capacity_nodes, uint32_t capacity_edges, const int32_t* comp_table,
                    int32_t* nodes, int32_t* edges, AdjStatus* status, hipStream_t stream);

// ---- level overlap (overlap.hip): the contingency table of an int32 plane and a plane of labels ------

constexpr int kOverlapRowWords = 8;    // vsg_render_overlap_row as int32 words
constexpr int kOverlapColWords = 6;    // vsg_render_overlap_col as int32 words
constexpr int kOverlapPairWords = 4;   // vsg_render_overlap_pair as int32 words
constexpr int kOverlapRowTotals = 5;   // words a frame row leaves for the count pass's totals

enum OvlFlag {
  OVL_FLAG_OVERFLOW = 1,   // a run had no slot: the emit pass found more runs than the count pass
  OVL_FLAG_RANGE = 2,      // a sorted key, a rank, a row, a column or a pair was out of range
};

// Written by the overlap kernels; read by the host after the count pass and at the end of a call.
struct OvlStatus {
  uint32_t runs;        // runs the count pass found
  uint32_t covered;     // pixels with P >= 0
  uint32_t labelled;    // pixels with B >= 0
  uint32_t both;        // pixels with both
  uint32_t max_label;   // the largest value of B (0 without a label)
  uint32_t emitted;     // slots the emit pass reserved
  uint32_t distinct;    // distinct (group or none, label or none) among the runs
  uint32_t rows, cols, pairs;
  uint32_t largest;     // most pairs of one row
  uint32_t flags;
};

// The runs of constant (P, B) of the two H x W planes (`plane`: row pitch W; `other`: row pitch
// other_pitch; negative: none), a run ending with its frame row, those with both values negative left out.
// emit false: status->runs = their number, ->covered, ->labelled and ->both = the pixels with P >= 0, with
// B >= 0 and with both, ->max_label = the largest label, summed over row_totals (height x
// kOverlapRowTotals words, every one written); keys and lengths are not looked at.  emit true:
// keys[k] = code(P) << (label_bits + 1) | code(B) and lengths[k] of every run, in no particular order,
// status->emitted of them; code(v) = v for v >= 0; "none" is 1 << group_bits for P and 1 << label_bits for
// B, every group below the one and every label below the other, both bit counts in [1, 31].  A slot at or
// beyond `capacity` is not written and raises OVL_FLAG_OVERFLOW.
void LaunchOverlapRuns(const int32_t* plane, const int32_t* other, size_t other_pitch, int width, int height,
                       int group_bits, int label_bits, bool emit, uint32_t capacity, unsigned long long* keys,
                       uint32_t* lengths, uint32_t* row_totals, OvlStatus* status, hipStream_t stream);
// n sorted runs with the scans of OvlRowHeads and OvlKeyHeads -> the list of distinct keys (key, start and rank: m, m + 1 and m
// entries; m bounds their number), the rows (capacity_rows entries, cleared to zero before) and the pairs
// (m entries) but for `col`, and the m (column key, index of the distinct key) operands of the column sort;
// status->distinct, ->rows, ->pairs and ->largest.  comp_table: null (id = group, component = -1), or the
// table of LaunchCompTable the groups index.
void LaunchOverlapTable(const unsigned long long* keys_sorted, const uint32_t* lengths_sorted,
                        const unsigned long long* row_heads, const unsigned long long* key_heads, uint32_t n,
                        uint32_t m, int group_bits, int label_bits, uint32_t max_group, uint32_t capacity_rows,
                        const int32_t* comp_table, unsigned long long* key, uint32_t* start, unsigned long long* rank,
                        int32_t* rows, int32_t* pairs, unsigned long long* ckeys, uint32_t* cvals, OvlStatus* status,
                        hipStream_t stream);
// m sorted column operands with their ranks -> the columns (m entries) and `col` of every pair;
// status->cols.  `first` has m + 1 entries; start and rank are those of LaunchOverlapTable.
void LaunchOverlapCols(const unsigned long long* ckeys_sorted, const uint32_t* cvals_sorted, const uint32_t* col_rank,
                       const uint32_t* start, const unsigned long long* rank, uint32_t m, int group_bits,
                       int label_bits, uint32_t* first, int32_t* cols, int32_t* pairs, OvlStatus* status,
                       hipStream_t stream);

// ---- boundary persistence (persistence.hip): all hierarchy levels' edges from the level-0 plane --------

enum PersFlag {
  PERS_FLAG_RANGE = 1,   // a region number, a node or an edge was out of range
};

// Written by the persistence kernels; read by the host at the end of a call.
struct PersStatus {
  unsigned long long edge_pixels;   // pixels with Q > 0
  unsigned long long top_pixels;    // pixels with Q == levels
  uint32_t flags, pad;
};

// The persistence plane of the H x W plane of dense region numbers (row pitch PlanePitch(width), -1: no
// region, the spare columns -1 as well): q[y * q_pitch + x] = the larger of the persistences of the pixel
// against its in-frame right and below neighbours, 0 where it equals both.  table: (levels - 1) rows of
// `regions` ancestors (persistence_table.h), not looked at when levels == 1; every number of the plane is
// below `regions`.  status->edge_pixels and ->top_pixels are added to.
void LaunchPersistPlane(const int32_t* plane, int pitch, int width, int height, const int32_t* table,
                        uint32_t regions, int levels, int32_t* q, size_t q_pitch, PersStatus* status,
                        hipStream_t stream);
// Every byte of the H rows of 3 * width: (s * (levels - Q) + levels / 2) / levels with s the source's byte,
// or 255 when src is null.  q: 16-byte aligned, q_pitch a multiple of 4.
void LaunchPersistCompose(const int32_t* q, size_t q_pitch, int width, int height, int levels, const uint8_t* src,
                          size_t src_stride, uint8_t* out, size_t out_stride, hipStream_t stream);
// persistence[e] of every directed edge of the level-0 graph (LaunchAdjTable's nodes and edges, region
// planes), hist[p] += shared_n4 of the edges with persistence p.  ids: the n_ids sorted region ids the
// table's columns stand for.  hist has levels + 1 entries, cleared to zero before.  No launch without an
// edge.
void LaunchPersistEdges(const int32_t* nodes, uint32_t n_nodes, const int32_t* edges, uint32_t n_edges,
                        const int32_t* ids, uint32_t n_ids, const int32_t* table, int levels, int32_t* persistence,
                        unsigned long long* hist, PersStatus* status, hipStream_t stream);
// level_sides[l] = half the sum of hist[p] over p > l, l in [0, levels).
void LaunchPersistSides(const unsigned long long* hist, int levels, long long* level_sides, hipStream_t stream);

// ---- level colours (colors.hip): colour sums of every group of a level, the mean-colour intervals ------

constexpr int kLevelColorWords = 18;     // vsg_render_level_color as int32 words
constexpr int kColorPartialWords = 8;    // one interval's partial: 3 sums, 3 sums of squares, min, max
constexpr size_t kColorAccBytes = 80;    // what a record gathers before it is finished

enum ColorFlag {
  COLOR_FLAG_RANGE = 1,   // an interval's record was out of range, or a record had no pixel
};

// Written by the colour kernels; read by the host at the end of a call.
struct ColorStatus {
  unsigned long long covered;   // sum of the records' areas
  uint32_t largest;             // most intervals of one record
  uint32_t flags;
};

// One partial of kColorPartialWords words per interval from the BGR24 frame `bgr` (rows `stride` bytes
// apart, device memory): the sums and the sums of squares of the three channels (uint32 each), the minima
// and the maxima packed as c0 | c1 << 8 | c2 << 16.  Only bytes [3 * left_x, 3 * right_x + 2] of row y are
// read.  Dword loads when bgr and stride are multiples of 4.
void LaunchColorRuns(const Interval* intervals, uint32_t n, int width, int height, const uint8_t* bgr, size_t stride,
                     uint32_t* partials, hipStream_t stream);
// The partials summed per record, then the records.  rank[i] - 1 is the record of interval i (the scan of
// HeadFlag or LabelHead; records are contiguous in the list).  acc: capacity_acc entries of kColorAccBytes,
// cleared to zero before.  table: table_words words per record, word 0 its id, word 1 (has_component) its
// component.  *count records exist (device memory); they are written to `records` unless there are more
// than `capacity`.  status->covered and ->largest are added to.
void LaunchColorTable(const Interval* intervals, const uint32_t* rank, const uint32_t* partials, uint32_t n,
                      uint32_t capacity_acc, void* acc, const int32_t* table, int table_words, bool has_component,
                      const uint32_t* count, uint32_t capacity, int32_t* records, ColorStatus* status,
                      hipStream_t stream);
// out[i] = interval i with the packed mean of its record as its value.
void LaunchColorIntervals(const Interval* intervals, const uint32_t* rank, uint32_t n, const int32_t* records,
                          uint32_t capacity, Interval* out, hipStream_t stream);

// ---- level pooling (pool.hip): float feature planes pooled by group, group values painted back ---------

constexpr int kPoolGroupWords = 4;          // vsg_render_pool_group as int32 words
constexpr int kPoolPlanarChannels = 8;      // channels a wavefront of the planar sums kernel takes
constexpr int kPoolLastChannels = 64;       // channels a wavefront of the channels-last sums kernel takes
constexpr int kPoolLongInterval = 64;       // planar: from this length on the whole wavefront sums one interval,
constexpr int kPoolGroupInterval = 16;      // from this one on 16 lanes do, from this one on four; a shorter one is
constexpr int kPoolQuadInterval = 4;        // summed by its own lane
constexpr uint32_t kPoolWaves = 1024;       // the slices the sums kernels want before a slice takes more intervals

enum PoolDtype { POOL_F32 = 0, POOL_F16 = 1, POOL_BF16 = 2 };
enum PoolStat { POOL_SUM = 1, POOL_SUM_SQ = 2, POOL_MIN = 4, POOL_MAX = 8 };
enum PoolFlag {
  POOL_FLAG_RANGE = 1,   // an interval's record was out of range, or a record had no pixel
};

// Written by the pool kernels; read by the host at the end of a call.
struct PoolStatus {
  unsigned long long covered;   // sum of the records' areas
  uint32_t largest;             // most intervals of one record
  uint32_t flags;
};

// Where the elements of a feature map are (strides in elements) and what they are.  channels_last: lanes go
// along the channels of a pixel (chan_stride 1); otherwise along x (pixel_stride 1).
struct PoolLayout {
  long long chan_stride, row_stride, pixel_stride;
  int channels, dtype;
  bool channels_last;
};

// The four statistics as dense [records][channels] matrices; null where one is not wanted.
struct PoolMatrices {
  double* sum;
  double* sum_sq;
  float* min;
  float* max;
};

// The intervals a slice of the list has: 64, or fewer (a power of two) while the list is short.  A function of
// n alone, so that the order of every sum is one of the list.
uint32_t PoolSlice(uint32_t n);
inline uint32_t PoolSlices(uint32_t n) {
  const uint32_t s = PoolSlice(n);
  return (n + s - 1) / s;
}
// Sums of every record that lies inside one slice into `out`, of every part of a record that goes on into
// another slice into `spill`: [slices][2][channels] per statistic, [s][0] the part that began before slice s,
// [s][1] the part that goes on behind it.  mask: the PoolStat bits wanted; the matrices of both have them.
// Only the elements of covered pixels are read.  No launch when n == 0.
void LaunchPoolSums(const Interval* intervals, const uint32_t* rank, uint32_t n, int width, int height,
                    const void* features, const PoolLayout& layout, int mask, const PoolMatrices& out,
                    const PoolMatrices& spill, hipStream_t stream);
// The records that span slices: their parts combined in slice order.
void LaunchPoolCombine(const uint32_t* rank, uint32_t n, int channels, int mask, const PoolMatrices& spill,
                       const PoolMatrices& out, hipStream_t stream);
// Area and interval count of every record (acc: two uint32 per record, cleared before), then the groups
// {id, component or -1, area, 0} and the status' totals.  table, table_words, has_component as for the colours.
void LaunchPoolGroups(const Interval* intervals, const uint32_t* rank, uint32_t n, uint32_t records, uint32_t* acc,
                      const int32_t* table, int table_words, bool has_component, int32_t* groups, PoolStatus* status,
                      hipStream_t stream);
// out[i] = interval i with its 1-based record as its value.
void LaunchPoolIntervals(const Interval* intervals, const uint32_t* rank, uint32_t n, Interval* out,
                         hipStream_t stream);
// out(c, y, x) = values[plane(y, x) - 1][c] converted to the layout's dtype (round to nearest even), `fill`
// where the plane holds 0 or a record beyond num_values.  Only the W elements of a row (planar) or the
// channels of a pixel (channels-last) are written.
void LaunchPoolGather(const uint32_t* plane, int pitch, int width, int height, const float* values,
                      uint32_t num_values, float fill, void* out, const PoolLayout& layout, hipStream_t stream);

// ---- level contours (contours.hip): the traced closed contours of every group of an int32 plane --------

constexpr int kLevelContourWords = 12;   // vsg_render_level_contour as int32 words

enum ContourFlag {
  CONTOUR_FLAG_OVERFLOW = 1,   // a contour had no slot: more than one contour per four cracks
  CONTOUR_FLAG_RANGE = 2,      // a crack, a successor, a leader, a rank, a contour or a vertex was out of range
};

// Written by the contour kernels; read by the host after the count pass and at the end of a call.
struct ContourStatus {
  unsigned long long cracks;   // pixel sides the count pass found
  uint32_t contours;           // cycles of the successor permutation
  uint32_t vertices;           // turn cracks
  uint32_t holes;              // contours with a negative area
  uint32_t largest;            // most cracks of one contour
  uint32_t flags, pad;
};

// Work space of ContourClassify's scan over `pixels` mask bytes.
size_t ContourClassifyTempBytes(uint32_t pixels);
// The count pass over the H x W plane (row pitch W; negative and everything outside the frame: no group):
// mask[p] = bit s set when side s (0 top, 1 right, 2 bottom, 3 left) of pixel p is a crack, offset[p] = the
// cracks of the pixels before p, status->cracks += their number.
hipError_t ContourClassify(void* temp, size_t temp_bytes, const int32_t* plane, int width, int height, uint8_t* mask,
                           uint32_t* offset, ContourStatus* status, hipStream_t stream);
// The emit pass: for crack i = offset[p] + (set bits of mask[p] below s) its key 4 p + s with bit 31 set when
// it is a turn crack, succ[i] = the crack the contour continues with, state[i] = {succ[i], i or ~0 (no turn)}.
// n: status->cracks as the host read it; key, succ and state have n entries.
void LaunchContourEmit(const int32_t* plane, int width, int height, const uint8_t* mask, const uint32_t* offset,
                       uint32_t n, uint32_t* key, uint32_t* succ, uint2* state, ContourStatus* status,
                       hipStream_t stream);
// The rounds of either doubling: ceil(log2 n), made even (a launch does two).
int ContourRounds(uint32_t n);
// Both doublings, rounds + 1 launches between state_a (k_contour_emit's) and state_b: leader[i] = the turn
// crack of smallest key of i's contour; returns the buffer (one of the two) whose .y is the number of turn
// cracks in [i, leader) along the contour, 0 for the leader.  The other buffer is free afterwards.
const uint2* LaunchContourTrace(const uint32_t* key, const uint32_t* succ, uint32_t n, int rounds, uint2* state_a,
                                uint2* state_b, uint32_t* leader, ContourStatus* status, hipStream_t stream);
// The summing rounds alone (k_contour_round<true>), rounds / 2 launches from `in` to `out` and back: for a
// state {next, weight} whose fixed points weigh 0, .y becomes the sum of the weights from i up to its fixed
// point.  Every .x has to be below n.  Returns the buffer that holds the result; the other one is free.
const uint2* LaunchContourSums(uint2* in, uint2* out, uint32_t n, int rounds, hipStream_t stream);
// ckeys[slot] = group << 32 | leader of every contour, in no order; status->contours.  ckeys has `capacity`
// entries, set to ~0 before so that unused slots sort last.
void LaunchContourLeaders(const uint32_t* leader, const uint32_t* key, const int32_t* plane, uint32_t n,
                          uint32_t capacity, unsigned long long* ckeys, ContourStatus* status, hipStream_t stream);
// count[j] and first[j] of sorted contour j (capacity entries each, 0 beyond the contours), place[leader] = j
// (n entries), then every turn crack's start corner at vertices[first + rank] and owner[that slot] = j
// (n slots each).  Three launches.
hipError_t ContourVertices(void* temp, size_t temp_bytes, const unsigned long long* ckeys_sorted, const uint32_t* key,
                           const uint32_t* succ, const uint32_t* leader, const uint2* ranked, uint32_t n,
                           uint32_t capacity, int width, uint32_t* place, uint32_t* count, uint32_t* first,
                           int32_t* vertices, uint32_t* owner, ContourStatus* status, hipStream_t stream);
// The records (capacity entries); status->vertices, ->holes and ->largest.  rank: the scan of HeadFlag over the sorted
// keys.  comp_table: null (id = group, component = -1, group = rank - 1), or the table of LaunchCompTable
// the groups index.  Three launches.
void LaunchContourTable(const unsigned long long* ckeys_sorted, const uint32_t* rank, const uint32_t* count,
                        const uint32_t* first, const int32_t* vertices, const uint32_t* owner, uint32_t n,
                        uint32_t capacity, uint32_t max_group, const int32_t* comp_table, int32_t* records,
                        ContourStatus* status, hipStream_t stream);

// ---- level mesh (mesh.hip): the contours cut at the junctions into shared segments -----------------------

constexpr int kMeshSegmentWords = 8;   // vsg_render_mesh_segment as int32 words
constexpr int kMeshLoopWords = 4;      // vsg_render_mesh_loop

enum MeshFlag {
  MESH_FLAG_RANGE = 1,   // a crack, a contour, a half, a segment or a vertex was out of range
};

// Written by the mesh kernels; read by the host after the split and at the end of a call.
struct MeshStatus {
  uint32_t junctions;   // corners with three or four sides
  uint32_t segments;    // owner halves
  uint32_t refs;        // halves
  uint32_t vertices;
  uint32_t closed, shared, longest;
  uint32_t flags;
};

// What the contour stages of a call left on the device.  n cracks; `contours` contours in list order.
struct MeshInput {
  const int32_t* plane;
  int width, height;
  const uint8_t* mask;
  const uint32_t* offset;
  uint32_t n;
  const uint32_t* key;
  const uint32_t* succ;
  const uint32_t* leader;
  const uint32_t* place;
  const uint2* ranked;
  uint32_t contours;
  const uint32_t* count;
  const int32_t* records;
};

// Per crack (n entries each): sides, the two doubling states, half, head_of and behind it last_of (2 n),
// seg_of, skeys.  Per contour: hasj, nrefs, first_ref.  heads: set by MeshSplit, one of the two states.
struct MeshCrackSpace {
  uint8_t* sides;
  uint2* state_a;
  uint2* state_b;
  const uint2* heads;
  uint32_t* half;
  uint32_t* head_of;
  uint32_t* seg_of;
  unsigned long long* skeys;
  uint32_t* hasj;
  uint32_t* nrefs;
  uint32_t* first_ref;
};

// Per segment: the sorted keys, scount, sfirst, the records.  vertex_slots vertices and their segments; the
// loops (one per contour) and the refs (one per half).
struct MeshSegmentSpace {
  unsigned long long* skeys_sorted;
  uint32_t* scount;
  uint32_t* sfirst;
  int32_t* segments;
  uint32_t vertex_slots;
  int32_t* vertices;
  uint32_t* vseg;
  int32_t* loops;
  int32_t* refs;
};

// Junction bits, the third doubling (rounds / 2 launches), the halves of every crack, head and last crack of
// every half, the unsorted owner keys; status->junctions, ->segments, ->refs.  ckeys_sorted: the contours'.
// 7 + rounds / 2 launches, the scan counted as one.
hipError_t MeshSplit(void* temp, size_t temp_bytes, const MeshInput& in, const unsigned long long* ckeys_sorted,
                     int rounds, MeshCrackSpace* w, MeshStatus* status, hipStream_t stream);
// The segments' sort, their vertices, records, loops, refs and lengths; status->vertices, ->closed, ->shared,
// ->longest.  n_segments, n_halves: as the host read them after MeshSplit.  11 launches, the sort and the
// scan counted as one each.
hipError_t MeshTables(void* temp, size_t temp_bytes, const MeshInput& in, const MeshCrackSpace& w,
                      const MeshSegmentSpace& t, uint32_t n_segments, uint32_t n_halves, int end_bit,
                      MeshStatus* status, hipStream_t stream);

// ---- mesh simplification (simplify.hip): Douglas-Peucker on the segments of the level mesh ----------------

constexpr int kSimplifyWavePoints = 256;    // the most corners of a segment a wavefront takes
constexpr int kSimplifyLdsPoints = 2048;    // the most corners whose state a workgroup keeps in LDS

enum SimplifyFlag {
  SIMPLIFY_FLAG_RANGE = 1,   // a segment, a vertex or a count was out of range
};

// Written by the simplification kernels; read by the host at the end of a call.
struct SimplifyStatus {
  uint32_t vertices_out;     // after the joint pass
  uint32_t vertices_kept;    // after the recursion
  uint32_t collapsed, single_closed, max_rounds, longest_in;
  uint32_t long_segments;    // segments of more than kSimplifyWavePoints corners
  uint32_t flags;
};

// The mesh's records and vertices (n_segments, slots - n_segments) and the stage's blocks.  A segment of c
// vertices keeps at most c + 1: segment s has the c + 1 slots from first_vertex + s on, of `slots` in all.
// Per slot: kept, kseg (the slot's segment, all ones where nothing was kept), lo, hi and two words of best (the
// state of a segment of more than kSimplifyLdsPoints corners).  Per segment: kcount (vertices kept), rounds,
// sflag (1: collapsed), long_list.
struct SimplifyView {
  const int32_t* segments;
  const int2* vertices;
  uint32_t n_segments, slots;
  double eps;                // (double)max_error, squared
  uint32_t threshold;        // an open segment of fewer lattice points collapses; 0: none does
  int2* kept;
  uint32_t* kseg;
  uint32_t* lo;
  uint32_t* hi;
  unsigned long long* best;
  uint32_t* kcount;
  uint32_t* rounds;
  uint32_t* sflag;
  uint32_t* long_list;
};

// The collapse rule, the sweeps and the rounds of every segment; kept, kseg, kcount, rounds, sflag.  3 launches:
// the clear of kseg, the wavefronts, the workgroups of the long segments.  status: cleared by the caller.
hipError_t SimplifyDp(const SimplifyView& m, SimplifyStatus* status, hipStream_t stream);
// The joint pass of every segment, in place in `kept`; ncount[s] = its new number of vertices.  1 launch.
hipError_t SimplifyClean(const SimplifyView& m, uint32_t* ncount, hipStream_t stream);
// nfirst = the scan of ncount, the vertices to their places, the records (n_segments of kMeshSegmentWords) and
// the counts of status.  3 launches, the scan counted as one.
hipError_t SimplifyTables(void* temp, size_t temp_bytes, const SimplifyView& m, const uint32_t* ncount, uint32_t* nfirst,
                          int32_t* segments_out, int32_t* vertices_out, SimplifyStatus* status, hipStream_t stream);

// ---- boundary distance (distance.hip): the squared distance to an edge set, the boundary benchmark ------

constexpr int kDistChunkRows = 32;        // rows of a column that one word of the edge set holds
constexpr int kBoundaryScoreWords = 4;    // vsg_render_boundary_score as int64 words
constexpr int32_t kDistanceNone = 0x7fffffff;

enum DistFlag {
  DIST_FLAG_RANGE = 1,   // a value of the persistence plane was outside [0, levels]
};

// Written by the distance kernels; read by the host after the classify pass and at the end of a call.
struct DistStatus {
  unsigned long long edge_pixels;   // pixels of the classified plane's edge set
  uint32_t max_distance;            // the largest finite value k_dist_rows wrote
  uint32_t flags;
};

// Chunks of kDistChunkRows rows in a frame of `height` rows; floor(sqrt(tolerance_sq)).
int DistChunks(int height);
int DistRadius(int tolerance_sq);
// The edge set of the H x W plane (rows `pitch` values apart): the pixels that differ from their in-frame
// right or below neighbour, every value counting (clamp: all negative values as one).  words[c * W + x] has
// bit r set when (x, kDistChunkRows * c + r) is one, DistChunks(height) x W words, every one written;
// status->edge_pixels += their number.
void LaunchDistClassify(const int32_t* plane, size_t pitch, int width, int height, bool clamp, uint32_t* words,
                        DistStatus* status, hipStream_t stream);
// gsq[y * W + x] = the square of the vertical distance from (x, y) to the nearest pixel of the edge set in
// column x, kDistanceNone when the column has none.
void LaunchDistColumns(const uint32_t* words, int width, int height, int32_t* gsq, hipStream_t stream);
// out[y * W + x] = min over u of (x - u)^2 + gsq[y * W + u], kDistanceNone when the row of gsq has nothing
// else; status->max_distance = the largest finite one.  The row is staged in dynamic LDS: width * 4 bytes and
// 4 for every 32 columns.
hipError_t LaunchDistRows(const int32_t* gsq, int width, int height, int32_t* out, DistStatus* status,
                          hipStream_t stream);
// hist_all[v] += 1 for every pixel of q (rows W apart) with v = q > 0, hist_near[v] += 1 for those with
// d <= tolerance_sq as well (d null: none, hist_near is not looked at).  levels + 1 entries each.
void LaunchDistMatch(const int32_t* q, const int32_t* d, int width, int height, int levels, int tolerance_sq,
                     uint32_t* hist_all, uint32_t* hist_near, DistStatus* status, hipStream_t stream);
// hist[m] += 1 for every pixel of the edge set `words` with m = max of q over the pixels at most
// sqrt(tolerance_sq) away > 0.  tolerance_sq in [0, 4096].
void LaunchDistDisc(const int32_t* q, const uint32_t* words, int width, int height, int levels, int tolerance_sq,
                    uint32_t* hist, DistStatus* status, hipStream_t stream);
// scores[l] = {sum over p > l of hist_all[p], of hist_near[p], status->edge_pixels, sum of hist_disc[p]} as
// int64, l in [0, levels).
void LaunchDistScores(const uint32_t* hist_all, const uint32_t* hist_near, const uint32_t* hist_disc, int levels,
                      const DistStatus* status, long long* scores, hipStream_t stream);

// ---- volume session (volume.hip): a level's regions accumulated over frames ---------------------------------

constexpr size_t kVolumeRowBytes = 152;   // vsg_render_volume_row
constexpr size_t kVolumeColBytes = 48;    // vsg_render_volume_col
constexpr size_t kVolumePairBytes = 24;   // vsg_render_volume_pair
constexpr size_t kVolumeGeoBytes = 40;    // what a region of a frame gathers: area, two sums, the box

enum VolumeFlag {
  VOLUME_FLAG_RANGE = 1,   // a record, a key or a slot was out of range, or the frame's lists disagree
};

// Written by the volume kernels; read by the host after the merge of an add and at the end of a table call.
struct VolumeStatus {
  unsigned long long covered;             // sum of the areas of the frame's regions
  uint32_t new_rows, new_cols, new_pairs;   // keys the merge did not find
  uint32_t flags;
};

// Area, sum of x, sum of y and box of every record of the interval list (rank[i] - 1 is the record of interval
// i, records contiguous).  geo: `capacity` entries of kVolumeGeoBytes, cleared to zero before.
void LaunchVolumeGeometry(const Interval* intervals, const uint32_t* rank, uint32_t n, uint32_t capacity, void* geo,
                          VolumeStatus* status, hipStream_t stream);

// One frame's lists on the device.  regions: kLevelRegionWords per region, word 0 its id.  colors (may be null):
// kLevelColorWords per region.  overlap_rows / _cols / _pairs (null without labels): the overlap table's.
struct VolumeFrame {
  int frame;
  const int32_t* regions;
  const void* geo;
  const int32_t* colors;
  const int32_t* overlap_rows;
  uint32_t n_rows;
  const int32_t* overlap_cols;
  uint32_t n_cols;
  const int32_t* overlap_pairs;
  uint32_t n_pairs;
};

// The session's three tables: n sorted keys and their records, room for cap of each.
struct VolumeTables {
  unsigned long long* row_keys;
  void* rows;
  uint32_t n_rows, cap_rows;
  unsigned long long* col_keys;
  void* cols;
  uint32_t n_cols, cap_cols;
  unsigned long long* pair_keys;
  void* pairs;
  uint32_t n_pairs, cap_pairs;
};

// Adds the frame's records to the tables: a key that is there is added to in place, a new one is written behind
// the sorted part, n + status->new_* entries afterwards.  Returns the number of launches (one per non-empty list).
int LaunchVolumeMerge(const VolumeFrame& frame, const VolumeTables& tables, VolumeStatus* status, hipStream_t stream);
// perm[i] = i.
void LaunchVolumeIota(uint32_t* perm, uint32_t n, hipStream_t stream);
// dst record i = src record perm[i]; record_bytes is a multiple of 8.
void LaunchVolumeGather(const void* src, void* dst, const uint32_t* perm, uint32_t n, size_t record_bytes,
                        hipStream_t stream);
// rows, cols, pairs: copies of the tables' records; fills first_pair, num_pairs, best_label and best_count of the
// rows, num_pairs, best_row and best_count of the columns, row and col of the pairs.  Returns the launches.
int LaunchVolumeReadout(const VolumeTables& tables, void* rows, void* cols, void* pairs, VolumeStatus* status,
                        hipStream_t stream);

// ---- tree cut (tree_cut.hip): the best non-horizontal cut of the hierarchy ---------------------------------

constexpr int kCutNodeWords = 12;   // vsg_render_cut_node as int32 words

enum CutFlag {
  CUT_FLAG_RANGE = 1,        // a leaf, a key, a node or a record was out of range
  CUT_FLAG_GAIN_ORDER = 2,   // the gain table is not strictly ascending by (level, id)
  CUT_FLAG_GAIN_RANGE = 4,   // a gain of the table is beyond +-2^32
};

// Written by the cut kernels; read by the host after the lift and after the records.
struct CutStatus {
  uint32_t flags;
  uint32_t tree_nodes;          // nodes of all levels
  uint32_t cut_nodes, pad;      // selected nodes
  long long total;              // sum of their gains
  unsigned long long covered;   // sum of their areas
};

// vsg_render_cut_gain.
struct CutGain {
  int32_t level, id;
  long long gain;
};
static_assert(sizeof(CutGain) == 16, "read as is");

// The node table, one array per field, T entries each.  area, leaves, children, sum have to be zero before
// LaunchCutNodeTable.
struct CutNodes {
  int32_t *level, *id, *parent, *best_label, *best_count;
  uint32_t *area, *leaves, *children, *keep;
  long long *gain, *split;
  unsigned long long* sum;   // what the children have added so far
};

// list: R entries of `words` int32 by ascending id, word 0 the id, word area_word the area.  ids: the n_ids
// ascending ids the ancestor table has columns for.
void LaunchCutLeaves(const int32_t* list, uint32_t words, uint32_t area_word, uint32_t R, const int32_t* ids,
                     uint32_t n_ids, int32_t* leaf_id, uint32_t* leaf_area, uint32_t* leaf_col, CutStatus* status,
                     hipStream_t stream);
// keys[l * R + j] = l << 32 | A_l(leaf j), vals[i] = i; table as in persistence.hip, n_ids values a row.
void LaunchCutNodeKeys(const int32_t* leaf_id, const uint32_t* leaf_col, uint32_t R, const int32_t* table,
                       uint32_t n_ids, uint32_t L, unsigned long long* keys, uint32_t* vals, hipStream_t stream);
// map[l * R + j] = node; level_first[0 .. L]; status->tree_nodes.  vals, rank: of the L * R sorted keys.
void LaunchCutNodeMap(const uint32_t* vals, const uint32_t* rank, uint32_t R, uint32_t L, uint32_t* map,
                      uint32_t* level_first, CutStatus* status, hipStream_t stream);
void LaunchCutNodeTable(const unsigned long long* keys, const uint32_t* vals, const uint32_t* rank,
                        const uint32_t* map, const uint32_t* leaf_area, uint32_t R, uint32_t L, uint32_t T,
                        const CutNodes& nodes, hipStream_t stream);
// pairs: P vsg_render_overlap_pair of level 0.  keys[l * P + e] = node << label_bits | label, counts likewise.
void LaunchCutPairKeys(const int32_t* pairs, uint32_t P, const uint32_t* map, uint32_t R, uint32_t L, int label_bits,
                       unsigned long long* keys, uint32_t* counts, hipStream_t stream);
// Sorted keys with their counts and ranks -> best[node] = count << 31 | (2^31 - 1 - label) of the best label.
// sums (n) and best (T) have to be zero before.  Two launches.
void LaunchCutBest(const unsigned long long* keys, const uint32_t* counts, const uint32_t* rank, uint32_t n,
                   int label_bits, uint32_t T, uint32_t* sums, unsigned long long* best, CutStatus* status,
                   hipStream_t stream);
void LaunchCutGainLabels(const unsigned long long* best, uint32_t T, int64_t penalty, const CutNodes& nodes,
                         hipStream_t stream);
void LaunchCutGainCheck(const CutGain* gains, size_t n, CutStatus* status, hipStream_t stream);
void LaunchCutGainLookup(const CutGain* gains, size_t n, uint32_t T, const CutNodes& nodes, hipStream_t stream);
// The dynamic programme: all levels in one workgroup, or the nodes [first, end) of one level.
void LaunchCutDpBlock(const uint32_t* level_first, uint32_t L, const CutNodes& nodes, hipStream_t stream);
void LaunchCutDpLevel(uint32_t first, uint32_t end, const CutNodes& nodes, hipStream_t stream);
// leaf_node[j]: the selected node of leaf j; selected[node] = 1 for those (zero before).
void LaunchCutSelect(const uint32_t* map, uint32_t R, uint32_t L, uint32_t T, const uint32_t* keep,
                     uint32_t* leaf_node, uint32_t* selected, CutStatus* status, hipStream_t stream);
// place: the inclusive scan of selected.  records: room for `capacity`; status->cut_nodes, total, covered.
void LaunchCutRecords(const uint32_t* selected, const uint32_t* place, uint32_t T, uint32_t capacity,
                      const CutNodes& nodes, int32_t* records, CutStatus* status, hipStream_t stream);
// ids, out: W * H int32, rows W apart.
void LaunchCutPaint(const int32_t* ids, int W, int H, const int32_t* leaf_id, uint32_t R, const uint32_t* leaf_node,
                    const uint32_t* place, int32_t* out, CutStatus* status, hipStream_t stream);

}  // namespace vsg_render_impl

#endif  // VSG_RENDER_RENDER_H_
