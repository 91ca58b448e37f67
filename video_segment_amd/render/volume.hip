// volume.hip -- a level's regions accumulated over frames: the supervoxel table of a volume session (gfx950).
//
// Input is what the level, colour and overlap pipelines leave on the device for one frame: the interval list
// {y, left_x, right_x, id} grouped by region with every interval's 1-based record (the scan of HeadFlag), the
// region table, the colour records, the overlap rows, columns and pairs.  The session keeps three tables, each
// a sorted array of 64-bit keys with one record per key: rows (key = id), columns (key = label) and pairs
// (key = id << 32 | label).  The records are the caller's records: vsg_render_volume_row, _col and _pair.
//
//   k_volume_geometry    a wavefront per slice of 64 intervals: area, sum of x (closed form per interval), sum
//                        of y and the box of every region, reduced by record as k_color_table does; a region
//                        inside one slice is stored, one that spans slices is combined with 64-bit integer
//                        atomics (add) and 32-bit integer atomics (max), which are order-free
//   k_volume_merge_*     a thread per record of the frame: binary search of its key in the sorted part of the
//                        table; a hit is added to in place (a frame's keys are distinct: no atomics), a miss
//                        takes a slot behind the sorted part and is counted in the status words
//   k_volume_iota,       the permutation the library radix sort carries with the keys of a table that got new
//   k_volume_gather      ones, and the records moved by it into the twin block, 8 bytes per thread
//   k_volume_rows_out    a thread per row: first_pair and num_pairs by two binary searches in the pairs' keys
//   k_volume_pairs_out   a thread per pair: row and col by binary search, the columns' num_pairs, and the
//                        largest count of its row and of its column with 64-bit integer atomics (max)
//   k_volume_best        a thread per pair: where its count is the largest of its row (column), its label (row)
//                        with a 32-bit integer atomic (min): ties go to the smallest
//
// Everything is integer arithmetic; no result depends on the order of execution.
#include "render.h"
#include "render_device.h"

namespace vsg_render_impl {

namespace {

constexpr int kVolumeBlock = 256;

struct VolumeRow {
  int32_t id, first_frame, last_frame, frames;
  int32_t min_x, min_y, max_x, max_y;
  int32_t first_pair, num_pairs, best_label, reserved0;
  long long volume, unlabelled, best_count;
  long long sum_x, sum_y, sum_t;
  long long sum[3], sum_sq[3];
  uint8_t lo[3], hi[3], reserved1[2];
};
static_assert(sizeof(VolumeRow) == kVolumeRowBytes, "vsg_render_volume_row");

struct VolumeCol {
  int32_t label, num_pairs, best_row, first_frame, last_frame, frames;
  long long volume, uncovered, best_count;
};
static_assert(sizeof(VolumeCol) == kVolumeColBytes, "vsg_render_volume_col");

struct VolumePair {
  int32_t row, col, label, frames;
  long long count;
};
static_assert(sizeof(VolumePair) == kVolumePairBytes, "vsg_render_volume_pair");

// What a region has gathered: minima as 0x7fffffff - min, so that the cleared (all zero) state is neutral for
// every field and all four extrema combine with a maximum.
struct GeoAcc {
  unsigned long long sum_x, sum_y, area;
  uint32_t inv_min_x, inv_min_y, max_x, max_y;
};
static_assert(sizeof(GeoAcc) == kVolumeGeoBytes, "sized by the host");

// The index of the first of n ascending keys that is not below `key`.
__device__ __forceinline__ uint32_t LowerBound(const unsigned long long* __restrict__ keys, uint32_t n,
                                               unsigned long long key) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (keys[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// One thread per interval, a wavefront per slice of 64; the segmented reduction of k_color_table.  `acc` has to
// be cleared to zero before.  A record at or beyond `capacity` raises VOLUME_FLAG_RANGE and is dropped.
__global__ __launch_bounds__(kVolumeBlock) void k_volume_geometry(const int4* __restrict__ intervals,
                                                                  const uint32_t* __restrict__ rank, uint32_t n,
                                                                  uint32_t capacity, GeoAcc* __restrict__ acc,
                                                                  VolumeStatus* __restrict__ status) {
  const uint32_t i = blockIdx.x * (uint32_t)kVolumeBlock + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool live = i < n;
  // a dead lane gets a record no live lane has: ranks are at least 1
  const uint32_t rec = live ? rank[i] - 1 : 0xffffffffu;
  unsigned long long sx = 0, sy = 0, area = 0;
  uint32_t inv_min_x = 0, inv_min_y = 0, max_x = 0, max_y = 0;
  if (live) {
    const int4 v = intervals[i];   // x = y, y = left_x, z = right_x
    const long long len = (long long)v.z - v.y + 1;
    if (len > 0 && v.x >= 0 && v.y >= 0) {
      area = (unsigned long long)len;
      sx = (unsigned long long)(((long long)v.y + v.z) * len / 2);   // (l + r) * len is even
      sy = (unsigned long long)((long long)v.x * len);
      inv_min_x = 0x7fffffffu - (uint32_t)v.y;
      inv_min_y = 0x7fffffffu - (uint32_t)v.x;
      max_x = (uint32_t)v.z;
      max_y = (uint32_t)v.x;
    }
  }
  const uint32_t slice = i - (uint32_t)lane;
  const uint32_t last = min(slice + 63u, n - 1u);
  const bool head = live && (lane == 0 || rank[i - 1] - 1 != rec);
  const bool open_before = live && lane == 0 && i > 0 && rank[i - 1] - 1 == rec;
  const bool open_behind = live && i == last && i + 1 < n && rank[i + 1] - 1 == rec;
  const unsigned long long heads = __ballot(head);
  const bool slice_open_behind = __ballot(open_behind) != 0ull;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o_rec = __shfl_down(rec, d);
    const bool take = lane + d < 64 && o_rec == rec;
    const unsigned long long o_sx = __shfl_down(sx, d), o_sy = __shfl_down(sy, d), o_area = __shfl_down(area, d);
    const uint32_t o_ix = __shfl_down(inv_min_x, d), o_iy = __shfl_down(inv_min_y, d);
    const uint32_t o_mx = __shfl_down(max_x, d), o_my = __shfl_down(max_y, d);
    if (take) {
      sx += o_sx;
      sy += o_sy;
      area += o_area;
      inv_min_x = max(inv_min_x, o_ix);
      inv_min_y = max(inv_min_y, o_iy);
      max_x = max(max_x, o_mx);
      max_y = max(max_y, o_my);
    }
  }
  if (!head) return;
  if (rec >= capacity) {
    atomicOr(&status->flags, (uint32_t)VOLUME_FLAG_RANGE);
    return;
  }
  const bool is_last_segment = lane == 63 || (heads >> (lane + 1)) == 0ull;
  const bool whole = !open_before && !(is_last_segment && slice_open_behind);
  GeoAcc* out = acc + rec;
  if (whole) {
    out->sum_x = sx;
    out->sum_y = sy;
    out->area = area;
    out->inv_min_x = inv_min_x;
    out->inv_min_y = inv_min_y;
    out->max_x = max_x;
    out->max_y = max_y;
  } else {
    atomicAdd(&out->sum_x, sx);
    atomicAdd(&out->sum_y, sy);
    atomicAdd(&out->area, area);
    atomicMax(&out->inv_min_x, inv_min_x);
    atomicMax(&out->inv_min_y, inv_min_y);
    atomicMax(&out->max_x, max_x);
    atomicMax(&out->max_y, max_y);
  }
}

// One thread per region of the frame.  A new row takes slot n_old + (its turn); the host has made room for
// n_old + n.  colors, overlap_rows: null when the session has none; record k of either belongs to region k.
__global__ __launch_bounds__(kVolumeBlock) void k_volume_merge_rows(
    const int32_t* __restrict__ regions, const GeoAcc* __restrict__ geo, const int32_t* __restrict__ colors,
    const int32_t* __restrict__ overlap_rows, uint32_t n, int frame, unsigned long long* __restrict__ keys,
    VolumeRow* __restrict__ rows, uint32_t n_old, uint32_t capacity, VolumeStatus* __restrict__ status) {
  const uint32_t k = blockIdx.x * (uint32_t)kVolumeBlock + threadIdx.x;
  unsigned long long covered = 0;
  if (k < n) {
    const int32_t id = regions[(size_t)k * kLevelRegionWords];
    const GeoAcc g = geo[k];
    const int32_t* c = colors ? colors + (size_t)k * kLevelColorWords : nullptr;
    const int32_t* o = overlap_rows ? overlap_rows + (size_t)k * kOverlapRowWords : nullptr;
    bool fine = id >= 0 && g.area > 0 && g.area <= 0x7fffffffull;
    if (c && (c[0] != id || (unsigned long long)(uint32_t)c[2] != g.area)) fine = false;
    if (o && (o[0] != id || (unsigned long long)(uint32_t)o[4] != g.area)) fine = false;
    uint32_t at = LowerBound(keys, n_old, (unsigned long long)(uint32_t)id);
    const bool hit = at < n_old && keys[at] == (unsigned long long)(uint32_t)id;
    if (fine && !hit) {
      at = n_old + atomicAdd(&status->new_rows, 1u);
      if (at >= capacity) fine = false;
    }
    if (!fine) {
      atomicOr(&status->flags, (uint32_t)VOLUME_FLAG_RANGE);
    } else {
      covered = g.area;
      VolumeRow r;
      if (hit) {
        r = rows[at];
      } else {
        keys[at] = (unsigned long long)(uint32_t)id;
        r.id = id;
        r.first_frame = frame;
        r.last_frame = frame;
        r.frames = 0;
        r.min_x = r.min_y = 0x7fffffff;
        r.max_x = r.max_y = -1;
        r.first_pair = r.num_pairs = 0;
        r.best_label = -1;
        r.reserved0 = 0;
        r.volume = r.unlabelled = r.best_count = 0;
        r.sum_x = r.sum_y = r.sum_t = 0;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          r.sum[ch] = r.sum_sq[ch] = 0;
          r.lo[ch] = c ? 255 : 0;
          r.hi[ch] = 0;
        }
        r.reserved1[0] = r.reserved1[1] = 0;
      }
      r.first_frame = min(r.first_frame, frame);
      r.last_frame = max(r.last_frame, frame);
      r.frames += 1;
      r.min_x = min(r.min_x, (int32_t)(0x7fffffffu - g.inv_min_x));
      r.min_y = min(r.min_y, (int32_t)(0x7fffffffu - g.inv_min_y));
      r.max_x = max(r.max_x, (int32_t)g.max_x);
      r.max_y = max(r.max_y, (int32_t)g.max_y);
      r.volume += (long long)g.area;
      r.sum_x += (long long)g.sum_x;
      r.sum_y += (long long)g.sum_y;
      r.sum_t += (long long)frame * (long long)g.area;
      if (o) r.unlabelled += (long long)o[5];
      if (c) {
        const uint32_t w16 = (uint32_t)c[16], w17 = (uint32_t)c[17];
        const uint32_t lo[3] = {w16 & 0xffu, (w16 >> 8) & 0xffu, (w16 >> 16) & 0xffu};
        const uint32_t hi[3] = {w16 >> 24, w17 & 0xffu, (w17 >> 8) & 0xffu};
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          r.sum[ch] += (long long)((unsigned long long)(uint32_t)c[4 + 2 * ch] |
                                   (unsigned long long)(uint32_t)c[5 + 2 * ch] << 32);
          r.sum_sq[ch] += (long long)((unsigned long long)(uint32_t)c[10 + 2 * ch] |
                                      (unsigned long long)(uint32_t)c[11 + 2 * ch] << 32);
          r.lo[ch] = (uint8_t)min((uint32_t)r.lo[ch], lo[ch]);
          r.hi[ch] = (uint8_t)max((uint32_t)r.hi[ch], hi[ch]);
        }
      }
      rows[at] = r;
    }
  }
  covered = WaveSum(covered);
  if ((threadIdx.x & 63) == 0 && covered) atomicAdd(&status->covered, covered);
}

// One thread per column of the frame's overlap table.
__global__ __launch_bounds__(kVolumeBlock) void k_volume_merge_cols(const int32_t* __restrict__ overlap_cols,
                                                                    uint32_t n, int frame,
                                                                    unsigned long long* __restrict__ keys,
                                                                    VolumeCol* __restrict__ cols, uint32_t n_old,
                                                                    uint32_t capacity,
                                                                    VolumeStatus* __restrict__ status) {
  const uint32_t k = blockIdx.x * (uint32_t)kVolumeBlock + threadIdx.x;
  if (k >= n) return;
  const int32_t* o = overlap_cols + (size_t)k * kOverlapColWords;   // label, area, uncovered
  const int32_t label = o[0];
  if (label < 0 || o[1] <= 0) {
    atomicOr(&status->flags, (uint32_t)VOLUME_FLAG_RANGE);
    return;
  }
  uint32_t at = LowerBound(keys, n_old, (unsigned long long)(uint32_t)label);
  const bool hit = at < n_old && keys[at] == (unsigned long long)(uint32_t)label;
  if (!hit) {
    at = n_old + atomicAdd(&status->new_cols, 1u);
    if (at >= capacity) {
      atomicOr(&status->flags, (uint32_t)VOLUME_FLAG_RANGE);
      return;
    }
  }
  VolumeCol c;
  if (hit) {
    c = cols[at];
  } else {
    keys[at] = (unsigned long long)(uint32_t)label;
    c.label = label;
    c.num_pairs = 0;
    c.best_row = -1;
    c.first_frame = c.last_frame = frame;
    c.frames = 0;
    c.volume = c.uncovered = c.best_count = 0;
  }
  c.first_frame = min(c.first_frame, frame);
  c.last_frame = max(c.last_frame, frame);
  c.frames += 1;
  c.volume += (long long)o[1];
  c.uncovered += (long long)o[2];
  cols[at] = c;
}

// One thread per pair of the frame's overlap table; its id is that of its row.
__global__ __launch_bounds__(kVolumeBlock) void k_volume_merge_pairs(const int32_t* __restrict__ overlap_pairs,
                                                                     const int32_t* __restrict__ overlap_rows,
                                                                     uint32_t n, uint32_t n_rows,
                                                                     unsigned long long* __restrict__ keys,
                                                                     VolumePair* __restrict__ pairs, uint32_t n_old,
                                                                     uint32_t capacity,
                                                                     VolumeStatus* __restrict__ status) {
  const uint32_t k = blockIdx.x * (uint32_t)kVolumeBlock + threadIdx.x;
  if (k >= n) return;
  const int32_t* o = overlap_pairs + (size_t)k * kOverlapPairWords;   // row, col, label, count
  const uint32_t row = (uint32_t)o[0];
  const int32_t label = o[2], count = o[3];
  const int32_t id = row < n_rows ? overlap_rows[(size_t)row * kOverlapRowWords] : -1;
  if (id < 0 || label < 0 || count <= 0) {
    atomicOr(&status->flags, (uint32_t)VOLUME_FLAG_RANGE);
    return;
  }
  const unsigned long long key = (unsigned long long)(uint32_t)id << 32 | (uint32_t)label;
  uint32_t at = LowerBound(keys, n_old, key);
  const bool hit = at < n_old && keys[at] == key;
  if (!hit) {
    at = n_old + atomicAdd(&status->new_pairs, 1u);
    if (at >= capacity) {
      atomicOr(&status->flags, (uint32_t)VOLUME_FLAG_RANGE);
      return;
    }
  }
  VolumePair p;
  if (hit) {
    p = pairs[at];
  } else {
    keys[at] = key;
    p.row = p.col = 0;
    p.label = label;
    p.frames = 0;
    p.count = 0;
  }
  p.frames += 1;
  p.count += (long long)count;
  pairs[at] = p;
}

__global__ __launch_bounds__(kVolumeBlock) void k_volume_iota(uint32_t* __restrict__ perm, uint32_t n) {
  const uint32_t i = blockIdx.x * (uint32_t)kVolumeBlock + threadIdx.x;
  if (i < n) perm[i] = i;
}

// dst record i = src record perm[i]; records of `words` 8-byte words, a thread per word.
__global__ __launch_bounds__(kVolumeBlock) void k_volume_gather(const unsigned long long* __restrict__ src,
                                                                unsigned long long* __restrict__ dst,
                                                                const uint32_t* __restrict__ perm, uint32_t n,
                                                                uint32_t words) {
  const unsigned long long t = (unsigned long long)blockIdx.x * kVolumeBlock + threadIdx.x;
  if (t >= (unsigned long long)n * words) return;
  const uint32_t i = (uint32_t)(t / words), w = (uint32_t)(t % words);
  const uint32_t from = perm[i];
  if (from < n) dst[t] = src[(size_t)from * words + w];
}

// One thread per row of the copy: its slice of the pairs.
__global__ __launch_bounds__(kVolumeBlock) void k_volume_rows_out(const unsigned long long* __restrict__ row_keys,
                                                                  uint32_t n_rows,
                                                                  const unsigned long long* __restrict__ pair_keys,
                                                                  uint32_t n_pairs, VolumeRow* __restrict__ rows) {
  const uint32_t k = blockIdx.x * (uint32_t)kVolumeBlock + threadIdx.x;
  if (k >= n_rows) return;
  const unsigned long long id = row_keys[k];
  const uint32_t first = LowerBound(pair_keys, n_pairs, id << 32);
  const uint32_t end = LowerBound(pair_keys, n_pairs, (id + 1) << 32);
  rows[k].first_pair = (int32_t)first;
  rows[k].num_pairs = (int32_t)(end - first);
}

// One thread per pair of the copy: row, col, and what its row and column gather with order-free atomics.
__global__ __launch_bounds__(kVolumeBlock) void k_volume_pairs_out(
    const unsigned long long* __restrict__ pair_keys, uint32_t n_pairs,
    const unsigned long long* __restrict__ row_keys, uint32_t n_rows,
    const unsigned long long* __restrict__ col_keys, uint32_t n_cols, VolumeRow* __restrict__ rows,
    VolumeCol* __restrict__ cols, VolumePair* __restrict__ pairs, VolumeStatus* __restrict__ status) {
  const uint32_t j = blockIdx.x * (uint32_t)kVolumeBlock + threadIdx.x;
  if (j >= n_pairs) return;
  const unsigned long long key = pair_keys[j];
  const unsigned long long id = key >> 32, label = key & 0xffffffffull;
  const uint32_t row = LowerBound(row_keys, n_rows, id);
  const uint32_t col = LowerBound(col_keys, n_cols, label);
  if (row >= n_rows || row_keys[row] != id || col >= n_cols || col_keys[col] != label) {
    atomicOr(&status->flags, (uint32_t)VOLUME_FLAG_RANGE);
    return;
  }
  pairs[j].row = (int32_t)row;
  pairs[j].col = (int32_t)col;
  const unsigned long long count = (unsigned long long)pairs[j].count;
  atomicMax(reinterpret_cast<unsigned long long*>(&rows[row].best_count), count);
  atomicMax(reinterpret_cast<unsigned long long*>(&cols[col].best_count), count);
  atomicAdd(&cols[col].num_pairs, 1);
}

// One thread per pair of the copy, after k_volume_pairs_out: best_label and best_row start as -1, the largest
// unsigned number.
__global__ __launch_bounds__(kVolumeBlock) void k_volume_best(uint32_t n_pairs, uint32_t n_rows, uint32_t n_cols,
                                                              VolumeRow* __restrict__ rows,
                                                              VolumeCol* __restrict__ cols,
                                                              const VolumePair* __restrict__ pairs) {
  const uint32_t j = blockIdx.x * (uint32_t)kVolumeBlock + threadIdx.x;
  if (j >= n_pairs) return;
  const VolumePair p = pairs[j];
  if ((uint32_t)p.row >= n_rows || (uint32_t)p.col >= n_cols) return;   // flagged by k_volume_pairs_out
  if (p.count == rows[p.row].best_count) {
    atomicMin(reinterpret_cast<uint32_t*>(&rows[p.row].best_label), (uint32_t)p.label);
  }
  if (p.count == cols[p.col].best_count) {
    atomicMin(reinterpret_cast<uint32_t*>(&cols[p.col].best_row), (uint32_t)p.row);
  }
}

dim3 GridFor(unsigned long long threads) { return dim3((unsigned)((threads + kVolumeBlock - 1) / kVolumeBlock)); }

}  // namespace

void LaunchVolumeGeometry(const Interval* intervals, const uint32_t* rank, uint32_t n, uint32_t capacity, void* geo,
                          VolumeStatus* status, hipStream_t stream) {
  if (n == 0 || capacity == 0) return;
  hipLaunchKernelGGL(k_volume_geometry, GridFor(n), dim3(kVolumeBlock), 0, stream,
                     reinterpret_cast<const int4*>(intervals), rank, n, capacity, static_cast<GeoAcc*>(geo), status);
}

int LaunchVolumeMerge(const VolumeFrame& f, const VolumeTables& t, VolumeStatus* status, hipStream_t stream) {
  int launches = 0;
  if (f.n_rows) {
    hipLaunchKernelGGL(k_volume_merge_rows, GridFor(f.n_rows), dim3(kVolumeBlock), 0, stream, f.regions,
                       static_cast<const GeoAcc*>(f.geo), f.colors, f.overlap_rows, f.n_rows, f.frame, t.row_keys,
                       static_cast<VolumeRow*>(t.rows), t.n_rows, t.cap_rows, status);
    ++launches;
  }
  if (f.n_cols) {
    hipLaunchKernelGGL(k_volume_merge_cols, GridFor(f.n_cols), dim3(kVolumeBlock), 0, stream, f.overlap_cols, f.n_cols,
                       f.frame, t.col_keys, static_cast<VolumeCol*>(t.cols), t.n_cols, t.cap_cols, status);
    ++launches;
  }
  if (f.n_pairs) {
    hipLaunchKernelGGL(k_volume_merge_pairs, GridFor(f.n_pairs), dim3(kVolumeBlock), 0, stream, f.overlap_pairs,
                       f.overlap_rows, f.n_pairs, f.n_rows, t.pair_keys, static_cast<VolumePair*>(t.pairs), t.n_pairs,
                       t.cap_pairs, status);
    ++launches;
  }
  return launches;
}

void LaunchVolumeIota(uint32_t* perm, uint32_t n, hipStream_t stream) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_volume_iota, GridFor(n), dim3(kVolumeBlock), 0, stream, perm, n);
}

void LaunchVolumeGather(const void* src, void* dst, const uint32_t* perm, uint32_t n, size_t record_bytes,
                        hipStream_t stream) {
  if (n == 0) return;
  const uint32_t words = (uint32_t)(record_bytes / 8);
  hipLaunchKernelGGL(k_volume_gather, GridFor((unsigned long long)n * words), dim3(kVolumeBlock), 0, stream,
                     static_cast<const unsigned long long*>(src), static_cast<unsigned long long*>(dst), perm, n,
                     words);
}

int LaunchVolumeReadout(const VolumeTables& t, void* rows, void* cols, void* pairs, VolumeStatus* status,
                        hipStream_t stream) {
  int launches = 0;
  if (t.n_rows) {
    hipLaunchKernelGGL(k_volume_rows_out, GridFor(t.n_rows), dim3(kVolumeBlock), 0, stream, t.row_keys, t.n_rows,
                       t.pair_keys, t.n_pairs, static_cast<VolumeRow*>(rows));
    ++launches;
  }
  if (t.n_pairs) {
    hipLaunchKernelGGL(k_volume_pairs_out, GridFor(t.n_pairs), dim3(kVolumeBlock), 0, stream, t.pair_keys, t.n_pairs,
                       t.row_keys, t.n_rows, t.col_keys, t.n_cols, static_cast<VolumeRow*>(rows),
                       static_cast<VolumeCol*>(cols), static_cast<VolumePair*>(pairs), status);
    hipLaunchKernelGGL(k_volume_best, GridFor(t.n_pairs), dim3(kVolumeBlock), 0, stream, t.n_pairs, t.n_rows, t.n_cols,
                       static_cast<VolumeRow*>(rows), static_cast<VolumeCol*>(cols),
                       static_cast<const VolumePair*>(pairs));
    launches += 2;
  }
  return launches;
}

}  // namespace vsg_render_impl
