// level.hip -- the regions of a hierarchy level from the filled id plane (gfx950): the device form of
// the reference's GetCompoundRegionRasterizations, RasterizationArea and
// ShapeMomentsFromRasterization (segment_util/segmentation_util.cpp:592-605, 644-693).
//
//   k_level_runs     one block per row: the maximal runs of equal id, as (id, position) keys and
//                    right ends; reads the plane once
//   radix sort       runs brought into (id, y, left_x) order, 64-bit key, 32-bit value
//   scan             rank of every run's region among the regions (a sum over segment heads)
//   k_level_table    one thread per sorted run: its interval {y, left_x, right_x, id}; a segment head
//                    also writes its region's id and first interval
//   k_level_moments  one wavefront per region: area, bounding box, and the reference's six f32 sums
//                    in interval order (also run per connected component, on the table of components.hip)
//   k_copy_lists     of lists.hip: regions and intervals to the caller's device memory, if the regions fit
//
// The moments' arithmetic is the reference's, operation for operation; every operation is rounded on
// its own (the file is compiled with -ffp-contract=off, and the rounding intrinsics say so again).
#include "render.h"
#include "render_device.h"

namespace vsg_render_impl {

namespace {

constexpr int kRunsBlock = 256;
constexpr int kWaves = kRunsBlock / 64;

// One block walks one row of the id plane in chunks of kRunsBlock pixels, a thread a pixel.  A pixel
// with an id is a run start when its left neighbour differs (or it is the row's first), a run end
// when its right neighbour differs (or it is the row's last).  The k-th start and the k-th end of a
// row belong to the same run, and at most one run is open at a chunk's end, so a chunk reserves one
// slot per start (one atomic per chunk); its ends go to those slots in order, the first of them to
// the slot carried over when a run was open.  A slot at or beyond `capacity` is not written and
// raises `overflow`; the count keeps counting.
__global__ __launch_bounds__(kRunsBlock) void k_level_runs(const int32_t* __restrict__ plane, int pitch, int W,
                                                           uint32_t capacity, unsigned long long* __restrict__ keys,
                                                           uint32_t* __restrict__ rights,
                                                           LevelStatus* __restrict__ status) {
  __shared__ int32_t s_id[kRunsBlock + 2];
  __shared__ uint32_t s_starts[kWaves], s_ends[kWaves];
  __shared__ uint32_t s_base, s_carry;
  const int y = blockIdx.x;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int32_t* row = plane + (size_t)y * pitch;
  bool open = false;   // block-uniform: a run of an earlier chunk has not ended yet
  for (int x0 = 0; x0 < W; x0 += kRunsBlock) {
    const int x = x0 + t;
    // columns outside the row count as uncovered: a run never continues across a row boundary
    s_id[t + 1] = x < W ? row[x] : -1;
    if (t == 0) s_id[0] = x0 > 0 ? row[x0 - 1] : -1;
    if (t == kRunsBlock - 1) s_id[kRunsBlock + 1] = x + 1 < W ? row[x + 1] : -1;
    __syncthreads();
    const int32_t id = s_id[t + 1];
    const bool start = id != -1 && (x == 0 || s_id[t] != id);
    const bool end = id != -1 && (x == W - 1 || s_id[t + 2] != id);
    const unsigned long long bs = __ballot(start), be = __ballot(end);
    if (lane == 0) {
      s_starts[wave] = (uint32_t)__popcll(bs);
      s_ends[wave] = (uint32_t)__popcll(be);
    }
    __syncthreads();
    uint32_t starts_before = 0, ends_before = 0, starts = 0, ends = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      if (w < wave) {
        starts_before += s_starts[w];
        ends_before += s_ends[w];
      }
      starts += s_starts[w];
      ends += s_ends[w];
    }
    if (t == 0 && starts) s_base = atomicAdd(&status->runs, starts);
    __syncthreads();
    const uint32_t base = s_base, carry = s_carry;   // read only where they were written
    const unsigned long long below = (1ull << lane) - 1;
    if (start) {
      const uint32_t slot = base + starts_before + (uint32_t)__popcll(bs & below);
      if (slot < capacity) {
        keys[slot] = (unsigned long long)(uint32_t)id << 32 | (uint32_t)(y * W + x);
      } else {
        status->overflow = 1u;
      }
    }
    if (end) {
      const uint32_t k = ends_before + (uint32_t)__popcll(be & below);   // k-th end of the chunk
      const uint32_t slot = open ? (k == 0 ? carry : base + k - 1) : base + k;
      if (slot < capacity) rights[slot] = (uint32_t)x;
    }
    // starts + open - ends runs are open now: 0 or 1
    const bool open_next = starts + (open ? 1u : 0u) > ends;
    __syncthreads();
    if (t == 0 && open_next && starts) s_carry = base + starts - 1;   // else the carried slot stays
    open = open_next;
  }
}

__device__ __forceinline__ bool IsHead(const unsigned long long* keys, uint32_t i) {
  return i == 0 || (uint32_t)(keys[i] >> 32) != (uint32_t)(keys[i - 1] >> 32);
}

// One thread per sorted run.  rank[i] = number of segment heads in [0, i]: the region of run i is
// rank[i] - 1.  n <= capacity of every array; a region index is below n.
__global__ __launch_bounds__(256) void k_level_table(const unsigned long long* __restrict__ keys,
                                                     const uint32_t* __restrict__ rights,
                                                     const uint32_t* __restrict__ rank, uint32_t n, int W,
                                                     uint32_t capacity_regions, int4* __restrict__ intervals,
                                                     int32_t* __restrict__ regions,
                                                     LevelStatus* __restrict__ status) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const unsigned long long key = keys[i];
  const int32_t id = (int32_t)(uint32_t)(key >> 32);
  const uint32_t pos = (uint32_t)key;
  intervals[i] = make_int4((int)(pos / (uint32_t)W), (int)(pos % (uint32_t)W), (int)rights[i], id);
  const uint32_t r = rank[i] - 1;
  if (IsHead(keys, i) && r < capacity_regions) {
    regions[(size_t)r * kLevelRegionWords + 0] = id;
    regions[(size_t)r * kLevelRegionWords + 1] = (int32_t)i;
  }
  if (i == n - 1) status->regions = r + 1;
}

__device__ __forceinline__ float LaneValue(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// One wavefront per region.  64 intervals at a time: every lane computes the six terms of its
// interval (they do not depend on each other), then the terms are added to the six sums one interval
// after the other, in interval order, as ShapeMomentsFromRasterization's loop does
// (segmentation_util.cpp:663-684).  The sums are wave-uniform.  Area and bounding box are integer
// reductions.
// The regions are the segments of any table of kWords int32 per entry whose word kFirst is the
// entry's first interval (a region of the level, or a connected component of one): the twelve words
// behind it are written, *count entries exist and *largest takes the most intervals of one.
template <int kWords, int kFirst>
__global__ __launch_bounds__(256) void k_level_moments(const int4* __restrict__ intervals, uint32_t n,
                                                       uint32_t capacity_regions, int32_t* __restrict__ regions,
                                                       const uint32_t* __restrict__ count,
                                                       uint32_t* __restrict__ largest) {
  const uint32_t r = (blockIdx.x * 256u + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  const uint32_t n_regions = *count;
  if (r >= n_regions || r >= capacity_regions) return;
  int32_t* out = regions + (size_t)r * kWords + (kFirst - 1);
  // one region per wavefront: both bounds are wave-uniform
  const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane(out[1]);
  const bool has_next = r + 1 < n_regions && r + 1 < capacity_regions;
  const uint32_t end = has_next ? (uint32_t)__builtin_amdgcn_readfirstlane(out[kWords + 1]) : n;
  if (first >= end || end > n) return;   // cannot happen; nothing outside the list is read

  float area_sum = 0.0f, mean_x = 0.0f, mean_y = 0.0f, moment_xx = 0.0f, moment_xy = 0.0f, moment_yy = 0.0f;
  int area = 0, min_x = 0x7fffffff, min_y = 0x7fffffff, max_x = -1, max_y = -1;
  for (uint32_t base = first; base < end; base += 64) {
    const uint32_t i = base + lane;
    const bool live = i < end;
    const int4 v = live ? intervals[i] : make_int4(0, 0, -1, 0);   // y, left_x, right_x, id
    const float m = (float)v.y, nn = (float)v.z, curr_y = (float)v.x;
    const float len = __fadd_rn(__fsub_rn(nn, m), 1.0f);
    const float center_x = (float)((double)__fadd_rn(nn, m) * 0.5);
    const float sum_x = __fmul_rn(center_x, len);
    const float sum_y = __fmul_rn(curr_y, len);
    const float t_xy = __fmul_rn(curr_y, sum_x);
    const float t_yy = __fmul_rn(curr_y, sum_y);
    // -m + 2 * m * m + n + 2 * m * n + 2 * n * n, left to right
    const float two_m = __fmul_rn(2.0f, m), two_n = __fmul_rn(2.0f, nn);
    float poly = __fadd_rn(-m, __fmul_rn(two_m, m));
    poly = __fadd_rn(poly, nn);
    poly = __fadd_rn(poly, __fmul_rn(two_m, nn));
    poly = __fadd_rn(poly, __fmul_rn(two_n, nn));
    const float t_xx = __fdiv_rn(__fmul_rn(len, poly), 6.0f);
    if (live) {
      area += v.z - v.y + 1;
      min_x = min(min_x, v.y);
      max_x = max(max_x, v.z);
      min_y = min(min_y, v.x);
      max_y = max(max_y, v.x);
    }
    const int count = (int)min(64u, end - base);   // wave-uniform
    for (int j = 0; j < count; ++j) {
      area_sum = __fadd_rn(area_sum, LaneValue(len, j));
      mean_x = __fadd_rn(mean_x, LaneValue(sum_x, j));
      mean_y = __fadd_rn(mean_y, LaneValue(sum_y, j));
      moment_xy = __fadd_rn(moment_xy, LaneValue(t_xy, j));
      moment_yy = __fadd_rn(moment_yy, LaneValue(t_yy, j));
      moment_xx = __fadd_rn(moment_xx, LaneValue(t_xx, j));
    }
  }
  area = WaveSum(area);
  min_x = WaveMin(min_x);
  min_y = WaveMin(min_y);
  max_x = WaveMax(max_x);
  max_y = WaveMax(max_y);
  if (lane == 0) {
    const float inv_area = __fdiv_rn(1.0f, area_sum);
    out[2] = (int32_t)(end - first);
    out[3] = area;
    out[4] = min_x;
    out[5] = min_y;
    out[6] = max_x;
    out[7] = max_y;
    out[8] = __float_as_int(area_sum);
    out[9] = __float_as_int(__fmul_rn(mean_x, inv_area));
    out[10] = __float_as_int(__fmul_rn(mean_y, inv_area));
    out[11] = __float_as_int(__fmul_rn(moment_xx, inv_area));
    out[12] = __float_as_int(__fmul_rn(moment_xy, inv_area));
    out[13] = __float_as_int(__fmul_rn(moment_yy, inv_area));
    atomicMax(largest, end - first);
  }
}

}  // namespace

void LaunchLevelRuns(const int32_t* plane, int pitch, int width, int height, uint32_t capacity,
                     unsigned long long* keys, uint32_t* rights, LevelStatus* status, hipStream_t stream) {
  hipLaunchKernelGGL(k_level_runs, dim3(height), dim3(kRunsBlock), 0, stream, plane, pitch, width, capacity, keys,
                     rights, status);
}

void LaunchLevelTable(const unsigned long long* keys_sorted, const uint32_t* rights_sorted, const uint32_t* rank,
                      uint32_t n, int width, uint32_t capacity_regions, Interval* intervals, int32_t* regions,
                      LevelStatus* status, hipStream_t stream) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_level_table, dim3((n + 255) / 256), dim3(256), 0, stream, keys_sorted, rights_sorted, rank, n,
                     width, capacity_regions, reinterpret_cast<int4*>(intervals), regions, status);
}

void LaunchLevelMoments(const Interval* intervals, uint32_t n, uint32_t capacity_regions, int32_t* regions,
                        LevelStatus* status, hipStream_t stream) {
  if (n == 0 || capacity_regions == 0) return;
  const uint32_t blocks = (capacity_regions + 3) / 4;   // a wavefront per region; regions <= capacity_regions
  hipLaunchKernelGGL((k_level_moments<kLevelRegionWords, 1>), dim3(blocks), dim3(256), 0, stream,
                     reinterpret_cast<const int4*>(intervals), n, capacity_regions, regions, &status->regions,
                     &status->largest);
}

void LaunchComponentMoments(const Interval* intervals, uint32_t n, uint32_t capacity_components,
                            int32_t* components, CompStatus* status, hipStream_t stream) {
  if (n == 0 || capacity_components == 0) return;
  const uint32_t blocks = (capacity_components + 3) / 4;
  hipLaunchKernelGGL((k_level_moments<kLevelComponentWords, 3>), dim3(blocks), dim3(256), 0, stream,
                     reinterpret_cast<const int4*>(intervals), n, capacity_components, components,
                     &status->components, &status->largest);
}

}  // namespace vsg_render_impl
