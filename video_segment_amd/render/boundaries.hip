// boundaries.hip -- the N4 boundary pixels of every group of an int32 plane (gfx950): the device form
// of the reference's GetBoundary (segment_util/segmentation_boundary.cpp:78-179) for all regions of a
// hierarchy level, or all their connected components, at once.  The plane is the id plane of
// vsg_render_id_image or the label image of vsg_render_level_components; -1 is "no group" and so is
// every position outside the frame.
//
//   k_bound_classify<count>  one block per row of the padded (W + 2) x (H + 2) grid: how many keys the
//                            row emits; one add per block
//   k_bound_classify<emit>   the same walk: the keys group << 32 | padded position, in no order; one
//                            add per block and step of 256 positions reserves their slots
//   radix sort               keys only, into (group, y, x) order
//   scan                     rank of every key's group among the groups (HeadFlag of render_scan.h)
//   k_bound_table            one thread per sorted key: its point {x, y}; a segment head also writes
//                            its record's id, component and first point
//   k_bound_finish           one thread per record: its number of points; the largest of them
//   k_copy_lists             of lists.hip: records and points to the caller's device memory, if the
//                            records fit
//
// inner: a position with P = g >= 0 and a neighbour != g emits (g, position).  outer: a position emits
// (g, position) for every distinct g >= 0 among its four neighbours that is not its own value; the
// neighbours are compared pairwise, so a position flanked by one group on several sides emits once.
// Keys are unique, which leaves the order of the slots free.
#include "render.h"
#include "render_device.h"

namespace vsg_render_impl {

namespace {

constexpr int kBoundBlock = 256;
constexpr int kBoundWaves = kBoundBlock / 64;

// One block walks padded row blockIdx.x (frame row y = blockIdx.x - 1) in steps of kBoundBlock padded
// positions, a thread a position.  The row itself goes through LDS with a halo of one position on each
// side; the rows above and below are read by the thread that needs them.  Positions beyond the padded
// row read -1 everywhere and emit nothing.
template <bool kEmit, bool kOuter>
__global__ __launch_bounds__(kBoundBlock) void k_bound_classify(const int32_t* __restrict__ plane, int W, int H,
                                                                uint32_t capacity,
                                                                unsigned long long* __restrict__ keys,
                                                                BoundStatus* __restrict__ status) {
  __shared__ int32_t s_row[kBoundBlock + 2];
  __shared__ uint32_t s_wave[kBoundWaves];
  __shared__ uint32_t s_base;
  const int py = blockIdx.x, y = py - 1;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int PW = W + 2;
  const unsigned long long below = (1ull << lane) - 1;
  uint32_t counted = 0;   // count only: keys of this thread over all steps
  for (int px0 = 0; px0 < PW; px0 += kBoundBlock) {
    const int px = px0 + t, x = px - 1;
    s_row[t + 1] = PlaneAt(plane, W, H, x, y);
    if (t == 0) s_row[0] = PlaneAt(plane, W, H, x - 1, y);
    if (t == kBoundBlock - 1) s_row[kBoundBlock + 1] = PlaneAt(plane, W, H, x + 1, y);
    __syncthreads();
    const int32_t c = s_row[t + 1], left = s_row[t], right = s_row[t + 2];
    const int32_t up = PlaneAt(plane, W, H, x, y - 1), down = PlaneAt(plane, W, H, x, y + 1);
    // the up to four groups this position emits a key for
    int32_t group[4];
    bool emit[4];
    if (kOuter) {
      group[0] = up;
      group[1] = left;
      group[2] = right;
      group[3] = down;
      emit[0] = up >= 0 && up != c;
      emit[1] = left >= 0 && left != c && left != up;
      emit[2] = right >= 0 && right != c && right != up && right != left;
      emit[3] = down >= 0 && down != c && down != up && down != left && down != right;
    } else {
      group[0] = c;
      emit[0] = c >= 0 && (up != c || left != c || right != c || down != c);
      emit[1] = emit[2] = emit[3] = false;
    }
    constexpr int kSlots = kOuter ? 4 : 1;
    if (!kEmit) {
#pragma unroll
      for (int j = 0; j < kSlots; ++j) counted += emit[j] ? 1u : 0u;
      __syncthreads();   // s_row is rewritten by the next step
      continue;
    }
    // rank within the wavefront: the keys of slot j of all lanes come after those of slots before j
    uint32_t offset[4], in_wave = 0;
#pragma unroll
    for (int j = 0; j < kSlots; ++j) {
      const unsigned long long b = __ballot(emit[j]);
      offset[j] = in_wave + (uint32_t)__popcll(b & below);
      in_wave += (uint32_t)__popcll(b);
    }
    uint32_t before;
    if (BlockReserve<kBoundWaves>(in_wave, s_wave, &s_base, &status->emitted, &before)) {
      const uint32_t base = s_base;
      const uint32_t pos = (uint32_t)py * (uint32_t)PW + (uint32_t)px;
#pragma unroll
      for (int j = 0; j < kSlots; ++j) {
        if (!emit[j]) continue;
        const uint32_t slot = base + before + offset[j];
        if (slot < capacity) keys[slot] = (unsigned long long)(uint32_t)group[j] << 32 | pos;
        else atomicOr(&status->flags, (uint32_t)BOUND_FLAG_OVERFLOW);
      }
    }
  }
  if (!kEmit) {
    counted = WaveSum(counted);
    if (lane == 0) s_wave[wave] = counted;
    __syncthreads();
    if (t == 0) {
      uint32_t total = 0;
#pragma unroll
      for (int w = 0; w < kBoundWaves; ++w) total += s_wave[w];
      if (total) atomicAdd(&status->points, (unsigned long long)total);
    }
  }
}

// One thread per sorted key i < n.  rank[i] = number of segment heads in [0, i].  What the sort hands
// back is checked before it is used as an index: a position outside the padded grid, a group above
// max_group or a record without a slot raises a flag, and nothing is written for it but the point
// slot i of the key itself.  comp_table: null, or the component table (kLevelComponentWords words an
// entry, id and component in words 0 and 1) the groups are indices of.
__global__ __launch_bounds__(256) void k_bound_table(const unsigned long long* __restrict__ keys,
                                                     const uint32_t* __restrict__ rank, uint32_t n, int W, int H,
                                                     uint32_t max_group, uint32_t capacity_records,
                                                     const int32_t* __restrict__ comp_table,
                                                     int2* __restrict__ points, int32_t* __restrict__ records,
                                                     BoundStatus* __restrict__ status) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const unsigned long long key = keys[i];
  const uint32_t group = (uint32_t)(key >> 32), pos = (uint32_t)key;
  const uint32_t PW = (uint32_t)W + 2, PH = (uint32_t)H + 2;
  const uint32_t py = pos / PW, px = pos % PW;
  const uint32_t r = rank[i] - 1;
  const bool good = py < PH && group <= max_group && r < capacity_records;
  if (!good) atomicOr(&status->flags, (uint32_t)BOUND_FLAG_RANGE);
  points[i] = good ? make_int2((int)px - 1, (int)py - 1) : make_int2(0, 0);
  const bool head = i == 0 || (uint32_t)(keys[i - 1] >> 32) != group;
  if (head && good) {
    int32_t* out = records + (size_t)r * kLevelBoundaryWords;
    if (comp_table) {
      // every component has a boundary point: the r-th group is component r
      if (r != group) atomicOr(&status->flags, (uint32_t)BOUND_FLAG_RANGE);
      out[0] = comp_table[(size_t)group * kLevelComponentWords + 0];
      out[1] = comp_table[(size_t)group * kLevelComponentWords + 1];
    } else {
      out[0] = (int32_t)group;
      out[1] = -1;
    }
    out[2] = (int32_t)i;
  }
  if (i == n - 1) status->boundaries = r + 1;
}

__global__ __launch_bounds__(256) void k_bound_finish(int32_t* __restrict__ records, uint32_t n,
                                                      uint32_t capacity_records, BoundStatus* __restrict__ status) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  const uint32_t n_records = status->boundaries;
  uint32_t mine = 0;
  if (r < n_records && r < capacity_records) {
    int32_t* out = records + (size_t)r * kLevelBoundaryWords;
    const uint32_t first = (uint32_t)out[2];
    const uint32_t end = r + 1 < n_records && r + 1 < capacity_records ? (uint32_t)out[kLevelBoundaryWords + 2] : n;
    mine = end > first && end <= n ? end - first : 0u;
    if (!mine) atomicOr(&status->flags, (uint32_t)BOUND_FLAG_RANGE);
    out[3] = (int32_t)mine;
  }
  mine = WaveMax(mine);
  if ((threadIdx.x & 63) == 0 && mine) atomicMax(&status->largest, mine);
}

}  // namespace

void LaunchBoundClassify(const int32_t* plane, int width, int height, bool outer, bool emit, uint32_t capacity,
                         unsigned long long* keys, BoundStatus* status, hipStream_t stream) {
  const dim3 grid(height + 2), block(kBoundBlock);
  if (emit && outer) {
    hipLaunchKernelGGL((k_bound_classify<true, true>), grid, block, 0, stream, plane, width, height, capacity, keys,
                       status);
  } else if (emit) {
    hipLaunchKernelGGL((k_bound_classify<true, false>), grid, block, 0, stream, plane, width, height, capacity, keys,
                       status);
  } else if (outer) {
    hipLaunchKernelGGL((k_bound_classify<false, true>), grid, block, 0, stream, plane, width, height, 0u, nullptr,
                       status);
  } else {
    hipLaunchKernelGGL((k_bound_classify<false, false>), grid, block, 0, stream, plane, width, height, 0u, nullptr,
                       status);
  }
}

void LaunchBoundTable(const unsigned long long* keys_sorted, const uint32_t* rank, uint32_t n, int width, int height,
                      uint32_t max_group, uint32_t capacity_records, const int32_t* comp_table, int32_t* points,
                      int32_t* records, BoundStatus* status, hipStream_t stream) {
  if (n == 0 || capacity_records == 0) return;
  hipLaunchKernelGGL(k_bound_table, dim3((n + 255) / 256), dim3(256), 0, stream, keys_sorted, rank, n, width, height,
                     max_group, capacity_records, comp_table, reinterpret_cast<int2*>(points), records, status);
  // the number of records is on the device only: a thread per slot, all but the first
  // status->boundaries of them leave at once
  hipLaunchKernelGGL(k_bound_finish, dim3((capacity_records + 255) / 256), dim3(256), 0, stream, records, n,
                     capacity_records, status);
}

}  // namespace vsg_render_impl
