// colors.hip -- per-group colour sums of a hierarchy level and the mean-colour interval list (gfx950).
//
// Input is what the level and component pipelines leave on the device: the interval list
// {y, left_x, right_x, id} grouped by record in record order, and the 1-based record of every interval
// (the scan of HeadFlag or LabelHead).  The plane P is not read again; the frame F is read once.
//
//   k_color_runs       a wavefront per 64 intervals (fewer when the list is short, so that the chip is
//                      filled all the same): one partial per interval (three sums, three sums of
//                      squares, packed minima and maxima); long intervals by all lanes, short ones by
//                      their own lane, as k_render_fill splits its work
//   k_color_table      a wavefront per slice of 64 intervals: segmented 64-bit reduction by record; a
//                      record that lies inside one slice is stored, one that spans slices is combined with
//                      64-bit integer atomics (add) and 32-bit integer atomics (max), which are order-free
//   k_color_finish     a thread per record: the caller's 72-byte record with its rounded mean
//   k_color_intervals  a thread per interval: the interval with value = its record's packed mean, which
//                      k_render_fill and k_render_compose then turn into the picture
//
// Everything is integer arithmetic; no result depends on the order of execution.
#include "render.h"
#include "render_device.h"

namespace vsg_render_impl {

namespace {

constexpr int kColorBlock = 256;         // 4 wavefronts, up to 64 intervals each
constexpr int kLongColorInterval = 16;   // from this length on the whole wavefront sums one interval
constexpr uint32_t kColorWaves = 2048;   // the wavefronts k_color_runs wants before one takes more intervals

// Running sums of one interval (or of a lane's share of one).  A whole interval fits uint32: the frame
// is at most 10224 wide and 10224 * 255 * 255 < 2^32.  Indexed with constants only, so that it stays in
// registers.
struct Sums {
  uint32_t s[3], q[3], lo[3], hi[3];
};

__device__ __forceinline__ void Clear(Sums& a) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    a.s[c] = 0u;
    a.q[c] = 0u;
    a.lo[c] = 255u;
    a.hi[c] = 0u;
  }
}

template <int C>
__device__ __forceinline__ void AddByte(Sums& a, uint32_t v) {
  a.s[C] += v;
  a.q[C] += v * v;
  a.lo[C] = min(a.lo[C], v);
  a.hi[C] = max(a.hi[C], v);
}

__device__ __forceinline__ void AddPixel(Sums& a, const uint8_t* __restrict__ p) {
  AddByte<0>(a, p[0]);
  AddByte<1>(a, p[1]);
  AddByte<2>(a, p[2]);
}

// Four pixels whose first byte is 4-byte aligned: B G R B | G R B G | R B G R.
__device__ __forceinline__ void AddFourPixels(Sums& a, uint32_t w0, uint32_t w1, uint32_t w2) {
  AddByte<0>(a, w0 & 0xffu);
  AddByte<1>(a, (w0 >> 8) & 0xffu);
  AddByte<2>(a, (w0 >> 16) & 0xffu);
  AddByte<0>(a, w0 >> 24);
  AddByte<1>(a, w1 & 0xffu);
  AddByte<2>(a, (w1 >> 8) & 0xffu);
  AddByte<0>(a, (w1 >> 16) & 0xffu);
  AddByte<1>(a, w1 >> 24);
  AddByte<2>(a, w2 & 0xffu);
  AddByte<0>(a, (w2 >> 8) & 0xffu);
  AddByte<1>(a, (w2 >> 16) & 0xffu);
  AddByte<2>(a, w2 >> 24);
}

struct alignas(4) Dwords3 {
  uint32_t w[3];
};

// A wavefront takes per_wave intervals (a power of two up to 64), one per lane of its first per_wave
// lanes.  Intervals of kLongColorInterval pixels and more are summed one after the other by all 64 lanes
// and reduced across the lanes; the short ones are summed by their own lane.  ALIGNED: bgr and stride are multiples of 4; a long interval is then read as 12-byte
// groups of four pixels starting at a multiple of four pixels of its row (whose first byte is 4-byte
// aligned), the up to three pixels before and after by single lanes.  Otherwise a lane reads a pixel as
// three bytes.  An interval that is not inside the frame (there is none) is not read and gives the empty
// partial.
template <bool ALIGNED>
__global__ __launch_bounds__(kColorBlock) void k_color_runs(const int4* __restrict__ intervals, uint32_t n, int W,
                                                            int H, const uint8_t* __restrict__ bgr, size_t stride,
                                                            int per_wave, uint4* __restrict__ partials) {
  const int lane = threadIdx.x & 63;
  const uint32_t wave = (blockIdx.x * (uint32_t)kColorBlock + threadIdx.x) >> 6;
  const uint32_t waves = gridDim.x * (uint32_t)(kColorBlock / 64);
  for (unsigned long long base = (unsigned long long)wave * per_wave; base < n;
       base += (unsigned long long)waves * per_wave) {
    const unsigned long long i = base + lane;
    const bool mine_exists = lane < per_wave && i < n;
    // x = y, y = left_x, z = right_x; padding lanes hold an empty interval
    int4 v = mine_exists ? intervals[i] : make_int4(0, 0, -1, 0);
    if (v.x < 0 || v.x >= H || v.y < 0 || v.z >= W) v = make_int4(0, 0, -1, 0);
    const int len = v.z - v.y + 1;
    Sums mine;
    Clear(mine);
    unsigned long long todo = __ballot(len >= kLongColorInterval);
    while (todo) {   // wave-uniform: `todo` is a scalar
      const int j = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int y = __builtin_amdgcn_readlane(v.x, j);
      const int lx = __builtin_amdgcn_readlane(v.y, j);
      const int rx = __builtin_amdgcn_readlane(v.z, j);
      const uint8_t* row = bgr + (size_t)y * stride;
      Sums a;
      Clear(a);
      if (ALIGNED) {
        const int body = min((lx + 3) & ~3, rx + 1);        // first pixel of the 12-byte groups
        const int tail = max(body, (rx + 1) & ~3);          // first pixel behind them
        const int n_head = body - lx, n_tail = rx + 1 - tail;   // at most three each
        if (lane < n_head + n_tail) AddPixel(a, row + 3 * (size_t)(lane < n_head ? lx + lane : tail + lane - n_head));
        for (int g = body / 4 + lane; g < tail / 4; g += 64) {
          const Dwords3 d = *reinterpret_cast<const Dwords3*>(row + 12 * (size_t)g);
          AddFourPixels(a, d.w[0], d.w[1], d.w[2]);
        }
      } else {
        for (int x = lx + lane; x <= rx; x += 64) AddPixel(a, row + 3 * (size_t)x);
      }
#pragma unroll
      for (int s = 32; s > 0; s >>= 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          a.s[c] += __shfl_xor(a.s[c], s);
          a.q[c] += __shfl_xor(a.q[c], s);
          a.lo[c] = min(a.lo[c], __shfl_xor(a.lo[c], s));
          a.hi[c] = max(a.hi[c], __shfl_xor(a.hi[c], s));
        }
      }
      if (lane == j) mine = a;
    }
    if (len > 0 && len < kLongColorInterval) {
      const uint8_t* p = bgr + (size_t)v.x * stride + 3 * (size_t)v.y;
      for (int k = 0; k < len; ++k) AddPixel(mine, p + 3 * k);
    }
    if (mine_exists) {
      partials[2 * i] = make_uint4(mine.s[0], mine.s[1], mine.s[2], mine.q[0]);
      partials[2 * i + 1] = make_uint4(mine.q[1], mine.q[2], mine.lo[0] | mine.lo[1] << 8 | mine.lo[2] << 16,
                                       mine.hi[0] | mine.hi[1] << 8 | mine.hi[2] << 16);
    }
  }
}

// What a record has gathered: minima as 255 - min, so that the cleared (all zero) state is neutral for
// every field and both extrema combine with a maximum.
struct ColorAcc {
  unsigned long long sum[3], sum_sq[3];
  uint32_t area, count, inv_lo[3], hi[3];
};
static_assert(sizeof(ColorAcc) == kColorAccBytes, "sized by the host");

// One thread per interval, a wavefront per slice of 64.  The slice is reduced by record with a segmented
// suffix sum (records are contiguous in the list, so "the lane d further has my record" implies that
// every lane in between has it); the first lane of every segment then holds the segment's totals.  A
// record whose first and last interval are both in the slice is stored; any other is added to with
// atomics.  `acc` has to be cleared to zero before.  A record at or beyond `capacity` raises
// COLOR_FLAG_RANGE and is dropped.
__global__ __launch_bounds__(kColorBlock) void k_color_table(const int4* __restrict__ intervals,
                                                             const uint32_t* __restrict__ rank,
                                                             const uint4* __restrict__ partials, uint32_t n,
                                                             uint32_t capacity, ColorAcc* __restrict__ acc,
                                                             ColorStatus* __restrict__ status) {
  const uint32_t i = blockIdx.x * (uint32_t)kColorBlock + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool live = i < n;
  // a dead lane gets a record no live lane has: ranks are at least 1
  const uint32_t rec = live ? rank[i] - 1 : 0xffffffffu;
  unsigned long long s[3] = {0, 0, 0}, q[3] = {0, 0, 0};
  uint32_t area = 0, count = 0, inv_lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  if (live) {
    const int4 v = intervals[i];
    const uint4 a = partials[2 * (size_t)i], b = partials[2 * (size_t)i + 1];
    s[0] = a.x;
    s[1] = a.y;
    s[2] = a.z;
    q[0] = a.w;
    q[1] = b.x;
    q[2] = b.y;
    area = (uint32_t)(v.z - v.y + 1);
    count = 1;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      inv_lo[c] = 255u - ((b.z >> (8 * c)) & 0xffu);
      hi[c] = (b.w >> (8 * c)) & 0xffu;
    }
  }
  // whether the record goes on before the slice's first and behind its last interval
  const uint32_t slice = i - (uint32_t)lane;
  const uint32_t last = min(slice + 63u, n - 1u);   // the slice has a live lane, or the wavefront ends below
  const bool head = live && (lane == 0 || rank[i - 1] - 1 != rec);
  const bool open_before = live && lane == 0 && i > 0 && rank[i - 1] - 1 == rec;
  const bool open_behind = live && i == last && i + 1 < n && rank[i + 1] - 1 == rec;
  const unsigned long long heads = __ballot(head);
  const bool slice_open_behind = __ballot(open_behind) != 0ull;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o_rec = __shfl_down(rec, d);
    const bool take = lane + d < 64 && o_rec == rec;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const unsigned long long o_s = __shfl_down(s[c], d), o_q = __shfl_down(q[c], d);
      const uint32_t o_lo = __shfl_down(inv_lo[c], d), o_hi = __shfl_down(hi[c], d);
      if (take) {
        s[c] += o_s;
        q[c] += o_q;
        inv_lo[c] = max(inv_lo[c], o_lo);
        hi[c] = max(hi[c], o_hi);
      }
    }
    const uint32_t o_area = __shfl_down(area, d), o_count = __shfl_down(count, d);
    if (take) {
      area += o_area;
      count += o_count;
    }
  }
  if (!head) return;
  if (rec >= capacity) {
    atomicOr(&status->flags, (uint32_t)COLOR_FLAG_RANGE);
    return;
  }
  // the last segment of the slice is the one without a head above it
  const bool is_last_segment = lane == 63 || (heads >> (lane + 1)) == 0ull;
  const bool whole = !open_before && !(is_last_segment && slice_open_behind);
  ColorAcc* out = acc + rec;
  if (whole) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      out->sum[c] = s[c];
      out->sum_sq[c] = q[c];
      out->inv_lo[c] = inv_lo[c];
      out->hi[c] = hi[c];
    }
    out->area = area;
    out->count = count;
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      atomicAdd(&out->sum[c], s[c]);
      atomicAdd(&out->sum_sq[c], q[c]);
      atomicMax(&out->inv_lo[c], inv_lo[c]);
      atomicMax(&out->hi[c], hi[c]);
    }
    atomicAdd(&out->area, area);
    atomicAdd(&out->count, count);
  }
}

// One thread per record: the 18 words of a vsg_render_level_color.  table: kWords-strided entries whose
// word 0 is the id and, with has_component, word 1 the component.  Nothing is written when there are more
// records than `capacity`; the totals are gathered all the same.
__global__ __launch_bounds__(256) void k_color_finish(const ColorAcc* __restrict__ acc,
                                                      const int32_t* __restrict__ table, int table_words,
                                                      int has_component, const uint32_t* __restrict__ count,
                                                      uint32_t capacity_acc, uint32_t capacity,
                                                      int32_t* __restrict__ records,
                                                      ColorStatus* __restrict__ status) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  const uint32_t n_records = min(*count, capacity_acc);
  unsigned long long covered = 0;
  uint32_t largest = 0;
  if (k < n_records) {
    const ColorAcc a = acc[k];
    covered = a.area;
    largest = a.count;
    if (a.area == 0u) {
      atomicOr(&status->flags, (uint32_t)COLOR_FLAG_RANGE);   // cannot happen: every record has an interval
    } else if (n_records <= capacity) {
      int32_t* out = records + (size_t)k * kLevelColorWords;
      uint32_t mean = 0;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        // rounded half up; at most 255
        const unsigned long long m = (2ull * a.sum[c] + a.area) / (2ull * a.area);
        mean |= (uint32_t)m << (8 * c);
        out[4 + 2 * c] = (int32_t)(uint32_t)a.sum[c];
        out[5 + 2 * c] = (int32_t)(uint32_t)(a.sum[c] >> 32);
        out[10 + 2 * c] = (int32_t)(uint32_t)a.sum_sq[c];
        out[11 + 2 * c] = (int32_t)(uint32_t)(a.sum_sq[c] >> 32);
      }
      const uint32_t lo0 = 255u - a.inv_lo[0], lo1 = 255u - a.inv_lo[1], lo2 = 255u - a.inv_lo[2];
      out[0] = table[(size_t)k * table_words];
      out[1] = has_component ? table[(size_t)k * table_words + 1] : -1;
      out[2] = (int32_t)a.area;
      out[3] = (int32_t)mean;   // reserved0 = 0
      out[16] = (int32_t)(lo0 | lo1 << 8 | lo2 << 16 | a.hi[0] << 24);
      out[17] = (int32_t)(a.hi[1] | a.hi[2] << 8);   // reserved1 = 0
    }
  }
  covered = WaveSum(covered);
  largest = WaveMax(largest);
  if ((threadIdx.x & 63) == 0 && covered) {
    atomicAdd(&status->covered, covered);
    atomicMax(&status->largest, largest);
  }
}

// One thread per interval: its value becomes the packed mean of its record.
__global__ __launch_bounds__(256) void k_color_intervals(const int4* __restrict__ intervals,
                                                         const uint32_t* __restrict__ rank, uint32_t n,
                                                         const int32_t* __restrict__ records, uint32_t capacity,
                                                         int4* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const int4 v = intervals[i];
  const uint32_t rec = rank[i] - 1;
  const uint32_t mean = rec < capacity ? (uint32_t)records[(size_t)rec * kLevelColorWords + 3] & 0xffffffu : 0u;
  out[i] = make_int4(v.x, v.y, v.z, (int)mean);
}

}  // namespace

void LaunchColorRuns(const Interval* intervals, uint32_t n, int width, int height, const uint8_t* bgr, size_t stride,
                     uint32_t* partials, hipStream_t stream) {
  if (n == 0) return;
  // a short list of long intervals would leave most of the chip idle at 64 intervals per wavefront
  int per_wave = 64;
  while (per_wave > 1 && n / (uint32_t)per_wave < kColorWaves) per_wave >>= 1;
  const uint32_t waves = (n + (uint32_t)per_wave - 1) / (uint32_t)per_wave;
  const uint32_t groups = (waves + kColorBlock / 64 - 1) / (kColorBlock / 64);
  const dim3 grid(groups < 4096u ? groups : 4096u), block(kColorBlock);
  const bool aligned = (uintptr_t)bgr % 4 == 0 && stride % 4 == 0;
  if (aligned) {
    hipLaunchKernelGGL(k_color_runs<true>, grid, block, 0, stream, reinterpret_cast<const int4*>(intervals), n, width,
                       height, bgr, stride, per_wave, reinterpret_cast<uint4*>(partials));
  } else {
    hipLaunchKernelGGL(k_color_runs<false>, grid, block, 0, stream, reinterpret_cast<const int4*>(intervals), n, width,
                       height, bgr, stride, per_wave, reinterpret_cast<uint4*>(partials));
  }
}

void LaunchColorTable(const Interval* intervals, const uint32_t* rank, const uint32_t* partials, uint32_t n,
                      uint32_t capacity_acc, void* acc, const int32_t* table, int table_words, bool has_component,
                      const uint32_t* count, uint32_t capacity, int32_t* records, ColorStatus* status,
                      hipStream_t stream) {
  if (n == 0 || capacity_acc == 0) return;
  hipLaunchKernelGGL(k_color_table, dim3((n + kColorBlock - 1) / kColorBlock), dim3(kColorBlock), 0, stream,
                     reinterpret_cast<const int4*>(intervals), rank, reinterpret_cast<const uint4*>(partials), n,
                     capacity_acc, static_cast<ColorAcc*>(acc), status);
  hipLaunchKernelGGL(k_color_finish, dim3((capacity_acc + 255) / 256), dim3(256), 0, stream,
                     static_cast<const ColorAcc*>(acc), table, table_words, has_component ? 1 : 0, count, capacity_acc,
                     capacity, records, status);
}

void LaunchColorIntervals(const Interval* intervals, const uint32_t* rank, uint32_t n, const int32_t* records,
                          uint32_t capacity, Interval* out, hipStream_t stream) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_color_intervals, dim3((n + 255) / 256), dim3(256), 0, stream,
                     reinterpret_cast<const int4*>(intervals), rank, n, records, capacity,
                     reinterpret_cast<int4*>(out));
}

}  // namespace vsg_render_impl
