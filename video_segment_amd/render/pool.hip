// pool.hip -- float feature planes pooled by the groups of a hierarchy level, and group values painted back
// into feature planes (gfx950).
//
// Input is what the level and component pipelines leave on the device, as for colors.hip: the interval list
// {y, left_x, right_x, id} grouped by record in record order and the 1-based record of every interval.  The
// list is cut into slices of PoolSlice(n) intervals (64 unless the list is short); the unit of work is a slice
// times a block of channels, one wavefront each.
//
//   k_pool_sums_planar  lanes along x.  An interval of kPoolLongInterval pixels or more is summed by all 64
//                       lanes, 16-byte loads where the address allows and the elements before and behind them
//                       by single lanes, then folded across the lanes once; one of 16 to 63 pixels by a group
//                       of 16 lanes, one of 4 to 15 by a group of four (four or sixteen intervals at a time,
//                       adjacent lanes on adjacent elements), one of up to three pixels by its own lane.
//                       kPoolPlanarChannels channels share the interval records.  The lanes' totals are then
//                       reduced by record with a segmented suffix sum.
//   k_pool_sums_last    lanes along c.  The wavefront walks its slice interval by interval and pixel by pixel;
//                       a pixel's channels are one coalesced read and a lane's accumulator is one channel.
//                       With fewer than 33 channels the lanes form 64 / Cp groups (Cp the channels rounded up to
//                       a power of two) that take every (64 / Cp)-th pixel and are folded when a record ends.
//   k_pool_combine      a record that spans slices: the slices' parts, added in slice order
//   k_pool_count        area and interval count of every record, with integer atomics (order-free)
//   k_pool_finish       a thread per record: the caller's 16-byte group; the status' totals
//   k_pool_intervals    a thread per interval: its value becomes its 1-based record, for k_render_fill
//   k_pool_gather_*     the painted record plane and a [records][channels] matrix into feature planes
//
// Every element is widened exactly to f64 and every sum is accumulated in f64.  There is no floating-point
// atomic: the order of every addition is a function of the interval list, the strides and the base address
// modulo 16, never of the scheduling.
#include "render.h"

namespace vsg_render_impl {

namespace {

struct Bf16 {
  uint16_t bits;
};

__device__ __forceinline__ float ToFloat(float v) { return v; }
__device__ __forceinline__ float ToFloat(_Float16 v) { return (float)v; }
__device__ __forceinline__ float ToFloat(Bf16 v) { return __uint_as_float((uint32_t)v.bits << 16); }

template <class T>
__device__ __forceinline__ T FromFloat(float v);
template <>
__device__ __forceinline__ float FromFloat<float>(float v) {
  return v;
}
template <>
__device__ __forceinline__ _Float16 FromFloat<_Float16>(float v) {
  return (_Float16)v;   // v_cvt_f16_f32, round to nearest even
}
template <>
__device__ __forceinline__ Bf16 FromFloat<Bf16>(float v) {
  const uint32_t u = __float_as_uint(v);
  if ((u & 0x7fffffffu) > 0x7f800000u) return Bf16{(uint16_t)((u >> 16) | 0x0040u)};   // NaN stays one
  return Bf16{(uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16)};
}

// What a lane has gathered of one channel.  Fields outside MASK are never read, so they cost nothing.
struct Acc {
  double s, q;
  float lo, hi;
};

__device__ __forceinline__ void Clear(Acc& a) {
  a.s = 0.0;
  a.q = 0.0;
  a.lo = __uint_as_float(0x7f800000u);
  a.hi = __uint_as_float(0xff800000u);
}

// min and max skip a NaN: both comparisons are false for one.
template <int MASK>
__device__ __forceinline__ void Add(Acc& a, float f) {
  const double v = (double)f;
  if (MASK & POOL_SUM) a.s += v;
  if (MASK & POOL_SUM_SQ) a.q += v * v;
  if (MASK & POOL_MIN) a.lo = f < a.lo ? f : a.lo;
  if (MASK & POOL_MAX) a.hi = f > a.hi ? f : a.hi;
}

template <int MASK>
__device__ __forceinline__ void Merge(Acc& a, const Acc& b) {
  if (MASK & POOL_SUM) a.s += b.s;
  if (MASK & POOL_SUM_SQ) a.q += b.q;
  if (MASK & POOL_MIN) a.lo = b.lo < a.lo ? b.lo : a.lo;
  if (MASK & POOL_MAX) a.hi = b.hi > a.hi ? b.hi : a.hi;
}

template <int MASK>
__device__ __forceinline__ Acc ShuffleXor(const Acc& a, int s) {
  Acc b;
  Clear(b);
  if (MASK & POOL_SUM) b.s = __shfl_xor(a.s, s);
  if (MASK & POOL_SUM_SQ) b.q = __shfl_xor(a.q, s);
  if (MASK & POOL_MIN) b.lo = __shfl_xor(a.lo, s);
  if (MASK & POOL_MAX) b.hi = __shfl_xor(a.hi, s);
  return b;
}

template <int MASK>
__device__ __forceinline__ Acc ShuffleDown(const Acc& a, int d) {
  Acc b;
  Clear(b);
  if (MASK & POOL_SUM) b.s = __shfl_down(a.s, d);
  if (MASK & POOL_SUM_SQ) b.q = __shfl_down(a.q, d);
  if (MASK & POOL_MIN) b.lo = __shfl_down(a.lo, d);
  if (MASK & POOL_MAX) b.hi = __shfl_down(a.hi, d);
  return b;
}

template <int MASK>
__device__ __forceinline__ void Store(const PoolMatrices& m, size_t at, const Acc& a) {
  if (MASK & POOL_SUM) m.sum[at] = a.s;
  if (MASK & POOL_SUM_SQ) m.sum_sq[at] = a.q;
  if (MASK & POOL_MIN) m.min[at] = a.lo;
  if (MASK & POOL_MAX) m.max[at] = a.hi;
}

template <int MASK>
__device__ __forceinline__ Acc Load(const PoolMatrices& m, size_t at) {
  Acc a;
  Clear(a);
  if (MASK & POOL_SUM) a.s = m.sum[at];
  if (MASK & POOL_SUM_SQ) a.q = m.sum_sq[at];
  if (MASK & POOL_MIN) a.lo = m.min[at];
  if (MASK & POOL_MAX) a.hi = m.max[at];
  return a;
}

// The 16 bytes at p, element by element in address order.
template <int MASK>
__device__ __forceinline__ void AddVector(Acc& a, const float* p) {
  const float4 w = *reinterpret_cast<const float4*>(p);
  Add<MASK>(a, w.x);
  Add<MASK>(a, w.y);
  Add<MASK>(a, w.z);
  Add<MASK>(a, w.w);
}
template <int MASK>
__device__ __forceinline__ void AddVector(Acc& a, const _Float16* p) {
  union {
    uint4 w;
    _Float16 h[8];
  } u;
  u.w = *reinterpret_cast<const uint4*>(p);
#pragma unroll
  for (int k = 0; k < 8; ++k) Add<MASK>(a, (float)u.h[k]);
}
template <int MASK>
__device__ __forceinline__ void AddVector(Acc& a, const Bf16* p) {
  const uint4 w = *reinterpret_cast<const uint4*>(p);
  const uint32_t d[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    Add<MASK>(a, __uint_as_float(d[k] << 16));
    Add<MASK>(a, __uint_as_float(d[k] & 0xffff0000u));
  }
}

// The interval of lane `lane` of a slice and its 0-based record; dead lanes hold an empty interval and a record
// no live lane has.  An interval that is not inside the frame (there is none) is emptied: nothing of it is read.
struct SliceLane {
  int4 v;
  uint32_t rec;
  bool live;
};

__device__ __forceinline__ SliceLane LoadSliceLane(const int4* __restrict__ intervals,
                                                   const uint32_t* __restrict__ rank, uint32_t n, int W, int H,
                                                   unsigned long long base, int per_wave, int lane) {
  SliceLane s;
  const unsigned long long i = base + lane;
  s.live = lane < per_wave && i < n;
  s.v = s.live ? intervals[i] : make_int4(0, 0, -1, 0);   // x = y, y = left_x, z = right_x
  if (s.v.x < 0 || s.v.x >= H || s.v.y < 0 || s.v.z >= W) s.v = make_int4(0, 0, -1, 0);
  s.rec = s.live ? rank[i] - 1 : 0xffffffffu;
  return s;
}

// Where the totals of a segment of a slice go: [s][0] of the spill when the record began before the slice, [s][1]
// when it goes on behind it, the record's row of the output otherwise.
template <int MASK>
__device__ __forceinline__ void StoreSegment(const PoolMatrices& out, const PoolMatrices& spill, uint32_t slice,
                                             uint32_t rec, int C, int c, bool open_before, bool open_behind,
                                             const Acc& a) {
  // the pointers are chosen one by one: choosing between the two structs would put both into scratch memory
  const bool parted = open_before || open_behind;
  const size_t at = (parted ? (size_t)slice * 2 + (open_before ? 0 : 1) : (size_t)rec) * C + c;
  if (MASK & POOL_SUM) (parted ? spill.sum : out.sum)[at] = a.s;
  if (MASK & POOL_SUM_SQ) (parted ? spill.sum_sq : out.sum_sq)[at] = a.q;
  if (MASK & POOL_MIN) (parted ? spill.min : out.min)[at] = a.lo;
  if (MASK & POOL_MAX) (parted ? spill.max : out.max)[at] = a.hi;
}

template <int MASK>
__device__ __forceinline__ Acc ShuffleFrom(const Acc& a, int from) {
  Acc b;
  Clear(b);
  if (MASK & POOL_SUM) b.s = __shfl(a.s, from);
  if (MASK & POOL_SUM_SQ) b.q = __shfl(a.q, from);
  if (MASK & POOL_MIN) b.lo = __shfl(a.lo, from);
  if (MASK & POOL_MAX) b.hi = __shfl(a.hi, from);
  return b;
}

// The intervals of the lanes in `cls`, too short for the whole wavefront, by groups of S lanes: 64 / S of them
// at a time, in the order of their lanes.  A group's lanes take every S-th pixel of its interval, so that its
// loads are S adjacent elements; the group is folded (log2 S steps) and the interval's lane takes the total.
// order: 64 bytes of LDS of the wavefront.  Called by all lanes.
template <class T, int MASK, int S>
__device__ __forceinline__ void SumByGroups(unsigned long long cls, const SliceLane& me, int lane,
                                            const T* __restrict__ feat, long long cs, long long rs, int c0, int C,
                                            unsigned char* order, Acc (&mine)[kPoolPlanarChannels]) {
  if (!cls) return;   // wave-uniform
  constexpr int G = 64 / S;
  const int total = __popcll(cls);
  const bool in = (cls >> lane) & 1ull;
  const int my_rank = __popcll(cls & ((1ull << lane) - 1ull));
  __syncthreads();
  if (in) order[my_rank] = (unsigned char)lane;
  __syncthreads();
  const int g = lane / S, sub = lane % S;
  for (int t = 0; t * G < total; ++t) {
    const int k = t * G + g;
    const bool busy = k < total;
    const int src = busy ? order[k] : 0;
    const int y = __shfl(me.v.x, src), lx = __shfl(me.v.y, src);
    const int right = __shfl(me.v.z, src);
    const int rx = busy ? right : lx - 1;   // a group without an interval reads nothing
    const bool take = in && my_rank / G == t;
#pragma unroll
    for (int cc = 0; cc < kPoolPlanarChannels; ++cc) {
      if (c0 + cc >= C) break;
      const T* row = feat + (long long)(c0 + cc) * cs + (long long)y * rs;
      Acc a;
      Clear(a);
      for (int x = lx + sub; x <= rx; x += S) Add<MASK>(a, ToFloat(row[x]));
#pragma unroll
      for (int s = S / 2; s > 0; s >>= 1) {
        const Acc b = ShuffleXor<MASK>(a, s);
        Merge<MASK>(a, b);
      }
      const Acc b = ShuffleFrom<MASK>(a, (my_rank % G) * S);
      if (take) mine[cc] = b;
    }
  }
}

template <class T, int MASK>
__global__ __launch_bounds__(64) void k_pool_sums_planar(const int4* __restrict__ intervals,
                                                         const uint32_t* __restrict__ rank, uint32_t n, int W, int H,
                                                         const T* __restrict__ feat, long long cs, long long rs, int C,
                                                         int per_wave, PoolMatrices out, PoolMatrices spill) {
  constexpr int CB = kPoolPlanarChannels;
  constexpr int V = 16 / (int)sizeof(T);   // elements of a 16-byte load
  const int lane = threadIdx.x;
  const uint32_t slice = blockIdx.x;
  const int c0 = blockIdx.y * CB;
  const unsigned long long base = (unsigned long long)slice * per_wave;
  const SliceLane me = LoadSliceLane(intervals, rank, n, W, H, base, per_wave, lane);
  const int len = me.v.z - me.v.y + 1;
  Acc mine[CB];
#pragma unroll
  for (int cc = 0; cc < CB; ++cc) Clear(mine[cc]);

  unsigned long long todo = __ballot(len >= kPoolLongInterval);
  while (todo) {   // wave-uniform
    const int j = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int y = __builtin_amdgcn_readlane(me.v.x, j);
    const int lx = __builtin_amdgcn_readlane(me.v.y, j);
    const int rx = __builtin_amdgcn_readlane(me.v.z, j);
#pragma unroll
    for (int cc = 0; cc < CB; ++cc) {
      if (c0 + cc >= C) break;
      const T* row = feat + (long long)(c0 + cc) * cs + (long long)y * rs;
      // the 16-byte groups start at the first element of the interval whose address is a multiple of 16
      const int mis = (int)(((uintptr_t)(row + lx) & 15u) / sizeof(T));
      const int body = min(lx + (mis ? V - mis : 0), rx + 1);
      const int n_vec = (rx + 1 - body) / V;
      const int tail = body + n_vec * V;
      const int n_head = body - lx, n_tail = rx + 1 - tail;   // below V each
      Acc a;
      Clear(a);
      if (lane < n_head + n_tail) Add<MASK>(a, ToFloat(row[lane < n_head ? lx + lane : tail + lane - n_head]));
      for (int g = lane; g < n_vec; g += 64) AddVector<MASK>(a, row + body + g * V);
#pragma unroll
      for (int s = 32; s > 0; s >>= 1) {
        const Acc b = ShuffleXor<MASK>(a, s);
        Merge<MASK>(a, b);
      }
      if (lane == j) mine[cc] = a;
    }
  }
  __shared__ unsigned char order[64];
  SumByGroups<T, MASK, 16>(__ballot(len >= kPoolGroupInterval && len < kPoolLongInterval), me, lane, feat, cs, rs, c0,
                           C, order, mine);
  SumByGroups<T, MASK, 4>(__ballot(len >= kPoolQuadInterval && len < kPoolGroupInterval), me, lane, feat, cs, rs, c0,
                          C, order, mine);
  if (len > 0 && len < kPoolQuadInterval) {   // one to three pixels: the interval's own lane
#pragma unroll
    for (int cc = 0; cc < CB; ++cc) {
      if (c0 + cc >= C) break;
      const T* p = feat + (long long)(c0 + cc) * cs + (long long)me.v.x * rs + me.v.y;
      for (int k = 0; k < len; ++k) Add<MASK>(mine[cc], ToFloat(p[k]));
    }
  }

  // ---- the lanes' totals by record: segmented suffix sum, as k_color_table's ----
  const unsigned long long i = base + lane;
  const uint32_t last = (uint32_t)min(base + (unsigned long long)per_wave, (unsigned long long)n) - 1u;
  const uint32_t before = __shfl_up(me.rec, 1);
  const bool head = me.live && (lane == 0 || before != me.rec);
  const bool open_before = me.live && lane == 0 && i > 0 && rank[i - 1] - 1 == me.rec;
  const bool last_open = me.live && i == last && i + 1 < n && rank[i + 1] - 1 == me.rec;
  const unsigned long long heads = __ballot(head);
  const bool slice_open_behind = __ballot(last_open) != 0ull;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o_rec = __shfl_down(me.rec, d);
    const bool take = lane + d < 64 && o_rec == me.rec;
#pragma unroll
    for (int cc = 0; cc < CB; ++cc) {
      const Acc b = ShuffleDown<MASK>(mine[cc], d);
      if (take) Merge<MASK>(mine[cc], b);
    }
  }
  if (!head) return;
  const bool is_last_segment = lane == 63 || (heads >> (lane + 1)) == 0ull;
#pragma unroll
  for (int cc = 0; cc < CB; ++cc) {
    if (c0 + cc >= C) break;
    StoreSegment<MASK>(out, spill, slice, me.rec, C, c0 + cc, open_before, is_last_segment && slice_open_behind,
                       mine[cc]);
  }
}

template <class T, int MASK>
__global__ __launch_bounds__(64) void k_pool_sums_last(const int4* __restrict__ intervals,
                                                       const uint32_t* __restrict__ rank, uint32_t n, int W, int H,
                                                       const T* __restrict__ feat, long long rs, long long ps, int C,
                                                       int per_wave, int cp_log2, PoolMatrices out,
                                                       PoolMatrices spill) {
  const int lane = threadIdx.x;
  const uint32_t slice = blockIdx.x;
  const int cp = 1 << cp_log2;                  // lanes along the channels
  static_assert(kPoolLastChannels == 64, "a lane per channel of the block");
  const int groups = 64 >> cp_log2, g = lane >> cp_log2;
  const int c = blockIdx.y * cp + (lane & (cp - 1));
  const bool active = c < C;
  const unsigned long long base = (unsigned long long)slice * per_wave;
  const SliceLane me = LoadSliceLane(intervals, rank, n, W, H, base, per_wave, lane);
  const int count = (int)min((unsigned long long)per_wave, (unsigned long long)n - base);
  const bool open_before = base > 0 && rank[base - 1] == rank[base];
  const bool open_behind = base + count < n && rank[base + count] == rank[base + count - 1];
  const T* mine = feat + (active ? c : 0);

  Acc a;
  Clear(a);
  uint32_t cur = __builtin_amdgcn_readlane(me.rec, 0);
  bool first_segment = true;
  for (int jj = 0; jj <= count; ++jj) {   // wave-uniform; jj == count flushes the last segment
    const int j = __builtin_amdgcn_readfirstlane(jj);
    const uint32_t rec = j < count ? (uint32_t)__builtin_amdgcn_readlane((int)me.rec, j) : ~cur;
    if (rec != cur) {
      for (int s = cp; s < 64; s <<= 1) {
        const Acc b = ShuffleXor<MASK>(a, s);
        Merge<MASK>(a, b);
      }
      if (active && g == 0) {
        StoreSegment<MASK>(out, spill, slice, cur, C, c, first_segment && open_before, j == count && open_behind, a);
      }
      Clear(a);
      cur = rec;
      first_segment = false;
    }
    if (j == count) break;
    const int y = __builtin_amdgcn_readlane(me.v.x, j);
    const int lx = __builtin_amdgcn_readlane(me.v.y, j);
    const int rx = __builtin_amdgcn_readlane(me.v.z, j);
    if (active) {
      const T* row = mine + (long long)y * rs;
#pragma unroll 4
      for (int x = lx + g; x <= rx; x += groups) Add<MASK>(a, ToFloat(row[(long long)x * ps]));
    }
  }
}

// A wavefront per slice and 64 channels.  The slice where a record that spans slices begins gathers it: its own
// [s][1], then [t][0] of every slice t the record goes on into, in slice order.
template <int MASK>
__global__ __launch_bounds__(64) void k_pool_combine(const uint32_t* __restrict__ rank, uint32_t n, int per_wave,
                                                     uint32_t slices, int C, PoolMatrices spill, PoolMatrices out) {
  const uint32_t s0 = blockIdx.x;
  const int c = blockIdx.y * 64 + threadIdx.x;
  const unsigned long long first = (unsigned long long)s0 * per_wave;
  const unsigned long long last = min(first + (unsigned long long)per_wave, (unsigned long long)n) - 1ull;
  if (last + 1 >= n) return;
  const uint32_t r = rank[last];
  if (rank[last + 1] != r) return;                                   // nothing goes on behind this slice
  if (rank[first] == r && first > 0 && rank[first - 1] == r) return;   // began before: a middle slice
  if (c >= C) return;
  Acc a = Load<MASK>(spill, ((size_t)s0 * 2 + 1) * C + c);
  for (uint32_t t = s0 + 1; t < slices; ++t) {
    const unsigned long long f = (unsigned long long)t * per_wave;
    const Acc b = Load<MASK>(spill, ((size_t)t * 2) * C + c);
    Merge<MASK>(a, b);
    const unsigned long long l = min(f + (unsigned long long)per_wave, (unsigned long long)n) - 1ull;
    if (rank[l] != r || l + 1 >= n || rank[l + 1] != r) break;
  }
  Store<MASK>(out, (size_t)(r - 1) * C + c, a);
}

// A thread per interval: area and interval count of its record.  Reduced by record within the wavefront first.
__global__ __launch_bounds__(256) void k_pool_count(const int4* __restrict__ intervals,
                                                    const uint32_t* __restrict__ rank, uint32_t n, uint32_t records,
                                                    uint32_t* __restrict__ acc, PoolStatus* __restrict__ status) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool live = i < n;
  const uint32_t rec = live ? rank[i] - 1 : 0xffffffffu;
  uint32_t area = 0, count = 0;
  if (live) {
    const int4 v = intervals[i];
    area = (uint32_t)(v.z - v.y + 1);
    count = 1;
  }
  const uint32_t before = __shfl_up(rec, 1);
  const bool head = live && (lane == 0 || before != rec);
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o_rec = __shfl_down(rec, d);
    const uint32_t o_area = __shfl_down(area, d), o_count = __shfl_down(count, d);
    if (lane + d < 64 && o_rec == rec) {
      area += o_area;
      count += o_count;
    }
  }
  if (!head) return;
  if (rec >= records) {
    atomicOr(&status->flags, (uint32_t)POOL_FLAG_RANGE);
    return;
  }
  atomicAdd(&acc[2 * (size_t)rec], area);
  atomicAdd(&acc[2 * (size_t)rec + 1], count);
}

__global__ __launch_bounds__(256) void k_pool_finish(const uint32_t* __restrict__ acc,
                                                     const int32_t* __restrict__ table, int table_words,
                                                     int has_component, uint32_t records,
                                                     int32_t* __restrict__ groups, PoolStatus* __restrict__ status) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  unsigned long long covered = 0;
  uint32_t largest = 0;
  if (k < records) {
    covered = acc[2 * (size_t)k];
    largest = acc[2 * (size_t)k + 1];
    if (covered == 0) atomicOr(&status->flags, (uint32_t)POOL_FLAG_RANGE);   // cannot happen
    if (groups) {
      int32_t* out = groups + (size_t)k * kPoolGroupWords;
      out[0] = table[(size_t)k * table_words];
      out[1] = has_component ? table[(size_t)k * table_words + 1] : -1;
      out[2] = (int32_t)covered;
      out[3] = 0;
    }
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    covered += __shfl_xor(covered, s);
    largest = max(largest, __shfl_xor(largest, s));
  }
  if ((threadIdx.x & 63) == 0 && covered) {
    atomicAdd(&status->covered, covered);
    atomicMax(&status->largest, largest);
  }
}

__global__ __launch_bounds__(256) void k_pool_intervals(const int4* __restrict__ intervals,
                                                        const uint32_t* __restrict__ rank, uint32_t n,
                                                        int4* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const int4 v = intervals[i];
  out[i] = make_int4(v.x, v.y, v.z, (int)rank[i]);
}

constexpr int kGatherChannels = 8;   // channels a thread of the planar gather writes

// Threads along x, a row per blockIdx.y, kGatherChannels channels per blockIdx.z.
template <class T>
__global__ __launch_bounds__(256) void k_pool_gather_planar(const uint32_t* __restrict__ plane, int pitch, int W,
                                                            const float* __restrict__ values, uint32_t num_values,
                                                            int C, float fill, T* __restrict__ out, long long cs,
                                                            long long rs) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  const int y = blockIdx.y;
  if (x >= W) return;
  const uint32_t r = plane[(size_t)y * pitch + x];
  const bool covered = r != 0u && r <= num_values;
  const int c0 = blockIdx.z * kGatherChannels;
#pragma unroll
  for (int cc = 0; cc < kGatherChannels; ++cc) {
    const int c = c0 + cc;
    if (c >= C) break;
    const float v = covered ? values[(size_t)(r - 1) * C + c] : fill;
    out[(long long)c * cs + (long long)y * rs + x] = FromFloat<T>(v);
  }
}

// Threads along (x, c) of a row, c fastest: a pixel's channels are one coalesced read and one coalesced write.
template <class T>
__global__ __launch_bounds__(256) void k_pool_gather_last(const uint32_t* __restrict__ plane, int pitch, int W,
                                                          const float* __restrict__ values, uint32_t num_values,
                                                          int C, float fill, T* __restrict__ out, long long rs,
                                                          long long ps) {
  const unsigned long long e = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  const int y = blockIdx.y;
  if (e >= (unsigned long long)W * C) return;
  const int x = (int)(e / (unsigned)C), c = (int)(e % (unsigned)C);
  const uint32_t r = plane[(size_t)y * pitch + x];
  const float v = r != 0u && r <= num_values ? values[(size_t)(r - 1) * C + c] : fill;
  out[(long long)y * rs + (long long)x * ps + c] = FromFloat<T>(v);
}

template <class T, int MASK>
void SumsOf(const int4* intervals, const uint32_t* rank, uint32_t n, int W, int H, const void* features,
            const PoolLayout& l, const PoolMatrices& out, const PoolMatrices& spill, hipStream_t stream) {
  const int per_wave = (int)PoolSlice(n);
  const uint32_t slices = PoolSlices(n);
  const T* feat = static_cast<const T*>(features);
  if (l.channels_last) {
    int cp_log2 = 0;
    while ((1 << cp_log2) < kPoolLastChannels && (1 << cp_log2) < l.channels) ++cp_log2;
    const int cp = 1 << cp_log2;
    const dim3 grid(slices, (unsigned)((l.channels + cp - 1) / cp));
    hipLaunchKernelGGL((k_pool_sums_last<T, MASK>), grid, dim3(64), 0, stream, intervals, rank, n, W, H, feat,
                       l.row_stride, l.pixel_stride, l.channels, per_wave, cp_log2, out, spill);
  } else {
    const dim3 grid(slices, (unsigned)((l.channels + kPoolPlanarChannels - 1) / kPoolPlanarChannels));
    hipLaunchKernelGGL((k_pool_sums_planar<T, MASK>), grid, dim3(64), 0, stream, intervals, rank, n, W, H, feat,
                       l.chan_stride, l.row_stride, l.channels, per_wave, out, spill);
  }
}

template <int MASK>
void SumsOfMask(const int4* intervals, const uint32_t* rank, uint32_t n, int W, int H, const void* features,
                const PoolLayout& l, const PoolMatrices& out, const PoolMatrices& spill, hipStream_t stream) {
  switch (l.dtype) {
    case POOL_F32: SumsOf<float, MASK>(intervals, rank, n, W, H, features, l, out, spill, stream); break;
    case POOL_F16: SumsOf<_Float16, MASK>(intervals, rank, n, W, H, features, l, out, spill, stream); break;
    default: SumsOf<Bf16, MASK>(intervals, rank, n, W, H, features, l, out, spill, stream); break;
  }
}

template <int MASK>
void CombineOfMask(const uint32_t* rank, uint32_t n, int channels, const PoolMatrices& spill, const PoolMatrices& out,
                   hipStream_t stream) {
  const uint32_t slices = PoolSlices(n);
  hipLaunchKernelGGL(k_pool_combine<MASK>, dim3(slices, (unsigned)((channels + 63) / 64)), dim3(64), 0, stream, rank,
                     n, (int)PoolSlice(n), slices, channels, spill, out);
}

template <class T>
void GatherOf(const uint32_t* plane, int pitch, int W, int H, const float* values, uint32_t num_values, float fill,
              void* out, const PoolLayout& l, hipStream_t stream) {
  const int C = l.channels;
  if (l.channels_last) {
    const unsigned long long per_row = (unsigned long long)W * C;
    hipLaunchKernelGGL(k_pool_gather_last<T>, dim3((unsigned)((per_row + 255) / 256), (unsigned)H), dim3(256), 0,
                       stream, plane, pitch, W, values, num_values, C, fill, static_cast<T*>(out), l.row_stride,
                       l.pixel_stride);
  } else {
    const dim3 grid((unsigned)((W + 255) / 256), (unsigned)H, (unsigned)((C + kGatherChannels - 1) / kGatherChannels));
    hipLaunchKernelGGL(k_pool_gather_planar<T>, grid, dim3(256), 0, stream, plane, pitch, W, values, num_values, C,
                       fill, static_cast<T*>(out), l.chan_stride, l.row_stride);
  }
}

}  // namespace

uint32_t PoolSlice(uint32_t n) {
  uint32_t slice = 64;
  while (slice > 1 && n / slice < kPoolWaves) slice >>= 1;
  return slice;
}

#define VSG_POOL_MASKS(CALL)                                                                                      \
  switch (mask) {                                                                                                 \
    case 1: CALL(1); break;   case 2: CALL(2); break;   case 3: CALL(3); break;   case 4: CALL(4); break;         \
    case 5: CALL(5); break;   case 6: CALL(6); break;   case 7: CALL(7); break;   case 8: CALL(8); break;         \
    case 9: CALL(9); break;   case 10: CALL(10); break; case 11: CALL(11); break; case 12: CALL(12); break;       \
    case 13: CALL(13); break; case 14: CALL(14); break; case 15: CALL(15); break; default: break;                 \
  }

void LaunchPoolSums(const Interval* intervals, const uint32_t* rank, uint32_t n, int width, int height,
                    const void* features, const PoolLayout& layout, int mask, const PoolMatrices& out,
                    const PoolMatrices& spill, hipStream_t stream) {
  if (n == 0) return;
  const int4* list = reinterpret_cast<const int4*>(intervals);
#define VSG_POOL_SUMS(M) SumsOfMask<M>(list, rank, n, width, height, features, layout, out, spill, stream)
  VSG_POOL_MASKS(VSG_POOL_SUMS)
#undef VSG_POOL_SUMS
}

void LaunchPoolCombine(const uint32_t* rank, uint32_t n, int channels, int mask, const PoolMatrices& spill,
                       const PoolMatrices& out, hipStream_t stream) {
  if (n == 0) return;
#define VSG_POOL_COMBINE(M) CombineOfMask<M>(rank, n, channels, spill, out, stream)
  VSG_POOL_MASKS(VSG_POOL_COMBINE)
#undef VSG_POOL_COMBINE
}

void LaunchPoolGroups(const Interval* intervals, const uint32_t* rank, uint32_t n, uint32_t records, uint32_t* acc,
                      const int32_t* table, int table_words, bool has_component, int32_t* groups, PoolStatus* status,
                      hipStream_t stream) {
  if (n == 0 || records == 0) return;
  hipLaunchKernelGGL(k_pool_count, dim3((n + 255) / 256), dim3(256), 0, stream,
                     reinterpret_cast<const int4*>(intervals), rank, n, records, acc, status);
  hipLaunchKernelGGL(k_pool_finish, dim3((records + 255) / 256), dim3(256), 0, stream, acc, table, table_words,
                     has_component ? 1 : 0, records, groups, status);
}

void LaunchPoolIntervals(const Interval* intervals, const uint32_t* rank, uint32_t n, Interval* out,
                         hipStream_t stream) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_pool_intervals, dim3((n + 255) / 256), dim3(256), 0, stream,
                     reinterpret_cast<const int4*>(intervals), rank, n, reinterpret_cast<int4*>(out));
}

void LaunchPoolGather(const uint32_t* plane, int pitch, int width, int height, const float* values,
                      uint32_t num_values, float fill, void* out, const PoolLayout& layout, hipStream_t stream) {
  switch (layout.dtype) {
    case POOL_F32: GatherOf<float>(plane, pitch, width, height, values, num_values, fill, out, layout, stream); break;
    case POOL_F16:
      GatherOf<_Float16>(plane, pitch, width, height, values, num_values, fill, out, layout, stream);
      break;
    default: GatherOf<Bf16>(plane, pitch, width, height, values, num_values, fill, out, layout, stream); break;
  }
}

}  // namespace vsg_render_impl
