// simplify.hip -- Douglas-Peucker on the segments of the level mesh (gfx950): what csrc/boundary.cpp's
// ApproxPolyDP gives for every segment's point list, computed where MeshTables left the corner lists.  The
// definition is in include/vsg_render.h.  Nothing is expanded to lattice points: along a straight run the
// distance to a chord is linear and the distance to a sweep's start strictly convex, so every maximum, first
// index on ties, falls on a corner.
//
//   k_simplify_dp_wave   one wavefront per segment of up to kSimplifyWavePoints corners, the state in LDS: the
//                        collapse rule; the sweeps of a closed curve; then rounds.  In a round every vertex
//                        between two neighbouring kept vertices offers its distance to their chord to the
//                        slice's word (one 64-bit atomic max of distance << 32 | ~index: the first index wins a
//                        tie); the slice keeps its farthest vertex when that fails the host's test and is done
//                        when it passes.  A segment ends with the round that keeps nothing.  Longer segments
//                        are put on a list.
//   k_simplify_dp_block  a fixed grid of workgroups over that list, the same rounds with the workgroup looping
//                        over the vertices; the state in LDS up to kSimplifyLdsPoints corners, in a block of
//                        the handle beyond
//   k_simplify_clean     one lane per segment: the host's in-place pass over almost straight joints, a chain
//                        in which every decision reads what the one before wrote
//   scan                 first_vertex of the new lists
//   k_simplify_compact   one thread per kept slot: the vertex to its place
//   k_simplify_records   one thread per segment: the record, the counts of the stats
//   k_copy_lists         of lists.hip: the four lists to the caller's device memory, if the vertices fit
//
// The number of rounds is bounded by the number of vertices, whatever the data.  A handle is at most 32768
// wide and high, so every cross product and every squared distance here is an integer below 2^32, exact in a
// double and in the upper half of the arg-max word; the tests themselves are the host's double expressions,
// operation for operation, with contraction off.  Every index read from memory is checked against its array
// before it is used.
#include "render.h"
#include "render_device.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace vsg_render_impl {

namespace {

constexpr int kSimplifyWave = 64;
constexpr int kSimplifyBlock = 1024;
constexpr int kSimplifyLongGrid = 256;
constexpr int kTableBlock = 256;
constexpr uint32_t kDone = 0x80000000u;      // in lo[v]: v is kept, or its slice has passed the test
constexpr uint32_t kIndexMask = 0x7fffffffu;
constexpr uint32_t kNone = 0xffffffffu;

typedef unsigned long long u64;

// What the rounds of one workgroup share.
struct RoundShared {
  u64 sweep;
  uint32_t any[2];
  uint32_t window_lo[2], window_hi[2];
  uint32_t wave_count[kSimplifyBlock / 64];
};

struct SegmentOf {
  uint32_t first, count, length, slot;   // slot: where its state and its kept vertices begin
  bool closed, ok;
};

__device__ __forceinline__ void Flag(SimplifyStatus* status) { atomicOr(&status->flags, (uint32_t)SIMPLIFY_FLAG_RANGE); }

__device__ __forceinline__ SegmentOf Load(const SimplifyView& m, uint32_t s) {
  const int32_t* rec = m.segments + (size_t)s * kMeshSegmentWords;
  SegmentOf g;
  g.first = (uint32_t)rec[2];
  g.count = (uint32_t)rec[3];
  g.length = (uint32_t)rec[4];
  g.closed = rec[5] != 0;
  g.slot = g.first + s;
  const uint32_t vertices_in = m.slots - m.n_segments;
  g.ok = g.count >= 2u && g.count <= vertices_in && g.first <= vertices_in - g.count;
  return g;
}

__device__ __forceinline__ bool Collapses(const SimplifyView& m, const SegmentOf& g) {
  return !g.closed && g.length + 1u < m.threshold;
}

// The rounds of segment s by the T threads of a workgroup.  lo, hi: count + 1 words each; best: two halves of
// `stride` words.
template <int T>
__device__ void DpSegment(const SimplifyView& m, uint32_t s, const SegmentOf& g, uint32_t* lo, uint32_t* hi, u64* best,
                          uint32_t stride, RoundShared* sh) {
  const uint32_t tid = threadIdx.x;
  const int lane = (int)(tid & 63u);
  const uint32_t count = g.count;
  const int2* pts = m.vertices + g.first;
  const double eps = m.eps;
  bool ring = g.closed;
  int sweeps = 3;
  {
    const int2 a = pts[0], b = pts[count - 1];
    if (!g.closed && a.x == b.x && a.y == b.y) {
      ring = true;
      sweeps = 1;
    }
  }
  uint32_t base = 0, last = count - 1u, arg = 0;
  if (ring) {
    // the farthest point from the start, then from that one, then from that one
    uint32_t start = 0;
    bool le_eps = false;
    for (int k = 0; k < sweeps; ++k) {
      __syncthreads();
      if (tid == 0) sh->sweep = 0;
      __syncthreads();
      const int2 sp = pts[start];
      u64 mine = 0;
      for (uint32_t j = 1u + tid; j < count; j += (uint32_t)T) {
        uint32_t i = start + j;
        if (i >= count) i -= count;
        const int2 pt = pts[i];
        const double dx = (double)(pt.x - sp.x), dy = (double)(pt.y - sp.y);
        const double dist = dx * dx + dy * dy;
        if (dist > 0) mine = max(mine, (u64)dist << 32 | (u64)(kNone - j));
      }
      mine = WaveMax(mine);
      if (lane == 0 && mine) atomicMax(&sh->sweep, mine);
      __syncthreads();
      const u64 key = sh->sweep;
      if (key) arg = kNone - (uint32_t)key;
      le_eps = (double)(key >> 32) <= eps;
      if (k + 1 < sweeps) start = (start + arg) % count;
    }
    base = start;
    last = count;
    if (le_eps) {
      // the whole curve lies within max_error of one point
      if (tid == 0) {
        m.kept[g.slot] = pts[base];
        m.kseg[g.slot] = s;
        if (!g.closed) {
          m.kept[g.slot + 1u] = pts[0];
          m.kseg[g.slot + 1u] = s;
        }
        m.kcount[s] = g.closed ? 1u : 2u;
        m.rounds[s] = 0;
      }
      return;
    }
  }
  auto point = [&](uint32_t v) {
    uint32_t i = base + v;
    if (i >= count) i -= count;
    return pts[i];
  };
  __syncthreads();
  for (uint32_t v = tid; v <= last; v += (uint32_t)T) {
    if (v == 0 || v == last || (ring && v == arg)) {
      lo[v] = v | kDone;
      hi[v] = v;
    } else if (ring) {
      lo[v] = v < arg ? 0u : arg;
      hi[v] = v < arg ? arg : last;
    } else {
      lo[v] = 0;
      hi[v] = last;
    }
    best[v] = 0;
    best[stride + v] = 0;
  }
  if (tid == 0) {
    sh->any[0] = sh->any[1] = 0;
    sh->window_lo[0] = 1u;
    sh->window_hi[0] = last - 1u;      // last >= 1; empty when last == 1
    sh->window_lo[1] = kNone;
    sh->window_hi[1] = 0;
  }
  __syncthreads();
  uint32_t rounds = 0;
  for (uint32_t r = 0; r <= last; ++r) {           // ends by construction: a round keeps a vertex or is the last
    const uint32_t p = r & 1u, q = p ^ 1u;
    const uint32_t from = sh->window_lo[p], to = sh->window_hi[p];
    if (from > to || to >= last) break;
    if (tid == 0) {
      sh->any[p] = 0;
      sh->window_lo[q] = kNone;
      sh->window_hi[q] = 0;
    }
    // every open vertex offers its distance to its slice.  The lanes of a wavefront hold consecutive vertices
    // and a slice is a run of them: the run is reduced in the wavefront first, its first lane does the atomic
    for (uint32_t v0 = from; v0 <= to; v0 += (uint32_t)T) {
      const uint32_t v = v0 + tid;
      uint32_t a = kNone;
      u64 key = 0;
      if (v <= to) {
        const uint32_t l = lo[v], b = hi[v];
        if (!(l & kDone) && l < v && b > v && b <= last) {
          a = l;
          if (v == a + 1u) best[q * stride + a] = 0;   // the word this slice's left part takes in the next round
          const int2 sp = point(a), ep = point(b), pt = point(v);
          const double dx = (double)(ep.x - sp.x), dy = (double)(ep.y - sp.y);
          const double dist = fabs((double)(pt.y - sp.y) * dx - (double)(pt.x - sp.x) * dy);
          if (dist > 0) key = (u64)dist << 32 | (u64)(kNone - v);
        }
      }
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t other_a = __shfl_down(a, d);
        const u64 other_key = (u64)__shfl_down((long long)key, d);
        if (lane + d < 64 && other_a == a) key = max(key, other_key);
      }
      const uint32_t before = __shfl_up(a, 1);
      if (a != kNone && key && (lane == 0 || before != a)) atomicMax(&best[p * stride + a], key);
    }
    __syncthreads();
    // every slice keeps its farthest vertex or is done
    bool kept_one = false;
    uint32_t open_lo = kNone, open_hi = 0;
    for (uint32_t v = from + tid; v <= to; v += (uint32_t)T) {
      const uint32_t a = lo[v];
      if (a & kDone) continue;
      const uint32_t b = hi[v];
      if (a >= v || b <= v || b > last) {
        lo[v] = a | kDone;
        continue;
      }
      const u64 key = best[p * stride + a];
      bool le_eps = true;
      uint32_t split = 0;
      if (key) {
        const int2 sp = point(a), ep = point(b);
        const double dx = (double)(ep.x - sp.x), dy = (double)(ep.y - sp.y);
        const double max_dist = (double)(key >> 32);
        le_eps = max_dist * max_dist <= eps * (dx * dx + dy * dy);
        split = kNone - (uint32_t)key;
      }
      if (le_eps || split <= a || split >= b) {
        lo[v] = a | kDone;
      } else if (v == split) {
        lo[v] = v | kDone;
        hi[v] = v;
        kept_one = true;
      } else {
        if (v < split) hi[v] = split;
        else lo[v] = split;
        open_lo = min(open_lo, v);
        open_hi = max(open_hi, v);
      }
    }
    if (kept_one) sh->any[p] = 1u;
    if (open_lo <= open_hi) {
      atomicMin(&sh->window_lo[q], open_lo);
      atomicMax(&sh->window_hi[q], open_hi);
    }
    __syncthreads();
    if (!sh->any[p]) break;
    ++rounds;
  }
  __syncthreads();
  // the kept vertices in order; a closed curve does not repeat its start
  const uint32_t limit = g.closed ? last : last + 1u;
  uint32_t running = 0;
  for (uint32_t v0 = 0; v0 < limit; v0 += (uint32_t)T) {
    const uint32_t v = v0 + tid;
    const bool keep = v < limit && (lo[v] & kIndexMask) == v;
    const u64 mask = __ballot(keep);
    const uint32_t before = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    uint32_t offset = 0, total = (uint32_t)__popcll(mask);
    if (T > 64) {
      if (lane == 0) sh->wave_count[tid >> 6] = total;
      __syncthreads();
      total = 0;
      for (uint32_t w = 0; w < (uint32_t)T / 64u; ++w) {
        const uint32_t c = sh->wave_count[w];
        if (w < (tid >> 6)) offset += c;
        total += c;
      }
      __syncthreads();
    }
    if (keep) {
      const uint32_t at = running + offset + before;
      if (at <= count) {
        m.kept[g.slot + at] = point(v);
        m.kseg[g.slot + at] = s;
      }
    }
    running += total;
  }
  if (tid == 0) {
    m.kcount[s] = min(running, count + 1u);
    m.rounds[s] = rounds;
  }
}

__global__ __launch_bounds__(kSimplifyWave) void k_simplify_dp_wave(SimplifyView m, SimplifyStatus* __restrict__ status) {
  __shared__ uint32_t lo[kSimplifyWavePoints + 1], hi[kSimplifyWavePoints + 1];
  __shared__ u64 best[2 * (kSimplifyWavePoints + 1)];
  __shared__ RoundShared sh;
  const uint32_t s = blockIdx.x;
  if (s >= m.n_segments) return;
  const SegmentOf g = Load(m, s);
  if (!g.ok) {
    if (threadIdx.x == 0) {
      Flag(status);
      m.kcount[s] = 0;
      m.rounds[s] = 0;
      m.sflag[s] = 0;
    }
    return;
  }
  if (Collapses(m, g)) {
    if (threadIdx.x == 0) {
      m.kept[g.slot] = m.vertices[g.first];
      m.kept[g.slot + 1u] = m.vertices[g.first + g.count - 1u];
      m.kseg[g.slot] = m.kseg[g.slot + 1u] = s;
      m.kcount[s] = 2u;
      m.rounds[s] = 0;
      m.sflag[s] = 1u;
    }
    return;
  }
  if (threadIdx.x == 0) m.sflag[s] = 0;
  if (g.count > (uint32_t)kSimplifyWavePoints) {
    if (threadIdx.x == 0) {
      const uint32_t k = atomicAdd(&status->long_segments, 1u);
      if (k < m.n_segments) m.long_list[k] = s;
    }
    return;
  }
  DpSegment<kSimplifyWave>(m, s, g, lo, hi, best, (uint32_t)kSimplifyWavePoints + 1u, &sh);
}

__global__ __launch_bounds__(kSimplifyBlock) void k_simplify_dp_block(SimplifyView m, SimplifyStatus* __restrict__ status) {
  __shared__ uint32_t lo[kSimplifyLdsPoints + 1], hi[kSimplifyLdsPoints + 1];
  __shared__ u64 best[2 * (kSimplifyLdsPoints + 1)];
  __shared__ RoundShared sh;
  const uint32_t n_long = min(status->long_segments, m.n_segments);
  for (uint32_t k = blockIdx.x; k < n_long; k += gridDim.x) {
    const uint32_t s = m.long_list[k];
    if (s >= m.n_segments) {
      if (threadIdx.x == 0) Flag(status);
      continue;
    }
    const SegmentOf g = Load(m, s);
    if (!g.ok) continue;                           // flagged by the wavefront that listed it
    __syncthreads();
    if (g.count <= (uint32_t)kSimplifyLdsPoints) {
      DpSegment<kSimplifyBlock>(m, s, g, lo, hi, best, (uint32_t)kSimplifyLdsPoints + 1u, &sh);
    } else {
      // slot + count + 1 <= slots: a segment has one slot more than it has vertices
      DpSegment<kSimplifyBlock>(m, s, g, m.lo + g.slot, m.hi + g.slot, m.best + 2 * (size_t)g.slot, g.count + 1u, &sh);
    }
  }
}

// The host's last stage, for segment s in place: reads run ahead of the writes, and the last read of a closed
// list wraps around to what was written first.
__global__ __launch_bounds__(kTableBlock) void k_simplify_clean(SimplifyView m, uint32_t* __restrict__ ncount) {
  const uint32_t s = blockIdx.x * (uint32_t)kTableBlock + threadIdx.x;
  if (s >= m.n_segments) return;
  const SegmentOf g = Load(m, s);
  const uint32_t cnt = g.ok ? min(m.kcount[s], g.count + 1u) : 0u;
  if (cnt == 0 || m.sflag[s]) {
    ncount[s] = cnt;
    return;
  }
  int2* d = m.kept + g.slot;
  const double eps = m.eps;
  const bool closed = g.closed;
  uint32_t new_count = cnt;
  uint32_t rd = closed ? cnt - 1u : 0u;
  auto read = [&]() {
    const int2 v = d[rd];
    if (++rd >= cnt) rd = 0;
    return v;
  };
  int2 start_pt = read();
  uint32_t wr = rd;
  int2 pt = read();
  const uint32_t end = closed ? cnt : cnt - 1u;
  for (uint32_t i = closed ? 0u : 1u; i < end && new_count > 2u; ++i) {
    const int2 end_pt = read();
    const double dx = (double)(end_pt.x - start_pt.x), dy = (double)(end_pt.y - start_pt.y);
    const double dist = fabs((double)(pt.x - start_pt.x) * dy - (double)(pt.y - start_pt.y) * dx);
    const double successive_inner_product = (double)(pt.x - start_pt.x) * (double)(end_pt.x - pt.x) +
                                            (double)(pt.y - start_pt.y) * (double)(end_pt.y - pt.y);
    if (dist * dist <= 0.5 * eps * (dx * dx + dy * dy) && dx != 0 && dy != 0 && successive_inner_product >= 0) {
      --new_count;
      d[wr] = start_pt = end_pt;
      if (++wr >= cnt) wr = 0;
      pt = read();
      ++i;
      continue;
    }
    d[wr] = start_pt = pt;
    if (++wr >= cnt) wr = 0;
    pt = end_pt;
  }
  if (!closed) d[wr] = pt;
  ncount[s] = new_count;
}

__global__ __launch_bounds__(kTableBlock) void k_simplify_compact(SimplifyView m, const uint32_t* __restrict__ ncount,
                                                                  const uint32_t* __restrict__ nfirst,
                                                                  int2* __restrict__ out) {
  const uint32_t q = blockIdx.x * (uint32_t)kTableBlock + threadIdx.x;
  if (q >= m.slots) return;
  const uint32_t s = m.kseg[q];
  if (s >= m.n_segments) return;                   // a slot no vertex was kept in
  const uint32_t slot = (uint32_t)m.segments[(size_t)s * kMeshSegmentWords + 2] + s;
  if (q < slot) return;
  const uint32_t k = q - slot;
  if (k >= ncount[s]) return;
  const uint32_t at = nfirst[s] + k;
  if (at < m.slots) out[at] = m.kept[q];
}

__global__ __launch_bounds__(kTableBlock) void k_simplify_records(SimplifyView m, const uint32_t* __restrict__ ncount,
                                                                  const uint32_t* __restrict__ nfirst,
                                                                  int32_t* __restrict__ segments_out,
                                                                  SimplifyStatus* __restrict__ status) {
  const uint32_t s = blockIdx.x * (uint32_t)kTableBlock + threadIdx.x;
  uint32_t kept = 0, rounds = 0, longest = 0;
  bool collapsed = false, single = false;
  if (s < m.n_segments) {
    const int32_t* rec = m.segments + (size_t)s * kMeshSegmentWords;
    int32_t* out = segments_out + (size_t)s * kMeshSegmentWords;
    const uint32_t c = ncount[s], f = nfirst[s];
    for (int k = 0; k < kMeshSegmentWords; ++k) out[k] = k == 2 ? (int32_t)f : k == 3 ? (int32_t)c : rec[k];
    if (c == 0 || (rec[5] == 0 && c < 2u)) Flag(status);
    kept = m.kcount[s];
    rounds = m.rounds[s];
    longest = (uint32_t)rec[3];
    collapsed = m.sflag[s] != 0;
    single = rec[5] != 0 && c == 1u;
    if (s == m.n_segments - 1u) status->vertices_out = f + c;
  }
  const uint32_t n_collapsed = (uint32_t)__popcll(__ballot(collapsed)), n_single = (uint32_t)__popcll(__ballot(single));
  kept = WaveSum(kept);
  rounds = WaveMax(rounds);
  longest = WaveMax(longest);
  if ((threadIdx.x & 63) == 0) {
    if (n_collapsed) atomicAdd(&status->collapsed, n_collapsed);
    if (n_single) atomicAdd(&status->single_closed, n_single);
    if (kept) atomicAdd(&status->vertices_kept, kept);
    if (rounds) atomicMax(&status->max_rounds, rounds);
    if (longest) atomicMax(&status->longest_in, longest);
  }
}

inline dim3 GridOf(uint32_t n) { return dim3((std::max(n, 1u) + kTableBlock - 1) / kTableBlock); }

}  // namespace

hipError_t SimplifyDp(const SimplifyView& m, SimplifyStatus* status, hipStream_t stream) {
  const hipError_t e = hipMemsetAsync(m.kseg, 0xff, (size_t)m.slots * sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_simplify_dp_wave, dim3(m.n_segments), dim3(kSimplifyWave), 0, stream, m, status);
  hipLaunchKernelGGL(k_simplify_dp_block, dim3(kSimplifyLongGrid), dim3(kSimplifyBlock), 0, stream, m, status);
  return hipGetLastError();
}

hipError_t SimplifyClean(const SimplifyView& m, uint32_t* ncount, hipStream_t stream) {
  hipLaunchKernelGGL(k_simplify_clean, GridOf(m.n_segments), dim3(kTableBlock), 0, stream, m, ncount);
  return hipGetLastError();
}

hipError_t SimplifyTables(void* temp, size_t temp_bytes, const SimplifyView& m, const uint32_t* ncount, uint32_t* nfirst,
                          int32_t* segments_out, int32_t* vertices_out, SimplifyStatus* status, hipStream_t stream) {
  const hipError_t e = ExclusiveSumU32(temp, temp_bytes, ncount, nfirst, (int)m.n_segments, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_simplify_compact, GridOf(m.slots), dim3(kTableBlock), 0, stream, m, ncount, nfirst,
                     reinterpret_cast<int2*>(vertices_out));
  hipLaunchKernelGGL(k_simplify_records, GridOf(m.n_segments), dim3(kTableBlock), 0, stream, m, ncount, nfirst,
                     segments_out, status);
  return hipGetLastError();
}

}  // namespace vsg_render_impl
