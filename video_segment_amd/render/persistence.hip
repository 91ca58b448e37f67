// persistence.hip -- boundary persistence (gfx950): for how many hierarchy levels a pixel side, or an edge
// of the level-0 adjacency graph, still separates two regions.
//
//   k_persist_plane    the level-0 plane painted with dense region numbers -> the persistence plane Q and
//                      the counts of Q > 0 and Q == L; a thread a tile of 4 x 4 pixels
//   k_persist_compose  Q and the source frame -> BGR24 rows
//   k_persist_edges    one thread per directed edge of the level-0 graph: its persistence, and its
//                      shared sides into a histogram over persistence values
//   k_persist_sides    one block: the histogram's suffix sums, halved, are the levels' boundary lengths
//
// The ancestor table (persistence_table.h) has L - 1 rows of R int32, row l - 1 holding A_l of every
// region.  "A_l(a) != A_l(b)" is monotone in l: true at 0 for a != b, and once false it stays false.  The
// persistence of a pair is the first l at which it is false, or L; Persistence() finds it by bisection,
// with two 4-byte gathers per step and none when L = 1.
#include "render.h"

namespace vsg_render_impl {

namespace {

// pers(a, b) of two dense region numbers (negative: no region).  table is not looked at when L == 1.
__device__ __forceinline__ int Persistence(int32_t a, int32_t b, const int32_t* __restrict__ table, uint32_t R,
                                           int L, uint32_t* flags) {
  if (a == b) return 0;
  if (a < 0 || b < 0) return L;
  if ((uint32_t)a >= R || (uint32_t)b >= R) {   // not a number the host gave out
    *flags |= PERS_FLAG_RANGE;
    return 0;
  }
  int lo = 0, hi = L;   // they differ at lo; they are equal at hi, or hi == L
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    const int32_t* row = table + (size_t)(mid - 1) * R;
    if (row[a] != row[b]) lo = mid;
    else hi = mid;
  }
  return hi;
}

constexpr int kTileX = 4, kTileY = 4;

// The tiling of k_render_compose: a thread reads the numbers of its 4 x 4 pixels, of the column to their
// right and of the row below (clamped to the last row, which so finds no difference below) and decides
// Q = max(pers(right), pers(below)) where either differs.  The plane has PlanePitch's spare columns, so
// both loads of a row stay inside it; columns >= W hold -1 and are masked.  q_vector: q and q_pitch
// allow a 16-byte store per tile row.
__global__ __launch_bounds__(256) void k_persist_plane(const int32_t* __restrict__ plane, int pitch, int W, int H,
                                                       const int32_t* __restrict__ table, uint32_t R, int L,
                                                       int32_t* __restrict__ q, size_t q_pitch, int q_vector,
                                                       PersStatus* __restrict__ status) {
  __shared__ uint32_t s_counts[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x0 = (blockIdx.x * 64 + lane) * kTileX;
  const int y0 = (blockIdx.y * 4 + wave) * kTileY;
  uint32_t edge = 0, top = 0, flags = 0;
  if (x0 < W && y0 < H) {
    const bool full = x0 + kTileX <= W;
    const int npx = full ? kTileX : W - x0;
    const int32_t* p = plane + (size_t)y0 * pitch + x0;
    int4 cur = *reinterpret_cast<const int4*>(p);
    int32_t cur_right = p[4];
#pragma unroll
    for (int ry = 0; ry < kTileY; ++ry) {
      const int y = y0 + ry;
      if (y >= H) break;
      const int yb = min(y + 1, H - 1);
      const int32_t* pb = plane + (size_t)yb * pitch + x0;
      const int4 below = *reinterpret_cast<const int4*>(pb);
      const int32_t below_right = pb[4];
      const int32_t c[5] = {cur.x, cur.y, cur.z, cur.w, cur_right};
      const int32_t d[4] = {below.x, below.y, below.z, below.w};
      int32_t out[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        int v = 0;
        if (x0 + k < W) {
          if (x0 + k + 1 < W && c[k] != c[k + 1]) v = Persistence(c[k], c[k + 1], table, R, L, &flags);
          if (c[k] != d[k]) v = max(v, Persistence(c[k], d[k], table, R, L, &flags));
          edge += v > 0;
          top += v == L;
        }
        out[k] = v;
      }
      int32_t* o = q + (size_t)y * q_pitch + x0;
      if (full && q_vector) {
        *reinterpret_cast<int4*>(o) = make_int4(out[0], out[1], out[2], out[3]);
      } else {
        for (int k = 0; k < npx; ++k) o[k] = out[k];
      }
      cur = below;
      cur_right = below_right;
    }
  }
  // a thread has at most 16 of either: both sums of a block fit 16 bits each
  uint32_t packed = edge | top << 16;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) packed += __shfl_down(packed, off, 64);
  if (lane == 0) s_counts[wave] = packed;
  if (flags) atomicOr(&status->flags, flags);
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t sum = s_counts[0] + s_counts[1] + s_counts[2] + s_counts[3];
    if (sum & 0xffffu) atomicAdd(&status->edge_pixels, (unsigned long long)(sum & 0xffffu));
    if (sum >> 16) atomicAdd(&status->top_pixels, (unsigned long long)(sum >> 16));
  }
}

struct alignas(4) PBytes12 {
  uint32_t w[3];
};

// (s * (L - q) + L / 2) / L; the two ends need no division.
__device__ __forceinline__ uint32_t Shade(uint32_t s, uint32_t q, uint32_t L) {
  if (q == 0) return s;
  if (q >= L) return 0u;
  return (s * (L - q) + L / 2) / L;
}

// Q (row pitch q_pitch, a multiple of 4 on a 16-byte aligned base) and the source frame -> BGR24.  src
// null: every source byte is 255.  ALIGNED: src, out and both strides are multiples of 4, full tiles are
// then moved as three dwords per row.
template <bool ALIGNED>
__global__ __launch_bounds__(256) void k_persist_compose(const int32_t* __restrict__ q, size_t q_pitch, int W, int H,
                                                         int L, const uint8_t* __restrict__ src, size_t src_stride,
                                                         uint8_t* __restrict__ out, size_t out_stride) {
  const int x0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * kTileX;
  const int y0 = (blockIdx.y * 4 + (threadIdx.x >> 6)) * kTileY;
  if (x0 >= W || y0 >= H) return;
  const bool full = x0 + kTileX <= W;
  const int npx = full ? kTileX : W - x0;
  const uint32_t height = (uint32_t)L;
#pragma unroll
  for (int ry = 0; ry < kTileY; ++ry) {
    const int y = y0 + ry;
    if (y >= H) break;
    const int32_t* qr = q + (size_t)y * q_pitch + x0;
    uint32_t v[4] = {0u, 0u, 0u, 0u};
    if (full) {
      const int4 t = *reinterpret_cast<const int4*>(qr);
      v[0] = (uint32_t)t.x, v[1] = (uint32_t)t.y, v[2] = (uint32_t)t.z, v[3] = (uint32_t)t.w;
    } else {
      for (int k = 0; k < npx; ++k) v[k] = (uint32_t)qr[k];
    }
    uint8_t* o = out + (size_t)y * out_stride + (size_t)x0 * 3;
    const uint8_t* s = src ? src + (size_t)y * src_stride + (size_t)x0 * 3 : nullptr;
    if (ALIGNED && full) {
      PBytes12 sv = {{0xffffffffu, 0xffffffffu, 0xffffffffu}};
      if (s) sv = *reinterpret_cast<const PBytes12*>(s);
      if ((v[0] | v[1] | v[2] | v[3]) != 0u) {   // no boundary in the tile row: the source as it is
        uint32_t byte[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) byte[k] = Shade((sv.w[k >> 2] >> (8 * (k & 3))) & 0xffu, v[k / 3], height);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          sv.w[k] = byte[4 * k] | byte[4 * k + 1] << 8 | byte[4 * k + 2] << 16 | byte[4 * k + 3] << 24;
        }
      }
      *reinterpret_cast<PBytes12*>(o) = sv;
    } else {
      for (int k = 0; k < npx * 3; ++k) o[k] = (uint8_t)Shade(s ? s[k] : 255u, v[k / 3], height);
    }
  }
}

constexpr int kEdgeBlock = 256;

// The column of region id `id` in the table: its rank among the n_ids sorted ids, or -1.
__device__ __forceinline__ int32_t ColumnOf(const int32_t* __restrict__ ids, uint32_t n_ids, int32_t id) {
  uint32_t lo = 0, hi = n_ids;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (ids[mid] < id) lo = mid + 1;
    else hi = mid;
  }
  return (lo < n_ids && ids[lo] == id) ? (int32_t)lo : -1;
}

// Edge e belongs to the last node whose first_edge is <= e (a node without edges starts where the next
// one does, so it is never the last).  persistence[e] = pers(the node's id, the neighbour's id);
// hist[p] += shared_n4.  hist has L + 1 entries.
__global__ __launch_bounds__(kEdgeBlock) void k_persist_edges(const int32_t* __restrict__ nodes, uint32_t n_nodes,
                                                              const int32_t* __restrict__ edges, uint32_t n_edges,
                                                              const int32_t* __restrict__ ids, uint32_t n_ids,
                                                              const int32_t* __restrict__ table, int L,
                                                              int32_t* __restrict__ persistence,
                                                              unsigned long long* __restrict__ hist,
                                                              PersStatus* __restrict__ status) {
  const uint32_t e = blockIdx.x * kEdgeBlock + threadIdx.x;
  if (e >= n_edges) return;
  uint32_t lo = 0, hi = n_nodes;   // first node with first_edge > e
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if ((uint32_t)nodes[(size_t)mid * kLevelNodeWords + 2] <= e) lo = mid + 1;
    else hi = mid;
  }
  uint32_t flags = 0;
  int p = 0;
  if (lo == 0) {
    flags = PERS_FLAG_RANGE;
  } else {
    const int32_t* node = nodes + (size_t)(lo - 1) * kLevelNodeWords;
    const int32_t* edge = edges + (size_t)e * kLevelEdgeWords;
    const int32_t a = ColumnOf(ids, n_ids, node[0]);
    const int32_t b = ColumnOf(ids, n_ids, edge[1]);
    if (a < 0 || b < 0 || a == b || e - (uint32_t)node[2] >= (uint32_t)node[3] || edge[2] < 0) {
      flags = PERS_FLAG_RANGE;
    } else {
      p = Persistence(a, b, table, n_ids, L, &flags);
      if (edge[2] > 0) atomicAdd(&hist[p], (unsigned long long)edge[2]);
    }
  }
  persistence[e] = p;
  if (flags) atomicOr(&status->flags, flags);
}

// level_sides[l] = half the sum of hist[p] over p > l (every side was added by both of its edges).  One
// block: a thread sums a contiguous chunk, the chunks' sums meet in LDS, the thread walks its chunk again
// from the top.
__global__ __launch_bounds__(kEdgeBlock) void k_persist_sides(const unsigned long long* __restrict__ hist, int L,
                                                              long long* __restrict__ level_sides) {
  __shared__ unsigned long long s_sum[kEdgeBlock];
  const int t = threadIdx.x;
  const int chunk = (L + kEdgeBlock - 1) / kEdgeBlock;
  const int begin = min(t * chunk, L), end = min(begin + chunk, L);
  unsigned long long mine = 0;
  for (int l = begin; l < end; ++l) mine += hist[l + 1];
  s_sum[t] = mine;
  __syncthreads();
  unsigned long long acc = 0;
  for (int u = t + 1; u < kEdgeBlock; ++u) acc += s_sum[u];
  for (int l = end - 1; l >= begin; --l) {
    acc += hist[l + 1];
    level_sides[l] = (long long)(acc / 2);
  }
}

}  // namespace

void LaunchPersistPlane(const int32_t* plane, int pitch, int width, int height, const int32_t* table,
                        uint32_t regions, int levels, int32_t* q, size_t q_pitch, PersStatus* status,
                        hipStream_t stream) {
  const int gx = ((width + kTileX - 1) / kTileX + 63) / 64;
  const int gy = ((height + kTileY - 1) / kTileY + 3) / 4;
  const int q_vector = ((uintptr_t)q % 16 == 0) && q_pitch % 4 == 0;
  hipLaunchKernelGGL(k_persist_plane, dim3(gx, gy), dim3(256), 0, stream, plane, pitch, width, height, table,
                     regions, levels, q, q_pitch, q_vector, status);
}

void LaunchPersistCompose(const int32_t* q, size_t q_pitch, int width, int height, int levels, const uint8_t* src,
                          size_t src_stride, uint8_t* out, size_t out_stride, hipStream_t stream) {
  const int gx = ((width + kTileX - 1) / kTileX + 63) / 64;
  const int gy = ((height + kTileY - 1) / kTileY + 3) / 4;
  const bool aligned = ((uintptr_t)out % 4 == 0) && out_stride % 4 == 0 &&
                       (!src || (((uintptr_t)src % 4 == 0) && src_stride % 4 == 0));
  if (aligned) {
    hipLaunchKernelGGL(k_persist_compose<true>, dim3(gx, gy), dim3(256), 0, stream, q, q_pitch, width, height,
                       levels, src, src_stride, out, out_stride);
  } else {
    hipLaunchKernelGGL(k_persist_compose<false>, dim3(gx, gy), dim3(256), 0, stream, q, q_pitch, width, height,
                       levels, src, src_stride, out, out_stride);
  }
}

void LaunchPersistEdges(const int32_t* nodes, uint32_t n_nodes, const int32_t* edges, uint32_t n_edges,
                        const int32_t* ids, uint32_t n_ids, const int32_t* table, int levels, int32_t* persistence,
                        unsigned long long* hist, PersStatus* status, hipStream_t stream) {
  if (n_edges == 0) return;
  hipLaunchKernelGGL(k_persist_edges, dim3((n_edges + kEdgeBlock - 1) / kEdgeBlock), dim3(kEdgeBlock), 0, stream,
                     nodes, n_nodes, edges, n_edges, ids, n_ids, table, levels, persistence, hist, status);
}

void LaunchPersistSides(const unsigned long long* hist, int levels, long long* level_sides, hipStream_t stream) {
  hipLaunchKernelGGL(k_persist_sides, dim3(1), dim3(kEdgeBlock), 0, stream, hist, levels, level_sides);
}

}  // namespace vsg_render_impl
