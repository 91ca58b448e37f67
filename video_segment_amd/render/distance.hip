// distance.hip -- the exact Euclidean distance transform of an edge set (gfx950), squared and in integers,
// and what the boundary benchmark counts with it.
//
//   k_dist_classify  an int32 plane -> its edge set (differs from the in-frame right or below neighbour) as
//                    one 32-bit word per column and chunk of 32 rows, bit r = row 32 * chunk + r; the count
//   k_dist_columns   the words -> g^2, g the vertical distance to the nearest edge pixel of the column
//   k_dist_rows      g^2 of a row (in LDS, with the minima of its groups of 32 columns) -> D = min over the
//                    row's columns u of (x - u)^2 + g(u)^2
//   k_dist_match     the persistence plane Q (and D of the other plane's edge set G) -> the histograms of Q
//                    over all pixels and over the pixels with D <= T
//   k_dist_disc      at the pixels of G: the maximum of Q over the disc of squared radius T, from an LDS tile
//                    of 16-bit values with a halo -> its histogram
//   k_dist_scores    one block: the three histograms' suffix sums are the levels' records
//
// The words are the whole interface between the passes: a column's chunk is one register, "the last edge row
// at or above" and "the first at or below" inside a chunk are a clz and a ctz, and a chunk without a bit is
// skipped with one load.  Every squared distance is below 2 * 32767^2 < 2^31; "none" is 0x7fffffff and is
// never added to.
#include "render.h"

namespace vsg_render_impl {

namespace {

constexpr int kRowsPerChunk = kDistChunkRows;
constexpr int kColumnsPerBlock = 256;
constexpr int32_t kNone = kDistanceNone;

// A thread a column's chunk: reads its 32 rows top down (lanes along x, so every load of a wave is one
// row segment), the right neighbour in the same row and the value below, which the next step reuses.
// clamp: every negative value is -1.
__global__ __launch_bounds__(kColumnsPerBlock) void k_dist_classify(const int32_t* __restrict__ plane, size_t pitch,
                                                                    int W, int H, int clamp,
                                                                    uint32_t* __restrict__ words,
                                                                    DistStatus* __restrict__ status) {
  __shared__ uint32_t s_counts[kColumnsPerBlock / 64];
  const int x = blockIdx.x * kColumnsPerBlock + threadIdx.x;
  const int chunk = blockIdx.y;
  const int y0 = chunk * kRowsPerChunk;
  uint32_t word = 0;
  if (x < W && y0 < H) {
    const bool has_right = x + 1 < W;
    const int32_t* p = plane + (size_t)y0 * pitch + x;
    int32_t cur = p[0];
    if (clamp) cur = max(cur, -1);
    const int rows = min(kRowsPerChunk, H - y0);
    for (int r = 0; r < rows; ++r) {
      int32_t right = cur, below = cur;
      if (has_right) {
        right = p[1];
        if (clamp) right = max(right, -1);
      }
      if (y0 + r + 1 < H) {
        below = p[pitch];
        if (clamp) below = max(below, -1);
      }
      if (cur != right || cur != below) word |= 1u << r;
      cur = below;
      p += pitch;
    }
    words[(size_t)chunk * W + x] = word;
  }
  uint32_t n = __popc(word);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off, 64);
  if ((threadIdx.x & 63) == 0) s_counts[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t sum = 0;
    for (int k = 0; k < kColumnsPerBlock / 64; ++k) sum += s_counts[k];
    if (sum) atomicAdd(&status->edge_pixels, (unsigned long long)sum);
  }
}

// A thread a column's chunk again.  The nearest edge row above the chunk and below it come from the other
// chunks' words, nearest first, one load per chunk passed; inside the chunk the word answers.
__global__ __launch_bounds__(kColumnsPerBlock) void k_dist_columns(const uint32_t* __restrict__ words, int W, int H,
                                                                   int chunks, int32_t* __restrict__ gsq) {
  const int x = blockIdx.x * kColumnsPerBlock + threadIdx.x;
  const int chunk = blockIdx.y;
  const int y0 = chunk * kRowsPerChunk;
  if (x >= W || y0 >= H) return;
  const uint32_t word = words[(size_t)chunk * W + x];
  int above = -1, below = -1;   // rows, -1: none
  for (int c = chunk - 1; c >= 0; --c) {
    const uint32_t w = words[(size_t)c * W + x];
    if (w) {
      above = c * kRowsPerChunk + 31 - __clz((int)w);
      break;
    }
  }
  for (int c = chunk + 1; c < chunks; ++c) {
    const uint32_t w = words[(size_t)c * W + x];
    if (w) {
      below = c * kRowsPerChunk + __ffs((int)w) - 1;
      break;
    }
  }
  const int rows = min(kRowsPerChunk, H - y0);
  int32_t* o = gsq + (size_t)y0 * W + x;
  for (int r = 0; r < rows; ++r) {
    const int y = y0 + r;
    const uint32_t upto = word & (0xffffffffu >> (31 - r));   // rows y0 .. y
    const uint32_t from = word >> r;                          // rows y .. y0 + 31
    const int up = upto ? y0 + 31 - __clz((int)upto) : above;
    const int down = from ? y + __ffs((int)from) - 1 : below;
    int g = -1;
    if (up >= 0) g = y - up;
    if (down >= 0 && (g < 0 || down - y < g)) g = down - y;
    *o = g < 0 ? kNone : g * g;   // g <= 32767
    o += W;
  }
}

constexpr int kRowBlock = 256;
constexpr int kRowGroup = 32;   // columns that share one entry of the row's minima

__host__ __device__ constexpr size_t RowBytes(int width) { return ((size_t)width * sizeof(int32_t) + 15) / 16 * 16; }

// One side of a pixel's search: the columns u = x + step, x + 2 step, ... (step -1 or +1) down to / up to
// `last`.  A column d away cannot give less than d^2, so the side ends at the first d with d^2 >= best.  A
// group of kRowGroup columns whose smallest g^2 plus the square of its nearest column's distance is no better
// than best is passed with that one read; "none" is skipped, never added to.
__device__ __forceinline__ int32_t SearchSide(const int32_t* s_row, const int32_t* s_min, int x, int step, int last,
                                              int32_t best) {
  int u = x + step;
  while (step < 0 ? u >= last : u <= last) {
    int d = step < 0 ? x - u : u - x;
    if (d * d >= best) break;
    const int group = u / kRowGroup;
    const int end = step < 0 ? max(group * kRowGroup, last) : min(group * kRowGroup + kRowGroup - 1, last);
    const int32_t m = s_min[group];
    if (m == kNone || m + d * d >= best) {
      u = end + step;
      continue;
    }
    for (; step < 0 ? u >= end : u <= end; u += step) {
      d = step < 0 ? x - u : u - x;
      const int dd = d * d;
      if (dd >= best) return best;
      const int32_t c = s_row[u];
      if (c != kNone) best = min(best, c + dd);
    }
  }
  return best;
}

// A block a row; the row's g^2 in LDS (dynamic: W int32, up to 128 KiB) and behind it the minimum of every
// group of 32 columns, taken with shuffles while the row is loaded.  A thread a pixel at a time: from
// best = g(x)^2 it searches to the left and to the right.  Every sum is at most 32767^2 + 32767^2.
__global__ __launch_bounds__(kRowBlock) void k_dist_rows(const int32_t* __restrict__ gsq, int W,
                                                         int32_t* __restrict__ out, DistStatus* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_dynamic[];
  int32_t* s_row = reinterpret_cast<int32_t*>(s_dynamic);
  int32_t* s_min = reinterpret_cast<int32_t*>(s_dynamic + RowBytes(W));
  const size_t row = (size_t)blockIdx.x * W;
  for (int base = 0; base < W; base += kRowBlock) {   // every lane takes part in the shuffles
    const int x = base + threadIdx.x;
    const int32_t v = x < W ? gsq[row + x] : kNone;
    if (x < W) s_row[x] = v;
    int32_t m = v;
#pragma unroll
    for (int off = kRowGroup / 2; off > 0; off >>= 1) m = min(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & (kRowGroup - 1)) == 0 && x < W) s_min[x / kRowGroup] = m;
  }
  __syncthreads();
  uint32_t largest = 0;
  for (int x = threadIdx.x; x < W; x += kRowBlock) {
    int32_t best = s_row[x];
    best = SearchSide(s_row, s_min, x, -1, 0, best);
    best = SearchSide(s_row, s_min, x, 1, W - 1, best);
    out[row + x] = best;
    if (best != kNone) largest = max(largest, (uint32_t)best);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) largest = max(largest, (uint32_t)__shfl_down(largest, off, 64));
  if ((threadIdx.x & 63) == 0 && largest) atomicMax(&status->max_distance, largest);
}

constexpr int kMatchBlock = 256;
constexpr int kLdsBins = 1024;   // histograms of up to this many bins are gathered in LDS first

// hist[bin] += 1 for every lane of the wavefront with bin >= 0, one atomic per distinct bin among them: the
// lanes of a wavefront are neighbouring pixels and mostly agree.  Every lane of the wavefront calls it.
__device__ __forceinline__ void WaveHistogram(uint32_t* hist, int bin) {
  unsigned long long todo = __ballot(bin >= 0);
  const int lane = threadIdx.x & 63;
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int value = __shfl(bin, leader, 64);
    const unsigned long long same = __ballot(bin == value);
    if (lane == leader) atomicAdd(&hist[value], (uint32_t)__popcll(same));
    todo &= ~same;
  }
}

constexpr int kMatchPerThread = 32;   // pixels of Q a thread of k_dist_match looks at

// A block 256 * 32 consecutive pixels of Q (rows W apart): hist_all[Q] += 1 where Q > 0, and hist_near[Q] += 1
// where also D <= T (d null: no pixel is near).  Both histograms have L + 1 entries; a Q outside [0, L] raises
// the flag.  Up to kLdsBins entries the block gathers both in LDS and adds what is not zero once, so that the
// adds to one word of the result number a few per block, not one per wavefront.
__global__ __launch_bounds__(kMatchBlock) void k_dist_match(const int32_t* __restrict__ q,
                                                            const int32_t* __restrict__ d, uint32_t n, int L, int T,
                                                            uint32_t* __restrict__ hist_all,
                                                            uint32_t* __restrict__ hist_near,
                                                            DistStatus* __restrict__ status) {
  __shared__ uint32_t s_hist[2][kLdsBins];
  const int bins = L + 1;
  const bool gather = bins <= kLdsBins;
  if (gather) {
    for (int k = threadIdx.x; k < bins; k += kMatchBlock) s_hist[0][k] = s_hist[1][k] = 0;
    __syncthreads();
  }
  uint32_t* all = gather ? s_hist[0] : hist_all;
  uint32_t* near_to = gather ? s_hist[1] : hist_near;
  const size_t base = (size_t)blockIdx.x * (kMatchBlock * kMatchPerThread) + threadIdx.x;
  uint32_t flags = 0;
  for (int i = 0; i < kMatchPerThread; ++i) {
    const size_t p = base + (size_t)i * kMatchBlock;
    int bin = -1, near = -1;
    if (p < n) {
      const int32_t v = q[p];
      if (v < 0 || v > L) {
        flags = DIST_FLAG_RANGE;
      } else if (v > 0) {
        bin = v;
        if (d && d[p] <= T) near = v;
      }
    }
    WaveHistogram(all, bin);
    if (d) WaveHistogram(near_to, near);
  }
  if (flags) atomicOr(&status->flags, flags);
  if (!gather) return;
  __syncthreads();
  for (int k = threadIdx.x; k < bins; k += kMatchBlock) {
    const uint32_t a = s_hist[0][k], b = s_hist[1][k];
    if (a) atomicAdd(&hist_all[k], a);
    if (b) atomicAdd(&hist_near[k], b);
  }
}

constexpr int kDiscTileW = 64, kDiscTileH = kRowsPerChunk;   // a tile's rows are one chunk of the words
constexpr int kDiscLdsBins = 512;                            // with the widest halo: 61440 + 2048 bytes of LDS

// A block a tile of 64 x 32 pixels, which is 64 words of G.  A tile without a pixel of G ends at once.
// Otherwise Q of the tile and of a halo of `radius` pixels goes to LDS as 16-bit values (Q <= L <= 65535;
// 0 outside the frame, which changes no maximum), and every thread standing on a pixel of G takes the
// maximum over the rows dy of the disc, each row's half width the integer root of T - dy^2.  hist[M] += 1
// where M > 0.  Dynamic LDS: the tile, (64 + 2 radius) x (32 + 2 radius) uint16, at most 61440 bytes, then
// the block's histogram (kDiscLdsBins entries; its first word also says whether the tile has a pixel of G).
__global__ __launch_bounds__(kMatchBlock) void k_dist_disc(const int32_t* __restrict__ q,
                                                           const uint32_t* __restrict__ words, int W, int H, int L,
                                                           int T, int radius, uint32_t* __restrict__ hist,
                                                           DistStatus* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_dynamic[];
  const int tw = kDiscTileW + 2 * radius, th = kDiscTileH + 2 * radius;
  uint16_t* s_tile = reinterpret_cast<uint16_t*>(s_dynamic);
  uint32_t* s_hist = reinterpret_cast<uint32_t*>(s_dynamic + ((size_t)tw * th * 2 + 15) / 16 * 16);
  const int x0 = blockIdx.x * kDiscTileW, y0 = blockIdx.y * kDiscTileH;
  const int lx = threadIdx.x & 63;
  const int bins = L + 1;
  const bool gather = bins <= kDiscLdsBins;
  uint32_t word = 0;
  if (x0 + lx < W) word = words[(size_t)blockIdx.y * W + x0 + lx];
  if (threadIdx.x == 0) s_hist[0] = 0;
  __syncthreads();
  if (word != 0 && threadIdx.x < 64) s_hist[0] = 1;
  __syncthreads();
  const bool any = s_hist[0] != 0;
  __syncthreads();
  if (!any) return;
  uint32_t flags = 0;
  for (int k = threadIdx.x; k < tw * th; k += kMatchBlock) {
    const int ty = k / tw, tx = k - ty * tw;
    const int gx = x0 - radius + tx, gy = y0 - radius + ty;
    int32_t v = 0;
    if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
      v = q[(size_t)gy * W + gx];
      if (v < 0 || v > L) {
        flags = DIST_FLAG_RANGE;
        v = 0;
      }
    }
    s_tile[k] = (uint16_t)v;
  }
  if (flags) atomicOr(&status->flags, flags);
  if (gather) {
    for (int k = threadIdx.x; k < bins; k += kMatchBlock) s_hist[k] = 0;
  }
  __syncthreads();
  // a thread has column lx and the rows wave, wave + 4, ... of the tile
  for (int ly = threadIdx.x >> 6; ly < kDiscTileH; ly += kMatchBlock / 64) {
    uint32_t best = 0;
    if (word >> ly & 1u) {
      for (int dy = -radius; dy <= radius; ++dy) {
        const int rem = T - dy * dy;
        if (rem < 0) continue;
        int half = (int)sqrtf((float)rem);
        while (half * half > rem) --half;
        while ((half + 1) * (half + 1) <= rem) ++half;
        const uint16_t* t = s_tile + (size_t)(ly + radius + dy) * tw + lx + radius;
        for (int dx = -half; dx <= half; ++dx) best = max(best, (uint32_t)t[dx]);
      }
    }
    WaveHistogram(gather ? s_hist : hist, best > 0 ? (int)best : -1);   // the wavefront is one row of the tile
  }
  if (!gather) return;
  __syncthreads();
  for (int k = threadIdx.x; k < bins; k += kMatchBlock) {
    const uint32_t n = s_hist[k];
    if (n) atomicAdd(&hist[k], n);
  }
}

// scores[l] = {sum of hist_all over p > l, of hist_near, status->edge_pixels, sum of hist_disc}, l in [0, L):
// k_persist_sides' scheme, three sums at once.  One block.
__global__ __launch_bounds__(kMatchBlock) void k_dist_scores(const uint32_t* __restrict__ hist_all,
                                                             const uint32_t* __restrict__ hist_near,
                                                             const uint32_t* __restrict__ hist_disc, int L,
                                                             const DistStatus* __restrict__ status,
                                                             long long* __restrict__ scores) {
  __shared__ unsigned long long s_sum[3][kMatchBlock];
  const int t = threadIdx.x;
  const int chunk = (L + kMatchBlock - 1) / kMatchBlock;
  const int begin = min(t * chunk, L), end = min(begin + chunk, L);
  const uint32_t* hist[3] = {hist_all, hist_near, hist_disc};
  for (int k = 0; k < 3; ++k) {
    unsigned long long mine = 0;
    for (int l = begin; l < end; ++l) mine += hist[k][l + 1];
    s_sum[k][t] = mine;
  }
  __syncthreads();
  unsigned long long acc[3] = {0, 0, 0};
  for (int k = 0; k < 3; ++k) {
    for (int u = t + 1; u < kMatchBlock; ++u) acc[k] += s_sum[k][u];
  }
  const long long other_edges = (long long)status->edge_pixels;
  for (int l = end - 1; l >= begin; --l) {
    for (int k = 0; k < 3; ++k) acc[k] += hist[k][l + 1];
    long long* o = scores + (size_t)l * kBoundaryScoreWords;
    o[0] = (long long)acc[0];
    o[1] = (long long)acc[1];
    o[2] = other_edges;
    o[3] = (long long)acc[2];
  }
}

}  // namespace

int DistChunks(int height) { return (height + kRowsPerChunk - 1) / kRowsPerChunk; }

void LaunchDistClassify(const int32_t* plane, size_t pitch, int width, int height, bool clamp, uint32_t* words,
                        DistStatus* status, hipStream_t stream) {
  const dim3 grid((width + kColumnsPerBlock - 1) / kColumnsPerBlock, DistChunks(height));
  hipLaunchKernelGGL(k_dist_classify, grid, dim3(kColumnsPerBlock), 0, stream, plane, pitch, width, height,
                     clamp ? 1 : 0, words, status);
}

void LaunchDistColumns(const uint32_t* words, int width, int height, int32_t* gsq, hipStream_t stream) {
  const dim3 grid((width + kColumnsPerBlock - 1) / kColumnsPerBlock, DistChunks(height));
  hipLaunchKernelGGL(k_dist_columns, grid, dim3(kColumnsPerBlock), 0, stream, words, width, height,
                     DistChunks(height), gsq);
}

hipError_t LaunchDistRows(const int32_t* gsq, int width, int height, int32_t* out, DistStatus* status,
                          hipStream_t stream) {
  const size_t groups = ((size_t)width + kRowGroup - 1) / kRowGroup;
  const size_t lds = RowBytes(width) + (groups * sizeof(int32_t) + 15) / 16 * 16;
  if (lds > 64 * 1024) {   // beyond what a kernel may ask for without saying so; 132 KiB at the widest frame
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_dist_rows),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_dist_rows, dim3(height), dim3(kRowBlock), lds, stream, gsq, width, out, status);
  return hipGetLastError();
}

void LaunchDistMatch(const int32_t* q, const int32_t* d, int width, int height, int levels, int tolerance_sq,
                     uint32_t* hist_all, uint32_t* hist_near, DistStatus* status, hipStream_t stream) {
  const uint32_t n = (uint32_t)width * (uint32_t)height;
  const uint32_t span = kMatchBlock * kMatchPerThread;
  hipLaunchKernelGGL(k_dist_match, dim3((n + span - 1) / span), dim3(kMatchBlock), 0, stream, q, d, n,
                     levels, tolerance_sq, hist_all, hist_near, status);
}

int DistRadius(int tolerance_sq) {
  int r = 0;
  while ((r + 1) * (r + 1) <= tolerance_sq) ++r;
  return r;
}

void LaunchDistDisc(const int32_t* q, const uint32_t* words, int width, int height, int levels, int tolerance_sq,
                    uint32_t* hist, DistStatus* status, hipStream_t stream) {
  const int radius = DistRadius(tolerance_sq);
  const size_t tile = (size_t)(kDiscTileW + 2 * radius) * (kDiscTileH + 2 * radius) * sizeof(uint16_t);
  const size_t lds = (tile + 15) / 16 * 16 + kDiscLdsBins * sizeof(uint32_t);
  const dim3 grid((width + kDiscTileW - 1) / kDiscTileW, DistChunks(height));
  hipLaunchKernelGGL(k_dist_disc, grid, dim3(kMatchBlock), lds, stream, q, words, width, height, levels,
                     tolerance_sq, radius, hist, status);
}

void LaunchDistScores(const uint32_t* hist_all, const uint32_t* hist_near, const uint32_t* hist_disc, int levels,
                      const DistStatus* status, long long* scores, hipStream_t stream) {
  hipLaunchKernelGGL(k_dist_scores, dim3(1), dim3(kMatchBlock), 0, stream, hist_all, hist_near, hist_disc, levels,
                     status, scores);
}

}  // namespace vsg_render_impl
