// edge_sort.hip -- K3 / K4 / K5: edge weights -> bucket keys, and the stable bucket sort of the
// edge slots (gfx950).  HBM-bound integer / light f32 work: coalesced plane loads, LDS staging,
// wave ballots; no MFMA.
//
// Reference behaviour restated (paths relative to the reference root):
//   segmentation/pixel_distance.h:141-157                (ColorDiff3L1 / ColorDiff3L2)
//   segmentation/segmentation_graph.h:158-162, 336       (bucket index, per-bucket push_back)
//   segmentation/dense_segmentation_graph.h:956-1142     (edge enumeration order)
// The reference appends every edge to the vector of its bucket in (scan order, neighbour order);
// an edge here is its *slot* (pix*4+k spatial, pix*9+k temporal), so a bucket list is the stable
// sort of the slot ids by bucket key.  With 2050 possible keys (buckets 0..2047, 2048 = virtual
// edges, one bin for edges that do not exist at the frame border) that is ONE counting sort:
//
//   K3/K4  per tile of 2048 / 1024 pixels: keys (u16 per slot, slot-major, written coalesced through
//          an LDS stage for the 9-key temporal case) + the tile's key histogram (LDS atomics),
//          stored as one dense row per tile:  hist[tile * 2050 + bin] -- 8 KB, coalesced, every
//          word written, so nothing zeroes the matrix first.          reads 12 (+12+8) B/px,
//                                                                        writes 8 / 18 B/px
//   scan   two launches for all lists of a frame.  k_hist_chunk_scan: a thread per (chunk of 64
//          tiles, bin) walks its column, leaves the exclusive prefix inside the chunk in place and
//          the chunk's total in chunk[c * 2050 + bin]; k_hist_chunk_bases turns the chunk totals
//          into offsets[bin] (start of every bin) and base[c][bin] = first output position of the
//          chunk's slots with that key.  No workgroup waits for another.
//   K5     per tile: one histogram per wavefront over its contiguous quarter of the tile, prefix
//          over the four wavefronts + hist row + base row (both read coalesced), then every
//          wavefront walks its quarter 64 slots at a time: the rank of a slot among the equal keys
//          of the step comes from one ballot per key bit that differs inside the step; the first
//          lane of every distinct bin takes the step's output range with a returning LDS add and
//          hands it to its group through a lane permute.  A wavefront's LDS operations execute in
//          issue order, so the adds of consecutive steps need no fence between them, and four
//          steps are in flight.  Stable by construction: tiles, quarters, steps and lanes are all
//          in slot order.  One grid covers the tiles of every list handed to the call.
//                                                                        reads 2 B, writes 4 B/slot
// No iota value array, no multi-pass radix sort: 8 B of traffic per slot instead of ~24.
#include "merge_common.h"

namespace vsg {

// Pixels per tile (one workgroup); the temporal tile is smaller so that its 9 keys per pixel stay
// a few steps per wavefront.
constexpr int kTilePxSpatial = 2048;
constexpr int kTilePxTemporal = 1024;
constexpr int kBinInvalid = kBucketSlots - 1; // 2049: slots of edges that do not exist
constexpr int kHistChunkTiles = 64;           // tiles (rows of the histogram matrix) per scan chunk

__device__ __forceinline__ float ColorDist(float ab, float ag, float ar, float bb, float bg,
                                           float br, int l1) {
  const float d1 = ab - bb, d2 = ag - bg, d3 = ar - br;
  if (l1) {
    // (fabs(d1)+fabs(d2)+fabs(d3)) * (1.0f/3.0f) evaluated in double (double fabs overloads).
    return (float)((fabs((double)d1) + fabs((double)d2) + fabs((double)d3)) *
                   (double)(1.0f / 3.0f));
  }
  return sqrtf((d1 * d1 + d2 * d2 + d3 * d3) * (1.0f / 3.0f));
}

__device__ __forceinline__ uint16_t BucketOf(float w) {
  const float scale = 2048.0f / (1.0f + 1e-6f);   // segmentation_graph.h:336
  return (uint16_t)(int)fminf(2048.0f, w * scale);
}

// x86 cvttss2si semantics for int(float): out of range / NaN -> INT_MIN.
__device__ __forceinline__ int TruncToIntX86(float v) {
  if (!(v < 2147483648.0f && v >= -2147483648.0f)) return (int)0x80000000;
  return (int)v;
}

// The tile's row of the matrix, every bin: 2050 consecutive words.
__device__ __forceinline__ void StoreTileHist(const int32_t* __restrict__ lds_hist, int tile,
                                              int32_t* __restrict__ hist) {
  int32_t* row = hist + (size_t)tile * kBucketSlots;
  for (int b = threadIdx.x; b < kBucketSlots; b += 256) row[b] = lds_hist[b];
}

// K3: slot = pix * 4 + k, k = 0 right, 1 bottom, 2 bottom-left, 3 bottom-right
// (AddSpatialEdgesImpl order, dense_segmentation_graph.h:971-996).
__global__ __launch_bounds__(256) void k_spatial_keys(const float* __restrict__ feat, int W, int H,
                                                       int l1, ushort4* __restrict__ keys,
                                                       int32_t* __restrict__ hist) {
  __shared__ int32_t lds_hist[kBucketSlots];
  for (int b = threadIdx.x; b < kBucketSlots; b += 256) lds_hist[b] = 0;
  __syncthreads();
  const size_t n = (size_t)W * H;
  const float* fb = feat;
  const float* fg = feat + n;
  const float* fr = feat + 2 * n;
  const size_t base = (size_t)blockIdx.x * kTilePxSpatial;
#pragma unroll 2
  for (int i = 0; i < kTilePxSpatial / 256; ++i) {
    const size_t pix = base + (size_t)i * 256 + threadIdx.x;
    if (pix >= n) break;
    const int y = (int)(pix / W), x = (int)(pix - (size_t)y * W);
    const float ab = fb[pix], ag = fg[pix], ar = fr[pix];
    ushort4 k4 = make_ushort4(kInvalidKey, kInvalidKey, kInvalidKey, kInvalidKey);
    const bool has_r = x < W - 1, has_b = y < H - 1, has_l = x > 0;
    if (has_r) {
      const size_t q = pix + 1;
      k4.x = BucketOf(ColorDist(ab, ag, ar, fb[q], fg[q], fr[q], l1));
    }
    if (has_b) {
      size_t q = pix + W;
      k4.y = BucketOf(ColorDist(ab, ag, ar, fb[q], fg[q], fr[q], l1));
      if (has_l) {
        q = pix + W - 1;
        k4.z = BucketOf(ColorDist(ab, ag, ar, fb[q], fg[q], fr[q], l1));
      }
      if (has_r) {
        q = pix + W + 1;
        k4.w = BucketOf(ColorDist(ab, ag, ar, fb[q], fg[q], fr[q], l1));
      }
    }
    keys[pix] = k4;
    atomicAdd(&lds_hist[k4.x == kInvalidKey ? kBinInvalid : k4.x], 1);
    atomicAdd(&lds_hist[k4.y == kInvalidKey ? kBinInvalid : k4.y], 1);
    atomicAdd(&lds_hist[k4.z == kInvalidKey ? kBinInvalid : k4.z], 1);
    atomicAdd(&lds_hist[k4.w == kInvalidKey ? kBinInvalid : k4.w], 1);
  }
  __syncthreads();
  StoreTileHist(lds_hist, blockIdx.x, hist);
}

// K4: slot = pix * 9 + (dy+1)*3 + (dx+1) around the (flow displaced) location in the previous
// slice (GetLocalEdges order TL,T,TR,L,C,R,BL,B,BR; dense_segmentation_graph.h:1011-1065,
// 1126-1135).  is_virtual: weight 1e10 -> bucket 2048 for every existing edge.
__global__ __launch_bounds__(256) void k_temporal_keys(const float* __restrict__ cur,
                                                        const float* __restrict__ prev,
                                                        const float* __restrict__ flow, int W,
                                                        int H, int l1, int is_virtual,
                                                        uint16_t* __restrict__ keys,
                                                        int32_t* __restrict__ prev_idx,
                                                        int32_t* __restrict__ hist) {
  __shared__ int32_t lds_hist[kBucketSlots];
  __shared__ __attribute__((aligned(16))) uint16_t stage[256 * 9];
  for (int b = threadIdx.x; b < kBucketSlots; b += 256) lds_hist[b] = 0;
  __syncthreads();
  const size_t n = (size_t)W * H;
  const size_t base = (size_t)blockIdx.x * kTilePxTemporal;
  for (int i = 0; i < kTilePxTemporal / 256; ++i) {
    const size_t pix0 = base + (size_t)i * 256;
    if (pix0 >= n) break;
    const size_t pix = pix0 + threadIdx.x;
    if (pix < n) {
      const int y = (int)(pix / W), x = (int)(pix - (size_t)y * W);
      int px = x, py = y;
      if (flow) {
        const float2 f = reinterpret_cast<const float2*>(flow)[pix];
        px = TruncToIntX86((float)x + f.x);
        py = TruncToIntX86((float)y + f.y);
        px = max(0, min(W - 1, px));
        py = max(0, min(H - 1, py));
      }
      prev_idx[pix] = py * W + px;
      float ab = 0, ag = 0, ar = 0;
      if (!is_virtual) {
        ab = cur[pix];
        ag = cur[n + pix];
        ar = cur[2 * n + pix];
      }
      int k = 0;
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx, ++k) {
          uint16_t key = kInvalidKey;
          const int qy = py + dy, qx = px + dx;
          if (qy >= 0 && qy < H && qx >= 0 && qx < W) {
            if (is_virtual) {
              key = (uint16_t)kNumBuckets;
            } else {
              const size_t q = (size_t)qy * W + qx;
              key = BucketOf(ColorDist(ab, ag, ar, prev[q], prev[n + q], prev[2 * n + q], l1));
            }
          }
          stage[threadIdx.x * 9 + k] = key;
          atomicAdd(&lds_hist[key == kInvalidKey ? kBinInvalid : key], 1);
        }
      }
    }
    __syncthreads();
    // 256 pixels x 9 keys x 2 B = 4608 contiguous bytes: coalesced 4-byte stores
    const int px_here = (int)min((size_t)256, n - pix0);
    const int words = (px_here * 9 + 1) / 2;
    uint32_t* out32 = reinterpret_cast<uint32_t*>(keys + pix0 * 9);   // pix0 * 18 B: 4-byte aligned
    const uint32_t* in32 = reinterpret_cast<const uint32_t*>(stage);
    if ((px_here * 9) & 1) {   // odd number of keys: the last one on its own
      for (int w = threadIdx.x; w < words - 1; w += 256) out32[w] = in32[w];
      if (threadIdx.x == 0) keys[pix0 * 9 + (size_t)px_here * 9 - 1] = stage[px_here * 9 - 1];
    } else {
      for (int w = threadIdx.x; w < words; w += 256) out32[w] = in32[w];
    }
    __syncthreads();
  }
  StoreTileHist(lds_hist, blockIdx.x, hist);
}

// ---- the lists of one call, as the scan and scatter kernels see them ------------------------------
struct SortListArgs {
  const uint16_t* keys;
  int32_t* hist;       // [num_tiles][kBucketSlots]
  int32_t* chunk;      // [2][num_chunks][kBucketSlots]: totals, bases
  int32_t* offsets;    // [kBucketSlots]
  uint32_t* slots;
  int num_tiles, num_chunks, per_px;
};
struct SortArgs {
  SortListArgs l[kEdgeSortMaxLists];
  unsigned long long n_px;
};

// ---- exclusive scan down the columns of the (tile-major) histogram matrices ----------------------
// grid (bins / 256, chunks of all lists).  Adjacent threads walk adjacent columns: every load and
// store of a wavefront is 256 contiguous bytes, eight rows in flight per thread.
__global__ __launch_bounds__(256) void k_hist_chunk_scan(SortArgs a) {
  int c = blockIdx.y, li = 0;
  while (c >= a.l[li].num_chunks) c -= a.l[li++].num_chunks;
  const SortListArgs& L = a.l[li];
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= kBucketSlots) return;
  const int t0 = c * kHistChunkTiles, t1 = min(L.num_tiles, t0 + kHistChunkTiles);
  int32_t* p = L.hist + (size_t)t0 * kBucketSlots + b;
  int run = 0;
  for (int t = t0; t < t1; t += 8, p += 8 * kBucketSlots) {
    int v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = t + k < t1 ? p[(size_t)k * kBucketSlots] : 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (t + k < t1) p[(size_t)k * kBucketSlots] = run;
      run += v[k];
    }
  }
  L.chunk[(size_t)c * kBucketSlots + b] = run;
}

// grid (3, lists), 1024 threads: workgroup r owns the bins [1024 r, 1024 r + 1024).  Chunk totals ->
// exclusive prefix over the chunks of a bin, bin totals -> exclusive prefix over the bins (offsets),
// base[c][bin] = their sum.  The bins before its own a workgroup only sums up (the totals are a few
// hundred KB in the cache); totals and bases are two arrays, so that no load waits for a store.
__global__ __launch_bounds__(1024) void k_hist_chunk_bases(SortArgs a) {
  __shared__ int32_t wave_sums[32];
  const SortListArgs& L = a.l[blockIdx.y];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int C = L.num_chunks;
  const int32_t* __restrict__ tot = L.chunk;
  int32_t* __restrict__ base = L.chunk + (size_t)C * kBucketSlots;
  // the bins before this workgroup's only add up; every load below is independent of the others
  int before_mine = 0;
  for (int r = 0; r < (int)blockIdx.x; ++r) {
    for (int c = 0; c < C; ++c) before_mine += tot[(size_t)c * kBucketSlots + r * 1024 + threadIdx.x];
  }
  const int b = blockIdx.x * 1024 + threadIdx.x;
  int sum = 0;
  if (b < kBucketSlots) {
    for (int c = 0; c < C; ++c) sum += tot[(size_t)c * kBucketSlots + b];
  }
  const int incl = WaveInclusiveSum(sum);
  const int earlier = WaveInclusiveSum(before_mine);
  if (lane == 63) {
    wave_sums[wave] = incl;
    wave_sums[16 + wave] = earlier;
  }
  __syncthreads();
  int run = incl - sum;
  for (int w = 0; w < 16; ++w) run += wave_sums[16 + w] + (w < wave ? wave_sums[w] : 0);
  if (b < kBucketSlots) {
    L.offsets[b] = run;
    for (int c = 0; c < C; ++c) {
      base[(size_t)c * kBucketSlots + b] = run;
      run += tot[(size_t)c * kBucketSlots + b];
    }
  }
}

// ---- K5: stable scatter of the slot ids ----------------------------------------------------------
// OR over the wavefront, in every lane's hands (DPP row shifts and broadcasts as WaveInclusiveSum).
__device__ __forceinline__ int WaveOr(int v) {
  int t = v | Dpp0<0x111, 0xf, 0xf>(v);
  t |= Dpp0<0x112, 0xf, 0xf>(v);
  int o = t | Dpp0<0x113, 0xf, 0xf>(v);
  o |= Dpp0<0x114, 0xf, 0xe>(o);
  o |= Dpp0<0x118, 0xf, 0xc>(o);
  o |= Dpp0<0x142, 0xa, 0xf>(o);
  o |= Dpp0<0x143, 0xc, 0xf>(o);
  return __builtin_amdgcn_readlane(o, 63);
}

// Lanes of the wavefront whose 12-bit bin equals this lane's: one ballot per bit in which any two
// lanes of the step differ.  The weights of neighbouring edges of a smoothed frame lie a few buckets
// apart (two to four such bits on the bench input), a step of one bucket has none; twelve at the
// worst (noise, or a step with a slot that does not exist in it), plus the OR.
__device__ __forceinline__ unsigned long long SameBinMask(int bin) {
  int varying = WaveOr(bin ^ __builtin_amdgcn_readfirstlane(bin));
  unsigned long long m = ~0ull;
  while (varying) {
    const int b = __builtin_ctz((unsigned)varying);
    varying &= varying - 1;
    const int bit = (bin >> b) & 1;
    const unsigned long long bal = __ballot(bit);
    m &= bit ? bal : ~bal;
  }
  return m;
}

// LDS of a workgroup: the four wavefronts' running positions per bin, tile-relative u16 (a tile has
// at most 9216 slots), two wavefronts to a word, beside one i32 base per bin: 24.6 KB, six workgroups
// per CU.  The keys come straight from memory (they are in the cache: the key kernels just wrote them).
constexpr int kScatterUnroll = 4;

template <int kPerPx, int kTilePx>
__device__ __forceinline__ void ScatterTile(const SortListArgs& L, size_t n_px, int tile, uint32_t* cnt,
                                            int32_t* base) {
  const size_t px0 = (size_t)tile * kTilePx;
  const int n_slots = (int)(min((size_t)kTilePx, n_px - px0) * kPerPx);
  const uint16_t* __restrict__ keys = L.keys + px0 * kPerPx;
  uint32_t* __restrict__ slots_out = L.slots;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int b = threadIdx.x; b < 2 * kBucketSlots; b += 256) cnt[b] = 0;
  __syncthreads();
  // this wavefront's counter of a bin: the word and the half of it
  uint32_t* my_cnt = cnt + (wave >> 1) * kBucketSlots;
  const int sh = 16 * (wave & 1);
  // the wavefront's contiguous quarter (a multiple of 64 slots)
  const int quarter = ((n_slots + 255) / 256) * 64;
  const int q_beg = min(n_slots, wave * quarter), q_end = min(n_slots, (wave + 1) * quarter);
  for (int i = q_beg + lane; i < q_end; i += 64) {
    const int key = keys[i];
    atomicAdd(&my_cnt[key == kInvalidKey ? kBinInvalid : key], 1u << sh);
  }
  __syncthreads();
  {
    const int32_t* __restrict__ hrow = L.hist + (size_t)tile * kBucketSlots;
    const int32_t* __restrict__ crow =
        L.chunk + ((size_t)L.num_chunks + (size_t)(tile / kHistChunkTiles)) * kBucketSlots;
    for (int b = threadIdx.x; b < kBucketSlots; b += 256) {
      const uint32_t w01 = cnt[b], w23 = cnt[kBucketSlots + b];
      const uint32_t c0 = w01 & 0xFFFFu, c1 = w01 >> 16, c2 = w23 & 0xFFFFu;
      // (the counts of a tile sum to 9216 at most: no half ever carries into its neighbour)
      cnt[b] = c0 << 16;
      cnt[kBucketSlots + b] = (c0 + c1) | ((c0 + c1 + c2) << 16);
      base[b] = hrow[b] + crow[b];
    }
  }
  __syncthreads();
  const uint32_t slot0 = (uint32_t)(px0 * kPerPx);
  for (int i0 = q_beg; i0 < q_end; i0 += 64 * kScatterUnroll) {
    int bin[kScatterUnroll], rank[kScatterUnroll], count[kScatterUnroll], first[kScatterUnroll];
    // nothing of this part depends on an earlier step: the key reads and ballots of all four come first
#pragma unroll
    for (int u = 0; u < kScatterUnroll; ++u) {
      const int i = i0 + u * 64 + lane;
      const int key = i < q_end ? (int)keys[i] : (int)kInvalidKey;
      bin[u] = key == kInvalidKey ? kBinInvalid : key;
    }
#pragma unroll
    for (int u = 0; u < kScatterUnroll; ++u) {
      const unsigned long long same = SameBinMask(bin[u]);
      rank[u] = (int)__popcll(same & ((1ull << lane) - 1ull));
      count[u] = (int)__popcll(same);
      first[u] = (int)__ffsll((long long)same) - 1;   // (never empty: the lane itself is in it)
    }
#pragma unroll
    for (int u = 0; u < kScatterUnroll; ++u) {
      // Slots of edges that do not exist are not listed (nothing ever reads that tail), and the
      // lanes past the quarter's end carry that bin too.
      uint32_t start = 0;
      if (rank[u] == 0 && bin[u] != kBinInvalid) {   // one lane per distinct bin takes the step's range
        const uint32_t old = __hip_atomic_fetch_add(&my_cnt[bin[u]], (uint32_t)count[u] << sh,
                                                    __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        start = (uint32_t)base[bin[u]] + ((old >> sh) & 0xFFFFu);
      }
      start = (uint32_t)__shfl((int)start, first[u]);
      if (bin[u] != kBinInvalid) slots_out[start + (uint32_t)rank[u]] = slot0 + (uint32_t)(i0 + u * 64 + lane);
    }
  }
}

// One workgroup per tile of every list of the call, the lists one after the other.
__global__ __launch_bounds__(256) void k_scatter_slots(SortArgs a) {
  __shared__ uint32_t cnt[2 * kBucketSlots];
  __shared__ int32_t base[kBucketSlots];
  int tile = blockIdx.x, li = 0;
  while (tile >= a.l[li].num_tiles) tile -= a.l[li++].num_tiles;
  const SortListArgs& L = a.l[li];
  if (L.per_px == 9) {
    ScatterTile<9, kTilePxTemporal>(L, (size_t)a.n_px, tile, cnt, base);
  } else {
    ScatterTile<4, kTilePxSpatial>(L, (size_t)a.n_px, tile, cnt, base);
  }
}

// ---- launchers -----------------------------------------------------------------------------------
static int NumTiles(size_t n_px, int per_px) {
  const int tile = per_px == 4 ? kTilePxSpatial : kTilePxTemporal;
  return (int)((n_px + tile - 1) / tile);
}
static int NumChunks(size_t n_px, int per_px) {
  return (NumTiles(n_px, per_px) + kHistChunkTiles - 1) / kHistChunkTiles;
}
// Scratch sizes (ints) of one list of a frame.
size_t EdgeSortHistInts(size_t n_px, int per_px) { return (size_t)kBucketSlots * NumTiles(n_px, per_px); }
// (the chunks' totals and, behind them, their bases)
size_t EdgeSortChunkInts(size_t n_px, int per_px) { return 2 * (size_t)kBucketSlots * NumChunks(n_px, per_px); }

void LaunchSpatialKeys(const float* feat, int W, int H, int l1, uint16_t* keys, int32_t* hist,
                       hipStream_t s) {
  const int T = NumTiles((size_t)W * H, 4);
  hipLaunchKernelGGL(k_spatial_keys, dim3(T), dim3(256), 0, s, feat, W, H, l1,
                     reinterpret_cast<ushort4*>(keys), hist);
  VSG_HIP(hipGetLastError());
}

void LaunchTemporalKeys(const float* cur, const float* prev, const float* flow, int W, int H,
                        int l1, int is_virtual, uint16_t* keys, int32_t* prev_idx, int32_t* hist,
                        hipStream_t s) {
  const int T = NumTiles((size_t)W * H, 9);
  hipLaunchKernelGGL(k_temporal_keys, dim3(T), dim3(256), 0, s, cur, prev, flow, W, H, l1,
                     is_virtual, keys, prev_idx, hist);
  VSG_HIP(hipGetLastError());
}

// The tile histograms of the lists (dense rows) -> offsets[0..kBucketSlots-1] = start of every bin of
// a list, then the stable scatter of the slot ids of the existing edges: three launches for all lists.
void LaunchBucketSort(const EdgeSortList* lists, int n_lists, size_t n_px, hipStream_t s) {
  VSG_REQUIRE(n_lists >= 1 && n_lists <= kEdgeSortMaxLists, -1, "unsupported number of lists");
  SortArgs a = {};
  a.n_px = n_px;
  int tiles = 0, chunks = 0;
  for (int i = 0; i < n_lists; ++i) {
    const EdgeSortList& in = lists[i];
    VSG_REQUIRE(in.per_px == 4 || in.per_px == 9, -1, "a list has 4 or 9 slots per pixel");
    SortListArgs& L = a.l[i];
    L.keys = in.keys;
    L.hist = in.hist;
    L.chunk = in.chunk;
    L.offsets = in.offsets;
    L.slots = in.slots;
    L.per_px = in.per_px;
    L.num_tiles = NumTiles(n_px, in.per_px);
    L.num_chunks = NumChunks(n_px, in.per_px);
    tiles += L.num_tiles;
    chunks += L.num_chunks;
  }
  hipLaunchKernelGGL(k_hist_chunk_scan, dim3((kBucketSlots + 255) / 256, chunks), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_hist_chunk_bases, dim3((kBucketSlots + 1023) / 1024, n_lists), dim3(1024), 0, s, a);
  hipLaunchKernelGGL(k_scatter_slots, dim3(tiles), dim3(256), 0, s, a);
  VSG_HIP(hipGetLastError());
}

}  // namespace vsg
