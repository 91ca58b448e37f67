// overlap.hip -- the contingency table of two int32 planes (gfx950): for every (group of P, label of B) the
// number of pixels where both hold, with the marginals of either side.  P is the id plane of
// vsg_render_id_image or the label image of vsg_render_level_components, B a plane of the caller's; a
// negative value is "none" on either side.
//
//   k_overlap_runs<count>  one block per frame row: the maximal runs of constant (P, B) with at least one of
//                          the two non-negative, counted; with them the covered, the labelled and the doubly
//                          covered pixels and the largest label; five words per row, no atomic
//   k_overlap_totals       one block: the rows' five words summed into the status block
//   k_overlap_runs<emit>   the same walk: (key, length) of every run, in no order; one add per block and step
//                          of 256 pixels reserves their slots
//   radix sort             (key, length) on the used bits, into (group, label) order
//   two scans              for every run the row heads and the pair heads in [0, i] in one 64-bit sum, and the
//                          heads of distinct keys with the lengths in [0, i] in another
//   k_overlap_table        one thread per sorted run: the head of a key writes the key, the pixels before it
//                          and its two ranks into the list of distinct keys
//   k_overlap_pairs        one thread per distinct key: its count is the difference of two prefix sums; a
//                          (group, label) writes its pair, a (group, none) the row's `unlabelled`, a row's
//                          first key id, component and first_pair; every key is handed to the column sort
//                          with its halves swapped
//   k_overlap_rows         one wavefront per row: num_pairs, area, and the arg-max over its pairs
//   radix sort, scan       the distinct keys by (label, group); the rank of every label
//   k_overlap_col_heads    one thread per distinct key: the head of a label writes it and where it starts
//   k_overlap_cols         one wavefront per column: area, uncovered, num_pairs, the arg-max over its keys,
//                          and `col` of every pair of the column
//   k_copy_lists           of lists.hip: the three lists to the caller's device memory, if all of them fit
//
// Key layout, gb = the bits of the largest group and lb = the bits of the largest label (1..31 each):
//   bits [0, lb + 1)               code(B): the label, or 1 << lb for "none", which sorts behind every label
//   bits [lb + 1, lb + gb + 2)     code(P): the group, or 1 << gb for "none", which sorts behind every group
// The column sort's key holds the same two fields the other way round.
#include "render.h"
#include "render_device.h"
#include "render_scan.h"

namespace vsg_render_impl {

namespace {

constexpr int kOvlBlock = 256;
constexpr int kOvlWaves = kOvlBlock / 64;
constexpr unsigned long long kOvlNone = ~0ull;   // the pair (-1, -1): no run
constexpr int kOvlTotals = kOverlapRowTotals;

// The pair of a pixel as one word, every negative value read as -1.
__device__ __forceinline__ unsigned long long OvlPair(int32_t p, int32_t b) {
  return (unsigned long long)(uint32_t)max(p, -1) << 32 | (uint32_t)max(b, -1);
}

// One block walks frame row blockIdx.x in steps of kOvlBlock pixels, a thread a pixel.  A pixel is a break
// when its pair differs from its left neighbour's (or it is the row's first), and a head when it is a break
// and its pair is not (-1, -1).  A head's run ends at the next break or with the row.  The next break is
// looked up in the step's ballots; a run that is still open at the end of a step keeps its slot, and the
// first break of a later step (or the row's end) writes its length.  At most one run is open at a time.
template <bool kEmit>
__global__ __launch_bounds__(kOvlBlock) void k_overlap_runs(const int32_t* __restrict__ plane,
                                                            const int32_t* __restrict__ other, size_t other_pitch,
                                                            int W, int group_bits, int label_bits,
                                                            uint32_t capacity, unsigned long long* __restrict__ keys,
                                                            uint32_t* __restrict__ lengths,
                                                            uint32_t* __restrict__ row_totals,
                                                            OvlStatus* __restrict__ status) {
  __shared__ unsigned long long s_pair[kOvlBlock + 1];
  __shared__ unsigned long long s_breaks[kOvlWaves], s_heads[kOvlWaves];
  __shared__ uint32_t s_base, s_carry_slot, s_carry_x;
  __shared__ uint32_t s_sum[kOvlWaves][kOvlTotals];
  const int y = blockIdx.x;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int32_t* row_p = plane + (size_t)y * W;
  const int32_t* row_b = other + (size_t)y * other_pitch;
  uint32_t n_heads = 0, n_covered = 0, n_labelled = 0, n_both = 0, max_label = 0;   // count only
  bool open = false;   // block-uniform: a run of an earlier step has not ended yet
  for (int x0 = 0; x0 < W; x0 += kOvlBlock) {
    const int x = x0 + t;
    const bool in = x < W;
    const int32_t p = in ? row_p[x] : -1, b = in ? row_b[x] : -1;
    const unsigned long long pair = OvlPair(p, b);
    s_pair[t + 1] = pair;
    if (t == 0) s_pair[0] = x0 > 0 ? OvlPair(row_p[x0 - 1], row_b[x0 - 1]) : kOvlNone;
    __syncthreads();
    const bool brk = in && (x == 0 || s_pair[t] != pair);
    const bool head = brk && pair != kOvlNone;
    if (!kEmit) {
      n_heads += head ? 1u : 0u;
      n_covered += p >= 0 ? 1u : 0u;
      n_labelled += b >= 0 ? 1u : 0u;
      n_both += p >= 0 && b >= 0 ? 1u : 0u;
      max_label = max(max_label, (uint32_t)max(b, 0));
      __syncthreads();   // s_pair is rewritten by the next step
      continue;
    }
    const unsigned long long bm = __ballot(brk), hm = __ballot(head);
    if (lane == 0) {
      s_breaks[wave] = bm;
      s_heads[wave] = hm;
    }
    __syncthreads();
    // block-uniform: the heads of the step, its first and its last break
    uint32_t before = 0, total = 0;
    int first = -1, last = -1;
    bool last_is_head = false;
#pragma unroll
    for (int w = 0; w < kOvlWaves; ++w) {
      const uint32_t c = (uint32_t)__popcll(s_heads[w]);
      if (w < wave) before += c;
      total += c;
      const unsigned long long m = s_breaks[w];
      if (m) {
        if (first < 0) first = w * 64 + __ffsll((long long)m) - 1;
        last = w * 64 + 63 - __clzll((long long)m);
        last_is_head = (s_heads[w] >> (last & 63)) & 1ull;
      }
    }
    if (t == 0 && total) s_base = atomicAdd(&status->emitted, total);
    const uint32_t carry_slot = s_carry_slot, carry_x = s_carry_x;   // read only where open
    __syncthreads();
    const bool last_step = x0 + kOvlBlock >= W;
    if (open) {
      // the run carried in ends at the step's first break, or with the row
      if (first >= 0) {
        if (t == first && carry_slot < capacity) lengths[carry_slot] = (uint32_t)x - carry_x;
      } else if (last_step) {
        if (t == 0 && carry_slot < capacity) lengths[carry_slot] = (uint32_t)W - carry_x;
      }
    }
    if (head) {
      const uint32_t slot = s_base + before + (uint32_t)__popcll(hm & ((1ull << lane) - 1));
      // the next break of the step behind this pixel
      int next = -1;
      const unsigned long long above = bm & ~((2ull << lane) - 1);
      if (above) {
        next = wave * 64 + __ffsll((long long)above) - 1;
      } else {
        for (int w = wave + 1; w < kOvlWaves && next < 0; ++w) {
          const unsigned long long m = s_breaks[w];
          if (m) next = w * 64 + __ffsll((long long)m) - 1;
        }
      }
      if (slot < capacity) {
        const unsigned long long code_p = p >= 0 ? (unsigned long long)(uint32_t)p : 1ull << group_bits;
        const unsigned long long code_b = b >= 0 ? (unsigned long long)(uint32_t)b : 1ull << label_bits;
        keys[slot] = code_p << (label_bits + 1) | code_b;
        if (next >= 0) lengths[slot] = (uint32_t)(next - t);
        else if (last_step) lengths[slot] = (uint32_t)(W - x);
      } else {
        atomicOr(&status->flags, (uint32_t)OVL_FLAG_OVERFLOW);
      }
      if (next < 0 && !last_step) {   // this is the step's last break: its run stays open
        s_carry_slot = slot;
        s_carry_x = (uint32_t)x;
      }
    }
    if (first >= 0) open = last_is_head;   // a step without a break changes nothing
  }
  if (!kEmit) {
    n_heads = WaveSum(n_heads);
    n_covered = WaveSum(n_covered);
    n_labelled = WaveSum(n_labelled);
    n_both = WaveSum(n_both);
    max_label = WaveMax(max_label);
    if (lane == 0) {
      s_sum[wave][0] = n_heads;
      s_sum[wave][1] = n_covered;
      s_sum[wave][2] = n_labelled;
      s_sum[wave][3] = n_both;
      s_sum[wave][4] = max_label;
    }
    __syncthreads();
    if (t == 0) {
      uint32_t sum[5] = {0, 0, 0, 0, 0};
#pragma unroll
      for (int w = 0; w < kOvlWaves; ++w) {
        for (int k = 0; k < 4; ++k) sum[k] += s_sum[w][k];
        sum[4] = max(sum[4], s_sum[w][4]);
      }
      // a thousand blocks adding to five words of one cache line take longer than the walk itself
      for (int k = 0; k < kOvlTotals; ++k) row_totals[(size_t)y * kOvlTotals + k] = sum[k];
    }
  }
}

// One block: the sums of words 0..3 and the maximum of word 4 over the H rows of row_totals.
__global__ __launch_bounds__(kOvlBlock) void k_overlap_totals(const uint32_t* __restrict__ row_totals, int H,
                                                              OvlStatus* __restrict__ status) {
  __shared__ uint32_t s_sum[kOvlWaves][kOvlTotals];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  uint32_t sum[kOvlTotals] = {0, 0, 0, 0, 0};
  for (int y = t; y < H; y += kOvlBlock) {
    for (int k = 0; k < 4; ++k) sum[k] += row_totals[(size_t)y * kOvlTotals + k];
    sum[4] = max(sum[4], row_totals[(size_t)y * kOvlTotals + 4]);
  }
  for (int k = 0; k < 4; ++k) sum[k] = WaveSum(sum[k]);
  sum[4] = WaveMax(sum[4]);
  if (lane == 0) {
    for (int k = 0; k < kOvlTotals; ++k) s_sum[wave][k] = sum[k];
  }
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < kOvlWaves; ++w) {
      for (int k = 0; k < 4; ++k) sum[k] += s_sum[w][k];
      sum[4] = max(sum[4], s_sum[w][4]);
    }
    status->runs = sum[0];
    status->covered = sum[1];
    status->labelled = sum[2];
    status->both = sum[3];
    status->max_label = sum[4];
  }
}

// One thread per sorted run i < n.  row_heads[i] = rows << 32 | pairs, key_heads[i] = distinct keys << 32 |
// pixels, each in [0, i].  The head of distinct key d writes key[d], start[d] = the pixels before it and
// rank[d] = row_heads at it; the last run writes start[distinct] and the three totals.  A key without a
// slot raises OVL_FLAG_RANGE.
__global__ __launch_bounds__(256) void k_overlap_table(const unsigned long long* __restrict__ keys,
                                                       const uint32_t* __restrict__ lengths,
                                                       const unsigned long long* __restrict__ row_heads,
                                                       const unsigned long long* __restrict__ key_heads, uint32_t n,
                                                       uint32_t capacity, unsigned long long* __restrict__ key,
                                                       uint32_t* __restrict__ start,
                                                       unsigned long long* __restrict__ rank,
                                                       OvlStatus* __restrict__ status) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const unsigned long long k = keys[i], seen = key_heads[i];
  const uint32_t distinct = (uint32_t)(seen >> 32);
  if (i == 0 || keys[i - 1] != k) {
    const uint32_t d = distinct - 1;
    if (d < capacity) {
      key[d] = k;
      start[d] = (uint32_t)seen - lengths[i];
      rank[d] = row_heads[i];
    } else {
      atomicOr(&status->flags, (uint32_t)OVL_FLAG_RANGE);
    }
  }
  if (i == n - 1) {
    if (distinct <= capacity) start[distinct] = (uint32_t)seen;
    status->distinct = distinct;
    status->rows = (uint32_t)(row_heads[i] >> 32);
    status->pairs = (uint32_t)row_heads[i];
  }
}

// One thread per slot d < m of the list of distinct keys; status->distinct of them are keys.  rows has
// been cleared to zero.  Every slot gets a column key: the key with its halves swapped, or (none, none)
// for a slot without a key, which sorts last.  comp_table: null, or the component table the groups index.
__global__ __launch_bounds__(256) void k_overlap_pairs(const unsigned long long* __restrict__ key,
                                                       const uint32_t* __restrict__ start,
                                                       const unsigned long long* __restrict__ rank, uint32_t m,
                                                       OvlBits bits, uint32_t max_group, uint32_t capacity_rows,
                                                       uint32_t capacity_pairs, const int32_t* __restrict__ comp_table,
                                                       int32_t* __restrict__ rows, int32_t* __restrict__ pairs,
                                                       unsigned long long* __restrict__ ckeys,
                                                       uint32_t* __restrict__ cvals,
                                                       OvlStatus* __restrict__ status) {
  const uint32_t d = blockIdx.x * 256u + threadIdx.x;
  if (d >= m) return;
  const uint32_t distinct = min(status->distinct, m);
  if (d >= distinct) {
    ckeys[d] = 1ull << (bits.group_bits + 1 + bits.label_bits) | 1ull << bits.group_bits;
    cvals[d] = 0xffffffffu;
    return;
  }
  const unsigned long long k = key[d];
  ckeys[d] = bits.Swapped(k);
  cvals[d] = d;
  if (bits.NoP(k)) return;   // pixels of no group: they count for the columns only
  const uint32_t count = start[d + 1] - start[d];
  const unsigned long long seen = rank[d];
  const uint32_t r = (uint32_t)(seen >> 32) - 1, group = (uint32_t)bits.P(k);
  const bool real = !bits.NoB(k);
  const uint32_t e = (uint32_t)seen - 1;   // of a real pair
  if (group > max_group || r >= capacity_rows || (real && e >= capacity_pairs) || (comp_table && r != group)) {
    atomicOr(&status->flags, (uint32_t)OVL_FLAG_RANGE);
    return;
  }
  int32_t* row = rows + (size_t)r * kOverlapRowWords;
  if (d == 0 || bits.P(key[d - 1]) != bits.P(k)) {
    row[0] = comp_table ? comp_table[(size_t)group * kLevelComponentWords + 0] : (int32_t)group;
    row[1] = comp_table ? comp_table[(size_t)group * kLevelComponentWords + 1] : -1;
    row[2] = (int32_t)((uint32_t)seen - (real ? 1u : 0u));
  }
  if (real) {
    reinterpret_cast<int4*>(pairs)[e] = make_int4((int)r, 0, (int)(uint32_t)bits.B(k), (int)count);
  } else {
    row[5] = (int32_t)count;
  }
}

// The larger of two (count, index) candidates packed as count << 32 | ~index: the largest count, and among
// equal counts the smallest index.  0 is "no candidate".
__device__ __forceinline__ unsigned long long OvlBest(unsigned long long a, unsigned long long b) {
  return a > b ? a : b;
}
__device__ __forceinline__ unsigned long long OvlWaveBest(unsigned long long v) {
  for (int s = 32; s > 0; s >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((uint32_t)v, s), hi = (uint32_t)__shfl_xor((uint32_t)(v >> 32), s);
    v = OvlBest(v, (unsigned long long)hi << 32 | lo);
  }
  return v;
}

// One wavefront per row r: its pairs are [first_pair, the next row's first_pair).  Writes num_pairs, area,
// best_label and best_count; status->largest takes the most pairs of a row.
__global__ __launch_bounds__(256) void k_overlap_rows(int32_t* __restrict__ rows, const int32_t* __restrict__ pairs,
                                                      uint32_t capacity_rows, uint32_t capacity_pairs,
                                                      OvlStatus* __restrict__ status) {
  const uint32_t r = (blockIdx.x * 256u + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  const uint32_t n_rows = status->rows, n_pairs = status->pairs;
  if (r >= n_rows || r >= capacity_rows || n_pairs > capacity_pairs) return;
  int32_t* row = rows + (size_t)r * kOverlapRowWords;
  const uint32_t first = (uint32_t)row[2];
  const uint32_t end = r + 1 < n_rows && r + 1 < capacity_rows ? (uint32_t)row[kOverlapRowWords + 2] : n_pairs;
  if (first > end || end > n_pairs) {
    if (lane == 0) atomicOr(&status->flags, (uint32_t)OVL_FLAG_RANGE);
    return;
  }
  uint32_t sum = 0;
  unsigned long long best = 0;
  for (uint32_t e = first + lane; e < end; e += 64) {
    const uint32_t count = (uint32_t)pairs[(size_t)e * kOverlapPairWords + 3];
    sum += count;
    best = OvlBest(best, (unsigned long long)count << 32 | (uint32_t)~e);
  }
  sum = WaveSum(sum);
  best = OvlWaveBest(best);
  if (lane == 0) {
    row[3] = (int32_t)(end - first);
    row[4] = (int32_t)(sum + (uint32_t)row[5]);
    row[6] = end > first ? pairs[(size_t)(~(uint32_t)best) * kOverlapPairWords + 2] : -1;
    row[7] = (int32_t)(uint32_t)(best >> 32);
    if (end > first) atomicMax(&status->largest, end - first);
  }
}

// One thread per sorted column key j < m, rank[j] = the labels in [0, j].  The head of column c writes the
// label and first[c] = j; the last key with a label writes first[columns] and status->cols.
__global__ __launch_bounds__(256) void k_overlap_col_heads(const unsigned long long* __restrict__ ckeys,
                                                           const uint32_t* __restrict__ rank, uint32_t m,
                                                           OvlBits bits, uint32_t capacity_cols,
                                                           int32_t* __restrict__ cols, uint32_t* __restrict__ first,
                                                           OvlStatus* __restrict__ status) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= m) return;
  const unsigned long long ckey = ckeys[j];
  if (bits.ColNoB(ckey)) return;
  const uint32_t c = rank[j] - 1;
  if (c >= capacity_cols) {
    atomicOr(&status->flags, (uint32_t)OVL_FLAG_RANGE);
    return;
  }
  if (j == 0 || bits.ColB(ckeys[j - 1]) != bits.ColB(ckey)) {
    cols[(size_t)c * kOverlapColWords + 0] = (int32_t)(uint32_t)bits.ColB(ckey);
    first[c] = j;
  }
  if (j == m - 1 || bits.ColNoB(ckeys[j + 1])) {
    first[c + 1] = j + 1;
    status->cols = c + 1;
  }
}

// One wavefront per column c: its keys are sorted column keys [first[c], first[c + 1]), by ascending group,
// which is ascending row.  Writes area, uncovered, num_pairs, best_row and best_count, and `col` of every
// pair of the column.
__global__ __launch_bounds__(256) void k_overlap_cols(const unsigned long long* __restrict__ ckeys,
                                                      const uint32_t* __restrict__ cvals,
                                                      const uint32_t* __restrict__ first,
                                                      const uint32_t* __restrict__ start,
                                                      const unsigned long long* __restrict__ rank, uint32_t m,
                                                      OvlBits bits, uint32_t capacity_cols, uint32_t capacity_pairs,
                                                      int32_t* __restrict__ cols, int32_t* __restrict__ pairs,
                                                      OvlStatus* __restrict__ status) {
  const uint32_t c = (blockIdx.x * 256u + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (c >= status->cols || c >= capacity_cols) return;
  const uint32_t begin = first[c], end = first[c + 1];
  if (begin >= end || end > m) {
    if (lane == 0) atomicOr(&status->flags, (uint32_t)OVL_FLAG_RANGE);
    return;
  }
  uint32_t area = 0, uncovered = 0, n_pairs = 0;
  unsigned long long best = 0;
  bool bad = false;
  for (uint32_t j = begin + lane; j < end; j += 64) {
    const uint32_t d = cvals[j];
    if (d >= m) {
      bad = true;
      continue;
    }
    const uint32_t count = start[d + 1] - start[d];
    area += count;
    if (bits.ColNoP(ckeys[j])) {
      uncovered += count;
      continue;
    }
    const unsigned long long seen = rank[d];
    const uint32_t r = (uint32_t)(seen >> 32) - 1, e = (uint32_t)seen - 1;
    if (e >= capacity_pairs) {
      bad = true;
      continue;
    }
    ++n_pairs;
    best = OvlBest(best, (unsigned long long)count << 32 | (uint32_t)~r);
    pairs[(size_t)e * kOverlapPairWords + 1] = (int32_t)c;
  }
  if (bad) atomicOr(&status->flags, (uint32_t)OVL_FLAG_RANGE);
  for (int s = 32; s > 0; s >>= 1) {   // one loop: as three WaveSum calls the kernel's register count changes
    area += __shfl_xor(area, s);
    uncovered += __shfl_xor(uncovered, s);
    n_pairs += __shfl_xor(n_pairs, s);
  }
  best = OvlWaveBest(best);
  if (lane == 0) {
    int32_t* col = cols + (size_t)c * kOverlapColWords;
    col[1] = (int32_t)area;
    col[2] = (int32_t)uncovered;
    col[3] = (int32_t)n_pairs;
    col[4] = n_pairs ? (int32_t)~(uint32_t)best : -1;
    col[5] = (int32_t)(uint32_t)(best >> 32);
  }
}

}  // namespace

void LaunchOverlapRuns(const int32_t* plane, const int32_t* other, size_t other_pitch, int width, int height,
                       int group_bits, int label_bits, bool emit, uint32_t capacity, unsigned long long* keys,
                       uint32_t* lengths, uint32_t* row_totals, OvlStatus* status, hipStream_t stream) {
  const dim3 grid(height), block(kOvlBlock);
  if (emit) {
    hipLaunchKernelGGL((k_overlap_runs<true>), grid, block, 0, stream, plane, other, other_pitch, width, group_bits,
                       label_bits, capacity, keys, lengths, nullptr, status);
  } else {
    hipLaunchKernelGGL((k_overlap_runs<false>), grid, block, 0, stream, plane, other, other_pitch, width, 1, 1, 0u,
                       nullptr, nullptr, row_totals, status);
    hipLaunchKernelGGL(k_overlap_totals, dim3(1), block, 0, stream, row_totals, height, status);
  }
}

void LaunchOverlapTable(const unsigned long long* keys_sorted, const uint32_t* lengths_sorted,
                        const unsigned long long* row_heads, const unsigned long long* key_heads, uint32_t n,
                        uint32_t m, int group_bits, int label_bits, uint32_t max_group, uint32_t capacity_rows,
                        const int32_t* comp_table, unsigned long long* key, uint32_t* start, unsigned long long* rank,
                        int32_t* rows, int32_t* pairs, unsigned long long* ckeys, uint32_t* cvals, OvlStatus* status,
                        hipStream_t stream) {
  if (n == 0 || m == 0) return;
  const OvlBits bits{group_bits, label_bits};
  hipLaunchKernelGGL(k_overlap_table, dim3((n + 255) / 256), dim3(256), 0, stream, keys_sorted, lengths_sorted,
                     row_heads, key_heads, n, m, key, start, rank, status);
  hipLaunchKernelGGL(k_overlap_pairs, dim3((m + 255) / 256), dim3(256), 0, stream, key, start, rank, m, bits,
                     max_group, capacity_rows, m, comp_table, rows, pairs, ckeys, cvals, status);
  // the number of rows is on the device only: a wavefront per slot, all but the first status->rows leave
  if (capacity_rows) {
    hipLaunchKernelGGL(k_overlap_rows, dim3((capacity_rows + 3) / 4), dim3(256), 0, stream, rows, pairs,
                       capacity_rows, m, status);
  }
}

void LaunchOverlapCols(const unsigned long long* ckeys_sorted, const uint32_t* cvals_sorted, const uint32_t* col_rank,
                       const uint32_t* start, const unsigned long long* rank, uint32_t m, int group_bits,
                       int label_bits, uint32_t* first, int32_t* cols, int32_t* pairs, OvlStatus* status,
                       hipStream_t stream) {
  if (m == 0) return;
  const OvlBits bits{group_bits, label_bits};
  hipLaunchKernelGGL(k_overlap_col_heads, dim3((m + 255) / 256), dim3(256), 0, stream, ckeys_sorted, col_rank, m,
                     bits, m, cols, first, status);
  hipLaunchKernelGGL(k_overlap_cols, dim3((m + 3) / 4), dim3(256), 0, stream, ckeys_sorted, cvals_sorted, first,
                     start, rank, m, bits, m, m, cols, pairs, status);
}

}  // namespace vsg_render_impl
