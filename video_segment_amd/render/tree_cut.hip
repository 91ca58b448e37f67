// tree_cut.hip -- the best non-horizontal cut of a hierarchy (gfx950): the partition into nodes of any level
// that maximises the sum of the nodes' gains.  Integers throughout; every sum is an integer atomic or a scan,
// so the bytes do not depend on the order of the threads.
//
// The leaves are the R regions of the level-0 plane (ascending id), the ancestor table (persistence_table.h)
// has a column for every region that paints; A_l of leaf j is table[l - 1][col[j]].
//
//   k_cut_leaves        id, area and ancestor column of every leaf from the level-0 list (overlap rows or
//                       level regions); one bisection per leaf
//   k_cut_node_keys     one key level << 32 | A_l(leaf) per (level, leaf), value l * R + j          L * R threads
//   (radix sort, scan)  sorted keys and the rank of every distinct key: the dense node numbers of all levels,
//                       ascending by (level, id).  Every level has R keys, so level l is entries [l R, (l + 1) R)
//   k_cut_node_map      (l, j) -> node; the first node of every level; the number of nodes       L * R threads
//   k_cut_node_table    level, id, parent of every node; area, leaves, children by integer atomics   L * R
//   k_cut_pair_keys     labels: one key node << label_bits | label per (level, level-0 pair), value count    L * P
//   (radix sort, scan)  on the used key bits; the rank of every distinct (node, label)
//   k_cut_pair_sums     the count of every distinct (node, label): one 32-bit atomic add per entry         L * P
//   k_cut_best          one 64-bit atomic max per distinct key on count << 31 | (2^31 - 1 - label): the largest
//                       count, ties to the smallest label                                                      L * P
//   k_cut_gain_labels   g = best_count - penalty                                                      T threads
//   k_cut_gain_check    a gain table: strictly ascending (level, id), |gain| <= 2^32               G threads
//   k_cut_gain_lookup   every node finds its gain by bisection (log2 G steps)                       T threads
//   k_cut_dp_block      one workgroup of 1024 threads walks the levels bottom-up: a node reads its children's
//                       sum S, decides keep = g >= S, and adds max(g, S) into its parent's S with a 64-bit
//                       integer atomic; a fence and __syncthreads() between levels.  One launch whatever L is.
//   k_cut_dp_level      the same for the nodes of one level: L launches, the kernel boundary is the barrier
//   k_cut_select        every leaf walks its ancestors from the top to the first kept node          R threads, <= L steps
//   (scan)              the record index of every selected node: ascending node number = ascending (level, id)
//   k_cut_records       48-byte records; the number of records, sum of gains and of areas           T threads
//   k_cut_paint         pixel -> leaf (bisection over the leaf ids, reused while the id repeats) -> record; four
//                       pixels a thread, 16-byte moves where the planes allow
//
// No kernel waits for another workgroup: there is no grid-wide barrier and no spinning anywhere.
#include "render.h"
#include "render_device.h"

namespace vsg_render_impl {

namespace {

typedef unsigned long long u64;

// The index of `id` in the ascending ids[0 .. n), or n.
__device__ __forceinline__ uint32_t FindId(const int32_t* __restrict__ ids, uint32_t n, int32_t id) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (ids[mid] < id) lo = mid + 1;
    else hi = mid;
  }
  return (lo < n && ids[lo] == id) ? lo : n;
}

__global__ __launch_bounds__(256) void k_cut_leaves(const int32_t* __restrict__ list, uint32_t words,
                                                    uint32_t area_word, uint32_t R, const int32_t* __restrict__ ids,
                                                    uint32_t n_ids, int32_t* __restrict__ leaf_id,
                                                    uint32_t* __restrict__ leaf_area, uint32_t* __restrict__ leaf_col,
                                                    CutStatus* __restrict__ status) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= R) return;
  const int32_t id = list[(size_t)j * words];
  const uint32_t col = FindId(ids, n_ids, id);
  if (col == n_ids || (j > 0 && list[(size_t)(j - 1) * words] >= id)) atomicOr(&status->flags, CUT_FLAG_RANGE);
  leaf_id[j] = id;
  leaf_area[j] = (uint32_t)list[(size_t)j * words + area_word];
  leaf_col[j] = col < n_ids ? col : 0u;
}

__global__ __launch_bounds__(256) void k_cut_node_keys(const int32_t* __restrict__ leaf_id,
                                                       const uint32_t* __restrict__ leaf_col, uint32_t R,
                                                       const int32_t* __restrict__ table, uint32_t n_ids, uint32_t n,
                                                       u64* __restrict__ keys, uint32_t* __restrict__ vals) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t l = i / R, j = i - l * R;
  const int32_t a = l == 0 ? leaf_id[j] : table[(size_t)(l - 1) * n_ids + leaf_col[j]];
  keys[i] = (u64)l << 32 | (uint32_t)a;
  vals[i] = i;
}

__global__ __launch_bounds__(256) void k_cut_node_map(const uint32_t* __restrict__ vals, const uint32_t* __restrict__ rank,
                                                      uint32_t R, uint32_t L, uint32_t n, uint32_t* __restrict__ map,
                                                      uint32_t* __restrict__ level_first, CutStatus* __restrict__ status) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t node = rank[i] - 1;
  const uint32_t v = vals[i];
  if (v >= n || v / R != i / R) {   // a key left its level: the sort saw other bits than the keys have
    atomicOr(&status->flags, CUT_FLAG_RANGE);
    return;
  }
  map[v] = node;
  if (i % R == 0) level_first[i / R] = node;
  if (i == n - 1) {
    level_first[L] = node + 1;
    status->tree_nodes = node + 1;
  }
}

__global__ __launch_bounds__(256) void k_cut_node_table(const u64* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                        const uint32_t* __restrict__ rank,
                                                        const uint32_t* __restrict__ map,
                                                        const uint32_t* __restrict__ leaf_area, uint32_t R, uint32_t L,
                                                        uint32_t n, uint32_t T, CutNodes nodes) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t node = rank[i] - 1;
  if (node >= T) return;
  const uint32_t v = vals[i];
  const uint32_t l = v / R, j = v - l * R;
  atomicAdd(&nodes.area[node], leaf_area[j]);
  atomicAdd(&nodes.leaves[node], 1u);
  if (i != 0 && keys[i] == keys[i - 1]) return;
  nodes.level[node] = (int32_t)l;
  nodes.id[node] = (int32_t)(uint32_t)keys[i];
  int32_t parent = -1;
  if (l + 1 < L) {
    parent = (int32_t)map[(size_t)(l + 1) * R + j];
    if ((uint32_t)parent < T) atomicAdd(&nodes.children[parent], 1u);
    else parent = -1;
  }
  nodes.parent[node] = parent;
}

__global__ __launch_bounds__(256) void k_cut_pair_keys(const int32_t* __restrict__ pairs, uint32_t P,
                                                       const uint32_t* __restrict__ map, uint32_t R, uint32_t n,
                                                       int label_bits, u64* __restrict__ keys,
                                                       uint32_t* __restrict__ counts) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t l = i / P, e = i - l * P;
  const int4 pair = reinterpret_cast<const int4*>(pairs)[e];   // row, col, label, count
  const uint32_t row = (uint32_t)pair.x < R ? (uint32_t)pair.x : 0u;
  keys[i] = (u64)map[(size_t)l * R + row] << label_bits | (uint32_t)pair.z;
  counts[i] = (uint32_t)pair.w;
}

__global__ __launch_bounds__(256) void k_cut_pair_sums(const uint32_t* __restrict__ counts,
                                                       const uint32_t* __restrict__ rank, uint32_t n,
                                                       uint32_t* __restrict__ sums) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  atomicAdd(&sums[rank[i] - 1], counts[i]);
}

__global__ __launch_bounds__(256) void k_cut_best(const u64* __restrict__ keys, const uint32_t* __restrict__ rank,
                                                  const uint32_t* __restrict__ sums, uint32_t n, int label_bits,
                                                  uint32_t T, u64* __restrict__ best, CutStatus* __restrict__ status) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const u64 key = keys[i];
  if (i != 0 && key == keys[i - 1]) return;
  const u64 node = key >> label_bits;
  const uint32_t label = (uint32_t)(key & ((1ull << label_bits) - 1));
  if (node >= T) {
    atomicOr(&status->flags, CUT_FLAG_RANGE);
    return;
  }
  atomicMax(&best[node], (u64)sums[rank[i] - 1] << 31 | (0x7fffffffu - label));
}

__global__ __launch_bounds__(256) void k_cut_gain_labels(const u64* __restrict__ best, uint32_t T, long long penalty,
                                                         CutNodes nodes) {
  const uint32_t node = blockIdx.x * 256u + threadIdx.x;
  if (node >= T) return;
  const u64 b = best[node];
  const uint32_t count = (uint32_t)(b >> 31);
  nodes.best_label[node] = count ? (int32_t)(0x7fffffffu - (uint32_t)(b & 0x7fffffffu)) : -1;
  nodes.best_count[node] = (int32_t)count;
  nodes.gain[node] = (long long)count - penalty;
}

__device__ __forceinline__ bool GainBefore(int32_t la, int32_t ia, int32_t lb, int32_t ib) {
  return la < lb || (la == lb && ia < ib);
}

__global__ __launch_bounds__(256) void k_cut_gain_check(const CutGain* __restrict__ gains, size_t n,
                                                        CutStatus* __restrict__ status) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const CutGain g = gains[i];
  uint32_t flags = 0;
  if (g.gain > (1ll << 32) || g.gain < -(1ll << 32)) flags |= CUT_FLAG_GAIN_RANGE;
  if (i > 0 && !GainBefore(gains[i - 1].level, gains[i - 1].id, g.level, g.id)) flags |= CUT_FLAG_GAIN_ORDER;
  if (flags) atomicOr(&status->flags, flags);
}

__global__ __launch_bounds__(256) void k_cut_gain_lookup(const CutGain* __restrict__ gains, size_t n, uint32_t T,
                                                         CutNodes nodes) {
  const uint32_t node = blockIdx.x * 256u + threadIdx.x;
  if (node >= T) return;
  const int32_t level = nodes.level[node], id = nodes.id[node];
  size_t lo = 0, hi = n;
  while (lo < hi) {
    const size_t mid = lo + ((hi - lo) >> 1);
    if (GainBefore(gains[mid].level, gains[mid].id, level, id)) lo = mid + 1;
    else hi = mid;
  }
  const bool found = lo < n && gains[lo].level == level && gains[lo].id == id;
  nodes.gain[node] = found ? gains[lo].gain : 0ll;
  nodes.best_label[node] = -1;
  nodes.best_count[node] = 0;
}

// One node of the dynamic programme.  Its children, all one level below, have added their opt into sum[node];
// the load is an atomic one, so that it reads what the atomics wrote and no older line of the vector cache.
__device__ __forceinline__ void CutNode(uint32_t node, const CutNodes& nodes) {
  const long long g = nodes.gain[node];
  const bool inner = nodes.children[node] != 0;
  const long long s = inner ? (long long)__hip_atomic_load(&nodes.sum[node], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                            : 0ll;
  const bool keep = !inner || g >= s;   // a tie keeps the coarser node
  nodes.keep[node] = keep ? 1u : 0u;
  nodes.split[node] = s;
  const int32_t parent = nodes.parent[node];
  if (parent >= 0) atomicAdd(&nodes.sum[parent], (u64)(keep ? g : s));
}

__global__ __launch_bounds__(1024) void k_cut_dp_block(const uint32_t* __restrict__ level_first, uint32_t L,
                                                       CutNodes nodes) {
  for (uint32_t l = 0; l < L; ++l) {
    const uint32_t end = level_first[l + 1];
    for (uint32_t node = level_first[l] + threadIdx.x; node < end; node += 1024u) CutNode(node, nodes);
    __threadfence();   // the atomics have reached the L2 before the next level reads the sums
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_cut_dp_level(uint32_t first, uint32_t end, CutNodes nodes) {
  const uint32_t node = first + blockIdx.x * 256u + threadIdx.x;
  if (node < end) CutNode(node, nodes);
}

__global__ __launch_bounds__(256) void k_cut_select(const uint32_t* __restrict__ map, uint32_t R, uint32_t L,
                                                    uint32_t T, const uint32_t* __restrict__ keep,
                                                    uint32_t* __restrict__ leaf_node, uint32_t* __restrict__ selected,
                                                    CutStatus* __restrict__ status) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= R) return;
  for (uint32_t l = L; l-- > 0;) {
    const uint32_t node = map[(size_t)l * R + j];
    if (node >= T) break;
    if (keep[node]) {
      leaf_node[j] = node;
      selected[node] = 1u;
      return;
    }
  }
  leaf_node[j] = 0;   // a leaf keeps itself: not reached
  atomicOr(&status->flags, CUT_FLAG_RANGE);
}

__global__ __launch_bounds__(256) void k_cut_records(const uint32_t* __restrict__ selected,
                                                     const uint32_t* __restrict__ place, uint32_t T, uint32_t capacity,
                                                     CutNodes nodes, int32_t* __restrict__ records,
                                                     CutStatus* __restrict__ status) {
  const uint32_t node = blockIdx.x * 256u + threadIdx.x;
  long long gain = 0;
  u64 area = 0;
  if (node < T && selected[node]) {
    const uint32_t k = place[node] - 1;
    gain = nodes.gain[node];
    area = nodes.area[node];
    if (k < capacity) {
      const uint32_t children = nodes.children[node];
      int32_t* r = records + (size_t)k * kCutNodeWords;
      const long long split = children ? nodes.split[node] : 0ll;
      reinterpret_cast<int4*>(r)[0] = make_int4(nodes.level[node], nodes.id[node], (int32_t)nodes.area[node],
                                                (int32_t)nodes.leaves[node]);
      reinterpret_cast<int4*>(r)[1] = make_int4((int32_t)children, nodes.best_label[node], nodes.best_count[node], 0);
      reinterpret_cast<int4*>(r)[2] = make_int4((int32_t)(uint32_t)(u64)gain, (int32_t)((u64)gain >> 32),
                                                (int32_t)(uint32_t)(u64)split, (int32_t)((u64)split >> 32));
    } else {
      atomicOr(&status->flags, CUT_FLAG_RANGE);
    }
  }
  if (node == T - 1) status->cut_nodes = place[node];
  gain = WaveSum(gain);
  area = WaveSum(area);
  if ((threadIdx.x & 63) == 0) {
    if (gain) atomicAdd(reinterpret_cast<u64*>(&status->total), (u64)gain);
    if (area) atomicAdd(&status->covered, area);
  }
}

// Four pixels of the W-pitched planes a thread; `vector`: both planes start on 16 bytes.
__global__ __launch_bounds__(256) void k_cut_paint(const int32_t* __restrict__ ids, size_t pixels,
                                                   const int32_t* __restrict__ leaf_id, uint32_t R,
                                                   const uint32_t* __restrict__ leaf_node,
                                                   const uint32_t* __restrict__ place, int vector,
                                                   int32_t* __restrict__ out, CutStatus* __restrict__ status) {
  const size_t at = ((size_t)blockIdx.x * 256u + threadIdx.x) * 4;
  if (at >= pixels) return;
  const int n = pixels - at >= 4 ? 4 : (int)(pixels - at);
  int32_t in[4] = {-1, -1, -1, -1}, v[4];
  if (n == 4 && vector) {
    const int4 t = *reinterpret_cast<const int4*>(ids + at);
    in[0] = t.x, in[1] = t.y, in[2] = t.z, in[3] = t.w;
  } else {
    for (int k = 0; k < n; ++k) in[k] = ids[at + k];
  }
  int32_t last_id = -1, last = -1;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (in[k] < 0) {
      v[k] = -1;
    } else if (in[k] == last_id) {
      v[k] = last;
    } else {
      const uint32_t j = FindId(leaf_id, R, in[k]);
      if (j == R) {
        atomicOr(&status->flags, CUT_FLAG_RANGE);
        v[k] = -1;
      } else {
        v[k] = (int32_t)place[leaf_node[j]] - 1;
      }
      last_id = in[k];
      last = v[k];
    }
  }
  if (n == 4 && vector) {
    *reinterpret_cast<int4*>(out + at) = make_int4(v[0], v[1], v[2], v[3]);
  } else {
    for (int k = 0; k < n; ++k) out[at + k] = v[k];
  }
}

inline unsigned Blocks(size_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

void LaunchCutLeaves(const int32_t* list, uint32_t words, uint32_t area_word, uint32_t R, const int32_t* ids,
                     uint32_t n_ids, int32_t* leaf_id, uint32_t* leaf_area, uint32_t* leaf_col, CutStatus* status,
                     hipStream_t stream) {
  if (R == 0) return;
  hipLaunchKernelGGL(k_cut_leaves, dim3(Blocks(R)), dim3(256), 0, stream, list, words, area_word, R, ids, n_ids,
                     leaf_id, leaf_area, leaf_col, status);
}

void LaunchCutNodeKeys(const int32_t* leaf_id, const uint32_t* leaf_col, uint32_t R, const int32_t* table,
                       uint32_t n_ids, uint32_t L, unsigned long long* keys, uint32_t* vals, hipStream_t stream) {
  const uint32_t n = L * R;
  if (n == 0) return;
  hipLaunchKernelGGL(k_cut_node_keys, dim3(Blocks(n)), dim3(256), 0, stream, leaf_id, leaf_col, R, table, n_ids, n,
                     keys, vals);
}

void LaunchCutNodeMap(const uint32_t* vals, const uint32_t* rank, uint32_t R, uint32_t L, uint32_t* map,
                      uint32_t* level_first, CutStatus* status, hipStream_t stream) {
  const uint32_t n = L * R;
  if (n == 0) return;
  hipLaunchKernelGGL(k_cut_node_map, dim3(Blocks(n)), dim3(256), 0, stream, vals, rank, R, L, n, map, level_first,
                     status);
}

void LaunchCutNodeTable(const unsigned long long* keys, const uint32_t* vals, const uint32_t* rank,
                        const uint32_t* map, const uint32_t* leaf_area, uint32_t R, uint32_t L, uint32_t T,
                        const CutNodes& nodes, hipStream_t stream) {
  const uint32_t n = L * R;
  if (n == 0) return;
  hipLaunchKernelGGL(k_cut_node_table, dim3(Blocks(n)), dim3(256), 0, stream, keys, vals, rank, map, leaf_area, R, L,
                     n, T, nodes);
}

void LaunchCutPairKeys(const int32_t* pairs, uint32_t P, const uint32_t* map, uint32_t R, uint32_t L, int label_bits,
                       unsigned long long* keys, uint32_t* counts, hipStream_t stream) {
  const uint32_t n = L * P;
  if (n == 0) return;
  hipLaunchKernelGGL(k_cut_pair_keys, dim3(Blocks(n)), dim3(256), 0, stream, pairs, P, map, R, n, label_bits, keys,
                     counts);
}

void LaunchCutBest(const unsigned long long* keys, const uint32_t* counts, const uint32_t* rank, uint32_t n,
                   int label_bits, uint32_t T, uint32_t* sums, unsigned long long* best, CutStatus* status,
                   hipStream_t stream) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_cut_pair_sums, dim3(Blocks(n)), dim3(256), 0, stream, counts, rank, n, sums);
  hipLaunchKernelGGL(k_cut_best, dim3(Blocks(n)), dim3(256), 0, stream, keys, rank, sums, n, label_bits, T, best,
                     status);
}

void LaunchCutGainLabels(const unsigned long long* best, uint32_t T, int64_t penalty, const CutNodes& nodes,
                         hipStream_t stream) {
  if (T == 0) return;
  hipLaunchKernelGGL(k_cut_gain_labels, dim3(Blocks(T)), dim3(256), 0, stream, best, T, (long long)penalty, nodes);
}

void LaunchCutGainCheck(const CutGain* gains, size_t n, CutStatus* status, hipStream_t stream) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_cut_gain_check, dim3(Blocks(n)), dim3(256), 0, stream, gains, n, status);
}

void LaunchCutGainLookup(const CutGain* gains, size_t n, uint32_t T, const CutNodes& nodes, hipStream_t stream) {
  if (T == 0) return;
  hipLaunchKernelGGL(k_cut_gain_lookup, dim3(Blocks(T)), dim3(256), 0, stream, gains, n, T, nodes);
}

void LaunchCutDpBlock(const uint32_t* level_first, uint32_t L, const CutNodes& nodes, hipStream_t stream) {
  hipLaunchKernelGGL(k_cut_dp_block, dim3(1), dim3(1024), 0, stream, level_first, L, nodes);
}

void LaunchCutDpLevel(uint32_t first, uint32_t end, const CutNodes& nodes, hipStream_t stream) {
  hipLaunchKernelGGL(k_cut_dp_level, dim3(Blocks(end - first)), dim3(256), 0, stream, first, end, nodes);
}

void LaunchCutSelect(const uint32_t* map, uint32_t R, uint32_t L, uint32_t T, const uint32_t* keep,
                     uint32_t* leaf_node, uint32_t* selected, CutStatus* status, hipStream_t stream) {
  if (R == 0) return;
  hipLaunchKernelGGL(k_cut_select, dim3(Blocks(R)), dim3(256), 0, stream, map, R, L, T, keep, leaf_node, selected,
                     status);
}

void LaunchCutRecords(const uint32_t* selected, const uint32_t* place, uint32_t T, uint32_t capacity,
                      const CutNodes& nodes, int32_t* records, CutStatus* status, hipStream_t stream) {
  if (T == 0) return;
  hipLaunchKernelGGL(k_cut_records, dim3(Blocks(T)), dim3(256), 0, stream, selected, place, T, capacity, nodes,
                     records, status);
}

void LaunchCutPaint(const int32_t* ids, int W, int H, const int32_t* leaf_id, uint32_t R, const uint32_t* leaf_node,
                    const uint32_t* place, int32_t* out, CutStatus* status, hipStream_t stream) {
  const size_t pixels = (size_t)W * H;
  if (pixels == 0) return;
  const int vector = ((reinterpret_cast<uintptr_t>(ids) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  hipLaunchKernelGGL(k_cut_paint, dim3(Blocks((pixels + 3) / 4)), dim3(256), 0, stream, ids, pixels, leaf_id, R,
                     leaf_node, place, vector, out, status);
}

}  // namespace vsg_render_impl
