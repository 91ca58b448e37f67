// adjacency.hip -- the region adjacency graph of an int32 plane (gfx950): which groups touch which, along
// how many pixel sides and at how many diagonal contacts, and how much of every group's perimeter lies
// on the frame edge and next to uncovered pixels.  The plane is the id plane of vsg_render_id_image or
// the label image of vsg_render_level_components; -1 is "no group".
//
//   k_adj_classify<count>  one block per frame row: how many keys the row emits; one add per block
//   k_adj_classify<emit>   the same walk: the keys (group, other, kind), in no order; one add per block
//                          and step of 256 positions reserves their slots
//   radix sort             keys only, on the used bits, into (group, other, kind) order
//   scan                   for every key the number of node heads (a new group) and of edge heads (a new
//                          (group, other) with a real other) in [0, i], in one 64-bit sum
//   k_adj_table            one thread per sorted key: a node head writes id, component and first_edge, an
//                          edge head the neighbour; the first and the last key of a run of equal keys
//                          add -i and i + 1 to the count the run stands for, which leaves its length
//   k_adj_finish           one thread per node: num_edges; the largest of them
//   k_adj_resolve          region planes only, one thread per edge: the neighbour's id -> its node index,
//                          by binary search in the node ids
//   k_copy_lists           of lists.hip: nodes and edges to the caller's device memory, if both fit
//
// Key layout, gb = the bits of the largest group (1..31):
//   bit 0                kind: 0 a pixel side, 1 a diagonal contact
//   bits [1, gb + 2)     other: the group across, or 1 << gb for the frame edge, 1 << gb | 1 for an
//                        uncovered pixel; both sort behind every group
//   bits [gb + 2, 2 gb + 2)  group
// A covered position emits one key per side that does not lead to its own group and, with diagonals, one
// per diagonal neighbour of another group: every key counts once, for the group of the position that
// emitted it, so the graph is symmetric without a single atomic on a count shared by two groups.
#include "render.h"
#include "render_device.h"
#include "render_scan.h"

namespace vsg_render_impl {

namespace {

constexpr int kAdjBlock = 256;
constexpr int kAdjWaves = kAdjBlock / 64;
constexpr int32_t kAdjOutside = -2;   // a position that is no pixel

// P at frame position (x, y), every negative value read as -1; kAdjOutside outside the frame.
__device__ __forceinline__ int32_t AdjAt(const int32_t* __restrict__ plane, int W, int H, int x, int y) {
  return (x >= 0 && x < W && y >= 0 && y < H) ? max(plane[(size_t)y * W + x], -1) : kAdjOutside;
}

// One block walks frame row blockIdx.x in steps of kAdjBlock positions, a thread a position.  The row
// itself goes through LDS with a halo of one position on each side; the rows above and below are read
// by the thread that needs them.  Positions beyond the row read kAdjOutside and emit nothing.
template <bool kEmit, bool kDiagonal>
__global__ __launch_bounds__(kAdjBlock) void k_adj_classify(const int32_t* __restrict__ plane, int W, int H,
                                                            int group_bits, uint32_t capacity,
                                                            unsigned long long* __restrict__ keys,
                                                            AdjStatus* __restrict__ status) {
  __shared__ int32_t s_row[kAdjBlock + 2];
  __shared__ uint32_t s_wave[kAdjWaves];
  __shared__ uint32_t s_base;
  const int y = blockIdx.x;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const unsigned long long below = (1ull << lane) - 1;
  constexpr int kSlots = kDiagonal ? 8 : 4;
  uint32_t counted = 0;   // count only: keys of this thread over all steps
  for (int x0 = 0; x0 < W; x0 += kAdjBlock) {
    const int x = x0 + t;
    s_row[t + 1] = AdjAt(plane, W, H, x, y);
    if (t == 0) s_row[0] = AdjAt(plane, W, H, x - 1, y);
    if (t == kAdjBlock - 1) s_row[kAdjBlock + 1] = AdjAt(plane, W, H, x + 1, y);
    __syncthreads();
    const int32_t c = s_row[t + 1];
    // sides first, then diagonals
    int32_t across[8];
    across[0] = AdjAt(plane, W, H, x, y - 1);
    across[1] = s_row[t];
    across[2] = s_row[t + 2];
    across[3] = AdjAt(plane, W, H, x, y + 1);
    if (kDiagonal) {
      across[4] = AdjAt(plane, W, H, x - 1, y - 1);
      across[5] = AdjAt(plane, W, H, x + 1, y - 1);
      across[6] = AdjAt(plane, W, H, x - 1, y + 1);
      across[7] = AdjAt(plane, W, H, x + 1, y + 1);
    }
    bool emit[8];
#pragma unroll
    for (int j = 0; j < kSlots; ++j) {
      emit[j] = c >= 0 && across[j] != c && (j < 4 || across[j] >= 0);
    }
    if (!kEmit) {
#pragma unroll
      for (int j = 0; j < kSlots; ++j) counted += emit[j] ? 1u : 0u;
      __syncthreads();   // s_row is rewritten by the next step
      continue;
    }
    // rank within the wavefront: the keys of slot j of all lanes come after those of slots before j
    uint32_t offset[8], in_wave = 0;
#pragma unroll
    for (int j = 0; j < kSlots; ++j) {
      const unsigned long long b = __ballot(emit[j]);
      offset[j] = in_wave + (uint32_t)__popcll(b & below);
      in_wave += (uint32_t)__popcll(b);
    }
    uint32_t before;
    if (BlockReserve<kAdjWaves>(in_wave, s_wave, &s_base, &status->emitted, &before)) {
      const uint32_t base = s_base;
      const unsigned long long mine = (unsigned long long)(uint32_t)c << (group_bits + 2);
#pragma unroll
      for (int j = 0; j < kSlots; ++j) {
        if (!emit[j]) continue;
        const int32_t a = across[j];
        const uint32_t other = a >= 0 ? (uint32_t)a : (1u << group_bits) | (a == kAdjOutside ? 0u : 1u);
        const uint32_t slot = base + before + offset[j];
        if (slot < capacity) keys[slot] = mine | (unsigned long long)other << 1 | (j < 4 ? 0ull : 1ull);
        else atomicOr(&status->flags, (uint32_t)ADJ_FLAG_OVERFLOW);
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
      for (int w = 0; w < kAdjWaves; ++w) total += s_wave[w];
      if (total) atomicAdd(&status->keys, (unsigned long long)total);
    }
  }
}

// One thread per sorted key i < n.  heads[i] = node heads << 32 | edge heads in [0, i].  What the sort
// hands back is checked before it is used as an index: a group or a neighbour above max_group, a
// neighbour equal to its group, a reserved value that is neither of the two, a diagonal contact with
// one of them, or a node or an edge without a slot raises ADJ_FLAG_RANGE, and nothing is written for
// that key.  nodes and edges have been cleared to zero.  comp_table: null, or the component table
// (kLevelComponentWords words an entry, id and component in words 0 and 1) the groups are indices of.
__global__ __launch_bounds__(256) void k_adj_table(const unsigned long long* __restrict__ keys,
                                                   const unsigned long long* __restrict__ heads, uint32_t n,
                                                   int group_bits, uint32_t max_group, uint32_t capacity_nodes,
                                                   uint32_t capacity_edges, const int32_t* __restrict__ comp_table,
                                                   int32_t* __restrict__ nodes, int32_t* __restrict__ edges,
                                                   AdjStatus* __restrict__ status) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const unsigned long long key = keys[i], seen = heads[i];
  const unsigned long long prev = i ? keys[i - 1] : 0ull, next = i + 1 < n ? keys[i + 1] : 0ull;
  if (i == n - 1) {
    status->nodes = (uint32_t)(seen >> 32);
    status->edges = (uint32_t)seen;
  }
  const unsigned long long group = AdjGroup(key, group_bits);
  const uint32_t other = AdjOther(key, group_bits);
  const bool diagonal = key & 1, reserved = AdjReserved(key, group_bits);
  const uint32_t r = (uint32_t)(seen >> 32) - 1, e = (uint32_t)seen - 1;
  bool good = group <= max_group && r < capacity_nodes;
  if (reserved) good = good && (other & ~(1u << group_bits)) <= 1u && !diagonal;
  else good = good && other <= max_group && other != (uint32_t)group && e < capacity_edges;
  if (comp_table && r != (uint32_t)group) good = false;   // every component has a side: group g is node g
  if (!good) {
    atomicOr(&status->flags, (uint32_t)ADJ_FLAG_RANGE);
    return;
  }
  int32_t* node = nodes + (size_t)r * kLevelNodeWords;
  int32_t* edge = edges + (size_t)(reserved ? 0u : e) * kLevelEdgeWords;
  const bool node_head = i == 0 || AdjGroup(prev, group_bits) != group;
  const bool pair_head = i == 0 || (prev >> 1) != (key >> 1);
  if (node_head) {
    node[0] = comp_table ? comp_table[(size_t)group * kLevelComponentWords + 0] : (int32_t)group;
    node[1] = comp_table ? comp_table[(size_t)group * kLevelComponentWords + 1] : -1;
    node[2] = (int32_t)((uint32_t)seen - (pair_head && !reserved ? 1u : 0u));
  }
  if (pair_head && !reserved) {
    edge[0] = (int32_t)other;   // a component's index is its node's; k_adj_resolve maps a region's id
    edge[1] = comp_table ? comp_table[(size_t)other * kLevelComponentWords + 0] : (int32_t)other;
  }
  // the run of keys equal to this one is one count: its length = (last + 1) - first
  const bool run_head = i == 0 || prev != key, run_tail = i == n - 1 || next != key;
  if (!run_head && !run_tail) return;
  const uint32_t add = (run_tail ? i + 1 : 0u) - (run_head ? i : 0u);
  uint32_t* count = reinterpret_cast<uint32_t*>(reserved ? node + 4 + (other & 1u) : edge + 2 + (diagonal ? 1 : 0));
  atomicAdd(count, add);
  if (!reserved && !diagonal) atomicAdd(reinterpret_cast<uint32_t*>(node + 6), add);
}

// One thread per node slot: num_edges from its own and its successor's first_edge.
__global__ __launch_bounds__(256) void k_adj_finish(int32_t* __restrict__ nodes, uint32_t capacity_nodes,
                                                    AdjStatus* __restrict__ status) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  const uint32_t n_nodes = status->nodes, n_edges = status->edges;
  uint32_t mine = 0;
  if (r < n_nodes && r < capacity_nodes) {
    int32_t* node = nodes + (size_t)r * kLevelNodeWords;
    const uint32_t first = (uint32_t)node[2];
    const uint32_t end = r + 1 < n_nodes && r + 1 < capacity_nodes ? (uint32_t)node[kLevelNodeWords + 2] : n_edges;
    if (end >= first && end <= n_edges) mine = end - first;
    else atomicOr(&status->flags, (uint32_t)ADJ_FLAG_RANGE);
    node[3] = (int32_t)mine;
  }
  mine = WaveMax(mine);
  if ((threadIdx.x & 63) == 0 && mine) atomicMax(&status->largest, mine);
}

// One thread per edge slot of a region plane: edge[0] holds the neighbour's id; its node is found by
// binary search in the node ids, which ascend.  An id that is no node raises ADJ_FLAG_RANGE.
__global__ __launch_bounds__(256) void k_adj_resolve(const int32_t* __restrict__ nodes, uint32_t capacity_nodes,
                                                     int32_t* __restrict__ edges, uint32_t capacity_edges,
                                                     AdjStatus* __restrict__ status) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  const uint32_t n_nodes = status->nodes, n_edges = status->edges;
  if (e >= n_edges || e >= capacity_edges || n_nodes > capacity_nodes) return;
  int32_t* edge = edges + (size_t)e * kLevelEdgeWords;
  const int32_t id = edge[1];
  uint32_t lo = 0, hi = n_nodes;   // the first node with an id >= id
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (nodes[(size_t)mid * kLevelNodeWords] < id) lo = mid + 1;
    else hi = mid;
  }
  if (lo < n_nodes && nodes[(size_t)lo * kLevelNodeWords] == id) edge[0] = (int32_t)lo;
  else atomicOr(&status->flags, (uint32_t)ADJ_FLAG_RANGE);
}

}  // namespace

void LaunchAdjClassify(const int32_t* plane, int width, int height, int group_bits, bool diagonal, bool emit,
                       uint32_t capacity, unsigned long long* keys, AdjStatus* status, hipStream_t stream) {
  const dim3 grid(height), block(kAdjBlock);
  if (emit && diagonal) {
    hipLaunchKernelGGL((k_adj_classify<true, true>), grid, block, 0, stream, plane, width, height, group_bits,
                       capacity, keys, status);
  } else if (emit) {
    hipLaunchKernelGGL((k_adj_classify<true, false>), grid, block, 0, stream, plane, width, height, group_bits,
                       capacity, keys, status);
  } else if (diagonal) {
    hipLaunchKernelGGL((k_adj_classify<false, true>), grid, block, 0, stream, plane, width, height, group_bits, 0u,
                       nullptr, status);
  } else {
    hipLaunchKernelGGL((k_adj_classify<false, false>), grid, block, 0, stream, plane, width, height, group_bits, 0u,
                       nullptr, status);
  }
}

void LaunchAdjTable(const unsigned long long* keys_sorted, const unsigned long long* heads, uint32_t n, int group_bits,
                    uint32_t max_group, uint32_t capacity_nodes, uint32_t capacity_edges, const int32_t* comp_table,
                    int32_t* nodes, int32_t* edges, AdjStatus* status, hipStream_t stream) {
  if (n == 0 || capacity_nodes == 0 || capacity_edges == 0) return;
  hipLaunchKernelGGL(k_adj_table, dim3((n + 255) / 256), dim3(256), 0, stream, keys_sorted, heads, n, group_bits,
                     max_group, capacity_nodes, capacity_edges, comp_table, nodes, edges, status);
  // the numbers of nodes and edges are on the device only: a thread per slot, all but the first
  // status->nodes (status->edges) of them leave at once
  hipLaunchKernelGGL(k_adj_finish, dim3((capacity_nodes + 255) / 256), dim3(256), 0, stream, nodes, capacity_nodes,
                     status);
  if (!comp_table) {
    hipLaunchKernelGGL(k_adj_resolve, dim3((capacity_edges + 255) / 256), dim3(256), 0, stream, nodes, capacity_nodes,
                       edges, capacity_edges, status);
  }
}

}  // namespace vsg_render_impl
