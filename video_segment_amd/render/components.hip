// components.hip -- the connected components of every region of a hierarchy level (gfx950): the device
// form of the reference's ConnectedComponents (segment_util/segmentation_util.cpp:1007-1101) applied
// to each region's rasterization, from the sorted runs level.hip leaves behind.
//
//   k_comp_init     parent[i] = i
//   k_comp_link     one thread per sorted run: its neighbours in the row above are a contiguous piece
//                   of the sorted runs (one binary search, then a walk); every pair is united in a
//                   lock-free union-find whose roots are the smallest run index of their set
//   k_comp_flatten  label[i] = find(i), and the (label, i) pairs for the sort
//   radix sort      stable, on the label: (region, component, y, left_x) order
//   scan            rank of every run's component among the components (a sum over segment heads)
//   k_comp_table    one thread per ordered run: its interval in the ordered list (and in the list
//                   LaunchFill paints the label image from); a segment head also writes its component's
//                   id, region and first interval, and a region's first head the region's first component
//   k_comp_finish   one thread per component: its index in its region and the region's count
//
// Area, bounding box and moments of a component are LaunchComponentMoments of level.hip on the table.
//
// Union-find.  parent[x] <= x always, and a word only ever decreases: a root r is hooked by
// atomicCAS(&parent[r], r, smaller root) and by nothing else, a non-root is only lowered to one of
// its ancestors (atomicMin).  A chain of parents is therefore strictly decreasing and ends after at
// most n steps whatever other threads do meanwhile; a failed hook means that another thread hooked
// the same root, of which there are fewer than n in a launch.  Both loops are counted against n and
// give up with COMP_FLAG_BOUND when the count runs out; no thread waits for another.
#include "render.h"
#include "render_device.h"

namespace vsg_render_impl {

namespace {

// every access to a parent word during k_comp_link is an agent-scope atomic: other workgroups hook
// and lower the same words in the same launch
__device__ __forceinline__ uint32_t LoadParent(const uint32_t* parent, uint32_t x) {
  return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of x, or kNoRoot after more than `bound` steps (then the flag is raised).  x < n.
constexpr uint32_t kNoRoot = 0xffffffffu;

__device__ __forceinline__ uint32_t Find(uint32_t* parent, uint32_t x, uint32_t bound, CompStatus* status) {
  for (uint32_t step = 0; step <= bound; ++step) {
    const uint32_t p = LoadParent(parent, x);
    if (p >= x) return x;   // p == x: a root (p > x cannot happen; it ends the walk all the same)
    const uint32_t g = LoadParent(parent, p);
    if (g < p) atomicMin(parent + x, g);   // path halving: x to its grandparent, an ancestor
    x = g < p ? g : p;
  }
  atomicOr(&status->flags, (uint32_t)COMP_FLAG_BOUND);
  return kNoRoot;
}

__device__ __forceinline__ void Unite(uint32_t* parent, uint32_t a, uint32_t b, uint32_t bound, CompStatus* status) {
  for (uint32_t attempt = 0; attempt <= bound; ++attempt) {
    a = Find(parent, a, bound, status);
    b = Find(parent, b, bound, status);
    if (a == kNoRoot || b == kNoRoot || a == b) return;
    const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
    const uint32_t seen = atomicCAS(parent + hi, hi, lo);
    if (seen == hi) return;
    // another thread hooked hi under `seen` < hi first: go on from there
    a = seen;
    b = lo;
  }
  atomicOr(&status->flags, (uint32_t)COMP_FLAG_BOUND);
}

__global__ __launch_bounds__(256) void k_comp_init(uint32_t* __restrict__ parent, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) parent[i] = i;
}

// One thread per sorted run i = (id, y, [l, r]).  With slack s (0 for N4, 1 for N8) run j of the same
// id in row y - 1 is a neighbour when left_j <= r + s and right_j >= l - s (ScanIntervalsNeighbored).
// The runs of one id and row are disjoint and ascending, so the neighbours are consecutive.  t = the
// first run whose key is at least (id, y - 1, max(l - s, 0)): every neighbour but possibly the one
// before it starts there; run t - 1 is one when it lies in that row and reaches l - s.  The walk ends
// with the row, with left_j > r + s, or at i (row y - 1 of the id lies before i).
__global__ __launch_bounds__(256) void k_comp_link(const unsigned long long* __restrict__ keys,
                                                   const uint32_t* __restrict__ rights, uint32_t n, int W,
                                                   int slack, uint32_t* __restrict__ parent,
                                                   CompStatus* __restrict__ status) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  uint32_t links = 0;
  if (i < n) {
    const unsigned long long key = keys[i];
    const uint32_t pos = (uint32_t)key, w = (uint32_t)W;
    const uint32_t y = pos / w, l = pos % w, r = rights[i];
    if (y > 0) {
      const unsigned long long id_bits = key & 0xffffffff00000000ull;
      const uint32_t row = (y - 1) * w;
      const uint32_t from = l > (uint32_t)slack ? l - (uint32_t)slack : 0u;
      const uint32_t to = r + (uint32_t)slack < w ? r + (uint32_t)slack : w - 1;
      const unsigned long long first_key = id_bits | (row + from), row_key = id_bits | row,
                               last_key = id_bits | (row + to);
      uint32_t lo = 0, hi = i;   // lower bound of first_key in [0, i)
      while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < first_key) lo = mid + 1;
        else hi = mid;
      }
      uint32_t j = lo;
      if (j > 0 && keys[j - 1] >= row_key && rights[j - 1] + (uint32_t)slack >= l) --j;
      for (; j < i && keys[j] <= last_key; ++j) {
        Unite(parent, i, j, n, status);
        ++links;
      }
    }
  }
  // one add per wavefront
  links = WaveSum(links);
  if ((threadIdx.x & 63) == 0 && links) atomicAdd(&status->links, (unsigned long long)links);
}

__global__ __launch_bounds__(256) void k_comp_flatten(uint32_t* __restrict__ parent, uint32_t n,
                                                      uint32_t* __restrict__ label, uint32_t* __restrict__ index,
                                                      CompStatus* __restrict__ status) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t root = Find(parent, i, n, status);
  label[i] = root == kNoRoot ? i : root;   // a label is always a run index; the flag fails the call
  index[i] = i;
}

// One thread per ordered position k.  order[k] < n is the sorted run there, label[k] its component's
// root, comp_rank[k] the number of heads in [0, k], region_rank[i] the (1-based) region of sorted run i.
__global__ __launch_bounds__(256) void k_comp_table(const uint32_t* __restrict__ label,
                                                    const uint32_t* __restrict__ order,
                                                    const uint32_t* __restrict__ comp_rank,
                                                    const uint32_t* __restrict__ region_rank,
                                                    const int4* __restrict__ intervals, uint32_t n,
                                                    uint32_t capacity_components, uint32_t capacity_regions,
                                                    int4* __restrict__ ordered, int4* __restrict__ fill,
                                                    int32_t* __restrict__ components,
                                                    uint32_t* __restrict__ region_first,
                                                    CompStatus* __restrict__ status) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n) return;
  const uint32_t i = order[k];
  if (i >= n) {   // cannot happen; nothing outside the lists is read
    atomicOr(&status->flags, (uint32_t)COMP_FLAG_BOUND);
    return;
  }
  const uint32_t c = comp_rank[k] - 1;
  const int4 v = intervals[i];   // y, left_x, right_x, id
  ordered[k] = v;
  if (fill) fill[k] = make_int4(v.x, v.y, v.z, (int)c);
  const bool head = k == 0 || label[k] != label[k - 1];
  if (head) {
    const uint32_t region = region_rank[i] - 1;
    if (c < capacity_components) {
      int32_t* out = components + (size_t)c * kLevelComponentWords;
      out[0] = v.w;
      out[1] = (int32_t)region;   // k_comp_finish turns it into the index within the region
      out[3] = (int32_t)k;
    } else {
      atomicOr(&status->flags, (uint32_t)COMP_FLAG_DROPPED);
    }
    const uint32_t before = k == 0 ? n : order[k - 1];
    const bool region_head = k == 0 || (before < n && region_rank[before] != region_rank[i]);
    if (region_head) {
      if (region < capacity_regions) region_first[region] = c;
      else atomicOr(&status->flags, (uint32_t)COMP_FLAG_DROPPED);
    }
  }
  if (k == n - 1) status->components = c + 1;
}

__global__ __launch_bounds__(256) void k_comp_finish(int32_t* __restrict__ components,
                                                     const uint32_t* __restrict__ region_first,
                                                     uint32_t capacity_components, uint32_t capacity_regions,
                                                     const uint32_t* __restrict__ n_regions_ptr,
                                                     const CompStatus* __restrict__ status) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  const uint32_t n_components = status->components, n_regions = *n_regions_ptr;
  if (c >= n_components || c >= capacity_components) return;
  int32_t* out = components + (size_t)c * kLevelComponentWords;
  const uint32_t region = (uint32_t)out[1];
  if (region >= n_regions || region >= capacity_regions) return;   // reported by k_comp_table
  const uint32_t first = region_first[region];
  const uint32_t next = region + 1 < n_regions && region + 1 < capacity_regions ? region_first[region + 1]
                                                                                : n_components;
  out[1] = (int32_t)(c - first);
  out[2] = (int32_t)(next - first);
}

}  // namespace

void LaunchCompLink(const unsigned long long* keys_sorted, const uint32_t* rights_sorted, uint32_t n, int width,
                    int slack, uint32_t* parent, uint32_t* label, uint32_t* index, CompStatus* status,
                    hipStream_t stream) {
  if (n == 0) return;
  const dim3 grid((n + 255) / 256), block(256);
  hipLaunchKernelGGL(k_comp_init, grid, block, 0, stream, parent, n);
  hipLaunchKernelGGL(k_comp_link, grid, block, 0, stream, keys_sorted, rights_sorted, n, width, slack, parent, status);
  hipLaunchKernelGGL(k_comp_flatten, grid, block, 0, stream, parent, n, label, index, status);
}

void LaunchCompTable(const uint32_t* label_sorted, const uint32_t* order, const uint32_t* comp_rank,
                     const uint32_t* region_rank, const Interval* intervals, uint32_t n,
                     uint32_t capacity_components, uint32_t capacity_regions, Interval* ordered, Interval* fill,
                     int32_t* components, uint32_t* region_first, const LevelStatus* level_status,
                     CompStatus* status, hipStream_t stream) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_comp_table, dim3((n + 255) / 256), dim3(256), 0, stream, label_sorted, order, comp_rank,
                     region_rank, reinterpret_cast<const int4*>(intervals), n, capacity_components, capacity_regions,
                     reinterpret_cast<int4*>(ordered), reinterpret_cast<int4*>(fill), components, region_first, status);
  // the number of components is on the device only: a thread per table slot, all but the first
  // status->components of them leave at once
  hipLaunchKernelGGL(k_comp_finish, dim3((capacity_components + 255) / 256), dim3(256), 0, stream, components,
                     region_first, capacity_components, capacity_regions, &level_status->regions, status);
}

}  // namespace vsg_render_impl
