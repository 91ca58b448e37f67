// contours.hip -- the closed contours of every group of an int32 plane (gfx950), traced along the pixel
// sides ("cracks") that separate a group from everything else.  The plane is the id plane of
// vsg_render_id_image or the label image of vsg_render_level_components; -1 is "no group" and so is every
// position outside the frame.  The definition is in include/vsg_render.h.
//
//   k_contour_classify   one thread per pixel: its 4-bit crack mask; the number of cracks, one add per block
//   scan                 offset[p] = cracks of the pixels before p, so that crack (p, side) has the dense
//                        index offset[p] + popcount(mask[p] below side): dense order is key order
//   k_contour_emit       one thread per pixel: every crack's key and turn bit, its successor's index (two
//                        reads of the plane, one of mask and offset) and the state of the first doubling
//   k_contour_round<0>   pointer doubling over the successor permutation between two buffers, two rounds
//                        a launch, ceil(log2 cracks) rounds or one more: {next, smallest turn crack seen}.
//                        Afterwards every crack knows its contour's leader, the turn crack of smallest key
//   k_contour_cut        the second doubling's state: the leader points at itself with weight 0, every
//                        other crack at its successor with weight 1 when it is a turn
//   k_contour_round<1>   the same rounds: {next, turn cracks from here up to the leader}
//   k_contour_leaders    one key group << 32 | leader per contour, in no order; one add per wavefront
//   radix sort, scan     the contours in (group, leader) order; their groups' ranks (HeadFlag of render_scan.h)
//   k_contour_heads      one thread per contour: its number of vertices, its place for its leader to find
//   scan                 first_vertex
//   k_contour_vertices   one thread per crack: a turn crack writes its start corner at first_vertex + rank
//   k_contour_table      one thread per contour: the record but for length, box and area
//   k_contour_measure    one thread per vertex: its side's length and cross product, its corner's box;
//                        reduced per contour inside the wavefront, then integer atomics per wavefront and
//                        contour
//   k_contour_finish     holes and the longest contour
//   k_copy_lists         of lists.hip: records and vertices to the caller's device memory, if both fit
//
// No thread follows a contour: every kernel is one thread per pixel, crack, contour or vertex with a bounded
// amount of work.  Everything is an integer; sums are exact and the atomics (add, min, max) commute, so the
// result does not depend on the order of execution.  Every index that was read from memory is checked
// against its array before it is used.
#include "render.h"
#include "render_device.h"

#include <algorithm>
#include <utility>

#include <hipcub/hipcub.hpp>

namespace vsg_render_impl {

namespace {

constexpr int kContourBlock = 256;
constexpr uint32_t kTurnBit = 0x80000000u;
constexpr uint32_t kNone = 0xffffffffu;

__global__ __launch_bounds__(kContourBlock) void k_contour_classify(const int32_t* __restrict__ plane, int W, int H,
                                                                    uint8_t* __restrict__ mask,
                                                                    ContourStatus* __restrict__ status) {
  __shared__ uint32_t s_wave[kContourBlock / 64];
  const uint32_t p = blockIdx.x * (uint32_t)kContourBlock + threadIdx.x;
  const uint32_t pixels = (uint32_t)W * (uint32_t)H;
  uint32_t m = 0;
  if (p < pixels) {
    const int x = (int)(p % (uint32_t)W), y = (int)(p / (uint32_t)W);
    const int32_t g = plane[p];
    if (g >= 0) {
#pragma unroll
      for (int s = 0; s < 4; ++s) m |= (PlaneAt(plane, W, H, x + Dx(s + 3), y + Dy(s + 3)) != g ? 1u : 0u) << s;
    }
    mask[p] = (uint8_t)m;
  }
  uint32_t count = (uint32_t)__popc(m);
  count = WaveSum(count);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = count;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t total = 0;
#pragma unroll
    for (int w = 0; w < kContourBlock / 64; ++w) total += s_wave[w];
    if (total) atomicAdd(&status->cracks, (unsigned long long)total);
  }
}

struct MaskCount {
  __host__ __device__ uint32_t operator()(uint8_t m) const {
    return (m & 1u) + ((m >> 1) & 1u) + ((m >> 2) & 1u) + ((m >> 3) & 1u);
  }
};
typedef hipcub::TransformInputIterator<uint32_t, MaskCount, const uint8_t*> MaskIterator;

__device__ __forceinline__ uint32_t Below(uint32_t m, int s) { return (uint32_t)__popc(m & ((1u << s) - 1u)); }

// One thread per pixel.  n: the cracks the count pass found; every array has n entries.
__global__ __launch_bounds__(kContourBlock) void k_contour_emit(const int32_t* __restrict__ plane, int W, int H,
                                                                const uint8_t* __restrict__ mask,
                                                                const uint32_t* __restrict__ offset, uint32_t n,
                                                                uint32_t* __restrict__ key, uint32_t* __restrict__ succ,
                                                                uint2* __restrict__ state,
                                                                ContourStatus* __restrict__ status) {
  const uint32_t p = blockIdx.x * (uint32_t)kContourBlock + threadIdx.x;
  if (p >= (uint32_t)W * (uint32_t)H) return;
  const uint32_t m = mask[p];
  if (!m) return;
  const int x = (int)(p % (uint32_t)W), y = (int)(p / (uint32_t)W);
  const int32_t g = plane[p];
  const uint32_t base = offset[p];
  for (int s = 0; s < 4; ++s) {
    if (!((m >> s) & 1u)) continue;
    const uint32_t i = base + Below(m, s);
    // the corner where the crack ends: A lies ahead on the group's side, B ahead on the other side
    const int ax = x + Dx(s), ay = y + Dy(s);
    const int bx = ax + Dx(s + 3), by = ay + Dy(s + 3);
    int qx = x, qy = y, qs = (s + 1) & 3;                      // right turn: the next side of this pixel
    if (PlaneAt(plane, W, H, ax, ay) == g) {
      if (PlaneAt(plane, W, H, bx, by) != g) {
        qx = ax, qy = ay, qs = s;                              // straight on: the same side of A
      } else {
        qx = bx, qy = by, qs = (s + 3) & 3;                    // left turn: the side of B
      }
    }
    const uint32_t q = (uint32_t)qy * (uint32_t)W + (uint32_t)qx;
    const uint32_t qm = mask[q];
    uint32_t j = offset[q] + Below(qm, qs);
    // the corner where it starts: a straight predecessor is the same side of the pixel behind
    const int px = x - Dx(s), py = y - Dy(s);
    const bool straight = PlaneAt(plane, W, H, px, py) == g && PlaneAt(plane, W, H, px + Dx(s + 3), py + Dy(s + 3)) != g;
    if (i >= n || j >= n || !((qm >> qs) & 1u)) {
      atomicOr(&status->flags, (uint32_t)CONTOUR_FLAG_RANGE);
      if (i >= n) continue;
      j = i;
    }
    key[i] = (4u * p + (uint32_t)s) | (straight ? 0u : kTurnBit);
    succ[i] = j;
    state[i] = make_uint2(j, straight ? kNone : i);
  }
}

// Two rounds of pointer doubling, one thread per crack: in -> out.  kSum false: .y = the smallest; true: the
// sum.  One round makes {b.x, a.y + b.y} of crack i and {d.x, c.y + d.y} of crack b.x; the second joins the
// two, so three dependent gathers do what two launches of one gather each would.  A round more than a contour
// needs changes nothing: the minimum is there already, and the second doubling's fixed point weighs 0.
// Every .x is below n: k_contour_emit and k_contour_cut wrote nothing else; the clamp keeps a read of a slot
// neither of them wrote inside the array.
template <bool kSum>
__global__ __launch_bounds__(kContourBlock) void k_contour_round(const uint2* __restrict__ in, uint2* __restrict__ out,
                                                                 uint32_t n) {
  const uint32_t i = blockIdx.x * (uint32_t)kContourBlock + threadIdx.x;
  if (i >= n) return;
  const uint2 a = in[i];
  const uint2 b = in[min(a.x, n - 1u)];
  const uint2 c = in[min(b.x, n - 1u)];
  const uint2 d = in[min(c.x, n - 1u)];
  out[i] = make_uint2(d.x, kSum ? a.y + b.y + c.y + d.y : min(min(a.y, b.y), min(c.y, d.y)));
}

// Between the doublings: led = the first one's result.  A crack without a leader in range is its own.
__global__ __launch_bounds__(kContourBlock) void k_contour_cut(const uint2* __restrict__ led,
                                                               const uint32_t* __restrict__ key,
                                                               const uint32_t* __restrict__ succ, uint32_t n,
                                                               uint32_t* __restrict__ leader, uint2* __restrict__ state,
                                                               ContourStatus* __restrict__ status) {
  const uint32_t i = blockIdx.x * (uint32_t)kContourBlock + threadIdx.x;
  if (i >= n) return;
  uint32_t l = led[i].y;
  if (l >= n) {
    atomicOr(&status->flags, (uint32_t)CONTOUR_FLAG_RANGE);
    l = i;
  }
  leader[i] = l;
  state[i] = l == i ? make_uint2(i, 0u) : make_uint2(succ[i], key[i] >> 31);
}

__global__ __launch_bounds__(kContourBlock) void k_contour_leaders(const uint32_t* __restrict__ leader,
                                                                   const uint32_t* __restrict__ key,
                                                                   const int32_t* __restrict__ plane, uint32_t n,
                                                                   uint32_t capacity,
                                                                   unsigned long long* __restrict__ ckeys,
                                                                   ContourStatus* __restrict__ status) {
  const uint32_t i = blockIdx.x * (uint32_t)kContourBlock + threadIdx.x;
  if (i >= n || leader[i] != i) return;
  const uint32_t slot = atomicAdd(&status->contours, 1u);   // one add per wavefront after the compiler
  if (slot >= capacity) {
    atomicOr(&status->flags, (uint32_t)CONTOUR_FLAG_OVERFLOW);
    return;
  }
  const uint32_t g = (uint32_t)plane[(key[i] & ~kTurnBit) >> 2];
  ckeys[slot] = (unsigned long long)g << 32 | i;
}

// One thread per slot of the sorted contour keys; the first status->contours of them are contours.
// ranked: the second doubling's result.
__global__ __launch_bounds__(kContourBlock) void k_contour_heads(const unsigned long long* __restrict__ ckeys,
                                                                 const uint32_t* __restrict__ succ,
                                                                 const uint2* __restrict__ ranked, uint32_t n,
                                                                 uint32_t capacity, uint32_t* __restrict__ count,
                                                                 uint32_t* __restrict__ place,
                                                                 ContourStatus* __restrict__ status) {
  const uint32_t j = blockIdx.x * (uint32_t)kContourBlock + threadIdx.x;
  if (j >= capacity) return;
  uint32_t c = 0;
  if (j < min(status->contours, capacity)) {
    const uint32_t l = (uint32_t)ckeys[j];
    if (l < n) {
      c = 1u + ranked[succ[l]].y;
      place[l] = j;
    }
    if (l >= n || c < 4u || c > n) {
      atomicOr(&status->flags, (uint32_t)CONTOUR_FLAG_RANGE);
      c = 0;
    }
  }
  count[j] = c;
}

__global__ __launch_bounds__(kContourBlock) void k_contour_vertices(const uint32_t* __restrict__ key,
                                                                    const uint32_t* __restrict__ leader,
                                                                    const uint2* __restrict__ ranked,
                                                                    const uint32_t* __restrict__ place,
                                                                    const uint32_t* __restrict__ count,
                                                                    const uint32_t* __restrict__ first, uint32_t n,
                                                                    uint32_t capacity, int W, int2* __restrict__ vertices,
                                                                    uint32_t* __restrict__ owner,
                                                                    ContourStatus* __restrict__ status) {
  const uint32_t i = blockIdx.x * (uint32_t)kContourBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t k = key[i];
  if (!(k & kTurnBit)) return;
  const uint32_t l = leader[i];
  const uint32_t j = place[l];
  if (j >= capacity) {
    atomicOr(&status->flags, (uint32_t)CONTOUR_FLAG_RANGE);
    return;
  }
  const uint32_t c = count[j], back = ranked[i].y;
  const uint32_t r = i == l ? 0u : c - back;   // back turn cracks lie in [i, leader)
  const uint32_t v = first[j] + r;
  if ((i != l && (back == 0 || back >= c)) || v >= n) {
    atomicOr(&status->flags, (uint32_t)CONTOUR_FLAG_RANGE);
    return;
  }
  const uint32_t p = (k & ~kTurnBit) >> 2;
  const int s = (int)(k & 3u);
  const int x = (int)(p % (uint32_t)W), y = (int)(p / (uint32_t)W);
  // where side s starts: top (x, y), right (x + 1, y), bottom (x + 1, y + 1), left (x, y + 1)
  vertices[v] = make_int2(x + (s == 1 || s == 2 ? 1 : 0), y + (s >= 2 ? 1 : 0));
  owner[v] = j;
}

// comp_table: null (id = the key's group, component = -1, group = its rank), or the component table the
// groups index.
__global__ __launch_bounds__(kContourBlock) void k_contour_table(const unsigned long long* __restrict__ ckeys,
                                                                 const uint32_t* __restrict__ rank,
                                                                 const uint32_t* __restrict__ count,
                                                                 const uint32_t* __restrict__ first, uint32_t capacity,
                                                                 uint32_t max_group,
                                                                 const int32_t* __restrict__ comp_table,
                                                                 int32_t* __restrict__ records,
                                                                 ContourStatus* __restrict__ status) {
  const uint32_t j = blockIdx.x * (uint32_t)kContourBlock + threadIdx.x;
  const uint32_t n_contours = min(status->contours, capacity);
  if (j >= n_contours) return;
  const uint32_t g = (uint32_t)(ckeys[j] >> 32);
  int32_t* out = records + (size_t)j * kLevelContourWords;
  if (g > max_group) {
    atomicOr(&status->flags, (uint32_t)CONTOUR_FLAG_RANGE);
    out[0] = out[1] = out[2] = -1;
  } else if (comp_table) {
    out[0] = comp_table[(size_t)g * kLevelComponentWords + 0];
    out[1] = comp_table[(size_t)g * kLevelComponentWords + 1];
    out[2] = (int32_t)g;
  } else {
    out[0] = (int32_t)g;
    out[1] = -1;
    out[2] = (int32_t)rank[j] - 1;
  }
  out[3] = (int32_t)first[j];
  out[4] = (int32_t)count[j];
  out[5] = 0;
  out[6] = out[7] = 0x7fffffff;
  out[8] = out[9] = (int32_t)0x80000000u;
  out[10] = out[11] = 0;
  if (j == n_contours - 1) status->vertices = first[j] + count[j];
}

// One thread per vertex slot; the first status->vertices are vertices.
__global__ __launch_bounds__(kContourBlock) void k_contour_measure(const int2* __restrict__ vertices,
                                                                   const uint32_t* __restrict__ owner,
                                                                   const uint32_t* __restrict__ count,
                                                                   const uint32_t* __restrict__ first, uint32_t n,
                                                                   uint32_t capacity, int32_t* __restrict__ records,
                                                                   ContourStatus* __restrict__ status) {
  const uint32_t v = blockIdx.x * (uint32_t)kContourBlock + threadIdx.x;
  const int lane = threadIdx.x & 63;
  uint32_t j = kNone;
  long long area = 0;
  int32_t length = 0, lo_x = 0x7fffffff, lo_y = 0x7fffffff, hi_x = (int32_t)0x80000000u, hi_y = (int32_t)0x80000000u;
  if (v < min(status->vertices, n)) {
    j = owner[v];
    if (j < capacity) {
      const uint32_t f = first[j], c = count[j];
      const uint32_t m = v - f;
      if (v >= f && m < c && f + c <= n) {
        const int2 a = vertices[v], b = vertices[m + 1 == c ? f : v + 1];
        area = (long long)a.x * b.y - (long long)b.x * a.y;
        length = abs(b.x - a.x) + abs(b.y - a.y);
        lo_x = hi_x = a.x;
        lo_y = hi_y = a.y;
      } else {
        j = kNone;
      }
    } else {
      j = kNone;
    }
    if (j == kNone) atomicOr(&status->flags, (uint32_t)CONTOUR_FLAG_RANGE);
  }
  // the vertices of a contour are consecutive: lane l gathers [l, l + 2s) of its own contour
  for (int s = 1; s < 64; s <<= 1) {
    const uint32_t oj = __shfl_down(j, s);
    const int a_lo = __shfl_down((int)(uint32_t)(unsigned long long)area, s);
    const int a_hi = __shfl_down((int)(uint32_t)((unsigned long long)area >> 32), s);
    const int32_t o_len = __shfl_down(length, s);
    const int32_t o_lx = __shfl_down(lo_x, s), o_ly = __shfl_down(lo_y, s);
    const int32_t o_hx = __shfl_down(hi_x, s), o_hy = __shfl_down(hi_y, s);
    if (lane + s < 64 && oj == j) {
      area += (long long)((unsigned long long)(uint32_t)a_hi << 32 | (uint32_t)a_lo);
      length += o_len;
      lo_x = min(lo_x, o_lx);
      lo_y = min(lo_y, o_ly);
      hi_x = max(hi_x, o_hx);
      hi_y = max(hi_y, o_hy);
    }
  }
  const uint32_t before = __shfl_up(j, 1);
  if (j != kNone && (lane == 0 || before != j)) {
    int32_t* out = records + (size_t)j * kLevelContourWords;
    atomicAdd(&out[5], length);
    atomicMin(&out[6], lo_x);
    atomicMin(&out[7], lo_y);
    atomicMax(&out[8], hi_x);
    atomicMax(&out[9], hi_y);
    atomicAdd(reinterpret_cast<unsigned long long*>(out + 10), (unsigned long long)area);
  }
}

__global__ __launch_bounds__(kContourBlock) void k_contour_finish(const int32_t* __restrict__ records,
                                                                  uint32_t capacity,
                                                                  ContourStatus* __restrict__ status) {
  const uint32_t j = blockIdx.x * (uint32_t)kContourBlock + threadIdx.x;
  uint32_t length = 0;
  bool hole = false;
  if (j < min(status->contours, capacity)) {
    const int32_t* rec = records + (size_t)j * kLevelContourWords;
    length = (uint32_t)rec[5];
    hole = rec[11] < 0;   // the high word of area2
  }
  const uint32_t holes = (uint32_t)__popcll(__ballot(hole));
  length = WaveMax(length);
  if ((threadIdx.x & 63) == 0) {
    if (holes) atomicAdd(&status->holes, holes);
    if (length) atomicMax(&status->largest, length);
  }
}

inline dim3 GridOf(uint32_t n) { return dim3((n + kContourBlock - 1) / kContourBlock); }

}  // namespace

size_t ContourClassifyTempBytes(uint32_t pixels) {
  size_t offsets = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, offsets, MaskIterator((const uint8_t*)nullptr, MaskCount()), (uint32_t*)nullptr,
                                         (int)pixels, (hipStream_t) nullptr);
  return offsets;
}

hipError_t ContourClassify(void* temp, size_t temp_bytes, const int32_t* plane, int width, int height, uint8_t* mask,
                           uint32_t* offset, ContourStatus* status, hipStream_t stream) {
  const uint32_t pixels = (uint32_t)width * (uint32_t)height;
  hipLaunchKernelGGL(k_contour_classify, GridOf(pixels), dim3(kContourBlock), 0, stream, plane, width, height, mask,
                     status);
  return hipcub::DeviceScan::ExclusiveSum(temp, temp_bytes, MaskIterator(mask, MaskCount()), offset, (int)pixels,
                                          stream);
}

void LaunchContourEmit(const int32_t* plane, int width, int height, const uint8_t* mask, const uint32_t* offset,
                       uint32_t n, uint32_t* key, uint32_t* succ, uint2* state, ContourStatus* status,
                       hipStream_t stream) {
  hipLaunchKernelGGL(k_contour_emit, GridOf((uint32_t)width * (uint32_t)height), dim3(kContourBlock), 0, stream, plane,
                     width, height, mask, offset, n, key, succ, state, status);
}

int ContourRounds(uint32_t n) {
  int rounds = 0;
  while (rounds < 32 && (1ull << rounds) < n) ++rounds;
  return (rounds + 1) / 2 * 2;
}

const uint2* LaunchContourTrace(const uint32_t* key, const uint32_t* succ, uint32_t n, int rounds, uint2* state_a,
                                uint2* state_b, uint32_t* leader, ContourStatus* status, hipStream_t stream) {
  uint2* in = state_a;
  uint2* out = state_b;
  for (int r = 0; r < rounds; r += 2) {
    hipLaunchKernelGGL((k_contour_round<false>), GridOf(n), dim3(kContourBlock), 0, stream, in, out, n);
    std::swap(in, out);
  }
  hipLaunchKernelGGL(k_contour_cut, GridOf(n), dim3(kContourBlock), 0, stream, in, key, succ, n, leader, out, status);
  std::swap(in, out);
  for (int r = 0; r < rounds; r += 2) {
    hipLaunchKernelGGL((k_contour_round<true>), GridOf(n), dim3(kContourBlock), 0, stream, in, out, n);
    std::swap(in, out);
  }
  return in;
}

const uint2* LaunchContourSums(uint2* in, uint2* out, uint32_t n, int rounds, hipStream_t stream) {
  for (int r = 0; r < rounds; r += 2) {
    hipLaunchKernelGGL((k_contour_round<true>), GridOf(n), dim3(kContourBlock), 0, stream, in, out, n);
    std::swap(in, out);
  }
  return in;
}

void LaunchContourLeaders(const uint32_t* leader, const uint32_t* key, const int32_t* plane, uint32_t n,
                          uint32_t capacity, unsigned long long* ckeys, ContourStatus* status, hipStream_t stream) {
  hipLaunchKernelGGL(k_contour_leaders, GridOf(n), dim3(kContourBlock), 0, stream, leader, key, plane, n, capacity,
                     ckeys, status);
}

hipError_t ContourVertices(void* temp, size_t temp_bytes, const unsigned long long* ckeys_sorted, const uint32_t* key,
                           const uint32_t* succ, const uint32_t* leader, const uint2* ranked, uint32_t n,
                           uint32_t capacity, int width, uint32_t* place, uint32_t* count, uint32_t* first,
                           int32_t* vertices, uint32_t* owner, ContourStatus* status, hipStream_t stream) {
  hipLaunchKernelGGL(k_contour_heads, GridOf(capacity), dim3(kContourBlock), 0, stream, ckeys_sorted, succ, ranked, n,
                     capacity, count, place, status);
  const hipError_t e = ExclusiveSumU32(temp, temp_bytes, count, first, (int)capacity, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_contour_vertices, GridOf(n), dim3(kContourBlock), 0, stream, key, leader, ranked, place, count,
                     first, n, capacity, width, reinterpret_cast<int2*>(vertices), owner, status);
  return hipSuccess;
}

void LaunchContourTable(const unsigned long long* ckeys_sorted, const uint32_t* rank, const uint32_t* count,
                        const uint32_t* first, const int32_t* vertices, const uint32_t* owner, uint32_t n,
                        uint32_t capacity, uint32_t max_group, const int32_t* comp_table, int32_t* records,
                        ContourStatus* status, hipStream_t stream) {
  hipLaunchKernelGGL(k_contour_table, GridOf(capacity), dim3(kContourBlock), 0, stream, ckeys_sorted, rank, count,
                     first, capacity, max_group, comp_table, records, status);
  hipLaunchKernelGGL(k_contour_measure, GridOf(n), dim3(kContourBlock), 0, stream,
                     reinterpret_cast<const int2*>(vertices), owner, count, first, n, capacity, records, status);
  hipLaunchKernelGGL(k_contour_finish, GridOf(capacity), dim3(kContourBlock), 0, stream, records, capacity, status);
}

}  // namespace vsg_render_impl
