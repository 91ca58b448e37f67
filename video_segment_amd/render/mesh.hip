// mesh.hip -- the shared-segment mesh of an int32 plane (gfx950): the contours of contours.hip cut at the
// junction corners into halves, every half paired with its twin on the other side, one of the two the
// segment.  The definition is in include/vsg_render.h.  The contour stages have run before: every crack i
// has key[i] (bit 31: turn), succ[i], leader[i], place[leader] = its contour j, ranked[i].y = the turn cracks
// in [i, leader); count[j], first[j] and the records of the contours are there as well.
//
//   k_mesh_junctions    one thread per crack: sides() of its start corner from four reads of P; a junction
//                       marks its contour; the junction corners, one add per wavefront (of the up to four
//                       cracks that start at a corner the first in side order counts it)
//   k_mesh_seed         one thread per crack: the head bit (start corner a junction, or the leader of a
//                       contour without one) and the doubling state: the leader points at itself with weight
//                       0, every other crack at its successor with weight head bit
//   k_contour_round<1>  the rounds of contours.hip: {next, heads in [i, leader)}
//   k_mesh_loop_counts  one thread per contour: its number of halves
//   scan                first_ref
//   k_mesh_halves       one thread per crack: its half = first_ref + the heads passed since the leader; a head
//                       enters itself, the last crack of a half itself; an owner head takes a slot for
//                       group << 32 | head, one add per wavefront after the compiler
//   radix sort          the segments in (group, first crack) order
//   k_mesh_seg_heads    one thread per segment: its half learns its index; its number of vertices
//   scan                first_vertex
//   k_mesh_vertices     one thread per crack of an owner half: its start corner when it is the first or a turn
//                       crack, the end corner too when it is the last of an open half
//   k_mesh_records      one thread per segment: the record but for length
//   k_mesh_links        one thread per half and per contour: the ref (through the twin crack's half where the
//                       half is not the owner, O(1)) and the loop record
//   k_mesh_measure      one thread per vertex: its side's length, reduced per segment inside the wavefront,
//                       then one integer add per wavefront and segment
//   k_mesh_finish       one thread per segment: closed, shared and the longest, one atomic each per wavefront
//   k_copy_lists        of lists.hip: the four lists to the caller's device memory, if all four fit
//
// No thread walks a contour or a segment.  Everything is an integer, the atomics are add and max, and where
// several threads store to one word they store the same value.  Every index read from memory is checked
// against its array before it is used.
#include "render.h"
#include "render_device.h"

#include <algorithm>

namespace vsg_render_impl {

namespace {

constexpr int kMeshBlock = 256;
constexpr uint32_t kNone = 0xffffffffu;
constexpr uint32_t kKeyMask = 0x7fffffffu;
constexpr uint8_t kHeadBit = 0x80;

__device__ __forceinline__ void Flag(MeshStatus* status) { atomicOr(&status->flags, (uint32_t)MESH_FLAG_RANGE); }

// What the contour stages left, and what the mesh kernels add per crack, half and contour.
struct MeshView {
  const int32_t* plane;
  int W, H;
  const uint8_t* mask;          // per pixel
  const uint32_t* offset;       // per pixel
  uint32_t n;                   // cracks
  const uint32_t* key;
  const uint32_t* succ;
  const uint32_t* leader;
  const uint32_t* place;
  const uint2* ranked;
  uint32_t contours;            // the number of contours; count, first, records, hasj, nrefs, first_ref
  const uint32_t* count;
  const int32_t* records;       // kLevelContourWords each
  const uint8_t* sides;         // per crack: sides() of the start corner, kHeadBit
  const uint2* heads;           // per crack: .y = heads in [i, leader)
  const uint32_t* nrefs;
  const uint32_t* first_ref;
};

// The contour of crack i, or kNone.
__device__ __forceinline__ uint32_t ContourOf(const MeshView& m, uint32_t i) {
  const uint32_t l = m.leader[i];
  if (l >= m.n) return kNone;
  const uint32_t j = m.place[l];
  return j < m.contours ? j : kNone;
}

// The dense index of the crack on the other side of crack i (pixel across, side + 2), or kNone when there is
// none: the other side is no group.
__device__ __forceinline__ uint32_t Twin(const MeshView& m, uint32_t i) {
  const uint32_t k = m.key[i] & kKeyMask;
  const uint32_t p = k >> 2;
  const int s = (int)(k & 3u);
  const int x = (int)(p % (uint32_t)m.W) + Dx(s + 3), y = (int)(p / (uint32_t)m.W) + Dy(s + 3);
  if (x < 0 || x >= m.W || y < 0 || y >= m.H) return kNone;
  const uint32_t q = (uint32_t)y * (uint32_t)m.W + (uint32_t)x;
  const uint32_t qm = m.mask[q];
  const int qs = (s + 2) & 3;
  if (!((qm >> qs) & 1u)) return kNone;
  const uint32_t t = m.offset[q] + (uint32_t)__popc(qm & ((1u << qs) - 1u));
  return t < m.n ? t : kNone;
}

// Turn cracks in [leader, i] of i's contour of c vertices, l its leader.
__device__ __forceinline__ uint32_t TurnsUpTo(const MeshView& m, uint32_t i, uint32_t l, uint32_t c) {
  return i == l ? 1u : c - min(m.ranked[i].y, c) + (m.key[i] >> 31);
}

// Turn cracks in (h, i] for crack i of the half with head h, both of contour j: i's vertex rank in the half.
// The half that holds a leader which is no head begins before the leader and ends after it: there the cracks
// from the leader on have passed every head of the contour, the ones before it none.
__device__ __forceinline__ uint32_t RankInHalf(const MeshView& m, uint32_t i, uint32_t h, uint32_t j, uint32_t half) {
  const uint32_t l = m.leader[i];
  const uint32_t c = m.count[j];
  const uint32_t ti = TurnsUpTo(m, i, l, c);
  if (h == l) return ti - 1u;
  const uint32_t th = TurnsUpTo(m, h, l, c);
  const bool after = half == m.first_ref[j] && (i == l || m.heads[i].y > (uint32_t)(m.sides[i] >> 7));
  return after ? ti + c - th : ti - th;
}

__global__ __launch_bounds__(kMeshBlock) void k_mesh_junctions(MeshView m, uint8_t* __restrict__ sides,
                                                               uint32_t* __restrict__ hasj,
                                                               MeshStatus* __restrict__ status) {
  const uint32_t i = blockIdx.x * (uint32_t)kMeshBlock + threadIdx.x;
  bool counts = false;
  if (i < m.n) {
    const uint32_t k = m.key[i] & kKeyMask;
    const uint32_t p = k >> 2;
    const int s = (int)(k & 3u);
    const int cx = (int)(p % (uint32_t)m.W) + (s == 1 || s == 2 ? 1 : 0), cy = (int)(p / (uint32_t)m.W) + (s >= 2 ? 1 : 0);
    const int32_t a = PlaneAt(m.plane, m.W, m.H, cx - 1, cy - 1), b = PlaneAt(m.plane, m.W, m.H, cx, cy - 1);
    const int32_t c = PlaneAt(m.plane, m.W, m.H, cx, cy), d = PlaneAt(m.plane, m.W, m.H, cx - 1, cy);
    const uint32_t sd = (a != b) + (b != c) + (c != d) + (d != a);
    sides[i] = (uint8_t)sd;
    if (sd >= 3u) {
      // the cracks that start here: top of c, right of d, bottom of a, left of b
      const int firstside = (c >= 0 && c != b) ? 0 : (d >= 0 && d != c) ? 1 : (a >= 0 && a != d) ? 2 : 3;
      counts = s == firstside;
      const uint32_t j = ContourOf(m, i);
      if (j == kNone) Flag(status);
      else hasj[j] = 1u;
    }
  }
  const uint32_t total = (uint32_t)__popcll(__ballot(counts));
  if ((threadIdx.x & 63) == 0 && total) atomicAdd(&status->junctions, total);
}

__global__ __launch_bounds__(kMeshBlock) void k_mesh_seed(MeshView m, const uint32_t* __restrict__ hasj,
                                                          uint8_t* __restrict__ sides, uint2* __restrict__ state,
                                                          MeshStatus* __restrict__ status) {
  const uint32_t i = blockIdx.x * (uint32_t)kMeshBlock + threadIdx.x;
  if (i >= m.n) return;
  const uint32_t j = ContourOf(m, i);
  const uint32_t sd = sides[i] & 7u;
  if (j == kNone) {
    Flag(status);
    state[i] = make_uint2(i, 0u);
    return;
  }
  const bool is_leader = m.leader[i] == i;
  const bool head = sd >= 3u || (is_leader && !hasj[j]);
  sides[i] = (uint8_t)(sd | (head ? kHeadBit : 0));
  state[i] = is_leader ? make_uint2(i, 0u) : make_uint2(min(m.succ[i], m.n - 1u), head ? 1u : 0u);
}

__global__ __launch_bounds__(kMeshBlock) void k_mesh_loop_counts(MeshView m, const unsigned long long* __restrict__ ckeys,
                                                                 uint32_t* __restrict__ nrefs,
                                                                 MeshStatus* __restrict__ status) {
  const uint32_t j = blockIdx.x * (uint32_t)kMeshBlock + threadIdx.x;
  if (j >= m.contours) return;
  const uint32_t l = (uint32_t)ckeys[j];
  uint32_t c = 0;
  if (l < m.n && m.succ[l] < m.n) c = (uint32_t)(m.sides[l] >> 7) + m.heads[m.succ[l]].y;
  if (c == 0 || c > m.n) {
    Flag(status);
    c = 1;
  }
  nrefs[j] = c;
}

__global__ __launch_bounds__(kMeshBlock) void k_mesh_halves(MeshView m, uint32_t* __restrict__ half,
                                                            uint32_t* __restrict__ head_of,
                                                            uint32_t* __restrict__ last_of,
                                                            unsigned long long* __restrict__ skeys,
                                                            MeshStatus* __restrict__ status) {
  const uint32_t i = blockIdx.x * (uint32_t)kMeshBlock + threadIdx.x;
  if (i >= m.n) return;
  if (i == 0) status->refs = m.first_ref[m.contours - 1] + m.nrefs[m.contours - 1];
  const uint32_t j = ContourOf(m, i);
  if (j == kNone) {
    Flag(status);
    half[i] = kNone;
    return;
  }
  const uint32_t l = m.leader[i];
  const uint32_t c = m.nrefs[j];
  const uint32_t ahead_all = c - (uint32_t)(m.sides[l] >> 7);               // heads but the leader
  const bool head = (m.sides[i] >> 7) != 0;
  uint32_t pos = 0;
  if (i != l) {
    const uint32_t b = m.heads[i].y;
    const uint32_t ahead = b - (head ? 1u : 0u);                             // heads in (i, leader)
    if (b < (head ? 1u : 0u) || ahead > ahead_all) {
      Flag(status);
      half[i] = kNone;
      return;
    }
    pos = (ahead_all - ahead) % c;                                           // heads in (leader, i], wrapped
  }
  const uint32_t hf = m.first_ref[j] + pos;
  if (hf >= m.n) {
    Flag(status);
    half[i] = kNone;
    return;
  }
  half[i] = hf;
  const uint32_t nx = m.succ[i];
  if (nx < m.n && (m.sides[nx] >> 7)) last_of[hf] = i;
  if (!head) return;
  head_of[hf] = i;
  const uint32_t k = m.key[i] & kKeyMask;
  const uint32_t p = k >> 2;
  const int s = (int)(k & 3u);
  const int32_t g = m.plane[p];
  const int32_t o = PlaneAt(m.plane, m.W, m.H, (int)(p % (uint32_t)m.W) + Dx(s + 3), (int)(p / (uint32_t)m.W) + Dy(s + 3));
  if (o < g) {
    const uint32_t slot = atomicAdd(&status->segments, 1u);
    if (slot < m.n) skeys[slot] = (unsigned long long)(uint32_t)g << 32 | i;
  }
}

// n_segments: status->segments as the host read it.
__global__ __launch_bounds__(kMeshBlock) void k_mesh_seg_heads(MeshView m, const unsigned long long* __restrict__ skeys,
                                                               uint32_t n_segments, uint32_t n_halves,
                                                               const uint32_t* __restrict__ half,
                                                               const uint32_t* __restrict__ last_of,
                                                               uint32_t* __restrict__ seg_of,
                                                               uint32_t* __restrict__ scount,
                                                               MeshStatus* __restrict__ status) {
  const uint32_t s = blockIdx.x * (uint32_t)kMeshBlock + threadIdx.x;
  if (s >= n_segments) return;
  const uint32_t h = (uint32_t)skeys[s];
  uint32_t nv = 0;
  if (h < m.n && (m.sides[h] >> 7)) {
    const uint32_t hf = half[h];
    const uint32_t j = ContourOf(m, h);
    if (hf < n_halves && j != kNone) {
      const uint32_t e = last_of[hf];
      if (e < m.n && half[e] == hf) {
        seg_of[hf] = s;
        const bool closed = (m.sides[h] & 7u) < 3u;
        nv = RankInHalf(m, e, h, j, hf) + (closed ? 1u : 2u);
      }
    }
  }
  if (nv < 2u || nv > m.n + 1u) {
    Flag(status);
    nv = 0;
  }
  scount[s] = nv;
}

__global__ __launch_bounds__(kMeshBlock) void k_mesh_vertices(MeshView m, uint32_t n_segments, uint32_t n_halves,
                                                              const uint32_t* __restrict__ half,
                                                              const uint32_t* __restrict__ head_of,
                                                              const uint32_t* __restrict__ last_of,
                                                              const uint32_t* __restrict__ seg_of,
                                                              const uint32_t* __restrict__ scount,
                                                              const uint32_t* __restrict__ sfirst, uint32_t capacity,
                                                              int2* __restrict__ vertices, uint32_t* __restrict__ vseg,
                                                              MeshStatus* __restrict__ status) {
  const uint32_t i = blockIdx.x * (uint32_t)kMeshBlock + threadIdx.x;
  if (i >= m.n) return;
  const uint32_t hf = half[i];
  if (hf >= n_halves) return Flag(status);
  const uint32_t s = seg_of[hf];
  if (s == kNone) return;                         // the other half is the owner
  const uint32_t h = head_of[hf];
  const uint32_t j = ContourOf(m, i);
  if (s >= n_segments || h >= m.n || j == kNone) return Flag(status);
  const uint32_t kk = m.key[i];
  const bool is_last = last_of[hf] == i && (m.sides[h] & 7u) >= 3u;
  if (i != h && !(kk & ~kKeyMask) && !is_last) return;
  const uint32_t r = RankInHalf(m, i, h, j, hf);
  const uint32_t f = sfirst[s], c = scount[s];
  const uint32_t p = (kk & kKeyMask) >> 2;
  const int sd = (int)(kk & 3u);
  const int x = (int)(p % (uint32_t)m.W) + (sd == 1 || sd == 2 ? 1 : 0), y = (int)(p / (uint32_t)m.W) + (sd >= 2 ? 1 : 0);
  if (i == h || (kk & ~kKeyMask)) {
    if (r >= c || f + r >= capacity) return Flag(status);
    vertices[f + r] = make_int2(x, y);
    vseg[f + r] = s;
  }
  if (is_last) {
    if (r + 1u >= c || f + r + 1u >= capacity) return Flag(status);
    vertices[f + r + 1u] = make_int2(x + Dx(sd), y + Dy(sd));
    vseg[f + r + 1u] = s;
  }
}

__global__ __launch_bounds__(kMeshBlock) void k_mesh_records(MeshView m, const unsigned long long* __restrict__ skeys,
                                                             uint32_t n_segments, uint32_t n_halves,
                                                             const uint32_t* __restrict__ half,
                                                             const uint32_t* __restrict__ last_of,
                                                             const uint32_t* __restrict__ scount,
                                                             const uint32_t* __restrict__ sfirst,
                                                             int32_t* __restrict__ segments,
                                                             MeshStatus* __restrict__ status) {
  const uint32_t s = blockIdx.x * (uint32_t)kMeshBlock + threadIdx.x;
  if (s >= n_segments) return;
  int32_t* out = segments + (size_t)s * kMeshSegmentWords;
  const uint32_t h = (uint32_t)skeys[s];
  int32_t right = -1, left = -1, closed = 0, start_sides = 0, end_sides = 0;
  bool ok = false;
  if (h < m.n) {
    const uint32_t j = ContourOf(m, h);
    const uint32_t hf = half[h];
    if (j != kNone && hf < n_halves) {
      right = m.records[(size_t)j * kLevelContourWords + 2];
      ok = true;
      const uint32_t t = Twin(m, h);
      if (t != kNone) {
        const uint32_t jt = ContourOf(m, t);
        if (jt == kNone) ok = false;
        else left = m.records[(size_t)jt * kLevelContourWords + 2];
      }
      closed = (m.sides[h] & 7u) < 3u ? 1 : 0;
      if (!closed) {
        const uint32_t e = last_of[hf];
        const uint32_t nx = e < m.n ? m.succ[e] : kNone;
        if (nx < m.n) {
          start_sides = (int32_t)(m.sides[h] & 7u);
          end_sides = (int32_t)(m.sides[nx] & 7u);
        } else {
          ok = false;
        }
      }
    }
  }
  if (!ok) Flag(status);
  out[0] = right;
  out[1] = left;
  out[2] = (int32_t)sfirst[s];
  out[3] = (int32_t)scount[s];
  out[4] = 0;
  out[5] = closed;
  out[6] = start_sides;
  out[7] = end_sides;
  if (s == n_segments - 1) status->vertices = sfirst[s] + scount[s];
}

// Thread t: ref t when t is a half, loop t when t is a contour.
__global__ __launch_bounds__(kMeshBlock) void k_mesh_links(MeshView m, uint32_t n_segments, uint32_t n_halves,
                                                           const uint32_t* __restrict__ half,
                                                           const uint32_t* __restrict__ head_of,
                                                           const uint32_t* __restrict__ seg_of,
                                                           int32_t* __restrict__ refs, int32_t* __restrict__ loops,
                                                           MeshStatus* __restrict__ status) {
  const uint32_t t = blockIdx.x * (uint32_t)kMeshBlock + threadIdx.x;
  if (t < n_halves) {
    uint32_t s = seg_of[t];
    int32_t ref = 0;
    if (s != kNone) {
      ref = (int32_t)s;
    } else {
      const uint32_t h = head_of[t];
      const uint32_t tw = h < m.n ? Twin(m, h) : kNone;
      const uint32_t th = tw != kNone ? half[tw] : kNone;
      s = th < n_halves ? seg_of[th] : kNone;
      ref = ~(int32_t)s;
    }
    if (s >= n_segments) {
      Flag(status);
      ref = 0;
    }
    refs[t] = ref;
  }
  if (t < m.contours) {
    int32_t* out = loops + (size_t)t * kMeshLoopWords;
    out[0] = m.records[(size_t)t * kLevelContourWords + 2];
    out[1] = (int32_t)m.first_ref[t];
    out[2] = (int32_t)m.nrefs[t];
    out[3] = m.records[(size_t)t * kLevelContourWords + 5];
  }
}

// One thread per vertex slot; the first status->vertices are vertices.
__global__ __launch_bounds__(kMeshBlock) void k_mesh_measure(const int2* __restrict__ vertices,
                                                             const uint32_t* __restrict__ vseg,
                                                             uint32_t n_segments, uint32_t capacity,
                                                             int32_t* __restrict__ segments,
                                                             MeshStatus* __restrict__ status) {
  const uint32_t v = blockIdx.x * (uint32_t)kMeshBlock + threadIdx.x;
  const int lane = threadIdx.x & 63;
  uint32_t s = kNone;
  int32_t length = 0;
  if (v < min(status->vertices, capacity)) {
    s = vseg[v];
    if (s < n_segments) {
      const int32_t* rec = segments + (size_t)s * kMeshSegmentWords;
      const uint32_t f = (uint32_t)rec[2], c = (uint32_t)rec[3];
      const uint32_t k = v - f;
      if (v >= f && k < c && f + c <= capacity) {
        if (k + 1u < c || rec[5]) {
          const int2 a = vertices[v], b = vertices[k + 1u == c ? f : v + 1u];
          length = abs(b.x - a.x) + abs(b.y - a.y);
        }
      } else {
        s = kNone;
      }
    } else {
      s = kNone;
    }
    if (s == kNone) Flag(status);
  }
  // the vertices of a segment are consecutive: lane l gathers [l, l + 2d) of its own segment
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t os = __shfl_down(s, d);
    const int32_t o_len = __shfl_down(length, d);
    if (lane + d < 64 && os == s) length += o_len;
  }
  const uint32_t before = __shfl_up(s, 1);
  if (s != kNone && (lane == 0 || before != s) && length) atomicAdd(&segments[(size_t)s * kMeshSegmentWords + 4], length);
}

__global__ __launch_bounds__(kMeshBlock) void k_mesh_finish(const int32_t* __restrict__ segments, uint32_t n_segments,
                                                            MeshStatus* __restrict__ status) {
  const uint32_t s = blockIdx.x * (uint32_t)kMeshBlock + threadIdx.x;
  uint32_t length = 0;
  bool closed = false, shared = false;
  if (s < n_segments) {
    const int32_t* rec = segments + (size_t)s * kMeshSegmentWords;
    length = (uint32_t)rec[4];
    closed = rec[5] != 0;
    shared = rec[1] >= 0;
  }
  const uint32_t n_closed = (uint32_t)__popcll(__ballot(closed)), n_shared = (uint32_t)__popcll(__ballot(shared));
  length = WaveMax(length);
  if ((threadIdx.x & 63) == 0) {
    if (n_closed) atomicAdd(&status->closed, n_closed);
    if (n_shared) atomicAdd(&status->shared, n_shared);
    if (length) atomicMax(&status->longest, length);
  }
}

inline dim3 GridOf(uint32_t n) { return dim3((std::max(n, 1u) + kMeshBlock - 1) / kMeshBlock); }

MeshView ViewOf(const MeshInput& in) {
  MeshView m;
  m.plane = in.plane;
  m.W = in.width;
  m.H = in.height;
  m.mask = in.mask;
  m.offset = in.offset;
  m.n = in.n;
  m.key = in.key;
  m.succ = in.succ;
  m.leader = in.leader;
  m.place = in.place;
  m.ranked = in.ranked;
  m.contours = in.contours;
  m.count = in.count;
  m.records = in.records;
  m.sides = nullptr;
  m.heads = nullptr;
  m.nrefs = nullptr;
  m.first_ref = nullptr;
  return m;
}

}  // namespace

hipError_t MeshSplit(void* temp, size_t temp_bytes, const MeshInput& in, const unsigned long long* ckeys_sorted,
                     int rounds, MeshCrackSpace* wp, MeshStatus* status, hipStream_t stream) {
  MeshCrackSpace& w = *wp;
  MeshView m = ViewOf(in);
  const uint32_t n = in.n;
  hipError_t e = hipMemsetAsync(w.hasj, 0, (size_t)in.contours * sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_mesh_junctions, GridOf(n), dim3(kMeshBlock), 0, stream, m, w.sides, w.hasj, status);
  hipLaunchKernelGGL(k_mesh_seed, GridOf(n), dim3(kMeshBlock), 0, stream, m, w.hasj, w.sides, w.state_a, status);
  m.sides = w.sides;
  w.heads = m.heads = LaunchContourSums(w.state_a, w.state_b, n, rounds, stream);
  hipLaunchKernelGGL(k_mesh_loop_counts, GridOf(in.contours), dim3(kMeshBlock), 0, stream, m, ckeys_sorted, w.nrefs,
                     status);
  e = ExclusiveSumU32(temp, temp_bytes, w.nrefs, w.first_ref, (int)in.contours, stream);
  if (e != hipSuccess) return e;
  m.nrefs = w.nrefs;
  m.first_ref = w.first_ref;
  // head_of and last_of lie next to each other: a half that nobody entered stays out of range
  e = hipMemsetAsync(w.head_of, 0xff, (size_t)n * 2 * sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_mesh_halves, GridOf(n), dim3(kMeshBlock), 0, stream, m, w.half, w.head_of, w.head_of + n,
                     w.skeys, status);
  return hipGetLastError();
}

hipError_t MeshTables(void* temp, size_t temp_bytes, const MeshInput& in, const MeshCrackSpace& w,
                      const MeshSegmentSpace& t, uint32_t n_segments, uint32_t n_halves, int end_bit,
                      MeshStatus* status, hipStream_t stream) {
  MeshView m = ViewOf(in);
  m.sides = w.sides;
  m.heads = w.heads;
  m.nrefs = w.nrefs;
  m.first_ref = w.first_ref;
  const uint32_t n = in.n;
  const uint32_t* last_of = w.head_of + n;
  hipError_t e = hipMemsetAsync(w.seg_of, 0xff, (size_t)n_halves * sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  e = SortKeysU64(temp, temp_bytes, w.skeys, t.skeys_sorted, (int64_t)n_segments, end_bit, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_mesh_seg_heads, GridOf(n_segments), dim3(kMeshBlock), 0, stream, m, t.skeys_sorted, n_segments,
                     n_halves, w.half, last_of, w.seg_of, t.scount, status);
  e = ExclusiveSumU32(temp, temp_bytes, t.scount, t.sfirst, (int)n_segments, stream);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(t.vseg, 0xff, (size_t)t.vertex_slots * sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_mesh_vertices, GridOf(n), dim3(kMeshBlock), 0, stream, m, n_segments, n_halves, w.half, w.head_of,
                     last_of, w.seg_of, t.scount, t.sfirst, t.vertex_slots, reinterpret_cast<int2*>(t.vertices), t.vseg,
                     status);
  hipLaunchKernelGGL(k_mesh_records, GridOf(n_segments), dim3(kMeshBlock), 0, stream, m, t.skeys_sorted, n_segments,
                     n_halves, w.half, last_of, t.scount, t.sfirst, t.segments, status);
  hipLaunchKernelGGL(k_mesh_links, GridOf(std::max(n_halves, in.contours)), dim3(kMeshBlock), 0, stream, m, n_segments,
                     n_halves, w.half, w.head_of, w.seg_of, t.refs, t.loops, status);
  hipLaunchKernelGGL(k_mesh_measure, GridOf(t.vertex_slots), dim3(kMeshBlock), 0, stream,
                     reinterpret_cast<const int2*>(t.vertices), t.vseg, n_segments, t.vertex_slots, t.segments, status);
  hipLaunchKernelGGL(k_mesh_finish, GridOf(n_segments), dim3(kMeshBlock), 0, stream, t.segments, n_segments, status);
  return hipGetLastError();
}

}  // namespace vsg_render_impl
