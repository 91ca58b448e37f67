// vector.hip -- polygon scan conversion of a whole frame's vectorizations (gfx950): the device form
// of the reference's RasterVectorization (segment_util/segmentation_util.cpp:1103-1236).
//
//   k_vec_walk    one thread per polygon line: its crossing with every row it is active in
//   radix sort    crossings brought together by (region index, row), 64-bit key
//   k_vec_pairs   one thread per crossing: its rank in its row under the reference's comparator,
//                 then its half of the scan interval it belongs to
//
// The arithmetic is the reference's, operation for operation: curr_x advances by one rounded f32
// addition per row, the removal test compares y_max with the int y + 1 converted to float, the
// comparator uses eps = 1e-3f, the interval ends are ceil(x - 1e-6f) and floor(x) with the
// exclusive-right rule.  The file is compiled with -ffp-contract=off.
#include "render.h"
#include "render_device.h"

namespace vsg_render_impl {

namespace {

constexpr int kVecBlock = 256;
constexpr float kEps = 1e-3f;     // EdgeEntry::operator<, segmentation_util.cpp:1116
constexpr float kTiny = 1e-6f;    // :1217, :1222

// Writes crossing k of line i at offset + k: the key (region index, row) and the value (curr_x, line).
// The row count was computed on the host with the same test; the loop is bounded by it, so a thread
// never writes outside [offset, offset + count) whatever the floats say.
__global__ __launch_bounds__(kVecBlock) void k_vec_walk(const VecLine* __restrict__ lines, int n_lines,
                                                        unsigned long long* __restrict__ keys,
                                                        unsigned long long* __restrict__ vals,
                                                        VecStatus* __restrict__ status) {
  const int i = blockIdx.x * kVecBlock + threadIdx.x;
  if (i >= n_lines) return;
  const VecLine l = lines[i];
  const unsigned long long hi = (unsigned long long)(uint32_t)l.region << kVecRowBits;
  float x = l.x;
  int y = l.y0;
  uint32_t k = 0;
  // active while !(y_max < y + 1), segmentation_util.cpp:1206; a line inserted and removed in the
  // same row (count 0) writes nothing
  for (; k < l.count && !(l.y_max < (float)(y + 1)); ++k, ++y) {
    keys[(size_t)l.offset + k] = hi | (unsigned long long)(uint32_t)y;
    vals[(size_t)l.offset + k] = (unsigned long long)__float_as_uint(x) << 32 | (uint32_t)i;
    x = __fadd_rn(x, l.dx);   // EdgeEntry::Advance, :1113
  }
  if (k != l.count || !(l.y_max < (float)(y + 1))) atomicOr(&status->flags, (uint32_t)VEC_FLAG_INTERNAL);
}

// EdgeEntry::operator< (segmentation_util.cpp:1115-1135): is a before b?
__device__ __forceinline__ bool EdgeLess(float ax, bool aleft, float adx, float bx, bool bleft, float bdx) {
  if (ax < __fsub_rn(bx, kEps)) return true;
  if (ax > __fadd_rn(bx, kEps)) return false;
  if (aleft && !bleft) return true;
  if (bleft && !aleft) return false;
  return adx < bdx;
}

// One thread per sorted crossing.  A group is a run of equal keys: the active edges of one region
// in one row.  The thread finds its group, counts the members that come before it (its rank; with a
// strict weak order and no two members the comparator cannot tell apart, the ranks are the sorted
// positions), and writes its half of interval (group start) / 2 + rank / 2: rank even is the left
// end, rank odd the right end.  Groups of any size take this path: a row of a comb-shaped region
// with hundreds of crossings is spread over as many threads, each of which reads the group once.
//
// Rows the reference does not define raise VEC_FLAG_UNSPECIFIED:
//   - the comparator is no strict weak order on the group: a pair whose eps tests disagree after
//     rounding; members m, a, b with a ~ m ~ b within eps but a, b apart; two members with equal
//     side and dx within eps of each other whose x differ;
//   - the group is odd;
//   - an end outside the row: left_x outside [0, W], right_x outside [-1, W - 1].
// An end outside the row is written clamped, and the list was cleared before this kernel, so
// k_render_fill stays inside the plane even on a call that is going to fail.
__global__ __launch_bounds__(kVecBlock) void k_vec_pairs(const unsigned long long* __restrict__ keys,
                                                         const unsigned long long* __restrict__ vals,
                                                         const VecLine* __restrict__ lines, uint32_t n_lines,
                                                         const uint32_t* __restrict__ region_value,
                                                         uint32_t n_regions, int64_t n, int W, int H,
                                                         int4* __restrict__ intervals,
                                                         VecStatus* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * kVecBlock + threadIdx.x;
  const bool live = i < n;
  bool head = false, bad = false, broken = false;
  int64_t size = 0;
  if (live) {
    const unsigned long long key = keys[i];
    int64_t gs = i, ge = i + 1;
    while (gs > 0 && keys[gs - 1] == key) --gs;
    while (ge < n && keys[ge] == key) ++ge;
    size = ge - gs;
    head = gs == i;
    if (head && (size & 1)) bad = true;

    const unsigned long long mine = vals[i];
    const float x = __uint_as_float((uint32_t)(mine >> 32));
    // k_vec_walk wrote every crossing, so every line, region and row read back here is in range;
    // should one not be, nothing outside the arrays or the frame is touched and the call fails
    uint32_t my_line = (uint32_t)mine, region = (uint32_t)(key >> kVecRowBits);
    int row = (int)(uint32_t)(key & ((1u << kVecRowBits) - 1));
    if (my_line >= n_lines || region >= n_regions || row >= H) {
      broken = true;
      my_line = 0;
      region = 0;
      row = 0;
    }
    const VecLine ml = lines[my_line];
    const bool left = ml.is_left != 0;
    const float dx = ml.dx;

    int64_t rank = 0;
    float eq_min = x, eq_max = x;   // extent of the members within eps of this one
    for (int64_t j = gs; j < ge; ++j) {
      if (j == i) continue;
      const unsigned long long v = vals[j];
      const float xj = __uint_as_float((uint32_t)(v >> 32));
      uint32_t line_j = (uint32_t)v;
      if (line_j >= n_lines) {
        broken = true;
        line_j = 0;
      }
      const VecLine lj = lines[line_j];
      const bool leftj = lj.is_left != 0;
      const float lo = fminf(x, xj), hi = fmaxf(x, xj);
      const bool lt = lo < __fsub_rn(hi, kEps), gt = hi > __fadd_rn(lo, kEps);
      if (lt != gt) bad = true;
      if (!lt && !gt) {
        eq_min = fminf(eq_min, xj);
        eq_max = fmaxf(eq_max, xj);
        if (leftj == left && lj.dx == dx && xj != x) bad = true;
      }
      const bool before = EdgeLess(xj, leftj, lj.dx, x, left, dx);
      const bool after = EdgeLess(x, left, dx, xj, leftj, lj.dx);
      // members the comparator cannot tell apart are identical here (else `bad`): index order
      if (before || (!after && j < i)) ++rank;
    }
    if (eq_min < __fsub_rn(eq_max, kEps) || eq_max > __fadd_rn(eq_min, kEps)) bad = true;

    int4* out = intervals + (gs >> 1) + (rank >> 1);
    if (!(rank & 1)) {
      const float lf = ceilf(__fsub_rn(x, kTiny));   // :1217
      int lx = 0;
      if (lf >= 0.0f && lf <= (float)W) lx = (int)lf;
      else bad = true;
      out->x = row;
      out->y = lx;
      out->w = (int)region_value[region];
    } else {
      const float rf = floorf(x);                    // :1219
      int rx = -1;
      if (rf >= -1.0f && rf <= (float)W) {
        rx = (int)rf;
        if (fabsf(__fsub_rn(x, (float)rx)) < kTiny) --rx;   // :1222, the right border is exclusive
        if (rx < -1 || rx > W - 1) {
          rx = -1;
          bad = true;
        }
      } else {
        bad = true;
      }
      out->z = rx;
    }
  }
  // statistics and the flag: one atomic of each kind per wavefront
  const unsigned long long heads = __ballot(head);
  long long largest = head ? (long long)size : 0;
  largest = WaveMax(largest);
  const bool any_bad = __ballot(bad) != 0, any_broken = __ballot(broken) != 0;
  if ((threadIdx.x & 63) == 0) {
    if (heads) atomicAdd(&status->groups, (unsigned long long)__popcll(heads));
    if (largest) atomicMax(&status->largest_group, (unsigned long long)largest);
    if (any_bad) atomicOr(&status->flags, (uint32_t)VEC_FLAG_UNSPECIFIED);
    if (any_broken) atomicOr(&status->flags, (uint32_t)VEC_FLAG_INTERNAL);
  }
}

}  // namespace

void LaunchVecWalk(const VecLine* lines, int n_lines, unsigned long long* keys, unsigned long long* vals,
                   VecStatus* status, hipStream_t stream) {
  if (n_lines <= 0) return;
  hipLaunchKernelGGL(k_vec_walk, dim3((n_lines + kVecBlock - 1) / kVecBlock), dim3(kVecBlock), 0, stream, lines,
                     n_lines, keys, vals, status);
}

void LaunchVecPairs(const unsigned long long* keys, const unsigned long long* vals, const VecLine* lines,
                    uint32_t n_lines, const uint32_t* region_value, uint32_t n_regions, int64_t n, int width,
                    int height, Interval* intervals, VecStatus* status, hipStream_t stream) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_vec_pairs, dim3((unsigned)((n + kVecBlock - 1) / kVecBlock)), dim3(kVecBlock), 0, stream, keys,
                     vals, lines, n_lines, region_value, n_regions, n, width, height,
                     reinterpret_cast<int4*>(intervals), status);
}

}  // namespace vsg_render_impl
