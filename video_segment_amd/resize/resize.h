// resize.h -- what libvsg_resize.so is made of, as the C ABI layer (resize_capi.cpp) uses it: the
// host-side filter tables and the two kernels of resize.hip.  tests/resize_model.py defines the
// arithmetic; the tables are built in f64 in the model's order of operations and the kernels
// perform their f32 operations in the model's order (the library is built with -ffp-contract=off).
#ifndef VSG_RESIZE_IMPL_H_
#define VSG_RESIZE_IMPL_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

namespace vsg_resize_impl {

// k_resize_h: a workgroup of H_THREADS threads takes H_ROWS input rows and a tile of output columns
// and keeps the tile's source bytes of each row in LDS; H_LDS_BUDGET bounds that block.
enum { H_THREADS = 256, H_ROWS = 4, H_TILE_COLS = 64, H_LDS_BUDGET = 32 * 1024 };
// k_resize_v: a thread produces 4 consecutive bytes of one output row.
enum { V_THREADS = 128 };

// The filter of one axis (vsg_resize_filter).  weights is n_out x max_taps, zero beyond a row's count.
struct Filter {
  int n_in = 0, n_out = 0, max_taps = 0;
  std::vector<int32_t> first, count;
  std::vector<float> weights;
};

// Keys cubic, a = -0.6, t >= 0.
inline double Keys(double t) {
  const double a = -0.6;
  if (t <= 1.0) return ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0;
  if (t < 2.0) return ((a * t - 5.0 * a) * t + 8.0 * a) * t - 4.0 * a;
  return 0.0;
}

// first / count of every output and the widest row; with fill, the normalised weights too.
inline void BuildFilter(int n_in, int n_out, bool fill, Filter* f) {
  f->n_in = n_in;
  f->n_out = n_out;
  f->first.assign((size_t)n_out, 0);
  f->count.assign((size_t)n_out, 0);
  const double r = (double)n_in / (double)n_out;
  const double s = std::max(1.0, r);
  const double R = 2.0 * s;
  int max_taps = 0;
  for (int o = 0; o < n_out; ++o) {
    const double c = ((double)o + 0.5) * r - 0.5;
    const int lo = (int)std::ceil(c - R), hi = (int)std::floor(c + R);
    f->first[(size_t)o] = lo;
    f->count[(size_t)o] = hi - lo + 1;
    max_taps = std::max(max_taps, hi - lo + 1);
  }
  f->max_taps = max_taps;
  f->weights.clear();
  if (!fill) return;
  f->weights.assign((size_t)n_out * max_taps, 0.0f);
  std::vector<double> w((size_t)max_taps);
  for (int o = 0; o < n_out; ++o) {
    const double c = ((double)o + 0.5) * r - 0.5;
    const int lo = f->first[(size_t)o], n = f->count[(size_t)o];
    double total = 0.0;
    for (int j = 0; j < n; ++j) {
      w[(size_t)j] = Keys(std::fabs(((double)(lo + j) - c) / s));
      total = total + w[(size_t)j];
    }
    for (int j = 0; j < n; ++j) f->weights[(size_t)o * max_taps + j] = (float)(w[(size_t)j] / total);
  }
}

// Source byte span [*b0, *b1) of one row that the output columns [o0, o1) read, as k_resize_h
// stages it: clamped at the row ends and, on the dword path, starting at a multiple of 4.
__host__ __device__ inline void TileSpan(const int32_t* first, const int32_t* count, int o0, int o1, int in_w,
                                         bool aligned, int* b0, int* b1) {
  int lo = first[o0], hi = first[o1 - 1] + count[o1 - 1] - 1;
  lo = lo < 0 ? 0 : (lo > in_w - 1 ? in_w - 1 : lo);
  hi = hi < 0 ? 0 : (hi > in_w - 1 ? in_w - 1 : hi);
  *b0 = aligned ? (lo * 3) & ~3 : lo * 3;
  *b1 = (hi + 1) * 3;
}

// BGR24 rows -> f32 intermediate of in_h rows of `pitch` floats (out_w * 3 used).  weights_t is the
// horizontal filter's weights transposed to max_taps x out_w.  span_stride: bytes of LDS per row, a
// multiple of 4 that holds the widest tile's span.
void LaunchResizeH(const uint8_t* in, size_t stride, int in_w, int in_h, int out_w, const int32_t* first,
                   const int32_t* count, const float* weights_t, int tile_cols, int span_stride, float* inter,
                   int pitch, hipStream_t s);
// Intermediate -> BGR24 rows of stride_out bytes; only out_w * 3 bytes of a row are written.
void LaunchResizeV(const float* inter, int pitch, int in_h, int out_w, int out_h, const int32_t* first,
                   const int32_t* count, const float* weights, int max_taps, uint8_t* out, size_t stride_out,
                   hipStream_t s);

}  // namespace vsg_resize_impl

#endif  // VSG_RESIZE_IMPL_H_
