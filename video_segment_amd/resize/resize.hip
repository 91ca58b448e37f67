// resize.hip -- the two kernels of libvsg_resize.so: k_resize_h (BGR24 rows -> f32 intermediate) and
// k_resize_v (intermediate -> BGR24).  Each output value is acc = 0; acc = fadd(acc, fmul(w, v)) over
// its taps in index order, as tests/resize_model.py has it; __fmul_rn / __fadd_rn keep the two
// operations apart whatever the contraction mode.  Loop bounds and gather indices come from the
// host's tables (resize.h: BuildFilter) and every index is clamped to the frame before it is used.
#include "resize.h"

namespace vsg_resize_impl {

namespace {

__device__ inline int ClampI(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// One workgroup: input rows [blockIdx.y * H_ROWS, +H_ROWS) x output columns [blockIdx.x * tile_cols,
// +tile_cols).  The source bytes the tile reads are one contiguous span per row (the tables are
// monotonic); it is staged in LDS with dword loads where the frame's base and stride are multiples
// of 4 (ALIGNED), bytewise otherwise.  A dword load never passes the row's last pixel: the rest of a
// row's span goes bytewise.  Then one (row, column, channel) per thread and pass, taps in order.
template <bool ALIGNED>
__global__ __launch_bounds__(H_THREADS) void k_resize_h(const uint8_t* __restrict__ in, size_t stride, int in_w,
                                                        int in_h, int out_w, const int32_t* __restrict__ first,
                                                        const int32_t* __restrict__ count,
                                                        const float* __restrict__ weights_t, int tile_cols,
                                                        int span_stride, float* __restrict__ inter, int pitch) {
  extern __shared__ __align__(16) uint8_t span[];
  const int tid = (int)threadIdx.x;
  const int o0 = (int)blockIdx.x * tile_cols;
  const int o1 = min(o0 + tile_cols, out_w);
  const int y0 = (int)blockIdx.y * H_ROWS;
  const int rows = min((int)H_ROWS, in_h - y0);
  if (o0 >= o1 || rows <= 0) return;
  int b0, b1;
  TileSpan(first, count, o0, o1, in_w, ALIGNED, &b0, &b1);
  if (b1 - b0 > span_stride) return;   // the host sized span_stride with the same TileSpan

  if (ALIGNED) {
    const int dw_end = b1 & ~3;               // b0 is a multiple of 4 and below b1
    const int ndw = (dw_end - b0) >> 2;
    for (int k = tid; k < rows * ndw; k += H_THREADS) {
      const int r = k / ndw, q = k - r * ndw;
      const uint8_t* src = in + (size_t)(y0 + r) * stride + b0;
      reinterpret_cast<uint32_t*>(span + (size_t)r * span_stride)[q] = reinterpret_cast<const uint32_t*>(src)[q];
    }
    const int tail = b1 - dw_end;             // 0 .. 3 bytes
    const int r = tid >> 2, q = dw_end + (tid & 3);
    if (r < rows && (tid & 3) < tail) span[(size_t)r * span_stride + (q - b0)] = in[(size_t)(y0 + r) * stride + q];
  } else {
    const int n = b1 - b0;
    for (int k = tid; k < rows * n; k += H_THREADS) {
      const int r = k / n, q = k - r * n;
      span[(size_t)r * span_stride + q] = in[(size_t)(y0 + r) * stride + b0 + q];
    }
  }
  __syncthreads();

  const int lo = b0 / 3 + (b0 % 3 ? 1 : 0);   // first whole pixel of the span
  const int hi = b1 / 3 - 1;
  const int row_items = (o1 - o0) * 3;
  for (int it = tid; it < rows * row_items; it += H_THREADS) {
    const int r = it / row_items, e = it - r * row_items;
    const int oc = e / 3, ch = e - oc * 3;
    const int o = o0 + oc;
    const int f = first[o], n = count[o];
    const uint8_t* row = span + (size_t)r * span_stride;
    float acc = 0.0f;
    for (int j = 0; j < n; ++j) {
      int p = ClampI(f + j, 0, in_w - 1);
      p = ClampI(p, lo, hi);                  // no effect: the tile's span covers its taps
      const float v = (float)row[p * 3 + ch - b0];
      acc = __fadd_rn(acc, __fmul_rn(weights_t[(size_t)j * out_w + o], v));
    }
    inter[(size_t)(y0 + r) * pitch + (size_t)o * 3 + ch] = acc;
  }
}

__device__ inline uint32_t ToByte(float v) {
  v = rintf(v);                               // half to even
  v = fminf(fmaxf(v, 0.0f), 255.0f);
  return (uint32_t)(int)v;
}

// One workgroup: V_THREADS * 4 consecutive bytes of output row blockIdx.y.  The intermediate's rows
// are `pitch` floats apart, a multiple of 4, so a thread reads one aligned float4 per tap; the
// row's weights are the same for the whole workgroup.  ALIGNED: the output's base and stride are
// multiples of 4 and whole dwords inside out_w * 3 are stored as such.
template <bool ALIGNED>
__global__ __launch_bounds__(V_THREADS) void k_resize_v(const float* __restrict__ inter, int pitch, int in_h,
                                                        int row_bytes, const int32_t* __restrict__ first,
                                                        const int32_t* __restrict__ count,
                                                        const float* __restrict__ weights, int max_taps,
                                                        uint8_t* __restrict__ out, size_t stride_out) {
  const int o = (int)blockIdx.y;
  const int e = ((int)blockIdx.x * V_THREADS + (int)threadIdx.x) * 4;
  if (e >= row_bytes) return;
  const int f = first[o], n = count[o];
  const float* w = weights + (size_t)o * max_taps;
  float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
  for (int j = 0; j < n; ++j) {
    const int i = ClampI(f + j, 0, in_h - 1);
    const float4 v = *reinterpret_cast<const float4*>(inter + (size_t)i * pitch + e);
    const float wj = w[j];
    a0 = __fadd_rn(a0, __fmul_rn(wj, v.x));
    a1 = __fadd_rn(a1, __fmul_rn(wj, v.y));
    a2 = __fadd_rn(a2, __fmul_rn(wj, v.z));
    a3 = __fadd_rn(a3, __fmul_rn(wj, v.w));
  }
  const uint32_t c0 = ToByte(a0), c1 = ToByte(a1), c2 = ToByte(a2), c3 = ToByte(a3);
  uint8_t* dst = out + (size_t)o * stride_out + e;
  if (ALIGNED && e + 4 <= row_bytes) {
    *reinterpret_cast<uint32_t*>(dst) = c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
  } else {
    dst[0] = (uint8_t)c0;                     // e < row_bytes
    if (e + 1 < row_bytes) dst[1] = (uint8_t)c1;
    if (e + 2 < row_bytes) dst[2] = (uint8_t)c2;
    if (e + 3 < row_bytes) dst[3] = (uint8_t)c3;
  }
}

}  // namespace

void LaunchResizeH(const uint8_t* in, size_t stride, int in_w, int in_h, int out_w, const int32_t* first,
                   const int32_t* count, const float* weights_t, int tile_cols, int span_stride, float* inter,
                   int pitch, hipStream_t s) {
  const dim3 grid((unsigned)((out_w + tile_cols - 1) / tile_cols), (unsigned)((in_h + H_ROWS - 1) / H_ROWS));
  const size_t lds = (size_t)H_ROWS * span_stride;
  const bool aligned = (reinterpret_cast<uintptr_t>(in) & 3) == 0 && (stride & 3) == 0;
  if (aligned) {
    hipLaunchKernelGGL(k_resize_h<true>, grid, dim3(H_THREADS), lds, s, in, stride, in_w, in_h, out_w, first, count,
                       weights_t, tile_cols, span_stride, inter, pitch);
  } else {
    hipLaunchKernelGGL(k_resize_h<false>, grid, dim3(H_THREADS), lds, s, in, stride, in_w, in_h, out_w, first, count,
                       weights_t, tile_cols, span_stride, inter, pitch);
  }
}

void LaunchResizeV(const float* inter, int pitch, int in_h, int out_w, int out_h, const int32_t* first,
                   const int32_t* count, const float* weights, int max_taps, uint8_t* out, size_t stride_out,
                   hipStream_t s) {
  const int row_bytes = out_w * 3;
  const int quads = (row_bytes + 3) / 4;
  const dim3 grid((unsigned)((quads + V_THREADS - 1) / V_THREADS), (unsigned)out_h);
  const bool aligned = (reinterpret_cast<uintptr_t>(out) & 3) == 0 && (stride_out & 3) == 0;
  if (aligned) {
    hipLaunchKernelGGL(k_resize_v<true>, grid, dim3(V_THREADS), 0, s, inter, pitch, in_h, row_bytes, first, count,
                       weights, max_taps, out, stride_out);
  } else {
    hipLaunchKernelGGL(k_resize_v<false>, grid, dim3(V_THREADS), 0, s, inter, pitch, in_h, row_bytes, first, count,
                       weights, max_taps, out, stride_out);
  }
}

}  // namespace vsg_resize_impl
