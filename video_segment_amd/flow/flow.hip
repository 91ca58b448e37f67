// flow.hip -- the kernels of libvsg_flow.so: luminance, pyrDown, gradient, the fused bicubic warp,
// the inner TV-L1 iteration, upsampling and the export of the result.  tests/flow_model.py defines
// every operation and its order; this file restates it one f32 operation at a time (the build uses
// -ffp-contract=off, and sqrtf and / are the correctly rounded ones).
#include "flow.h"

namespace vsg_flow_impl {
namespace {

constexpr int kThreads = 256;

inline int Blocks(int64_t n) { return (int)((n + kThreads - 1) / kThreads); }

__global__ __launch_bounds__(kThreads) void k_luminance_bgr(const uint8_t* __restrict__ bgr, size_t stride, int W,
                                                            int H, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (int64_t)W * H) return;
  const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
  const uint8_t* p = bgr + (size_t)y * stride + (size_t)x * 3;
  const int v = (1868 * (int)p[0] + 9617 * (int)p[1] + 4899 * (int)p[2] + 8192) >> 14;
  out[i] = (float)v;
}

__global__ __launch_bounds__(kThreads) void k_luminance_u8(const uint8_t* __restrict__ lum, size_t stride, int W,
                                                           int H, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (int64_t)W * H) return;
  const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
  out[i] = (float)lum[(size_t)y * stride + x];
}

__device__ __forceinline__ int Reflect101(int i, int n) {
  if (i < 0) i = -i;
  if (i >= n) i = 2 * n - 2 - i;
  return i;
}

// Sources have both sides >= 16 (a level below that is never built), so one reflection suffices.
__global__ __launch_bounds__(kThreads) void k_pyr_down(const float* __restrict__ src, int W, int H,
                                                       float* __restrict__ dst, int w2, int h2) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= w2 * h2) return;
  const int y = i / w2, x = i - y * w2;
  int xs[5];
  for (int k = 0; k < 5; ++k) xs[k] = Reflect101(2 * x + k - 2, W);
  float row[5];
  for (int k = 0; k < 5; ++k) {
    const float* s = src + (size_t)Reflect101(2 * y + k - 2, H) * W;
    row[k] = s[xs[2]] * 6.0f + (s[xs[1]] + s[xs[3]]) * 4.0f + s[xs[0]] + s[xs[4]];
  }
  dst[i] = (row[2] * 6.0f + (row[1] + row[3]) * 4.0f + row[0] + row[4]) * (1.0f / 256.0f);
}

__global__ __launch_bounds__(kThreads) void k_gradient(const float* __restrict__ I, int W, int H,
                                                       float* __restrict__ Ix, float* __restrict__ Iy) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= W * H) return;
  const int y = i / W, x = i - y * W;
  const int xp = min(x + 1, W - 1), xm = max(x - 1, 0), yp = min(y + 1, H - 1), ym = max(y - 1, 0);
  Ix[i] = 0.5f * (I[(size_t)y * W + xp] - I[(size_t)y * W + xm]);
  Iy[i] = 0.5f * (I[(size_t)yp * W + x] - I[(size_t)ym * W + x]);
}

__device__ __forceinline__ void CubicWeights(float t, float w[4]) {
  const float A = -0.75f;
  const float t1 = t + 1.0f;
  w[0] = ((A * t1 + 3.75f) * t1 - 6.0f) * t1 + 3.0f;
  w[1] = ((1.25f * t - 2.25f) * t) * t + 1.0f;
  const float s = 1.0f - t;
  w[2] = ((1.25f * s - 2.25f) * s) * s + 1.0f;
  w[3] = ((1.0f - w[0]) - w[1]) - w[2];
}

// Three bicubic gathers (I1, I1x, I1y) at (x + u1, y + u2) with shared addresses and weights, then
// grad and rho_c.  Every tap is bounds-checked, so no value of u can make it read outside a plane.
__global__ __launch_bounds__(kThreads) void k_warp(const float* __restrict__ I0, const float* __restrict__ I1,
                                                   const float* __restrict__ I1x, const float* __restrict__ I1y,
                                                   const float2* __restrict__ Ua, const float2* __restrict__ Ub,
                                                   const int* __restrict__ state, int W, int H,
                                                   float4* __restrict__ g) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= W * H) return;
  const int y = i / W, x = i - y * W;
  const float2 u = (state[ST_CUR] ? Ub : Ua)[i];
  const float fx = (float)x + u.x, fy = (float)y + u.y;
  const float fxf = floorf(fx), fyf = floorf(fy);
  float wx[4], wy[4];
  CubicWeights(fx - fxf, wx);
  CubicWeights(fy - fyf, wy);
  const int ix = (int)fminf(fmaxf(fxf, -4.0f), (float)(W + 4));
  const int iy = (int)fminf(fmaxf(fyf, -4.0f), (float)(H + 4));
  float rows[3][4];
  for (int r = 0; r < 4; ++r) {
    const int yy = iy + r - 1;
    const bool yok = yy >= 0 && yy < H;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (int c = 0; c < 4; ++c) {
      const int xx = ix + c - 1;
      const bool ok = yok && xx >= 0 && xx < W;
      const size_t a = ok ? (size_t)yy * W + xx : 0;
      const float v0 = (ok ? I1[a] : 0.0f) * wx[c];
      const float v1 = (ok ? I1x[a] : 0.0f) * wx[c];
      const float v2 = (ok ? I1y[a] : 0.0f) * wx[c];
      if (c == 0) {
        acc[0] = v0; acc[1] = v1; acc[2] = v2;
      } else {
        acc[0] = acc[0] + v0; acc[1] = acc[1] + v1; acc[2] = acc[2] + v2;
      }
    }
    for (int k = 0; k < 3; ++k) rows[k][r] = acc[k];
  }
  float val[3];
  for (int k = 0; k < 3; ++k) {
    val[k] = ((rows[k][0] * wy[0] + rows[k][1] * wy[1]) + rows[k][2] * wy[2]) + rows[k][3] * wy[3];
  }
  const float I1w = val[0], I1wx = val[1], I1wy = val[2];
  const float grad = I1wx * I1wx + I1wy * I1wy;
  const float rho_c = ((I1w - I1wx * u.x) - I1wy * u.y) - I0[i];
  g[i] = make_float4(I1wx, I1wy, grad, rho_c);
}

// u(n) of one pixel from u(n-1) and p(n-1): thresholding step, backward-difference divergence,
// u = v + theta * div p.  Returns the pixel's own old u and p as well.
__device__ __forceinline__ float2 UNew(int x, int y, int W, const float4* __restrict__ g,
                                       const float2* __restrict__ U, const float2* __restrict__ Px,
                                       const float2* __restrict__ Py, Params prm, float2* u_old, float2* px_old,
                                       float2* py_old) {
  const size_t i = (size_t)y * W + x;
  const float4 gi = g[i];   // I1wx, I1wy, grad, rho_c
  const float2 u = U[i], px = Px[i], py = Py[i];
  const float2 left = x > 0 ? Px[i - 1] : make_float2(0.0f, 0.0f);
  const float2 up = y > 0 ? Py[i - W] : make_float2(0.0f, 0.0f);
  const float rho = gi.w + (gi.x * u.x + gi.y * u.y);
  float d1 = 0.0f, d2 = 0.0f;
  if (rho < (-prm.l_t) * gi.z) {
    d1 = prm.l_t * gi.x;
    d2 = prm.l_t * gi.y;
  } else if (rho > prm.l_t * gi.z) {
    d1 = (-prm.l_t) * gi.x;
    d2 = (-prm.l_t) * gi.y;
  } else if (gi.z > 1.1920929e-07f) {
    const float fi = (-rho) / gi.z;
    d1 = fi * gi.x;
    d2 = fi * gi.y;
  }
  const float v1 = u.x + d1, v2 = u.y + d2;
  const float div1 = (px.x - left.x) + (py.x - up.x);
  const float div2 = (px.y - left.y) + (py.y - up.y);
  *u_old = u;
  *px_old = px;
  *py_old = py;
  return make_float2(v1 + prm.theta * div1, v2 + prm.theta * div2);
}

// One inner iteration.  A workgroup computes u(n) for its tile and the one-pixel apron to the right
// and below into LDS, then p(n) for its tile from the forward differences of u(n).  Both u and p
// are double-buffered in global memory (neighbouring workgroups read the old values).  Px = (p11,
// p21), Py = (p12, p22): the left neighbour is needed of Px only, the upper one of Py only.
// The per-pixel error terms are summed in f64: a fixed tree per workgroup, then the workgroup that
// delivers last adds the partial sums in index order, so the sum does not depend on scheduling.
__global__ __launch_bounds__(ITER_TX* ITER_TY) void k_iterate(const float4* __restrict__ g, float2* Ua, float2* Ub,
                                                              float2* Pxa, float2* Pxb, float2* Pya, float2* Pyb,
                                                              int* state, int slot, double* partials, int W, int H,
                                                              Params prm, double threshold) {
  if (state[ST_STOP + slot]) return;   // uniform over the grid: written by the previous launch only
  const int cur = state[ST_CUR];
  const float2* __restrict__ U = cur ? Ub : Ua;
  const float2* __restrict__ Px = cur ? Pxb : Pxa;
  const float2* __restrict__ Py = cur ? Pyb : Pya;
  float2* __restrict__ Un = cur ? Ua : Ub;
  float2* __restrict__ Pxn = cur ? Pxa : Pxb;
  float2* __restrict__ Pyn = cur ? Pya : Pyb;

  __shared__ float2 su[ITER_TY + 1][ITER_TX + 1];
  __shared__ double sred[ITER_TX * ITER_TY];
  __shared__ int s_last;
  const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * ITER_TX + tx;
  const int x0 = blockIdx.x * ITER_TX, y0 = blockIdx.y * ITER_TY;
  const int x = x0 + tx, y = y0 + ty;
  const bool inside = x < W && y < H;
  float2 u_old, px = make_float2(0.0f, 0.0f), py = make_float2(0.0f, 0.0f);
  double e = 0.0;
  if (inside) {
    const float2 un = UNew(x, y, W, g, U, Px, Py, prm, &u_old, &px, &py);
    su[ty][tx] = un;
    Un[(size_t)y * W + x] = un;
    const float e1 = un.x - u_old.x, e2 = un.y - u_old.y;
    e = (double)(e1 * e1 + e2 * e2);
  }
  if (tid < ITER_TX + ITER_TY + 1) {   // apron: row below, column to the right, corner
    int lx, ly;
    if (tid < ITER_TX) {
      lx = tid;
      ly = ITER_TY;
    } else {
      lx = ITER_TX;
      ly = tid - ITER_TX;
    }
    const int ax = x0 + lx, ay = y0 + ly;
    if (ax < W && ay < H) {
      float2 a, b, c;
      su[ly][lx] = UNew(ax, ay, W, g, U, Px, Py, prm, &a, &b, &c);
    }
  }
  __syncthreads();
  if (inside) {
    const float2 u = su[ty][tx];
    float u1x = 0.0f, u2x = 0.0f, u1y = 0.0f, u2y = 0.0f;
    if (x + 1 < W) {
      const float2 r = su[ty][tx + 1];
      u1x = r.x - u.x;
      u2x = r.y - u.y;
    }
    if (y + 1 < H) {
      const float2 d = su[ty + 1][tx];
      u1y = d.x - u.x;
      u2y = d.y - u.y;
    }
    const float ng1 = 1.0f + prm.taut * sqrtf(u1x * u1x + u1y * u1y);
    const float ng2 = 1.0f + prm.taut * sqrtf(u2x * u2x + u2y * u2y);
    const size_t i = (size_t)y * W + x;
    Pxn[i] = make_float2((px.x + prm.taut * u1x) / ng1, (px.y + prm.taut * u2x) / ng2);
    Pyn[i] = make_float2((py.x + prm.taut * u1y) / ng1, (py.y + prm.taut * u2y) / ng2);
  }

  // ---- error: fixed tree in the workgroup ----
  sred[tid] = e;
  __syncthreads();
  for (int s = ITER_TX * ITER_TY / 2; s > 0; s >>= 1) {
    if (tid < s) sred[tid] = sred[tid] + sred[tid + s];
    __syncthreads();
  }
  const unsigned nblocks = gridDim.x * gridDim.y;
  const unsigned bid = blockIdx.y * gridDim.x + blockIdx.x;
  unsigned long long* pbits = reinterpret_cast<unsigned long long*>(partials);
  if (tid == 0) {
    __hip_atomic_store(&pbits[bid], (unsigned long long)__double_as_longlong(sred[0]), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    // release our partial sum, acquire everybody else's
    const unsigned prev = __hip_atomic_fetch_add(reinterpret_cast<unsigned*>(&state[ST_COUNTER]), 1u,
                                                 __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    s_last = prev == nblocks - 1;
  }
  __syncthreads();
  if (!s_last) return;
  // ---- last workgroup: ordered pass over the partial sums ----
  double acc = 0.0;
  for (unsigned k = tid; k < nblocks; k += ITER_TX * ITER_TY) {
    acc = acc + __longlong_as_double((long long)__hip_atomic_load(&pbits[k], __ATOMIC_RELAXED,
                                                                  __HIP_MEMORY_SCOPE_AGENT));
  }
  sred[tid] = acc;
  __syncthreads();
  for (int s = ITER_TX * ITER_TY / 2; s > 0; s >>= 1) {
    if (tid < s) sred[tid] = sred[tid] + sred[tid + s];
    __syncthreads();
  }
  if (tid == 0) {
    const double error = sred[0];
    state[ST_CUR] = cur ^ 1;
    state[ST_ITERS] = state[ST_ITERS] + 1;
    state[ST_COUNTER] = 0;
    if (!(error > threshold)) state[ST_STOP + slot] = 1;
  }
}

__device__ __forceinline__ void UpsampleAxis(int d, int n_dst, int n_src, int* i0, int* i1, float* t) {
  const float f = ((float)d + 0.5f) * ((float)n_src / (float)n_dst) - 0.5f;
  const float ff = floorf(f);
  const int i = (int)ff;
  *i0 = min(max(i, 0), n_src - 1);
  *i1 = min(max(i + 1, 0), n_src - 1);
  *t = f - ff;
}

__global__ __launch_bounds__(kThreads) void k_upsample(float2* Ua, float2* Ub, const int* __restrict__ state, int w,
                                                       int h, int W, int H) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= W * H) return;
  const int cur = state[ST_CUR];
  const float2* __restrict__ src = cur ? Ub : Ua;
  float2* __restrict__ dst = cur ? Ua : Ub;
  const int y = i / W, x = i - y * W;
  int xa, xb, ya, yb;
  float tx, ty;
  UpsampleAxis(x, W, w, &xa, &xb, &tx);
  UpsampleAxis(y, H, h, &ya, &yb, &ty);
  const float2 a = src[(size_t)ya * w + xa], b = src[(size_t)ya * w + xb];
  const float2 c = src[(size_t)yb * w + xa], d = src[(size_t)yb * w + xb];
  const float top1 = a.x * (1.0f - tx) + b.x * tx, bot1 = c.x * (1.0f - tx) + d.x * tx;
  const float top2 = a.y * (1.0f - tx) + b.y * tx, bot2 = c.y * (1.0f - tx) + d.y * tx;
  dst[i] = make_float2((top1 * (1.0f - ty) + bot1 * ty) * 2.0f, (top2 * (1.0f - ty) + bot2 * ty) * 2.0f);
}

__global__ void k_flip(int* state) { state[ST_CUR] = state[ST_CUR] ^ 1; }

__global__ __launch_bounds__(kThreads) void k_export(const float2* __restrict__ Ua, const float2* __restrict__ Ub,
                                                     const int* __restrict__ state, int64_t n,
                                                     float2* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) out[i] = (state[ST_CUR] ? Ub : Ua)[i];
}

}  // namespace

void LaunchLuminanceBgr(const uint8_t* bgr, size_t stride, int W, int H, float* out, hipStream_t s) {
  hipLaunchKernelGGL(k_luminance_bgr, dim3(Blocks((int64_t)W * H)), dim3(kThreads), 0, s, bgr, stride, W, H, out);
}

void LaunchLuminanceU8(const uint8_t* lum, size_t stride, int W, int H, float* out, hipStream_t s) {
  hipLaunchKernelGGL(k_luminance_u8, dim3(Blocks((int64_t)W * H)), dim3(kThreads), 0, s, lum, stride, W, H, out);
}

void LaunchPyrDown(const float* src, int W, int H, float* dst, hipStream_t s) {
  const int w2 = (W + 1) / 2, h2 = (H + 1) / 2;
  hipLaunchKernelGGL(k_pyr_down, dim3(Blocks((int64_t)w2 * h2)), dim3(kThreads), 0, s, src, W, H, dst, w2, h2);
}

void LaunchGradient(const float* I, int W, int H, float* Ix, float* Iy, hipStream_t s) {
  hipLaunchKernelGGL(k_gradient, dim3(Blocks((int64_t)W * H)), dim3(kThreads), 0, s, I, W, H, Ix, Iy);
}

void LaunchWarp(const float* I0, const float* I1, const float* I1x, const float* I1y, const float2* Ua,
                const float2* Ub, const int* state, int W, int H, float4* g, hipStream_t s) {
  hipLaunchKernelGGL(k_warp, dim3(Blocks((int64_t)W * H)), dim3(kThreads), 0, s, I0, I1, I1x, I1y, Ua, Ub, state, W,
                     H, g);
}

void LaunchIterate(const float4* g, float2* Ua, float2* Ub, float2* Pxa, float2* Pxb, float2* Pya, float2* Pyb,
                   int* state, int slot, double* partials, int W, int H, Params prm, double threshold,
                   hipStream_t s) {
  const dim3 grid((W + ITER_TX - 1) / ITER_TX, (H + ITER_TY - 1) / ITER_TY);
  hipLaunchKernelGGL(k_iterate, grid, dim3(ITER_TX, ITER_TY), 0, s, g, Ua, Ub, Pxa, Pxb, Pya, Pyb, state, slot,
                     partials, W, H, prm, threshold);
}

void LaunchUpsample(float2* Ua, float2* Ub, const int* state, int w, int h, int W, int H, hipStream_t s) {
  hipLaunchKernelGGL(k_upsample, dim3(Blocks((int64_t)W * H)), dim3(kThreads), 0, s, Ua, Ub, state, w, h, W, H);
}

void LaunchFlip(int* state, hipStream_t s) { hipLaunchKernelGGL(k_flip, dim3(1), dim3(1), 0, s, state); }

void LaunchExport(const float2* Ua, const float2* Ub, const int* state, int64_t n, float2* out, hipStream_t s) {
  hipLaunchKernelGGL(k_export, dim3(Blocks(n)), dim3(kThreads), 0, s, Ua, Ub, state, n, out);
}

}  // namespace vsg_flow_impl
