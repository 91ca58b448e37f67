// flow.h -- kernels of libvsg_flow.so (flow.hip) as the C ABI layer (flow_capi.cpp) launches them.
// tests/flow_model.py defines the arithmetic; every kernel performs its f32 operations in the
// model's order (the library is built with -ffp-contract=off).
#ifndef VSG_FLOW_IMPL_H_
#define VSG_FLOW_IMPL_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vsg_flow_impl {

// Device-side state of one calc(I0, I1): ints, cleared by one memset before the calc.
//   [ST_CUR]     which of the two u / p buffer sets holds the current values
//   [ST_ITERS]   inner iterations that did work
//   [ST_COUNTER] blocks of the running iteration that have delivered their partial sum
//   [ST_STOP+k]  1 once the stop test of (scale, warp) slot k has fired
enum { ST_CUR = 0, ST_ITERS = 1, ST_COUNTER = 2, ST_STOP = 4 };

// The iteration kernel's tile: one thread per pixel, ITER_TX x ITER_TY threads.
enum { ITER_TX = 32, ITER_TY = 8 };

inline int IterBlocks(int W, int H) { return ((W + ITER_TX - 1) / ITER_TX) * ((H + ITER_TY - 1) / ITER_TY); }

struct Params {
  float theta, l_t, taut;
};

void LaunchLuminanceBgr(const uint8_t* bgr, size_t stride, int W, int H, float* out, hipStream_t s);
void LaunchLuminanceU8(const uint8_t* lum, size_t stride, int W, int H, float* out, hipStream_t s);
void LaunchPyrDown(const float* src, int W, int H, float* dst, hipStream_t s);
void LaunchGradient(const float* I, int W, int H, float* Ix, float* Iy, hipStream_t s);
// g = (I1wx, I1wy, grad, rho_c) per pixel, from u = U[state[ST_CUR]].
void LaunchWarp(const float* I0, const float* I1, const float* I1x, const float* I1y, const float2* Ua,
                const float2* Ub, const int* state, int W, int H, float4* g, hipStream_t s);
// One inner iteration of slot `slot`: reads set state[ST_CUR], writes the other, and its last block
// sums `partials` (IterBlocks doubles) in index order, flips ST_CUR, counts the iteration and sets
// the slot's stop flag unless error > threshold.  Returns at once when the flag is already set.
void LaunchIterate(const float4* g, float2* Ua, float2* Ub, float2* Pxa, float2* Pxb, float2* Pya, float2* Pyb,
                   int* state, int slot, double* partials, int W, int H, Params prm, double threshold,
                   hipStream_t s);
// U[cur ^ 1] (W x H) = 2 * bilinear(U[cur] (w x h)); LaunchFlip then makes it the current set.
void LaunchUpsample(float2* Ua, float2* Ub, const int* state, int w, int h, int W, int H, hipStream_t s);
void LaunchFlip(int* state, hipStream_t s);
void LaunchExport(const float2* Ua, const float2* Ub, const int* state, int64_t n, float2* out, hipStream_t s);

}  // namespace vsg_flow_impl

#endif  // VSG_FLOW_IMPL_H_
