// render_device.h -- device helpers the render kernels share (gfx950, 64 lanes a wavefront).  Included by the
// .hip files only.
#ifndef VSG_RENDER_RENDER_DEVICE_H_
#define VSG_RENDER_RENDER_DEVICE_H_

#include <cstdint>

#include <hip/hip_runtime.h>

namespace vsg_render_impl {

// P at frame position (x, y) of the H x W plane (row pitch W); -1 outside the frame.
__device__ __forceinline__ int32_t PlaneAt(const int32_t* __restrict__ plane, int W, int H, int x, int y) {
  return (x >= 0 && x < W && y >= 0 && y < H) ? plane[(size_t)y * W + x] : -1;
}

// Direction of travel along side s of a pixel (a "crack"): top +x, right +y, bottom -x, left -y.  The pixel
// across side s lies at Dx(s + 3), Dy(s + 3).
__device__ __forceinline__ int Dx(int s) { return (s & 3) == 0 ? 1 : (s & 3) == 2 ? -1 : 0; }
__device__ __forceinline__ int Dy(int s) { return (s & 3) == 1 ? 1 : (s & 3) == 3 ? -1 : 0; }

// The xor butterfly over the 64 lanes, from 32 down to 1: every lane gets the result.  A float or double sum
// adds in exactly this order.
template <class T>
__device__ __forceinline__ T WaveSum(T v) {
  for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
  return v;
}
template <class T>
__device__ __forceinline__ T WaveMax(T v) {
  for (int s = 32; s > 0; s >>= 1) v = max(v, (T)__shfl_xor(v, s));
  return v;
}
template <class T>
__device__ __forceinline__ T WaveMin(T v) {
  for (int s = 32; s > 0; s >>= 1) v = min(v, (T)__shfl_xor(v, s));
  return v;
}

// One add to *counter per block reserves a slot for every item of its kWaves wavefronts.  in_wave: the items of
// this thread's wavefront, as the caller's ballots count them.  Returns the block's items; when there are any,
// *s_base is the block's first slot and *before the items of the wavefronts before this one.  Every thread of
// the block calls; s_wave (kWaves words) and s_base are the block's LDS.
template <int kWaves>
__device__ __forceinline__ uint32_t BlockReserve(uint32_t in_wave, uint32_t* s_wave, uint32_t* s_base,
                                                 uint32_t* counter, uint32_t* before) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (lane == 0) s_wave[wave] = in_wave;
  __syncthreads();
  uint32_t total = 0;
  *before = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    if (w < wave) *before += s_wave[w];
    total += s_wave[w];
  }
  if (t == 0 && total) *s_base = atomicAdd(counter, total);
  __syncthreads();
  return total;
}

}  // namespace vsg_render_impl

#endif  // VSG_RENDER_RENDER_DEVICE_H_
