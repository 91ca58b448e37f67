// render.hip -- the two kernels of libvsg_render.so (gfx950).
//
//   k_render_fill     scan intervals -> one uint32 per pixel (packed colour, or region id)
//   k_render_compose  that plane + source frame -> BGR24 rows: edge rule, blend, concatenation
//
// Both are bound by memory: a frame costs one plane clear and two launches whatever the number of
// regions and intervals (DESIGN.md section 8 has the byte counts and the measured rates).
#include "render.h"

namespace vsg_render_impl {

namespace {

constexpr int kFillBlock = 256;      // 4 wavefronts, 64 intervals each per step
constexpr int kLongInterval = 16;    // from this length on the whole wavefront paints one interval

// A wavefront takes 64 intervals, one per lane.  Intervals of kLongInterval pixels and more are
// painted one after the other by all 64 lanes (one dword per lane, 256 contiguous bytes per store
// instruction, which is the full-rate store shape on this chip); the short ones are painted by
// their own lane.  Short intervals of different regions lie in different rows, so their stores
// cannot be coalesced whatever the lane assignment; a frame made of them is bound by the number of
// partial-line writes, not by bytes.
__global__ __launch_bounds__(kFillBlock) void k_render_fill(const int4* __restrict__ intervals, int n,
                                                            uint32_t* __restrict__ plane, int pitch) {
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * kFillBlock + threadIdx.x) >> 6;
  const int waves = gridDim.x * (kFillBlock / 64);
  for (long long base = (long long)wave * 64; base < n; base += (long long)waves * 64) {
    const long long i = base + lane;
    // x = y, y = left_x, z = right_x, w = value; padding lanes hold an empty interval
    const int4 v = i < n ? intervals[i] : make_int4(0, 0, -1, 0);
    const int len = v.z - v.y + 1;
    unsigned long long todo = __ballot(len >= kLongInterval);
    while (todo) {   // wave-uniform: `todo` is a scalar
      const int j = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int y = __builtin_amdgcn_readlane(v.x, j);
      const int lx = __builtin_amdgcn_readlane(v.y, j);
      const int l = __builtin_amdgcn_readlane(len, j);
      const uint32_t value = (uint32_t)__builtin_amdgcn_readlane(v.w, j);
      uint32_t* row = plane + (size_t)y * pitch + lx;
      for (int k = lane; k < l; k += 64) row[k] = value;
    }
    if (len > 0 && len < kLongInterval) {
      uint32_t* row = plane + (size_t)v.x * pitch + v.y;
      for (int k = 0; k < len; ++k) row[k] = (uint32_t)v.w;
    }
  }
}

// cv::addWeighted on 8-bit data as DESIGN.md section 8 states it: two f32 products, one f32 sum, each
// rounded on its own (no fused multiply-add), round half to even, saturated.
__device__ __forceinline__ uint32_t Blend(uint32_t s, uint32_t r, float a, float b) {
  const float t = __fadd_rn(__fmul_rn((float)s, a), __fmul_rn((float)r, b));
  return (uint32_t)fminf(fmaxf(rintf(t), 0.0f), 255.0f);
}

struct alignas(4) Bytes12 {
  uint32_t w[3];
};

constexpr int kPxPerThread = 4;     // 12 output bytes: three dwords per row
constexpr int kRowsPerThread = 4;   // the row below a thread's last row is read once per 4 rows

// One thread decides 4 x 4 pixels.  It reads the colours of its pixels, of the column to their
// right and of the row below (clamped to the last row, so that the last row finds no difference
// below), applies the edge rule and writes 12 bytes per row.
//
// The reference's highlight loop (segmentation_render.h:159-182) works in place, yet every
// comparison it makes reads the pixel itself (not yet overwritten: it is the one being decided),
// its right neighbour (decided later in the same row) and the pixel below (decided in a later
// row).  No comparison reads a value the loop has already blackened, so every pixel is a function
// of the filled plane alone and all of them can be decided independently, as here.
//
// ALIGNED: src, out and both strides are multiples of 4, rows are then moved as dwords.
template <bool ALIGNED>
__global__ __launch_bounds__(256) void k_render_compose(const uint32_t* __restrict__ plane, int pitch, int W,
                                                        int H, const uint8_t* __restrict__ src,
                                                        size_t src_stride, uint8_t* __restrict__ out,
                                                        size_t out_stride, int highlight_edges, int mode,
                                                        float a, float b) {
  const int x0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * kPxPerThread;
  const int y0 = (blockIdx.y * 4 + (threadIdx.x >> 6)) * kRowsPerThread;
  if (x0 >= W || y0 >= H) return;
  const bool full = x0 + kPxPerThread <= W;
  const int npx = full ? kPxPerThread : W - x0;

  // PlanePitch keeps both loads inside the row; columns >= W hold the clear value and are masked
  const uint32_t* p = plane + (size_t)y0 * pitch + x0;
  uint4 cur = *reinterpret_cast<const uint4*>(p);
  uint32_t cur_right = p[4];
#pragma unroll
  for (int ry = 0; ry < kRowsPerThread; ++ry) {
    const int y = y0 + ry;
    if (y >= H) break;
    const int yb = min(y + 1, H - 1);
    const uint32_t* pb = plane + (size_t)yb * pitch + x0;
    const uint4 below = *reinterpret_cast<const uint4*>(pb);
    const uint32_t below_right = pb[4];

    const uint32_t c[5] = {cur.x & 0xffffffu, cur.y & 0xffffffu, cur.z & 0xffffffu, cur.w & 0xffffffu,
                           cur_right & 0xffffffu};
    const uint32_t d[4] = {below.x & 0xffffffu, below.y & 0xffffffu, below.z & 0xffffffu,
                           below.w & 0xffffffu};
    uint32_t r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool edge = (x0 + k + 1 < W && c[k] != c[k + 1]) || c[k] != d[k];
      r[k] = (highlight_edges && edge) ? 0u : c[k];
    }

    uint8_t* o = out + (size_t)y * out_stride + (size_t)x0 * 3;
    const uint8_t* s = mode != COMPOSE_RENDER ? src + (size_t)y * src_stride + (size_t)x0 * 3 : nullptr;
    uint8_t* o2 = out + (size_t)(y + H) * out_stride + (size_t)x0 * 3;   // COMPOSE_CONCAT only
    if (ALIGNED && full) {
      Bytes12 sv = {{0u, 0u, 0u}};
      if (mode != COMPOSE_RENDER) sv = *reinterpret_cast<const Bytes12*>(s);
      Bytes12 ov;
      if (mode == COMPOSE_BLEND) {
        uint32_t byte[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) {
          const uint32_t sb = (sv.w[k >> 2] >> (8 * (k & 3))) & 0xffu;
          const uint32_t rb = (r[k / 3] >> (8 * (k % 3))) & 0xffu;
          byte[k] = Blend(sb, rb, a, b);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          ov.w[k] = byte[4 * k] | byte[4 * k + 1] << 8 | byte[4 * k + 2] << 16 | byte[4 * k + 3] << 24;
        }
      } else {
        ov.w[0] = r[0] | r[1] << 24;
        ov.w[1] = r[1] >> 8 | r[2] << 16;
        ov.w[2] = r[2] >> 16 | r[3] << 8;
      }
      *reinterpret_cast<Bytes12*>(o) = ov;
      if (mode == COMPOSE_CONCAT) *reinterpret_cast<Bytes12*>(o2) = sv;
    } else {
      for (int k = 0; k < npx * 3; ++k) {
        const uint32_t rb = (r[k / 3] >> (8 * (k % 3))) & 0xffu;
        if (mode == COMPOSE_BLEND) {
          o[k] = (uint8_t)Blend(s[k], rb, a, b);
        } else {
          o[k] = (uint8_t)rb;
          if (mode == COMPOSE_CONCAT) o2[k] = s[k];
        }
      }
    }
    cur = below;
    cur_right = below_right;
  }
}

}  // namespace

void LaunchFill(const Interval* intervals, int64_t n, uint32_t* plane, int pitch, hipStream_t stream) {
  if (n <= 0) return;
  // memory-bound: enough blocks to fill the chip, the rest grid-strides
  const int64_t groups = (n + kFillBlock - 1) / kFillBlock;
  const int grid = (int)(groups < 2048 ? groups : 2048);
  hipLaunchKernelGGL(k_render_fill, dim3(grid), dim3(kFillBlock), 0, stream,
                     reinterpret_cast<const int4*>(intervals), (int)n, plane, pitch);
}

void LaunchCompose(const uint32_t* plane, int pitch, int width, int height, const uint8_t* src,
                   size_t src_stride, uint8_t* out, size_t out_stride, int highlight_edges, int mode,
                   float alpha, hipStream_t stream) {
  const float a = 1.0f - alpha, b = alpha;
  const int gx = ((width + kPxPerThread - 1) / kPxPerThread + 63) / 64;
  const int gy = ((height + kRowsPerThread - 1) / kRowsPerThread + 3) / 4;
  const bool aligned = ((uintptr_t)out % 4 == 0) && out_stride % 4 == 0 &&
                       (mode == COMPOSE_RENDER || (((uintptr_t)src % 4 == 0) && src_stride % 4 == 0));
  if (aligned) {
    hipLaunchKernelGGL(k_render_compose<true>, dim3(gx, gy), dim3(256), 0, stream, plane, pitch, width,
                       height, src, src_stride, out, out_stride, highlight_edges, mode, a, b);
  } else {
    hipLaunchKernelGGL(k_render_compose<false>, dim3(gx, gy), dim3(256), 0, stream, plane, pitch, width,
                       height, src, src_stride, out, out_stride, highlight_edges, mode, a, b);
  }
}

}  // namespace vsg_render_impl
