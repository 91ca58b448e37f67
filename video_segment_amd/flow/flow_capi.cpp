// flow_capi.cpp -- extern "C" entry points declared in include/vsg_flow.h: the handle with its
// device blocks (all sized at creation), the two luminance pyramids that swap roles from frame to
// frame, and the launch sequence of OpticalFlowDual_TVL1::calc around the kernels of flow.hip.
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/vsg_flow.h"
#include "flow.h"
#include "../common/capi_support.h"

namespace {

using namespace vsg_flow_impl;

const int kScales = 5;          // nscales
const float kTau = 0.25f, kLambda = 0.15f, kTheta = 0.3f;

enum Stage { STAGE_PYRAMID = 0, STAGE_WARP, STAGE_ITERATE, STAGE_EXPORT, STAGE_COUNT };

struct Level {
  int W, H;
  size_t offset;   // in floats, into a pyramid block
};

}  // namespace

struct vsg_flow {
  vsg_flow_options opt;
  int device = 0, W = 0, H = 0;
  size_t N = 0;                 // W * H
  std::vector<Level> levels;    // finest first
  hipStream_t stream = nullptr;
  StageClock clock;
  // device blocks, all allocated by vsg_flow_create
  Block d_in;                     // a host frame's bytes, packed
  Block d_pyr[2];
  Block d_ix, d_iy, d_g, d_u, d_p, d_out, d_partials;
  Block d_state;                  // two calcs' states
  Block h_state;                  // pinned
  int state_ints = 0;
  int cur_pyr = 0;                // which pyramid the incoming frame is written to
  bool have_prev = false;
  int64_t allocations = 0;
  vsg_flow_stats stats;

  ~vsg_flow() {
    if (!stream) return;
    (void)hipStreamSynchronize(stream);
    (void)hipStreamDestroy(stream);
  }

  // OpticalFlowDual_TVL1::calc(I0, I1) on the two pyramids; the result is U[state[ST_CUR]].
  void Calc(const float* pyr0, const float* pyr1, int* state) {
    const int warps = opt.warps, iterations = opt.iterations;
    Params prm;
    prm.theta = kTheta;
    prm.l_t = kLambda * kTheta;
    prm.taut = kTau / kTheta;
    float2 *Ua = d_u.As<float2>(), *Ub = Ua + N;
    float *ix = d_ix.As<float>(), *iy = d_iy.As<float>();
    float4* g = d_g.As<float4>();
    float2* p = d_p.As<float2>();
    VSG_HIP(hipMemsetAsync(state, 0, (size_t)state_ints * sizeof(int), stream));
    int s = (int)levels.size() - 1;
    VSG_HIP(hipMemsetAsync(Ua, 0, (size_t)levels[s].W * levels[s].H * sizeof(float2), stream));
    stats.launches += 2;
    for (;;) {
      const Level& L = levels[s];
      const size_t n = (size_t)L.W * L.H;
      const float *I0 = pyr0 + L.offset, *I1 = pyr1 + L.offset;
      float2 *Pxa = p, *Pxb = p + n, *Pya = p + 2 * n, *Pyb = p + 3 * n;
      VSG_HIP(hipMemsetAsync(p, 0, 4 * n * sizeof(float2), stream));
      LaunchGradient(I1, L.W, L.H, ix, iy, stream);
      stats.launches += 2;
      const double threshold = 0.01 * 0.01 * (double)n;
      for (int w = 0; w < warps; ++w) {
        LaunchWarp(I0, I1, ix, iy, Ua, Ub, state, L.W, L.H, g, stream);
        clock.Mark(STAGE_WARP);
        const int slot = s * warps + w;
        for (int k = 0; k < iterations; ++k) {
          LaunchIterate(g, Ua, Ub, Pxa, Pxb, Pya, Pyb, state, slot, d_partials.As<double>(), L.W, L.H, prm, threshold,
                        stream);
        }
        clock.Mark(STAGE_ITERATE);
        stats.launches += 1 + iterations;
      }
      if (s == 0) break;
      --s;
      LaunchUpsample(Ua, Ub, state, L.W, L.H, levels[s].W, levels[s].H, stream);
      LaunchFlip(state, stream);
      stats.launches += 2;
    }
    VSG_HIP(hipGetLastError());
  }
};

namespace {

void Process(vsg_flow* h, const uint8_t* in, size_t stride, int mem_in, int channels, float* backward_out,
             float* forward_out, int mem_out, int* has_flow) {
  if (!h) Throw(VSG_ERR_INVALID, "handle is null");
  if (!in) Throw(VSG_ERR_INVALID, "frame is null");
  if (!has_flow) Throw(VSG_ERR_INVALID, "has_flow is null");
  CheckMem(mem_in, "frame");
  CheckMem(mem_out, "flow");
  const int W = h->W, H = h->H;
  const size_t row_bytes = (size_t)W * channels;
  if (stride < row_bytes) Throw(VSG_ERR_INVALID, "stride is smaller than a row of the frame");
  const bool want_b = h->opt.flow_type != VSG_FLOW_FORWARD, want_f = h->opt.flow_type != VSG_FLOW_BACKWARD;
  if (h->have_prev && want_b && !backward_out) Throw(VSG_ERR_INVALID, "backward_out is null");
  if (h->have_prev && want_f && !forward_out) Throw(VSG_ERR_INVALID, "forward_out is null");
  DeviceGuard guard(h->device);
  std::memset(&h->stats, 0, sizeof(h->stats));
  h->stats.scales = (int)h->levels.size();
  hipStream_t st = h->stream;

  // ---- frame to the device, luminance, pyramid ----
  h->clock.Begin(st);
  const uint8_t* src = in;
  size_t src_stride = stride;
  if (mem_in == VSG_MEM_HOST) {
    VSG_HIP(hipMemcpy2DAsync(h->d_in.p, row_bytes, in, stride, row_bytes, H, hipMemcpyHostToDevice, st));
    ++h->stats.launches;
    src = h->d_in.As<uint8_t>();
    src_stride = row_bytes;
  }
  float* pyr = h->d_pyr[h->cur_pyr].As<float>();
  if (channels == 3) LaunchLuminanceBgr(src, src_stride, W, H, pyr, st);
  else LaunchLuminanceU8(src, src_stride, W, H, pyr, st);
  ++h->stats.launches;
  for (size_t s = 1; s < h->levels.size(); ++s) {
    LaunchPyrDown(pyr + h->levels[s - 1].offset, h->levels[s - 1].W, h->levels[s - 1].H, pyr + h->levels[s].offset, st);
    ++h->stats.launches;
  }
  VSG_HIP(hipGetLastError());
  h->clock.Mark(STAGE_PYRAMID);

  // ---- flow ----
  const bool flow = h->have_prev;
  if (flow) {
    const float *cur = pyr, *prev = h->d_pyr[h->cur_pyr ^ 1].As<float>();
    float2* u = h->d_u.As<float2>();
    int *d_state = h->d_state.As<int>(), *h_state = h->h_state.As<int>();
    int calc = 0;
    for (int dir = 0; dir < 2; ++dir) {   // 0: backward = calc(current, previous); 1: forward
      if (dir == 0 ? !want_b : !want_f) continue;
      int* state = d_state + (size_t)calc * h->state_ints;
      h->Calc(dir == 0 ? cur : prev, dir == 0 ? prev : cur, state);
      float* out = dir == 0 ? backward_out : forward_out;
      float2* dst = mem_out == VSG_MEM_DEVICE ? reinterpret_cast<float2*>(out)
                                              : h->d_out.As<float2>() + (size_t)calc * h->N;
      LaunchExport(u, u + h->N, state, (int64_t)h->N, dst, st);
      VSG_HIP(hipGetLastError());
      ++h->stats.launches;
      if (mem_out == VSG_MEM_HOST) {
        VSG_HIP(hipMemcpyAsync(out, dst, h->N * sizeof(float2), hipMemcpyDeviceToHost, st));
        ++h->stats.launches;
      }
      h->clock.Mark(STAGE_EXPORT);
      ++calc;
    }
    VSG_HIP(hipMemcpyAsync(h_state, d_state, (size_t)calc * h->state_ints * sizeof(int),
                           hipMemcpyDeviceToHost, st));
    ++h->stats.launches;
    VSG_HIP(hipStreamSynchronize(st));
    for (int c = 0; c < calc; ++c) h->stats.iterations_run += h_state[(size_t)c * h->state_ints + ST_ITERS];
  } else {
    VSG_HIP(hipStreamSynchronize(st));
  }
  h->stats.host_syncs = 1;
  float us[STAGE_COUNT];
  h->clock.Read(us, STAGE_COUNT);
  h->stats.pyramid_us = us[STAGE_PYRAMID];
  h->stats.warp_us = us[STAGE_WARP];
  h->stats.iterate_us = us[STAGE_ITERATE];
  h->stats.export_us = us[STAGE_EXPORT];
  h->stats.device_allocations = h->allocations;
  h->cur_pyr ^= 1;
  h->have_prev = true;
  *has_flow = flow ? 1 : 0;
}

}  // namespace

extern "C" {

const char* vsg_flow_last_error(void) { return g_last_error.c_str(); }

void vsg_flow_default_options(vsg_flow_options* o) {
  if (!o) return;
  o->flow_type = VSG_FLOW_BACKWARD;
  o->iterations = 10;
  o->warps = 2;
  o->device = -1;
}

int vsg_flow_luminance(const uint8_t* bgr, size_t stride, int width, int height, uint8_t* out) {
  return Guard([&] {
    if (!bgr || !out) Throw(VSG_ERR_INVALID, "null argument");
    if (width <= 0 || height <= 0 || stride < (size_t)width * 3) Throw(VSG_ERR_INVALID, "bad frame size or stride");
    for (int y = 0; y < height; ++y) {
      const uint8_t* p = bgr + (size_t)y * stride;
      for (int x = 0; x < width; ++x, p += 3) {
        out[(size_t)y * width + x] = (uint8_t)((1868 * p[0] + 9617 * p[1] + 4899 * p[2] + 8192) >> 14);
      }
    }
  });
}

int vsg_flow_create(const vsg_flow_options* o, int width, int height, vsg_flow** out) {
  return Guard([&] {
    if (!out) Throw(VSG_ERR_INVALID, "handle pointer is null");
    *out = nullptr;
    vsg_flow_options opt;
    vsg_flow_default_options(&opt);
    if (o) opt = *o;
    // the kernels index a plane with an int
    if (width <= 0 || height <= 0 || width > (1 << 14) || height > (1 << 14)) Throw(VSG_ERR_INVALID, "bad frame size");
    if (opt.flow_type < VSG_FLOW_BACKWARD || opt.flow_type > VSG_FLOW_BOTH) Throw(VSG_ERR_INVALID, "bad flow_type");
    if (opt.iterations < 1 || opt.iterations > 1000) Throw(VSG_ERR_INVALID, "iterations has to be in [1, 1000]");
    if (opt.warps < 1 || opt.warps > 64) Throw(VSG_ERR_INVALID, "warps has to be in [1, 64]");
    std::unique_ptr<vsg_flow> h(new vsg_flow);
    h->device = SelectDevice(opt.device, "libvsg_flow");
    h->opt = opt;
    h->W = width;
    h->H = height;
    h->N = (size_t)width * height;
    std::memset(&h->stats, 0, sizeof(h->stats));
    // the pyramid stops before the first level with a side below 16
    size_t total = 0;
    for (int w = width, ht = height; (int)h->levels.size() < kScales; w = (w + 1) / 2, ht = (ht + 1) / 2) {
      if (!h->levels.empty() && (w < 16 || ht < 16)) break;
      h->levels.push_back(Level{w, ht, total});
      total += (size_t)w * ht;
    }
    DeviceGuard guard(h->device);
    VSG_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    const int calcs = opt.flow_type == VSG_FLOW_BOTH ? 2 : 1;
    h->clock.Create((size_t)2 + calcs * (kScales * 2 * opt.warps + 1));
    h->state_ints = ST_STOP + kScales * opt.warps;
    const size_t N = h->N;
    h->h_state.pinned = true;
    const size_t state_bytes = (size_t)2 * h->state_ints * sizeof(int);
    const struct { Block* block; size_t bytes; } blocks[] = {
        {&h->d_in, N * 3},
        {&h->d_pyr[0], total * sizeof(float)},
        {&h->d_pyr[1], total * sizeof(float)},
        {&h->d_ix, N * sizeof(float)},
        {&h->d_iy, N * sizeof(float)},
        {&h->d_g, N * sizeof(float4)},
        {&h->d_u, 2 * N * sizeof(float2)},
        {&h->d_p, 4 * N * sizeof(float2)},
        {&h->d_out, (size_t)calcs * N * sizeof(float2)},
        {&h->d_partials, (size_t)IterBlocks(width, height) * sizeof(double)},
        {&h->d_state, state_bytes},
        {&h->h_state, state_bytes},
    };
    for (const auto& b : blocks) b.block->Reserve(b.bytes, &h->allocations);
    *out = h.release();
  });
}

void vsg_flow_destroy(vsg_flow* h) { DestroyOnDevice(h); }

int vsg_flow_process_frame(vsg_flow* h, const uint8_t* bgr, size_t stride, int mem_in, float* backward_out,
                           float* forward_out, int mem_out, int* has_flow) {
  return Guard([&] { Process(h, bgr, stride, mem_in, 3, backward_out, forward_out, mem_out, has_flow); });
}

int vsg_flow_process_luminance(vsg_flow* h, const uint8_t* lum, size_t stride, int mem_in, float* backward_out,
                               float* forward_out, int mem_out, int* has_flow) {
  return Guard([&] { Process(h, lum, stride, mem_in, 1, backward_out, forward_out, mem_out, has_flow); });
}

int vsg_flow_restart(vsg_flow* h) {
  return Guard([&] {
    if (!h) Throw(VSG_ERR_INVALID, "handle is null");
    h->have_prev = false;
  });
}

int vsg_flow_last_stats(vsg_flow* h, vsg_flow_stats* s) {
  return Guard([&] {
    if (!h || !s) Throw(VSG_ERR_INVALID, "null argument");
    *s = h->stats;
  });
}

}  // extern "C"
