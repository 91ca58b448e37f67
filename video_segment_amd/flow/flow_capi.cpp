// flow_capi.cpp -- extern "C" entry points declared in include/vsg_flow.h: the handle with its
// device blocks (all sized at creation), the two luminance pyramids that swap roles from frame to
// frame, and the launch sequence of OpticalFlowDual_TVL1::calc around the kernels of flow.hip.
#include <algorithm>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/vsg_flow.h"
#include "flow.h"

namespace {

using namespace vsg_flow_impl;

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

[[noreturn]] void Throw(int code, const std::string& msg) { throw Error(code, msg); }

#define FLOW_HIP(call)                                                                          \
  do {                                                                                          \
    hipError_t e_ = (call);                                                                     \
    if (e_ != hipSuccess) Throw(VSG_ERR_DEVICE, std::string(hipGetErrorString(e_)) + " in " #call); \
  } while (0)

thread_local std::string g_last_error;

template <class F>
int Guard(F&& f) {
  try {
    f();
    return VSG_OK;
  } catch (const Error& e) {
    g_last_error = e.what();
    return e.code;
  } catch (const std::exception& e) {
    g_last_error = e.what();
    return VSG_ERR_INTERNAL;
  }
}

// Binds the calling thread to the handle's device for the duration of a call.
class DeviceGuard {
 public:
  explicit DeviceGuard(int device) {
    if (hipGetDevice(&prev_) != hipSuccess) return;
    if (prev_ != device) {
      FLOW_HIP(hipSetDevice(device));
      changed_ = true;
    }
  }
  ~DeviceGuard() {
    if (changed_) (void)hipSetDevice(prev_);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;

 private:
  int prev_ = -1;
  bool changed_ = false;
};

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
  std::vector<hipEvent_t> events;
  std::vector<int> event_stage;   // stage that ended at event k of the running call
  size_t events_used = 0;
  // device blocks, all allocated by vsg_flow_create
  uint8_t* d_in = nullptr;        // a host frame's bytes, packed
  float* d_pyr[2] = {nullptr, nullptr};
  float *d_ix = nullptr, *d_iy = nullptr;
  float4* d_g = nullptr;
  float2 *d_u = nullptr, *d_p = nullptr, *d_out = nullptr;
  double* d_partials = nullptr;
  int* d_state = nullptr;         // two calcs' states
  int* h_state = nullptr;         // pinned
  int state_ints = 0;
  int cur_pyr = 0;                // which pyramid the incoming frame is written to
  bool have_prev = false;
  int64_t allocations = 0;
  vsg_flow_stats stats;

  template <class T>
  void Alloc(T** p, size_t count) {
    FLOW_HIP(hipMalloc(reinterpret_cast<void**>(p), std::max<size_t>(count, 1) * sizeof(T)));
    ++allocations;
  }

  ~vsg_flow() {
    if (stream) (void)hipStreamSynchronize(stream);
    for (void* p : {(void*)d_in, (void*)d_pyr[0], (void*)d_pyr[1], (void*)d_ix, (void*)d_iy, (void*)d_g, (void*)d_u,
                    (void*)d_p, (void*)d_out, (void*)d_partials, (void*)d_state}) {
      if (p) (void)hipFree(p);
    }
    if (h_state) (void)hipHostFree(h_state);
    for (hipEvent_t e : events) {
      if (e) (void)hipEventDestroy(e);
    }
    if (stream) (void)hipStreamDestroy(stream);
  }

  void Mark(int stage) {
    if (events_used >= events.size()) Throw(VSG_ERR_INTERNAL, "event pool exhausted");
    FLOW_HIP(hipEventRecord(events[events_used], stream));
    event_stage[events_used++] = stage;
  }

  // OpticalFlowDual_TVL1::calc(I0, I1) on the two pyramids; the result is U[state[ST_CUR]].
  void Calc(const float* pyr0, const float* pyr1, int* state) {
    const int warps = opt.warps, iterations = opt.iterations;
    Params prm;
    prm.theta = kTheta;
    prm.l_t = kLambda * kTheta;
    prm.taut = kTau / kTheta;
    float2 *Ua = d_u, *Ub = d_u + N;
    FLOW_HIP(hipMemsetAsync(state, 0, (size_t)state_ints * sizeof(int), stream));
    int s = (int)levels.size() - 1;
    FLOW_HIP(hipMemsetAsync(Ua, 0, (size_t)levels[s].W * levels[s].H * sizeof(float2), stream));
    stats.launches += 2;
    for (;;) {
      const Level& L = levels[s];
      const size_t n = (size_t)L.W * L.H;
      const float *I0 = pyr0 + L.offset, *I1 = pyr1 + L.offset;
      float2 *Pxa = d_p, *Pxb = d_p + n, *Pya = d_p + 2 * n, *Pyb = d_p + 3 * n;
      FLOW_HIP(hipMemsetAsync(d_p, 0, 4 * n * sizeof(float2), stream));
      LaunchGradient(I1, L.W, L.H, d_ix, d_iy, stream);
      stats.launches += 2;
      const double threshold = 0.01 * 0.01 * (double)n;
      for (int w = 0; w < warps; ++w) {
        LaunchWarp(I0, I1, d_ix, d_iy, Ua, Ub, state, L.W, L.H, d_g, stream);
        Mark(STAGE_WARP);
        const int slot = s * warps + w;
        for (int k = 0; k < iterations; ++k) {
          LaunchIterate(d_g, Ua, Ub, Pxa, Pxb, Pya, Pyb, state, slot, d_partials, L.W, L.H, prm, threshold, stream);
        }
        Mark(STAGE_ITERATE);
        stats.launches += 1 + iterations;
      }
      if (s == 0) break;
      --s;
      LaunchUpsample(Ua, Ub, state, L.W, L.H, levels[s].W, levels[s].H, stream);
      LaunchFlip(state, stream);
      stats.launches += 2;
    }
    FLOW_HIP(hipGetLastError());
  }
};

namespace {

void CheckMem(int mem, const char* what) {
  if (mem != VSG_MEM_HOST && mem != VSG_MEM_DEVICE) Throw(VSG_ERR_INVALID, std::string(what) + ": unknown memory kind");
}

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
  h->events_used = 0;
  hipStream_t st = h->stream;

  // ---- frame to the device, luminance, pyramid ----
  h->Mark(STAGE_COUNT);
  const uint8_t* src = in;
  size_t src_stride = stride;
  if (mem_in == VSG_MEM_HOST) {
    FLOW_HIP(hipMemcpy2DAsync(h->d_in, row_bytes, in, stride, row_bytes, H, hipMemcpyHostToDevice, st));
    ++h->stats.launches;
    src = h->d_in;
    src_stride = row_bytes;
  }
  float* pyr = h->d_pyr[h->cur_pyr];
  if (channels == 3) LaunchLuminanceBgr(src, src_stride, W, H, pyr, st);
  else LaunchLuminanceU8(src, src_stride, W, H, pyr, st);
  ++h->stats.launches;
  for (size_t s = 1; s < h->levels.size(); ++s) {
    LaunchPyrDown(pyr + h->levels[s - 1].offset, h->levels[s - 1].W, h->levels[s - 1].H, pyr + h->levels[s].offset, st);
    ++h->stats.launches;
  }
  FLOW_HIP(hipGetLastError());
  h->Mark(STAGE_PYRAMID);

  // ---- flow ----
  const bool flow = h->have_prev;
  if (flow) {
    const float *cur = pyr, *prev = h->d_pyr[h->cur_pyr ^ 1];
    int calc = 0;
    for (int dir = 0; dir < 2; ++dir) {   // 0: backward = calc(current, previous); 1: forward
      if (dir == 0 ? !want_b : !want_f) continue;
      int* state = h->d_state + (size_t)calc * h->state_ints;
      h->Calc(dir == 0 ? cur : prev, dir == 0 ? prev : cur, state);
      float* out = dir == 0 ? backward_out : forward_out;
      float2* dst = mem_out == VSG_MEM_DEVICE ? reinterpret_cast<float2*>(out) : h->d_out + (size_t)calc * h->N;
      LaunchExport(h->d_u, h->d_u + h->N, state, (int64_t)h->N, dst, st);
      FLOW_HIP(hipGetLastError());
      ++h->stats.launches;
      if (mem_out == VSG_MEM_HOST) {
        FLOW_HIP(hipMemcpyAsync(out, dst, h->N * sizeof(float2), hipMemcpyDeviceToHost, st));
        ++h->stats.launches;
      }
      h->Mark(STAGE_EXPORT);
      ++calc;
    }
    FLOW_HIP(hipMemcpyAsync(h->h_state, h->d_state, (size_t)calc * h->state_ints * sizeof(int),
                            hipMemcpyDeviceToHost, st));
    ++h->stats.launches;
    FLOW_HIP(hipStreamSynchronize(st));
    for (int c = 0; c < calc; ++c) h->stats.iterations_run += h->h_state[(size_t)c * h->state_ints + ST_ITERS];
  } else {
    FLOW_HIP(hipStreamSynchronize(st));
  }
  h->stats.host_syncs = 1;
  float us[STAGE_COUNT + 1] = {0, 0, 0, 0, 0};
  for (size_t k = 1; k < h->events_used; ++k) {
    float ms = 0;
    FLOW_HIP(hipEventElapsedTime(&ms, h->events[k - 1], h->events[k]));
    us[h->event_stage[k]] += ms * 1000.0f;
  }
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
    int n = 0;
    const hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
      Throw(VSG_ERR_DEVICE, "no usable HIP device (libvsg_flow has no CPU fallback): " +
                                std::string(e != hipSuccess ? hipGetErrorString(e) : "device count is 0"));
    }
    if (opt.device >= n) Throw(VSG_ERR_DEVICE, "device ordinal out of range");
    std::unique_ptr<vsg_flow> h(new vsg_flow);
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
    if (opt.device >= 0) h->device = opt.device;
    else FLOW_HIP(hipGetDevice(&h->device));
    DeviceGuard guard(h->device);
    FLOW_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    const int calcs = opt.flow_type == VSG_FLOW_BOTH ? 2 : 1;
    h->events.assign((size_t)2 + calcs * (kScales * 2 * opt.warps + 1), nullptr);
    h->event_stage.assign(h->events.size(), 0);
    for (hipEvent_t& ev : h->events) FLOW_HIP(hipEventCreate(&ev));
    h->state_ints = ST_STOP + kScales * opt.warps;
    const size_t N = h->N;
    h->Alloc(&h->d_in, N * 3);
    h->Alloc(&h->d_pyr[0], total);
    h->Alloc(&h->d_pyr[1], total);
    h->Alloc(&h->d_ix, N);
    h->Alloc(&h->d_iy, N);
    h->Alloc(&h->d_g, N);
    h->Alloc(&h->d_u, 2 * N);
    h->Alloc(&h->d_p, 4 * N);
    h->Alloc(&h->d_out, (size_t)calcs * N);
    h->Alloc(&h->d_partials, (size_t)IterBlocks(width, height));
    h->Alloc(&h->d_state, (size_t)2 * h->state_ints);
    FLOW_HIP(hipHostMalloc(reinterpret_cast<void**>(&h->h_state), (size_t)2 * h->state_ints * sizeof(int),
                           hipHostMallocDefault));
    ++h->allocations;
    *out = h.release();
  });
}

void vsg_flow_destroy(vsg_flow* h) {
  if (!h) return;
  int prev = -1;
  const bool have = hipGetDevice(&prev) == hipSuccess;
  (void)hipSetDevice(h->device);
  delete h;
  if (have) (void)hipSetDevice(prev);
}

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
