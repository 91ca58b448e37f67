// resize_capi.cpp -- extern "C" entry points declared in include/vsg_resize.h: the size rule of the
// reference's reader, the filter tables, and the handle with its device blocks (tables uploaded at
// creation, the f32 intermediate, staging blocks for host frames that only grow) around the two
// kernels of resize.hip.
#include <cmath>
#include <cstring>
#include <memory>
#include <string>

#include "../../include/vsg_resize.h"
#include "resize.h"
#include "../common/capi_support.h"

namespace {

using namespace vsg_resize_impl;

const int kMaxSide = 65535;

int RoundUp4(int v) { return (v + 3) & ~3; }

// video_reader_unit.cpp:155-206.  The f32 products and std::ceil on a float are the reference's.
void OutputSize(int mode, float factor, int size, int in_w, int in_h, int* out_w, int* out_h, int* width_step) {
  if (in_w < 1 || in_h < 1 || in_w > kMaxSide || in_h > kMaxSide) Throw(VSG_ERR_INVALID, "frame size outside [1, 65535]");
  float f = 1.0f;
  switch (mode) {
    case VSG_RESIZE_NONE:
      break;
    case VSG_RESIZE_BY_FACTOR:
      if (factor > 1.0f) Throw(VSG_ERR_INVALID, "Only downscaling is supported.");
      f = factor;
      break;
    case VSG_RESIZE_TO_MIN_SIZE:
    case VSG_RESIZE_TO_MAX_SIZE: {
      if (size <= 0) Throw(VSG_ERR_INVALID, "downscale size has to be positive");
      const float a = size * (1.0f / in_w), b = size * (1.0f / in_h);
      f = mode == VSG_RESIZE_TO_MIN_SIZE ? std::max(a, b) : std::min(a, b);
      f = std::min(1.0f, f);   // cap to downscaling
      break;
    }
    default:
      Throw(VSG_ERR_INVALID, "unknown downscale mode");
  }
  if (!(f > 0.0f)) Throw(VSG_ERR_INVALID, "the downscaled frame would be empty");
  int w = (int)std::ceil(in_w * f);
  const int h = (int)std::ceil(in_h * f);
  w += w % 2;   // force even widths
  if (w < 1 || h < 1) Throw(VSG_ERR_INVALID, "the downscaled frame would be empty");
  if (out_w) *out_w = w;
  if (out_h) *out_h = h;
  if (width_step) *width_step = RoundUp4(w * 3);
}

enum Stage { STAGE_UPLOAD = 0, STAGE_H, STAGE_V, STAGE_DOWNLOAD, STAGE_COPY, STAGE_COUNT };

}  // namespace

struct vsg_resize {
  vsg_resize_options opt;
  int device = 0;
  int in_w = 0, in_h = 0, out_w = 0, out_h = 0, width_step = 0;
  bool identity = false;
  Filter fh, fv;                 // host tables (weights dropped after the upload)
  int taps_h = 0, taps_v = 0;
  int tile_cols = 0, span_stride = 0, pitch = 0;
  hipStream_t stream = nullptr;
  StageClock clock;
  // device blocks: tables and the intermediate from creation, the staging blocks on first use
  Block d_first_h, d_count_h, d_first_v, d_count_v, d_weights_ht, d_weights_v, d_inter, d_in, d_out;
  int64_t allocations = 0;
  vsg_resize_stats stats;

  ~vsg_resize() {
    if (!stream) return;
    (void)hipStreamSynchronize(stream);
    (void)hipStreamDestroy(stream);
  }
};

namespace {

// The widest tile of output columns whose source spans, H_ROWS of them, fit the LDS budget.
void ChooseTile(vsg_resize* h) {
  for (int cols = H_TILE_COLS; cols >= 1; cols /= 2) {
    int widest = 0;
    for (int o0 = 0; o0 < h->out_w; o0 += cols) {
      int b0, b1;
      TileSpan(h->fh.first.data(), h->fh.count.data(), o0, std::min(o0 + cols, h->out_w), h->in_w, true, &b0, &b1);
      widest = std::max(widest, b1 - b0);
    }
    const int span_stride = RoundUp4(widest);
    if ((size_t)H_ROWS * span_stride <= (size_t)H_LDS_BUDGET) {
      h->tile_cols = cols;
      h->span_stride = span_stride;
      return;
    }
  }
  Throw(VSG_ERR_INTERNAL, "no tile of the horizontal pass fits its LDS budget");
}

void Process(vsg_resize* h, const uint8_t* in, size_t stride_in, int mem_in, uint8_t* out, size_t stride_out,
             int mem_out) {
  if (!h) Throw(VSG_ERR_INVALID, "handle is null");
  if (!in) Throw(VSG_ERR_INVALID, "input frame is null");
  if (!out) Throw(VSG_ERR_INVALID, "output frame is null");
  CheckMem(mem_in, "input frame");
  CheckMem(mem_out, "output frame");
  const size_t row_in = (size_t)h->in_w * 3, row_out = (size_t)h->out_w * 3;
  if (stride_in < row_in) Throw(VSG_ERR_INVALID, "stride_in is smaller than a row of the input frame");
  if (stride_out < row_out) Throw(VSG_ERR_INVALID, "stride_out is smaller than a row of the output frame");
  DeviceGuard guard(h->device);
  std::memset(&h->stats, 0, sizeof(h->stats));
  hipStream_t st = h->stream;
  h->clock.Begin(st);

  if (h->identity) {   // out == in on both axes: the frame is copied, no filter runs
    if (mem_in == VSG_MEM_HOST && mem_out == VSG_MEM_HOST) {   // nothing for the device to do
      for (int y = 0; y < h->in_h; ++y) std::memcpy(out + (size_t)y * stride_out, in + (size_t)y * stride_in, row_in);
    } else {
      const hipMemcpyKind kind = mem_in == VSG_MEM_HOST    ? hipMemcpyHostToDevice
                                 : mem_out == VSG_MEM_HOST ? hipMemcpyDeviceToHost
                                                           : hipMemcpyDeviceToDevice;
      VSG_HIP(hipMemcpy2DAsync(out, stride_out, in, stride_in, row_in, (size_t)h->in_h, kind, st));
      ++h->stats.launches;
    }
    h->clock.Mark(STAGE_COPY);
  } else {
    const uint8_t* src = in;
    size_t src_stride = stride_in;
    if (mem_in == VSG_MEM_HOST) {
      const size_t packed = (size_t)RoundUp4((int)row_in);
      h->d_in.Reserve(packed * h->in_h, &h->allocations);
      VSG_HIP(hipMemcpy2DAsync(h->d_in.p, packed, in, stride_in, row_in, (size_t)h->in_h, hipMemcpyHostToDevice, st));
      ++h->stats.launches;
      h->clock.Mark(STAGE_UPLOAD);
      src = h->d_in.As<uint8_t>();
      src_stride = packed;
    }
    uint8_t* dst = out;
    size_t dst_stride = stride_out;
    if (mem_out == VSG_MEM_HOST) {
      h->d_out.Reserve((size_t)h->width_step * h->out_h, &h->allocations);
      dst = h->d_out.As<uint8_t>();
      dst_stride = (size_t)h->width_step;
    }
    float* inter = h->d_inter.As<float>();
    LaunchResizeH(src, src_stride, h->in_w, h->in_h, h->out_w, h->d_first_h.As<int32_t>(), h->d_count_h.As<int32_t>(),
                  h->d_weights_ht.As<float>(), h->tile_cols, h->span_stride, inter, h->pitch, st);
    VSG_HIP(hipGetLastError());
    h->clock.Mark(STAGE_H);
    LaunchResizeV(inter, h->pitch, h->in_h, h->out_w, h->out_h, h->d_first_v.As<int32_t>(), h->d_count_v.As<int32_t>(),
                  h->d_weights_v.As<float>(), h->taps_v, dst, dst_stride, st);
    VSG_HIP(hipGetLastError());
    h->clock.Mark(STAGE_V);
    h->stats.launches += 2;
    if (mem_out == VSG_MEM_HOST) {
      VSG_HIP(hipMemcpy2DAsync(out, stride_out, dst, dst_stride, row_out, (size_t)h->out_h, hipMemcpyDeviceToHost, st));
      ++h->stats.launches;
      h->clock.Mark(STAGE_DOWNLOAD);
    }
    h->stats.taps_h = h->taps_h;
    h->stats.taps_v = h->taps_v;
  }
  VSG_HIP(hipStreamSynchronize(st));
  h->stats.host_syncs = 1;
  float us[STAGE_COUNT];
  h->clock.Read(us, STAGE_COUNT);
  h->stats.upload_us = us[STAGE_UPLOAD];
  h->stats.horizontal_us = us[STAGE_H];
  h->stats.vertical_us = us[STAGE_V];
  h->stats.download_us = us[STAGE_DOWNLOAD];
  h->stats.copy_us = us[STAGE_COPY];
  h->stats.device_allocations = h->allocations;
}

}  // namespace

extern "C" {

const char* vsg_resize_last_error(void) { return g_last_error.c_str(); }

void vsg_resize_default_options(vsg_resize_options* o) {
  if (!o) return;
  o->mode = VSG_RESIZE_NONE;
  o->factor = 0.5f;
  o->size = 0;
  o->device = -1;
}

int vsg_resize_output_size(int mode, float factor, int size, int in_w, int in_h, int* out_w, int* out_h,
                           int* width_step) {
  return Guard([&] { OutputSize(mode, factor, size, in_w, in_h, out_w, out_h, width_step); });
}

int vsg_resize_filter(int n_in, int n_out, int32_t* first, int32_t* count, float* weights, size_t capacity,
                      int* max_taps) {
  return Guard([&] {
    if (!max_taps) Throw(VSG_ERR_INVALID, "max_taps is null");
    *max_taps = 0;
    if (n_in < 1 || n_out < 1 || n_in > kMaxSide || n_out > kMaxSide) Throw(VSG_ERR_INVALID, "size outside [1, 65535]");
    Filter f;
    BuildFilter(n_in, n_out, false, &f);
    *max_taps = f.max_taps;
    if (!first && !count && !weights && capacity == 0) return;   // the caller asked for max_taps
    if (!first || !count || !weights || capacity < (size_t)n_out * f.max_taps) {
      Throw(VSG_ERR_INVALID, "the tables need n_out ints each and n_out * max_taps floats");
    }
    BuildFilter(n_in, n_out, true, &f);
    std::memcpy(first, f.first.data(), (size_t)n_out * sizeof(int32_t));
    std::memcpy(count, f.count.data(), (size_t)n_out * sizeof(int32_t));
    std::memcpy(weights, f.weights.data(), f.weights.size() * sizeof(float));
  });
}

int vsg_resize_create(const vsg_resize_options* o, int in_w, int in_h, vsg_resize** out) {
  return Guard([&] {
    if (!out) Throw(VSG_ERR_INVALID, "handle pointer is null");
    *out = nullptr;
    vsg_resize_options opt;
    vsg_resize_default_options(&opt);
    if (o) opt = *o;
    std::unique_ptr<vsg_resize> h(new vsg_resize);
    h->opt = opt;
    h->in_w = in_w;
    h->in_h = in_h;
    std::memset(&h->stats, 0, sizeof(h->stats));
    OutputSize(opt.mode, opt.factor, opt.size, in_w, in_h, &h->out_w, &h->out_h, &h->width_step);
    h->identity = h->out_w == in_w && h->out_h == in_h;
    if (!h->identity) {
      BuildFilter(in_w, h->out_w, false, &h->fh);
      if (h->fh.max_taps > VSG_RESIZE_MAX_TAPS_H) {
        Throw(VSG_ERR_INVALID, "horizontal downscale ratio too large: " + std::to_string(h->fh.max_taps) +
                                   " source pixels per output pixel, the limit is " +
                                   std::to_string((int)VSG_RESIZE_MAX_TAPS_H));
      }
      BuildFilter(in_w, h->out_w, true, &h->fh);
      BuildFilter(in_h, h->out_h, true, &h->fv);
      h->taps_h = h->fh.max_taps;
      h->taps_v = h->fv.max_taps;
      h->pitch = RoundUp4(h->out_w * 3);
      ChooseTile(h.get());
    }
    h->device = SelectDevice(opt.device, "libvsg_resize");
    DeviceGuard guard(h->device);
    VSG_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    h->clock.Create(STAGE_COUNT + 1);
    if (!h->identity) {
      const size_t nw = (size_t)h->out_w, nh = (size_t)h->out_h;
      std::vector<float> wt((size_t)h->taps_h * nw);   // max_taps x out_w: a tap's weights are contiguous
      for (size_t oo = 0; oo < nw; ++oo) {
        for (size_t j = 0; j < (size_t)h->taps_h; ++j) wt[j * nw + oo] = h->fh.weights[oo * h->taps_h + j];
      }
      const size_t inter_bytes = (size_t)h->pitch * in_h * sizeof(float);
      const struct { Block* block; const void* from; size_t bytes; } tables[] = {
          {&h->d_first_h, h->fh.first.data(), nw * sizeof(int32_t)},
          {&h->d_count_h, h->fh.count.data(), nw * sizeof(int32_t)},
          {&h->d_weights_ht, wt.data(), wt.size() * sizeof(float)},
          {&h->d_first_v, h->fv.first.data(), nh * sizeof(int32_t)},
          {&h->d_count_v, h->fv.count.data(), nh * sizeof(int32_t)},
          {&h->d_weights_v, h->fv.weights.data(), h->fv.weights.size() * sizeof(float)},
      };
      for (const auto& t : tables) t.block->Reserve(t.bytes, &h->allocations);
      h->d_inter.Reserve(inter_bytes, &h->allocations);
      hipStream_t st = h->stream;
      for (const auto& t : tables) VSG_HIP(hipMemcpyAsync(t.block->p, t.from, t.bytes, hipMemcpyHostToDevice, st));
      VSG_HIP(hipMemsetAsync(h->d_inter.p, 0, inter_bytes, st));   // the rows' padding
      VSG_HIP(hipStreamSynchronize(st));
      h->fh.weights = std::vector<float>();
      h->fv.weights = std::vector<float>();
    }
    *out = h.release();
  });
}

void vsg_resize_destroy(vsg_resize* h) { DestroyOnDevice(h); }

int vsg_resize_get_output_size(vsg_resize* h, int* out_w, int* out_h, int* width_step) {
  return Guard([&] {
    if (!h) Throw(VSG_ERR_INVALID, "handle is null");
    if (out_w) *out_w = h->out_w;
    if (out_h) *out_h = h->out_h;
    if (width_step) *width_step = h->width_step;
  });
}

int vsg_resize_process(vsg_resize* h, const uint8_t* bgr_in, size_t stride_in, int mem_in, uint8_t* bgr_out,
                       size_t stride_out, int mem_out) {
  return Guard([&] { Process(h, bgr_in, stride_in, mem_in, bgr_out, stride_out, mem_out); });
}

int vsg_resize_last_stats(vsg_resize* h, vsg_resize_stats* s) {
  return Guard([&] {
    if (!h || !s) Throw(VSG_ERR_INVALID, "null argument");
    *s = h->stats;
  });
}

}  // extern "C"
