// capi_frame.inc -- the handle's life, its options and the calls that paint a whole frame: vsg_render_frame,
// vsg_render_id_image, vsg_render_rasterize.  A part of render_capi.cpp, after capi_level.inc.
extern "C" {

const char* vsg_render_last_error(void) { return g_last_error.c_str(); }

void vsg_render_default_options(vsg_render_options* o) {
  if (!o) return;
  o->blend_alpha = 0.5f;
  o->hierarchy_level = 0.0f;
  o->highlight_edges = 1;
  o->concat_with_source = 0;
  o->has_video = 1;
  o->device = -1;
}

size_t vsg_render_default_stride(int width) {
  size_t step = (size_t)width * 3;
  if (step % 4) step += 4 - step % 4;
  return step;
}

void vsg_render_color(int region_id, uint8_t c[3]) { GlibcColor(region_id, c); }

int vsg_render_create(const vsg_render_options* o, int width, int height, vsg_render** out) {
  return Guard([&] {
    if (!out) Throw(VSG_ERR_INVALID, "handle pointer is null");
    *out = nullptr;
    vsg_render_options opt;
    vsg_render_default_options(&opt);
    if (o) opt = *o;
    if (width <= 0 || height <= 0 || width > (1 << 15) || height > (1 << 15)) Throw(VSG_ERR_INVALID, "bad frame size");
    if (!(opt.hierarchy_level >= 0.0f && opt.hierarchy_level <= 1e6f)) Throw(VSG_ERR_INVALID, "bad hierarchy_level");
    if (!std::isfinite(opt.blend_alpha)) Throw(VSG_ERR_INVALID, "bad blend_alpha");
    if (opt.concat_with_source && !opt.has_video) {
      Throw(VSG_ERR_INVALID, "Request concatenation with source but no video stream present.");
    }
    if (!opt.has_video) opt.blend_alpha = 1.0f;   // segmentation_unit.cpp:486-490
    std::unique_ptr<vsg_render> h(new vsg_render);
    h->device = SelectDevice(opt.device, "libvsg_render");
    h->opt = opt;
    h->W = width;
    h->H = height;
    h->pitch = vsg_render_impl::PlanePitch(width);
    std::memset(&h->stats, 0, sizeof(h->stats));
    h->h_intervals.pinned = true;
    h->h_other.pinned = true;
    DeviceGuard guard(h->device);
    VSG_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    // the clocks' events in this order, then the first block
    h->clock.Create(STAGE_COUNT + 1);
    h->vec.Init();
    h->lvl.Init();
    h->comp.Init();
    h->bound.Init();
    h->adj.Init();
    h->ovl.Init();
    h->pers.Init();
    h->color.Init();
    h->pool.Init();
    h->cont.Init();
    h->dist.Init();
    h->mesh.Init();
    h->simp.Init();
    h->vol.Init();
    h->cut.Init();
    h->d_plane.Reserve((size_t)h->pitch * height * sizeof(uint32_t), &h->allocations);
    *out = h.release();
  });
}

void vsg_render_destroy(vsg_render* h) { DestroyOnDevice(h); }

int vsg_render_frame(vsg_render* h, const uint8_t* seg, size_t seg_len, const uint8_t* bgr, size_t stride,
                     int mem_in, uint8_t* out, size_t out_stride, int mem_out) {
  return Guard([&] {
    if (!h) Throw(VSG_ERR_INVALID, "handle is null");
    if (!out) Throw(VSG_ERR_INVALID, "out is null");
    CheckMem(mem_in, "bgr");
    CheckMem(mem_out, "out");
    const int W = h->W, H = h->H;
    const size_t row_bytes = (size_t)W * 3;
    const bool video = h->opt.has_video != 0;
    if (video && !bgr) Throw(VSG_ERR_INVALID, "the handle was created with has_video: bgr is null");
    if (video && stride < row_bytes) Throw(VSG_ERR_INVALID, "stride is smaller than 3 * width");
    if (out_stride == 0) out_stride = vsg_render_default_stride(W);
    if (out_stride < row_bytes) Throw(VSG_ERR_INVALID, "out_stride is smaller than 3 * width");
    const int out_rows = h->opt.concat_with_source ? 2 * H : H;
    DeviceGuard guard(h->device);
    std::memset(&h->stats, 0, sizeof(h->stats));
    std::memset(&h->vec.stats, 0, sizeof(h->vec.stats));

    // ---- host: decode, hierarchy state (segmentation_unit.cpp:567-591), colour table ----
    const double t0 = NowMs();
    bool vector = false;
    const Hierarchy& hier = Ingest(h, seg, seg_len, &vector);
    if (!h->level_resolved) {
      const int size = (int)h->desc.hierarchy.size();   // the first frame's own hierarchy
      float lvl = h->opt.hierarchy_level;
      if (lvl != std::floor(lvl)) lvl = (float)(int)(lvl * size);
      h->level = std::min<int>((int)lvl, size - 1);
      h->level_resolved = true;
    }
    // HierarchyColorGenerator's own clamps (segmentation_render.cpp:40-50)
    int level = h->level;
    if (level > 0 && hier.empty()) level = 0;
    if (!hier.empty() && level >= (int)hier.size()) level = (int)hier.size() - 1;
    if (h->colors.size() > (1u << 20)) h->colors.clear();
    auto color_of = [&](int mapped) {
      auto it = h->colors.find(mapped);
      if (it == h->colors.end()) {
        uint8_t c[3];
        GlibcColor(mapped, c);
        it = h->colors.emplace(mapped, (uint32_t)c[0] | (uint32_t)c[1] << 8 | (uint32_t)c[2] << 16).first;
      }
      return it->second;
    };
    int64_t n_cross = 0;
    if (vector) {
      h->stats.distinct_ids = AssignRegionValues(h, level, hier, color_of);
      n_cross = h->BuildLines();
    } else {
      h->stats.distinct_ids = AssignValues(h, level, hier, color_of);
    }
    const int64_t n_intervals = vector ? n_cross / 2 : (int64_t)h->intervals.size();
    h->stats.intervals = n_intervals;
    const double t1 = NowMs();
    h->stats.decode_ms = t1 - t0;

    // ---- uploads (and, for a vector-only desc, the scan conversion that makes the list) ----
    if (vector) h->RunVector(n_cross);
    else h->UploadIntervals();
    SourceFrame src{nullptr, 0};
    if (video) src = UploadSource(h, bgr, stride, mem_in, &h->stats.launches);
    const PictureOut dst = StagePicture(h, out, out_stride, out_rows, mem_out);
    h->stats.upload_ms = NowMs() - t1;

    // ---- device: clear, fill, compose ----
    uint32_t* plane = static_cast<uint32_t*>(h->d_plane.p);
    h->clock.Begin(h->stream);
    VSG_HIP(hipMemsetAsync(plane, 0, (size_t)h->pitch * H * sizeof(uint32_t), h->stream));
    h->clock.Mark(STAGE_CLEAR);
    vsg_render_impl::LaunchFill(static_cast<const Interval*>(h->d_intervals.p), n_intervals, plane, h->pitch,
                                h->stream);
    h->clock.Mark(STAGE_FILL);
    const int mode = h->opt.concat_with_source ? vsg_render_impl::COMPOSE_CONCAT
                     : video                   ? vsg_render_impl::COMPOSE_BLEND
                                               : vsg_render_impl::COMPOSE_RENDER;
    vsg_render_impl::LaunchCompose(plane, h->pitch, W, H, src.p, src.stride, dst.p, dst.stride, h->opt.highlight_edges,
                                   mode, h->opt.blend_alpha, h->stream);
    VSG_HIP(hipGetLastError());
    h->clock.Mark(STAGE_COMPOSE);
    h->stats.launches += 2 + (n_intervals == 0 ? 0 : 1);
    if (mem_out == VSG_MEM_HOST) {
      VSG_HIP(hipMemcpy2DAsync(out, out_stride, dst.p, dst.stride, row_bytes, out_rows, hipMemcpyDeviceToHost,
                               h->stream));
      ++h->stats.launches;
    }
    h->FinishStats();
    if (vector) h->CheckVector();
  });
}

int vsg_render_id_image(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int32_t* out, int mem_out) {
  return Guard([&] {
    if (!h) Throw(VSG_ERR_INVALID, "handle is null");
    if (!out) Throw(VSG_ERR_INVALID, "out is null");
    CheckMem(mem_out, "out");
    const size_t bytes = (size_t)h->W * h->H * sizeof(int32_t);
    DeviceGuard guard(h->device);
    uint32_t* ids = reinterpret_cast<uint32_t*>(out);   // device output: painted in place
    if (mem_out == VSG_MEM_HOST) {
      h->d_ids.Reserve(bytes, &h->allocations);
      ids = static_cast<uint32_t*>(h->d_ids.p);
    }
    const bool vector = PaintIds(h, seg, seg_len, level, ids, [](int mapped) { return (uint32_t)mapped; });
    h->clock.Mark(STAGE_COMPOSE);   // nothing is composed: the two marks are back to back
    if (mem_out == VSG_MEM_HOST) {
      VSG_HIP(hipMemcpyAsync(out, ids, bytes, hipMemcpyDeviceToHost, h->stream));
      ++h->stats.launches;
    }
    h->FinishStats();
    if (vector) h->CheckVector();
  });
}

int vsg_render_rasterize(vsg_render* h, const uint8_t* seg, size_t seg_len, int32_t* out, size_t capacity_intervals,
                         size_t* count, int mem_out) {
  return Guard([&] {
    if (!h) Throw(VSG_ERR_INVALID, "handle is null");
    if (!count) Throw(VSG_ERR_INVALID, "count is null");
    *count = 0;
    CheckMem(mem_out, "out");
    if (!seg && seg_len) Throw(VSG_ERR_INVALID, "seg is null");
    DeviceGuard guard(h->device);
    std::memset(&h->stats, 0, sizeof(h->stats));
    std::memset(&h->vec.stats, 0, sizeof(h->vec.stats));
    const double t0 = NowMs();
    // the handle's kept hierarchy is left alone: this call renders nothing
    ParseDesc(seg, seg_len, h->W, h->H, true, &h->desc, &h->intervals);
    if (!h->desc.has_mesh) Throw(VSG_ERR_INVALID, "the SegmentationDesc has no vector_mesh");
    h->vec.region_value.assign(h->desc.region_ids.begin(), h->desc.region_ids.end());
    const int64_t n_cross = h->BuildLines();
    const size_t n = (size_t)(n_cross / 2);
    h->stats.intervals = (int64_t)n;
    h->stats.distinct_ids = (int64_t)h->desc.region_ids.size();
    *count = n;
    if (!out && capacity_intervals == 0) return;   // asked for the count only
    if (n > capacity_intervals) {
      Throw(VSG_ERR_INVALID, "capacity_intervals is " + std::to_string(capacity_intervals) + ", the frame has " +
                                 std::to_string(n) + " intervals");
    }
    if (n && !out) Throw(VSG_ERR_INVALID, "out is null");
    const double t1 = NowMs();
    h->stats.decode_ms = t1 - t0;
    h->RunVector(n_cross);
    h->stats.upload_ms = NowMs() - t1;
    if (n) {
      VSG_HIP(hipMemcpyAsync(out, h->d_intervals.p, n * sizeof(Interval),
                             mem_out == VSG_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, h->stream));
      ++h->stats.launches;
    }
    VSG_HIP(hipStreamSynchronize(h->stream));
    h->stats.device_allocations = h->allocations;
    h->CheckVector();
  });
}

VSG_RENDER_LAST_STATS(vsg_render_last_vector_stats, vsg_render_vector_stats, vec.stats)

int vsg_render_level(vsg_render* h, int* level) {
  return Guard([&] {
    if (!h || !level) Throw(VSG_ERR_INVALID, "null argument");
    if (!h->level_resolved) Throw(VSG_ERR_STATE, "no frame has been rendered yet");
    *level = h->level;
  });
}

VSG_RENDER_LAST_STATS(vsg_render_last_stats, vsg_render_stats, stats)

}  // extern "C"
