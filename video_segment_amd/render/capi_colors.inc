// capi_colors.inc -- vsg_render_level_colors and vsg_render_mean_frame.  A part of render_capi.cpp.
namespace {

// vsg_render_level_colors (picture == nullptr) and vsg_render_mean_frame (colors == nullptr) behind their
// argument checks that need no handle.  keep (vsg_render_volume_add; connectedness 0, no outputs): the records
// are written to h->color.records all the same, and *keep receives the front half, whose lists stay in h->lvl.
void LevelColors(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness, const uint8_t* bgr,
                 size_t stride, int mem_in, vsg_render_level_color* colors, size_t capacity_colors, size_t* num_colors,
                 uint8_t* picture, size_t out_stride, int mem_out, LevelFront* keep = nullptr) {
  using namespace vsg_render_impl;
  static_assert(sizeof(vsg_render_level_color) == kLevelColorWords * sizeof(int32_t), "moved as int32 words");
  static_assert(sizeof(vsg_render_color_stats) == 56, "as the header says");
  const int W = h->W, H = h->H;
  const size_t row_bytes = (size_t)W * 3;
  if (stride < row_bytes) Throw(VSG_ERR_INVALID, "stride is smaller than 3 * width");
  if (picture) {
    if (out_stride == 0) out_stride = vsg_render_default_stride(W);
    if (out_stride < row_bytes) Throw(VSG_ERR_INVALID, "out_stride is smaller than 3 * width");
  }
  const bool count_only = !picture && !colors && capacity_colors == 0;
  if (!picture && !colors && capacity_colors) Throw(VSG_ERR_INVALID, "colors is null");
  CheckFrameBelow2Pow32(h);
  DeviceGuard guard(h->device);
  vsg_render_color_stats& ks = h->color.stats;
  std::memset(&ks, 0, sizeof(ks));

  // ---- the interval list grouped by record, every interval's record, id and component of every record ----
  const Interval* list = nullptr;
  const uint32_t* rank = nullptr;
  const int32_t* table = nullptr;
  const uint32_t* d_count = nullptr;
  int table_words = 0;
  uint32_t n = 0, cap_records = 0;
  vsg_render_level_stats ls;   // of the shared front half; the last level_regions call's stay
  std::memset(&ls, 0, sizeof(ls));
  if (connectedness == 0) {
    LevelFront f = PaintLevelRuns(h, seg, seg_len, level, &ls);
    n = f.n;
    if (n) SortLevelRuns(h, &f, &ls);
    list = f.intervals;
    rank = f.rank;
    table = f.regions;
    table_words = kLevelRegionWords;
    d_count = &f.status->regions;
    cap_records = f.cap_regions;
    if (keep) *keep = f;
    ks.plane_us = h->stats.clear_us + h->stats.fill_us + ls.runs_us;
    h->stats.launches += ls.launches;
  } else {
    size_t n_components = 0, n_intervals = 0;
    LevelComponents(h, seg, seg_len, level, connectedness, nullptr, 0, &n_components, nullptr, 0, &n_intervals, nullptr,
                    VSG_MEM_DEVICE, true);
    n = (uint32_t)n_intervals;
    list = h->comp.intervals.As<Interval>();
    rank = h->comp.work.As<uint32_t>() + (size_t)5 * n;   // LevelComponents' comp_rank
    table = h->comp.table.As<int32_t>();
    table_words = kLevelComponentWords;
    d_count = &h->comp.status.As<CompStatus>()->components;
    cap_records = (uint32_t)n_components;
    const vsg_render_component_stats& cs = h->comp.stats;
    ks.plane_us = h->stats.clear_us + h->stats.fill_us + cs.runs_us + cs.sort_us + cs.link_us + cs.order_us +
                  cs.label_us;
  }
  ks.launches = h->stats.launches;
  ks.intervals = n;
  if (n && cap_records == 0) Throw(VSG_ERR_INTERNAL, "the plane has groups the desc has no ids for");

  // ---- blocks, all before anything that uses them is enqueued ----
  struct Seen {
    ColorStatus status;
    uint32_t records, pad[3];
  };
  const size_t record_bytes = (size_t)cap_records * sizeof(vsg_render_level_color);
  const bool host_table = colors && mem_out == VSG_MEM_HOST;
  h->color.status.Reserve(sizeof(ColorStatus), &h->allocations);
  h->color.seen.Reserve(sizeof(Seen) + (host_table ? record_bytes : 0), &h->allocations);
  h->color.partials.Reserve((size_t)n * kColorPartialWords * sizeof(uint32_t), &h->allocations);
  h->color.acc.Reserve((size_t)cap_records * kColorAccBytes, &h->allocations);
  if (host_table || picture || keep) h->color.records.Reserve(record_bytes, &h->allocations);
  if (picture) h->color.intervals.Reserve((size_t)n * sizeof(Interval), &h->allocations);
  ColorStatus* status = h->color.status.As<ColorStatus>();
  Seen* seen = h->color.seen.As<Seen>();
  std::memset(seen, 0, sizeof(Seen));
  int launches = 0;

  // ---- F: where it is, or to the device with the default stride ----
  h->color.clock.Begin(h->stream);
  const SourceFrame src = UploadSource(h, bgr, stride, mem_in, &launches);
  const int out_rows = h->opt.concat_with_source ? 2 * H : H;
  const PictureOut dst = picture ? StagePicture(h, picture, out_stride, out_rows, mem_out) : PictureOut{nullptr, 0};
  h->color.clock.Mark(CLR_UPLOAD);

  // ---- partials, table ----
  uint32_t* partials = h->color.partials.As<uint32_t>();
  LaunchColorRuns(list, n, W, H, src.p, src.stride, partials, h->stream);
  VSG_HIP(hipGetLastError());
  h->color.clock.Mark(CLR_SUMS);
  // where the records go: the caller's device memory (the kernel decides there whether they fit), or the
  // handle's block; nowhere in a count-only call
  int32_t* records = nullptr;
  uint32_t capacity = 0;
  if (picture || host_table || keep) {
    records = h->color.records.As<int32_t>();
    capacity = cap_records;
  } else if (colors) {
    records = reinterpret_cast<int32_t*>(colors);
    capacity = (uint32_t)std::min<size_t>(capacity_colors, cap_records);
  }
  VSG_HIP(hipMemsetAsync(status, 0, sizeof(ColorStatus), h->stream));
  ++launches;
  if (n) {
    VSG_HIP(hipMemsetAsync(h->color.acc.p, 0, (size_t)cap_records * kColorAccBytes, h->stream));
    LaunchColorTable(list, rank, partials, n, cap_records, h->color.acc.p, table, table_words, connectedness != 0,
                     d_count, capacity, records, status, h->stream);
    VSG_HIP(hipGetLastError());
    VSG_HIP(hipMemcpyAsync(&seen->records, d_count, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    launches += 5;   // k_color_runs, the clear, k_color_table, k_color_finish, the count
  }
  h->color.clock.Mark(CLR_TABLE);

  // ---- the picture: vsg_render_frame's clear, fill and compose on the intervals with the means ----
  if (picture) {
    const bool video = h->opt.has_video != 0;
    Interval* painted = h->color.intervals.As<Interval>();
    uint32_t* plane = h->d_plane.As<uint32_t>();
    LaunchColorIntervals(list, rank, n, records, capacity, painted, h->stream);
    VSG_HIP(hipMemsetAsync(plane, 0, (size_t)h->pitch * H * sizeof(uint32_t), h->stream));
    LaunchFill(painted, n, plane, h->pitch, h->stream);
    const int mode = h->opt.concat_with_source ? COMPOSE_CONCAT : video ? COMPOSE_BLEND : COMPOSE_RENDER;
    LaunchCompose(plane, h->pitch, W, H, src.p, src.stride, dst.p, dst.stride, h->opt.highlight_edges, mode,
                  h->opt.blend_alpha, h->stream);
    VSG_HIP(hipGetLastError());
    launches += 2 + (n ? 2 : 0);
    h->color.clock.Mark(CLR_PAINT);
    if (mem_out == VSG_MEM_HOST) {
      VSG_HIP(hipMemcpy2DAsync(picture, out_stride, dst.p, dst.stride, row_bytes, out_rows, hipMemcpyDeviceToHost,
                               h->stream));
      ++launches;
    }
  }
  if (host_table && n) {
    VSG_HIP(hipMemcpyAsync(seen + 1, records, record_bytes, hipMemcpyDeviceToHost, h->stream));
    ++launches;
  }
  VSG_HIP(hipMemcpyAsync(&seen->status, status, sizeof(ColorStatus), hipMemcpyDeviceToHost, h->stream));
  ++launches;
  VSG_HIP(hipStreamSynchronize(h->stream));
  {
    float us[CLR_STAGES];
    h->color.clock.Read(us, CLR_STAGES);
    ks.plane_us += us[CLR_UPLOAD];
    ks.sums_us = us[CLR_SUMS];
    ks.table_us = us[CLR_TABLE];
    ks.paint_us = us[CLR_PAINT];
    if (n && connectedness == 0) {
      float lus[LVL_COUNT];
      h->lvl.clock.Read(lus, LVL_COUNT);
      ks.plane_us += lus[LVL_SORT] + lus[LVL_TABLE];
    }
  }
  ks.launches += launches;
  h->stats.launches += launches;
  h->stats.device_allocations = h->allocations;
  const uint32_t n_records = seen->records;
  if ((n == 0) != (n_records == 0) || n_records > cap_records || (connectedness != 0 && n_records != cap_records)) {
    Throw(VSG_ERR_INTERNAL, "the level has other groups than the desc has ids for");
  }
  if ((seen->status.flags & COLOR_FLAG_RANGE) || seen->status.largest > n) {
    Throw(VSG_ERR_INTERNAL, "an interval's record is out of range");
  }
  ks.groups = n_records;
  ks.covered = (int64_t)seen->status.covered;
  ks.largest_group_intervals = seen->status.largest;
  if (num_colors) *num_colors = n_records;
  if (picture || count_only) return;
  if (n_records > capacity_colors) {
    Throw(VSG_ERR_INVALID, "the level has " + std::to_string(n_records) + " groups, the capacity is " +
                               std::to_string(capacity_colors));
  }
  if (host_table && n_records) std::memcpy(colors, seen + 1, (size_t)n_records * sizeof(vsg_render_level_color));
}

// The refusals of both calls that are answered before the handle is dereferenced.
void CheckColorArguments(const vsg_render* h, int connectedness, const uint8_t* bgr, int mem_in, int mem_out) {
  if (!h) Throw(VSG_ERR_INVALID, "handle is null");
  if (!bgr) Throw(VSG_ERR_INVALID, "bgr is null");
  if (mem_in != VSG_MEM_HOST && mem_in != VSG_MEM_DEVICE) {
    Throw(VSG_ERR_INVALID, "mem_in is neither VSG_MEM_HOST nor VSG_MEM_DEVICE");
  }
  if (mem_out != VSG_MEM_HOST && mem_out != VSG_MEM_DEVICE) {
    Throw(VSG_ERR_INVALID, "mem_out is neither VSG_MEM_HOST nor VSG_MEM_DEVICE");
  }
  CheckConnectedness(connectedness, true);
}

}  // namespace

extern "C" {

int vsg_render_level_colors(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness,
                            const uint8_t* bgr, size_t stride, int mem_in, vsg_render_level_color* colors,
                            size_t capacity_colors, size_t* num_colors, int mem_out) {
  return Guard([&] {
    if (!num_colors) Throw(VSG_ERR_INVALID, "the count pointer is null");
    *num_colors = 0;
    CheckColorArguments(h, connectedness, bgr, mem_in, mem_out);
    LevelColors(h, seg, seg_len, level, connectedness, bgr, stride, mem_in, colors, capacity_colors, num_colors,
                nullptr, 0, mem_out);
  });
}

int vsg_render_mean_frame(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness,
                          const uint8_t* bgr, size_t stride, int mem_in, uint8_t* out, size_t out_stride,
                          int mem_out) {
  return Guard([&] {
    if (!out) Throw(VSG_ERR_INVALID, "out is null");
    CheckColorArguments(h, connectedness, bgr, mem_in, mem_out);
    LevelColors(h, seg, seg_len, level, connectedness, bgr, stride, mem_in, nullptr, 0, nullptr, out, out_stride,
                mem_out);
  });
}

VSG_RENDER_LAST_STATS(vsg_render_last_color_stats, vsg_render_color_stats, color.stats)

}  // extern "C"
