// capi_pool.inc -- vsg_render_level_pool and vsg_render_level_unpool.  A part of render_capi.cpp.
namespace {

using vsg_render_impl::PoolLayout;
using vsg_render_impl::PoolMatrices;

size_t PoolElementBytes(int dtype) { return dtype == VSG_POOL_F32 ? 4 : 2; }

// The refusals of a feature map's description that need no handle; the layout the kernels take.
PoolLayout CheckPoolLayout(const void* p, const char* what, int dtype, int channels, ptrdiff_t chan_stride,
                           ptrdiff_t row_stride, ptrdiff_t pixel_stride) {
  if (dtype != VSG_POOL_F32 && dtype != VSG_POOL_F16 && dtype != VSG_POOL_BF16) {
    Throw(VSG_ERR_INVALID, "dtype is none of VSG_POOL_F32, VSG_POOL_F16, VSG_POOL_BF16");
  }
  if (channels < 1 || channels > 65535) Throw(VSG_ERR_INVALID, "channels is outside [1, 65535]");
  if (chan_stride < 0 || row_stride < 0 || pixel_stride < 0) Throw(VSG_ERR_INVALID, "a stride is negative");
  if ((uintptr_t)p % PoolElementBytes(dtype) != 0) {
    Throw(VSG_ERR_INVALID, std::string(what) + " is not aligned to its element size");
  }
  PoolLayout l;
  l.chan_stride = chan_stride;
  l.row_stride = row_stride;
  l.pixel_stride = pixel_stride;
  l.channels = channels;
  l.dtype = dtype;
  if (pixel_stride == 1) {
    l.channels_last = false;
  } else if (chan_stride == 1 && pixel_stride >= channels) {
    l.channels_last = true;
  } else {
    Throw(VSG_ERR_INVALID, "the strides are neither planar (pixel_stride 1) nor channels-last (chan_stride 1, "
                           "pixel_stride >= channels)");
  }
  return l;
}

// Rows and planes have to be disjoint: compared with the handle's size.
void CheckPoolDisjoint(const vsg_render* h, const PoolLayout& l, const char* what) {
  const long long W = h->W, H = h->H, C = l.channels;
  bool ok;
  if (l.channels_last) {
    ok = H == 1 || l.row_stride >= (W - 1) * l.pixel_stride + C;
  } else {
    ok = H == 1 || l.row_stride >= W;
    if (ok && C > 1) {
      const bool behind = l.chan_stride >= (H - 1) * l.row_stride + W;
      const bool by_row = l.chan_stride >= W && (H == 1 || l.row_stride >= (C - 1) * l.chan_stride + W);
      ok = behind || by_row;
    }
  }
  if (!ok) Throw(VSG_ERR_INVALID, std::string("the strides of ") + what + " let rows or planes overlap");
}

// The elements from the first to the last one of a map of the handle's size.
size_t PoolSpanBytes(const vsg_render* h, const PoolLayout& l) {
  const long long last = (l.channels - 1) * l.chan_stride + (h->H - 1) * l.row_stride + (h->W - 1) * l.pixel_stride;
  return (size_t)(last + 1) * PoolElementBytes(l.dtype);
}

// Where a host map's span lies in the handle's block: at its own address modulo 16, so that the kernels take the
// same 16-byte groups as for the map itself.
char* StagePoolSpan(vsg_render* h, const void* host, size_t bytes) {
  h->pool.features.Reserve(bytes + 16, &h->allocations);
  return h->pool.features.As<char>() + ((uintptr_t)host & 15u);
}

// The interval list grouped by record, every interval's record, id and component of every record: the front
// half of LevelColors.
struct PoolFront {
  const Interval* list = nullptr;
  const uint32_t* rank = nullptr;
  const int32_t* table = nullptr;
  int table_words = 0;
  uint32_t n = 0, records = 0;
};

struct PoolSeen {
  PoolStatus status;
  uint32_t records, pad[3];
};

// Makes the list and waits for the number of records.  Fills plane_us, launches, intervals of the family's stats.
PoolFront PoolFrontHalf(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness) {
  using namespace vsg_render_impl;
  vsg_render_pool_stats& ks = h->pool.stats;
  PoolFront p;
  uint32_t cap_records = 0;
  h->pool.status.Reserve(sizeof(PoolStatus), &h->allocations);
  h->pool.seen.Reserve(sizeof(PoolSeen), &h->allocations);
  PoolSeen* seen = h->pool.seen.As<PoolSeen>();
  std::memset(seen, 0, sizeof(PoolSeen));
  int launches = 0;
  if (connectedness == 0) {
    vsg_render_level_stats ls;   // of the shared front half; the last level_regions call's stay
    std::memset(&ls, 0, sizeof(ls));
    LevelFront f = PaintLevelRuns(h, seg, seg_len, level, &ls);
    p.n = f.n;
    if (p.n) SortLevelRuns(h, &f, &ls);
    p.list = f.intervals;
    p.rank = f.rank;
    p.table = f.regions;
    p.table_words = kLevelRegionWords;
    cap_records = f.cap_regions;
    ks.plane_us = h->stats.clear_us + h->stats.fill_us + ls.runs_us;
    h->stats.launches += ls.launches;
    if (p.n) {
      VSG_HIP(hipMemcpyAsync(&seen->records, &f.status->regions, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
      VSG_HIP(hipStreamSynchronize(h->stream));
      ++launches;
      float lus[LVL_COUNT];
      h->lvl.clock.Read(lus, LVL_COUNT);
      ks.plane_us += lus[LVL_SORT] + lus[LVL_TABLE];
      p.records = seen->records;
    }
  } else {
    size_t n_components = 0, n_intervals = 0;
    LevelComponents(h, seg, seg_len, level, connectedness, nullptr, 0, &n_components, nullptr, 0, &n_intervals, nullptr,
                    VSG_MEM_DEVICE, true);
    p.n = (uint32_t)n_intervals;
    p.list = h->comp.intervals.As<Interval>();
    p.rank = h->comp.work.As<uint32_t>() + (size_t)5 * p.n;   // LevelComponents' comp_rank
    p.table = h->comp.table.As<int32_t>();
    p.table_words = kLevelComponentWords;
    cap_records = (uint32_t)n_components;
    p.records = cap_records;
    const vsg_render_component_stats& cs = h->comp.stats;
    ks.plane_us = h->stats.clear_us + h->stats.fill_us + cs.runs_us + cs.sort_us + cs.link_us + cs.order_us +
                  cs.label_us;
  }
  h->stats.launches += launches;
  ks.launches = h->stats.launches;
  ks.intervals = p.n;
  if ((p.n == 0) != (p.records == 0) || p.records > cap_records || p.records > p.n) {
    Throw(VSG_ERR_INTERNAL, "the level has other groups than the desc has ids for");
  }
  return p;
}

// Area and interval count of every record and the groups (may be null) on the stream.
void EnqueuePoolGroups(vsg_render* h, const PoolFront& p, bool has_component, int32_t* groups, int* launches) {
  using namespace vsg_render_impl;
  PoolStatus* status = h->pool.status.As<PoolStatus>();
  VSG_HIP(hipMemsetAsync(status, 0, sizeof(PoolStatus), h->stream));
  ++*launches;
  if (!p.n) return;
  VSG_HIP(hipMemsetAsync(h->pool.acc.p, 0, (size_t)p.records * 2 * sizeof(uint32_t), h->stream));
  LaunchPoolGroups(p.list, p.rank, p.n, p.records, h->pool.acc.As<uint32_t>(), p.table, p.table_words, has_component,
                   groups, status, h->stream);
  VSG_HIP(hipGetLastError());
  *launches += 3;
}

// The status words after the call's work has drained; the counts of the stats.
void ReadPoolStatus(vsg_render* h, const PoolFront& p, int* launches) {
  PoolSeen* seen = h->pool.seen.As<PoolSeen>();
  VSG_HIP(hipMemcpyAsync(&seen->status, h->pool.status.p, sizeof(PoolStatus), hipMemcpyDeviceToHost, h->stream));
  ++*launches;
  VSG_HIP(hipStreamSynchronize(h->stream));
  if ((seen->status.flags & vsg_render_impl::POOL_FLAG_RANGE) || seen->status.largest > p.n) {
    Throw(VSG_ERR_INTERNAL, "an interval's record is out of range");
  }
  vsg_render_pool_stats& ks = h->pool.stats;
  ks.groups = p.records;
  ks.covered = (int64_t)seen->status.covered;
  ks.largest_group_intervals = seen->status.largest;
}

void FinishPoolStats(vsg_render* h, int launches) {
  vsg_render_pool_stats& ks = h->pool.stats;
  float us[POOL_STAGES];
  h->pool.clock.Read(us, POOL_STAGES);
  ks.plane_us += us[POOL_UPLOAD];
  ks.sums_us = us[POOL_SUMS];
  ks.table_us = us[POOL_TABLE];
  ks.paint_us = us[POOL_PAINT];
  ks.launches += launches;
  h->stats.launches += launches;
  h->stats.device_allocations = h->allocations;
}

void LevelPool(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness, const void* features,
               const PoolLayout& layout, int mem_in, vsg_render_pool_group* groups, double* sum, double* sum_sq,
               float* mn, float* mx, size_t capacity_groups, size_t* num_groups, int mem_out) {
  using namespace vsg_render_impl;
  static_assert(sizeof(vsg_render_pool_group) == kPoolGroupWords * sizeof(int32_t), "moved as int32 words");
  static_assert(sizeof(vsg_render_pool_stats) == 64, "as the header says");
  static_assert(VSG_POOL_F32 == POOL_F32 && VSG_POOL_F16 == POOL_F16 && VSG_POOL_BF16 == POOL_BF16, "one numbering");
  CheckPoolDisjoint(h, layout, "features");
  const int mask = (sum ? POOL_SUM : 0) | (sum_sq ? POOL_SUM_SQ : 0) | (mn ? POOL_MIN : 0) | (mx ? POOL_MAX : 0);
  const bool any_out = groups || mask;
  if (!any_out && capacity_groups) Throw(VSG_ERR_INVALID, "every output is null");
  const bool count_only = !any_out;
  CheckFrameBelow2Pow32(h);
  DeviceGuard guard(h->device);
  vsg_render_pool_stats& ks = h->pool.stats;
  std::memset(&ks, 0, sizeof(ks));

  const PoolFront p = PoolFrontHalf(h, seg, seg_len, level, connectedness);
  const size_t R = p.records, C = (size_t)layout.channels;
  *num_groups = R;
  if (!count_only && R > capacity_groups) {
    Throw(VSG_ERR_INVALID, "the level has " + std::to_string(R) + " groups, the capacity is " +
                               std::to_string(capacity_groups));
  }

  // ---- blocks, all before anything that uses them is enqueued ----
  const bool host_out = !count_only && mem_out == VSG_MEM_HOST;
  const size_t cells = R * C;
  const size_t group_bytes = groups ? R * sizeof(vsg_render_pool_group) : 0;
  const size_t f64_bytes = cells * sizeof(double), f32_bytes = cells * sizeof(float);
  h->pool.acc.Reserve(R * 2 * sizeof(uint32_t), &h->allocations);
  PoolMatrices out{sum, sum_sq, mn, mx};
  int32_t* d_groups = reinterpret_cast<int32_t*>(groups);
  if (host_out) {
    h->pool.out.Reserve(group_bytes + 2 * f64_bytes + 2 * f32_bytes, &h->allocations);
    char* at = h->pool.out.As<char>();
    out.sum = sum ? reinterpret_cast<double*>(at) : nullptr;
    at += f64_bytes;
    out.sum_sq = sum_sq ? reinterpret_cast<double*>(at) : nullptr;
    at += f64_bytes;
    out.min = mn ? reinterpret_cast<float*>(at) : nullptr;
    at += f32_bytes;
    out.max = mx ? reinterpret_cast<float*>(at) : nullptr;
    at += f32_bytes;
    d_groups = groups ? reinterpret_cast<int32_t*>(at) : nullptr;
  }
  PoolMatrices spill{nullptr, nullptr, nullptr, nullptr};
  if (mask && p.n) {
    const size_t parts = (size_t)PoolSlices(p.n) * 2 * C;
    h->pool.spill.Reserve(parts * (2 * sizeof(double) + 2 * sizeof(float)), &h->allocations);
    char* at = h->pool.spill.As<char>();
    spill.sum = reinterpret_cast<double*>(at);
    spill.sum_sq = spill.sum + parts;
    spill.min = reinterpret_cast<float*>(spill.sum_sq + parts);
    spill.max = spill.min + parts;
  }
  int launches = 0;

  // ---- the features: where they are, or to the device with their strides ----
  h->pool.clock.Begin(h->stream);
  const void* d_features = features;
  if (mem_in == VSG_MEM_HOST && mask && p.n) {
    const size_t bytes = PoolSpanBytes(h, layout);
    char* to = StagePoolSpan(h, features, bytes);
    VSG_HIP(hipMemcpyAsync(to, features, bytes, hipMemcpyHostToDevice, h->stream));
    ++launches;
    d_features = to;
  }
  h->pool.clock.Mark(POOL_UPLOAD);

  // ---- sums ----
  if (mask && p.n) {
    LaunchPoolSums(p.list, p.rank, p.n, h->W, h->H, d_features, layout, mask, out, spill, h->stream);
    VSG_HIP(hipGetLastError());
    ++launches;
  }
  h->pool.clock.Mark(POOL_SUMS);
  if (mask && p.n) {
    LaunchPoolCombine(p.rank, p.n, layout.channels, mask, spill, out, h->stream);
    VSG_HIP(hipGetLastError());
    ++launches;
  }
  EnqueuePoolGroups(h, p, connectedness != 0, d_groups, &launches);
  h->pool.clock.Mark(POOL_TABLE);
  ReadPoolStatus(h, p, &launches);
  if (mask) ks.feature_bytes = ks.covered * (int64_t)C * (int64_t)PoolElementBytes(layout.dtype);
  if (host_out && R) {
    launches += DeliverToHost(h, &h->pool.seen, sizeof(PoolSeen),
                              {{out.sum, sum ? f64_bytes : 0, sum},
                               {out.sum_sq, sum_sq ? f64_bytes : 0, sum_sq},
                               {out.min, mn ? f32_bytes : 0, mn},
                               {out.max, mx ? f32_bytes : 0, mx},
                               {d_groups, group_bytes, groups}});
  }
  FinishPoolStats(h, launches);
}

void LevelUnpool(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness, const float* values,
                 size_t num_values, int mem_in, float fill, void* out, const PoolLayout& layout, int mem_out) {
  using namespace vsg_render_impl;
  CheckPoolDisjoint(h, layout, "out");
  CheckFrameBelow2Pow32(h);
  DeviceGuard guard(h->device);
  vsg_render_pool_stats& ks = h->pool.stats;
  std::memset(&ks, 0, sizeof(ks));
  const int W = h->W, H = h->H;

  const PoolFront p = PoolFrontHalf(h, seg, seg_len, level, connectedness);
  const size_t R = p.records, C = (size_t)layout.channels;
  if (num_values != R) {
    Throw(VSG_ERR_INVALID, "the level has " + std::to_string(R) + " groups, values has " + std::to_string(num_values));
  }
  if (R && !values) Throw(VSG_ERR_INVALID, "values is null");

  // ---- blocks ----
  const size_t value_bytes = R * C * sizeof(float);
  const size_t span = PoolSpanBytes(h, layout);
  h->pool.acc.Reserve(R * 2 * sizeof(uint32_t), &h->allocations);
  h->pool.intervals.Reserve((size_t)p.n * sizeof(Interval), &h->allocations);
  const float* d_values = values;
  void* d_out = out;
  int launches = 0;
  h->pool.clock.Begin(h->stream);
  if (mem_in == VSG_MEM_HOST && R) {
    h->pool.values.Reserve(value_bytes, &h->allocations);
    VSG_HIP(hipMemcpyAsync(h->pool.values.p, values, value_bytes, hipMemcpyHostToDevice, h->stream));
    ++launches;
    d_values = h->pool.values.As<float>();
  }
  if (mem_out == VSG_MEM_HOST) {
    // the span goes to the device as it is and comes back with the map's elements replaced: what lies between
    // them stays what it was
    d_out = StagePoolSpan(h, out, span);
    VSG_HIP(hipMemcpyAsync(d_out, out, span, hipMemcpyHostToDevice, h->stream));
    ++launches;
  }
  h->pool.clock.Mark(POOL_UPLOAD);
  EnqueuePoolGroups(h, p, connectedness != 0, nullptr, &launches);
  h->pool.clock.Mark(POOL_TABLE);

  // ---- the paint: every interval's record into the handle's plane, then the gather ----
  uint32_t* plane = h->d_plane.As<uint32_t>();
  Interval* painted = h->pool.intervals.As<Interval>();
  VSG_HIP(hipMemsetAsync(plane, 0, (size_t)h->pitch * H * sizeof(uint32_t), h->stream));
  LaunchPoolIntervals(p.list, p.rank, p.n, painted, h->stream);
  LaunchFill(painted, p.n, plane, h->pitch, h->stream);
  LaunchPoolGather(plane, h->pitch, W, H, d_values, (uint32_t)R, fill, d_out, layout, h->stream);
  VSG_HIP(hipGetLastError());
  launches += 2 + (p.n ? 2 : 0);
  h->pool.clock.Mark(POOL_PAINT);
  if (mem_out == VSG_MEM_HOST) {
    VSG_HIP(hipMemcpyAsync(out, d_out, span, hipMemcpyDeviceToHost, h->stream));
    ++launches;
  }
  ReadPoolStatus(h, p, &launches);
  FinishPoolStats(h, launches);
}

// The refusals of both calls that are answered before the handle is dereferenced, but for the layout's.
void CheckPoolArguments(const vsg_render* h, int connectedness, int mem_in, int mem_out) {
  if (!h) Throw(VSG_ERR_INVALID, "handle is null");
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

int vsg_render_level_pool(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness,
                          const void* features, int dtype, int channels, ptrdiff_t chan_stride, ptrdiff_t row_stride,
                          ptrdiff_t pixel_stride, int mem_in, vsg_render_pool_group* groups, double* sum,
                          double* sum_sq, float* min, float* max, size_t capacity_groups, size_t* num_groups,
                          int mem_out) {
  return Guard([&] {
    if (!num_groups) Throw(VSG_ERR_INVALID, "the count pointer is null");
    *num_groups = 0;
    if (!h) Throw(VSG_ERR_INVALID, "handle is null");
    if (!features) Throw(VSG_ERR_INVALID, "features is null");
    CheckPoolArguments(h, connectedness, mem_in, mem_out);
    const PoolLayout layout = CheckPoolLayout(features, "features", dtype, channels, chan_stride, row_stride,
                                              pixel_stride);
    LevelPool(h, seg, seg_len, level, connectedness, features, layout, mem_in, groups, sum, sum_sq, min, max,
              capacity_groups, num_groups, mem_out);
  });
}

int vsg_render_level_unpool(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness,
                            const float* values, size_t num_values, int channels, int mem_in, float fill, void* out,
                            int dtype, ptrdiff_t chan_stride, ptrdiff_t row_stride, ptrdiff_t pixel_stride,
                            int mem_out) {
  return Guard([&] {
    if (!h) Throw(VSG_ERR_INVALID, "handle is null");
    if (!out) Throw(VSG_ERR_INVALID, "out is null");
    if (!values && num_values) Throw(VSG_ERR_INVALID, "values is null");
    CheckPoolArguments(h, connectedness, mem_in, mem_out);
    const PoolLayout layout = CheckPoolLayout(out, "out", dtype, channels, chan_stride, row_stride, pixel_stride);
    LevelUnpool(h, seg, seg_len, level, connectedness, values, num_values, mem_in, fill, out, layout, mem_out);
  });
}

VSG_RENDER_LAST_STATS(vsg_render_last_pool_stats, vsg_render_pool_stats, pool.stats)

}  // extern "C"
