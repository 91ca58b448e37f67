// capi_level.inc -- what every call that maps a desc to a hierarchy level shares: ingest, the values of the
// regions, the id plane, its runs, their components, the level plane of the later families; and the entry
// points vsg_render_level_regions and vsg_render_level_components.  A part of render_capi.cpp.
namespace {

// Parses the desc, applies the hierarchy bookkeeping both entry points share (a desc that carries a
// hierarchy replaces the kept one) and returns the hierarchy to map ids with.
const Hierarchy& Ingest(vsg_render* h, const uint8_t* seg, size_t seg_len, bool* vector) {
  if (!seg && seg_len) Throw(VSG_ERR_INVALID, "seg is null");
  *vector = IsVectorOnly(seg, seg_len);
  ParseDesc(seg, seg_len, h->W, h->H, *vector, &h->desc, &h->intervals);
  if (!h->desc.hierarchy.empty()) h->kept = h->desc.hierarchy;
  return h->kept;
}

// Sets every interval's value to value_of(mapped id of its region); returns the distinct mapped ids.
template <class ValueOf>
int64_t AssignValues(vsg_render* h, int level, const Hierarchy& hier, ValueOf value_of) {
  std::unordered_map<int32_t, uint32_t> seen;   // one lookup and one colour per distinct id and frame
  const ParsedDesc& d = h->desc;
  for (size_t r = 0; r < d.region_ids.size(); ++r) {
    if (d.region_begin[r] == d.region_begin[r + 1]) continue;
    const int mapped = level > 0 ? ParentId(d.region_ids[r], level, hier) : d.region_ids[r];
    auto it = seen.find(mapped);
    if (it == seen.end()) it = seen.emplace(mapped, value_of(mapped)).first;
    for (size_t k = d.region_begin[r]; k < d.region_begin[r + 1]; ++k) h->intervals[k].value = it->second;
  }
  return (int64_t)seen.size();
}

// The same for a vector-only desc: one value per region that has a polygon, in h->vec.region_value.
template <class ValueOf>
int64_t AssignRegionValues(vsg_render* h, int level, const Hierarchy& hier, ValueOf value_of) {
  std::unordered_map<int32_t, uint32_t> seen;
  const ParsedDesc& d = h->desc;
  h->vec.region_value.assign(d.region_ids.size(), 0u);
  for (size_t r = 0; r < d.region_ids.size(); ++r) {
    if (d.region_poly_begin[r] == d.region_poly_begin[r + 1]) continue;
    const int mapped = level > 0 ? ParentId(d.region_ids[r], level, hier) : d.region_ids[r];
    auto it = seen.find(mapped);
    if (it == seen.end()) it = seen.emplace(mapped, value_of(mapped)).first;
    h->vec.region_value[r] = it->second;
  }
  return (int64_t)seen.size();
}

// The front half of vsg_render_id_image: ingests the desc, checks the level, maps every region to
// value_of(its id at `level`) and paints the W-pitched plane `ids` (device memory; -1 where no region
// is).  Leaves clock between STAGE_FILL and the next mark, and the vector path's status in flight:
// the caller calls CheckVector after its synchronisation when the desc was vector-only (returned).
// The plane's rows are `pitch` values apart, all of them cleared; ready() is called once every region has
// its value, before any device work.
template <class ValueOf, class Ready>
bool PaintIdsAt(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, uint32_t* ids, int pitch,
                ValueOf value_of, Ready ready) {
  const int H = h->H;
  std::memset(&h->stats, 0, sizeof(h->stats));
  std::memset(&h->vec.stats, 0, sizeof(h->vec.stats));
  const double t0 = NowMs();
  bool vector = false;
  const Hierarchy& hier = Ingest(h, seg, seg_len, &vector);
  if (level < 0 || (level > 0 && level >= (int)hier.size())) {
    Throw(VSG_ERR_INVALID, "level " + std::to_string(level) + " is not in the hierarchy (" +
                               std::to_string(hier.size()) + " levels)");
  }
  int64_t n_cross = 0;
  if (vector) {
    h->stats.distinct_ids = AssignRegionValues(h, level, hier, value_of);
    n_cross = h->BuildLines();
  } else {
    h->stats.distinct_ids = AssignValues(h, level, hier, value_of);
  }
  const int64_t n_intervals = vector ? n_cross / 2 : (int64_t)h->intervals.size();
  h->stats.intervals = n_intervals;
  ready();
  const double t1 = NowMs();
  h->stats.decode_ms = t1 - t0;
  if (vector) h->RunVector(n_cross);
  else h->UploadIntervals();
  const size_t bytes = (size_t)pitch * H * sizeof(int32_t);
  h->stats.upload_ms = NowMs() - t1;
  h->clock.Begin(h->stream);
  VSG_HIP(hipMemsetAsync(ids, 0xff, bytes, h->stream));   // -1: no region
  h->clock.Mark(STAGE_CLEAR);
  vsg_render_impl::LaunchFill(static_cast<const Interval*>(h->d_intervals.p), n_intervals, ids, pitch, h->stream);
  VSG_HIP(hipGetLastError());
  h->clock.Mark(STAGE_FILL);
  h->stats.launches += 1 + (n_intervals == 0 ? 0 : 1);
  return vector;
}

// The W-pitched plane of vsg_render_id_image and the level calls.
template <class ValueOf>
bool PaintIds(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, uint32_t* ids, ValueOf value_of) {
  return PaintIdsAt(h, seg, seg_len, level, ids, h->W, value_of, [] {});
}

// What the front half of the level calls leaves behind: n runs, unsorted (keys, rights) and, after
// SortLevelRuns, sorted with their regions' ranks, as intervals, and with id and first interval of every
// region in `regions`.
struct LevelFront {
  bool vector = false;
  uint32_t n = 0, cap_runs = 0, cap_regions = 0;
  int32_t max_id = 0;
  unsigned long long* keys = nullptr;
  uint32_t* rights = nullptr;
  LevelStatus* status = nullptr;
  unsigned long long* keys_sorted = nullptr;
  uint32_t* rights_sorted = nullptr;
  uint32_t* rank = nullptr;
  int32_t* regions = nullptr;
  Interval* intervals = nullptr;
};

// The id plane of the level calls in h->d_ids, as vsg_render_id_image paints it, with their rule for
// ids; *max_id receives the largest id.  Returns whether the desc was vector-only; the rest as PaintIds.
bool PaintLevelPlane(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int32_t* max_id) {
  h->d_ids.Reserve((size_t)h->W * h->H * sizeof(int32_t), &h->allocations);
  *max_id = 0;
  return PaintIds(h, seg, seg_len, level, h->d_ids.As<uint32_t>(), [&](int mapped) {
    // -1 is the plane's "no region"; the sort key takes the id as an unsigned number
    if (mapped < 0) Throw(VSG_ERR_INVALID, "region id " + std::to_string(mapped) + " is negative");
    *max_id = std::max(*max_id, mapped);
    return (uint32_t)mapped;
  });
}

// Paints the id plane as vsg_render_id_image does, finds its runs and waits for their number, which
// sizes everything after it.  Fills the run fields of *ls.
LevelFront PaintLevelRuns(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, vsg_render_level_stats* ls) {
  using namespace vsg_render_impl;
  const int W = h->W, H = h->H;
  LevelFront f;
  // ---- the id plane, as vsg_render_id_image paints it ----
  f.vector = PaintLevelPlane(h, seg, seg_len, level, &f.max_id);

  // ---- runs ----
  // Intervals that do not overlap give at most one run each; every end of an interval that lies
  // on another one can add a run.  The kernel drops what has no slot and says so.
  const uint64_t painted = (uint64_t)h->stats.intervals;
  const uint32_t cap_runs = (uint32_t)std::min<uint64_t>(2 * painted + 1, (uint64_t)W * H);
  h->lvl.runs.Reserve((size_t)cap_runs * 12, &h->allocations);
  h->lvl.status.Reserve(sizeof(LevelStatus), &h->allocations);
  h->lvl.seen.Reserve(2 * sizeof(LevelStatus), &h->allocations);
  f.cap_runs = cap_runs;
  f.keys = h->lvl.runs.As<unsigned long long>();
  f.rights = reinterpret_cast<uint32_t*>(f.keys + cap_runs);
  f.status = h->lvl.status.As<LevelStatus>();
  LevelStatus* seen = h->lvl.seen.As<LevelStatus>();   // [0] after the runs, [1] at the end
  VSG_HIP(hipMemsetAsync(f.status, 0, sizeof(LevelStatus), h->stream));
  h->lvl.clock.Begin(h->stream);
  LaunchLevelRuns(h->d_ids.As<int32_t>(), W, W, H, cap_runs, f.keys, f.rights, f.status, h->stream);
  VSG_HIP(hipGetLastError());
  h->lvl.clock.Mark(LVL_RUNS);
  VSG_HIP(hipMemcpyAsync(&seen[0], f.status, sizeof(LevelStatus), hipMemcpyDeviceToHost, h->stream));
  ls->launches = 3;
  VSG_HIP(hipStreamSynchronize(h->stream));   // the run count sizes everything below
  {
    float us[STAGE_COUNT], lus[LVL_COUNT];
    h->clock.Read(us, STAGE_COUNT);
    h->stats.clear_us = us[STAGE_CLEAR];
    h->stats.fill_us = us[STAGE_FILL];
    h->lvl.clock.Read(lus, LVL_COUNT);
    ls->runs_us = lus[LVL_RUNS];
  }
  if (f.vector) h->CheckVector();
  if (seen[0].overflow || seen[0].runs > cap_runs) Throw(VSG_ERR_INTERNAL, "more runs than the intervals allow");
  f.n = seen[0].runs;
  ls->runs = f.n;
  // every region has a run, and every id of the plane is one of the host's distinct mapped ids
  f.cap_regions = (uint32_t)std::min<uint64_t>(f.n, (uint64_t)h->stats.distinct_ids);
  return f;
}

// The n > 0 runs into (id, y, left_x) order, their regions' ranks, the interval list and the heads of
// the region table; restarts the level clock and leaves it after LVL_TABLE.
void SortLevelRuns(vsg_render* h, LevelFront* f, vsg_render_level_stats* ls) {
  using namespace vsg_render_impl;
  const uint32_t n = f->n;
  const int end_bit = 32 + BitsFor((uint64_t)f->max_id, 31);
  const size_t temp_bytes = LevelTempBytes(n, end_bit);
  h->d_sort_temp.Reserve(temp_bytes, &h->allocations);
  h->lvl.sorted.Reserve((size_t)n * 16, &h->allocations);
  h->lvl.regions.Reserve((size_t)f->cap_regions * sizeof(vsg_render_level_region), &h->allocations);
  h->lvl.intervals.Reserve((size_t)n * sizeof(Interval), &h->allocations);
  f->keys_sorted = h->lvl.sorted.As<unsigned long long>();
  f->rights_sorted = reinterpret_cast<uint32_t*>(f->keys_sorted + n);
  f->rank = f->rights_sorted + n;
  f->regions = h->lvl.regions.As<int32_t>();
  f->intervals = h->lvl.intervals.As<Interval>();
  h->lvl.clock.Begin(h->stream);
  VSG_HIP(SortPairsU64U32(h->d_sort_temp.p, temp_bytes, f->keys, f->keys_sorted, f->rights, f->rights_sorted, n,
                          end_bit, h->stream));
  h->lvl.clock.Mark(LVL_SORT);
  VSG_HIP(HeadScan(h->d_sort_temp.p, temp_bytes, HeadFlag{f->keys_sorted}, f->rank, n, h->stream));
  LaunchLevelTable(f->keys_sorted, f->rights_sorted, f->rank, n, h->W, f->cap_regions, f->intervals, f->regions,
                   f->status, h->stream);
  VSG_HIP(hipGetLastError());
  h->lvl.clock.Mark(LVL_TABLE);
  ls->launches += 3;   // the sort and the scan count as one each
}

// vsg_render_level_components behind its argument checks.  labels_only: the call is made for
// vsg_render_level_boundaries, which needs the label image in h->comp.labels and id and component of every
// entry of h->comp.table and nothing else: no output is looked at, no capacity is checked, the moments
// are not computed and nothing is delivered but the two counts.
void LevelComponents(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness,
                     vsg_render_level_component* components, size_t capacity_components, size_t* num_components,
                     int32_t* intervals, size_t capacity_intervals, size_t* num_intervals, int32_t* label_image,
                     int mem_out, bool labels_only) {
  using namespace vsg_render_impl;
  CheckMem(mem_out, "outputs");
  const bool count_only = !labels_only && !components && !intervals && !label_image && capacity_components == 0 &&
                          capacity_intervals == 0;
  const bool paint_labels = labels_only || label_image;
  const int W = h->W, H = h->H;
  CheckFrameBelow2Pow32(h);
  DeviceGuard guard(h->device);
  vsg_render_component_stats& cs = h->comp.stats;
  std::memset(&cs, 0, sizeof(cs));
  vsg_render_level_stats ls;   // of the shared front half; the last level_regions call's stay
  std::memset(&ls, 0, sizeof(ls));

  LevelFront f = PaintLevelRuns(h, seg, seg_len, level, &ls);
  const uint32_t n = f.n;
  *num_intervals = n;
  cs.runs = n;
  cs.runs_us = ls.runs_us;
  if (!count_only && !labels_only && n && n <= capacity_intervals && (!components || !intervals)) {
    Throw(VSG_ERR_INVALID, "an output is null");
  }
  h->comp.status.Reserve(sizeof(CompStatus), &h->allocations);
  h->comp.seen.Reserve(2 * sizeof(CompStatus) + sizeof(LevelStatus), &h->allocations);
  CompStatus* status = h->comp.status.As<CompStatus>();
  CompStatus* seen = h->comp.seen.As<CompStatus>();   // [0] once the table is made, [1] at the end
  LevelStatus* seen_level = reinterpret_cast<LevelStatus*>(seen + 2);
  std::memset(seen, 0, 2 * sizeof(CompStatus) + sizeof(LevelStatus));
  Interval* ordered = nullptr;
  Interval* fill = nullptr;
  int32_t* table = nullptr;
  int launches = 0;
  if (!n) h->comp.clock.Begin(h->stream);   // an empty frame still clears the label image
  if (n) {
    // ---- the runs sorted by (id, y, left_x), as vsg_render_level_regions has them ----
    const int label_bits = BitsFor((uint64_t)(n - 1), 32);
    const size_t temp_bytes = MaxBytes({SortPairsU32U32TempBytes(n, label_bits), HeadScanTempBytes<LabelHead>(n)});
    h->d_sort_temp.Reserve(temp_bytes, &h->allocations);   // before anything that uses the block is enqueued
    SortLevelRuns(h, &f, &ls);

    // ---- union-find, order, table ----
    h->comp.work.Reserve((size_t)n * 6 * sizeof(uint32_t), &h->allocations);
    h->comp.table.Reserve((size_t)n * sizeof(vsg_render_level_component), &h->allocations);
    h->comp.intervals.Reserve((size_t)n * sizeof(Interval), &h->allocations);
    h->comp.first.Reserve((size_t)f.cap_regions * sizeof(uint32_t), &h->allocations);
    if (paint_labels) h->comp.fill.Reserve((size_t)n * sizeof(Interval), &h->allocations);
    uint32_t* parent = h->comp.work.As<uint32_t>();
    uint32_t* label = parent + n;
    uint32_t* index = label + n;
    uint32_t* label_sorted = index + n;
    uint32_t* order = label_sorted + n;
    uint32_t* comp_rank = order + n;
    ordered = h->comp.intervals.As<Interval>();
    fill = paint_labels ? h->comp.fill.As<Interval>() : nullptr;
    table = h->comp.table.As<int32_t>();
    VSG_HIP(hipMemsetAsync(status, 0, sizeof(CompStatus), h->stream));
    h->comp.clock.Begin(h->stream);
    LaunchCompLink(f.keys_sorted, f.rights_sorted, n, W, connectedness == VSG_RENDER_CONNECT_N8 ? 1 : 0, parent,
                   label, index, status, h->stream);
    VSG_HIP(hipGetLastError());
    h->comp.clock.Mark(CMP_LINK);
    VSG_HIP(SortPairsU32U32(h->d_sort_temp.p, temp_bytes, label, label_sorted, index, order, n, label_bits, h->stream));
    VSG_HIP(HeadScan(h->d_sort_temp.p, temp_bytes, LabelHead{label_sorted}, comp_rank, n, h->stream));
    // a run has at most one component: n slots hold them all
    LaunchCompTable(label_sorted, order, comp_rank, f.rank, f.intervals, n, n, f.cap_regions, ordered, fill, table,
                    h->comp.first.As<uint32_t>(), f.status, status, h->stream);
    VSG_HIP(hipGetLastError());
    h->comp.clock.Mark(CMP_ORDER);
    VSG_HIP(hipMemcpyAsync(&seen[0], status, sizeof(CompStatus), hipMemcpyDeviceToHost, h->stream));
    VSG_HIP(hipMemcpyAsync(seen_level, f.status, sizeof(LevelStatus), hipMemcpyDeviceToHost, h->stream));
    launches += 11;   // the clear, five kernels, two copies; the sorts and the scans count as one each
    VSG_HIP(hipStreamSynchronize(h->stream));   // the number of components decides what is delivered
    if (seen_level->regions == 0 || seen_level->regions > f.cap_regions) {
      Throw(VSG_ERR_INTERNAL, "the plane has more regions than the desc has ids");
    }
    if (seen[0].flags & COMP_FLAG_BOUND) Throw(VSG_ERR_INTERNAL, "the union-find did not end within its bound");
    if ((seen[0].flags & COMP_FLAG_DROPPED) || seen[0].components == 0 || seen[0].components > n) {
      Throw(VSG_ERR_INTERNAL, "a component had no slot");
    }
  }
  const uint32_t n_components = seen[0].components;
  *num_components = n_components;
  cs.regions = seen_level->regions;
  cs.components = n_components;
  cs.links = (int64_t)seen[0].links;
  auto finish = [&] {
    float us[CMP_COUNT], lus[LVL_COUNT];
    h->comp.clock.Read(us, CMP_COUNT);
    cs.link_us = us[CMP_LINK];
    cs.order_us = us[CMP_ORDER];
    cs.moments_us = us[CMP_MOMENTS];
    cs.label_us = us[CMP_LABEL];
    if (n) {
      h->lvl.clock.Read(lus, LVL_COUNT);
      cs.sort_us = lus[LVL_SORT] + lus[LVL_TABLE];
    }
    cs.launches = ls.launches + launches;
    h->stats.launches += cs.launches;
    h->stats.device_allocations = h->allocations;
  };
  if (count_only) {
    finish();
    return;
  }
  if (!labels_only && (n > capacity_intervals || n_components > capacity_components)) {
    finish();
    Throw(VSG_ERR_INVALID, "the level has " + std::to_string(n_components) + " components and " +
                               std::to_string(n) + " intervals, the capacities are " +
                               std::to_string(capacity_components) + " and " + std::to_string(capacity_intervals));
  }

  // ---- moments, label image, outputs ----
  if (n) h->comp.clock.Mark(CMP_WAIT);
  const hipMemcpyKind kind = mem_out == VSG_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  if (n && !labels_only) {
    LaunchComponentMoments(ordered, n, n_components, table, status, h->stream);
    VSG_HIP(hipGetLastError());
    h->comp.clock.Mark(CMP_MOMENTS);
    ++launches;
  }
  if (paint_labels) {
    const size_t bytes = (size_t)W * H * sizeof(int32_t);
    uint32_t* plane = reinterpret_cast<uint32_t*>(label_image);   // device output: painted in place
    if (labels_only || mem_out == VSG_MEM_HOST) {
      h->comp.labels.Reserve(bytes, &h->allocations);
      plane = h->comp.labels.As<uint32_t>();
    }
    VSG_HIP(hipMemsetAsync(plane, 0xff, bytes, h->stream));   // -1: no component
    LaunchFill(fill, n, plane, W, h->stream);
    VSG_HIP(hipGetLastError());
    h->comp.clock.Mark(CMP_LABEL);
    launches += 1 + (n ? 1 : 0);
    if (!labels_only && mem_out == VSG_MEM_HOST) {
      VSG_HIP(hipMemcpyAsync(label_image, plane, bytes, hipMemcpyDeviceToHost, h->stream));
      ++launches;
    }
  }
  if (n && !labels_only) {
    VSG_HIP(hipMemcpyAsync(components, table, (size_t)n_components * sizeof(vsg_render_level_component), kind,
                           h->stream));
    VSG_HIP(hipMemcpyAsync(intervals, ordered, (size_t)n * sizeof(Interval), kind, h->stream));
    VSG_HIP(hipMemcpyAsync(&seen[1], status, sizeof(CompStatus), hipMemcpyDeviceToHost, h->stream));
    launches += 3;
  }
  VSG_HIP(hipStreamSynchronize(h->stream));
  cs.largest_component_intervals = seen[1].largest;
  finish();
}

// The plane the boundary, adjacency, overlap and contour families classify: the level's ids, or the indices of
// its regions' components, whose id and component comp_table then holds.
struct LevelPlane {
  const int32_t* plane = nullptr;
  const int32_t* comp_table = nullptr;
  uint32_t max_group = 0;
  uint64_t groups_bound = 0;   // no more groups than this
  bool vector = false;         // the desc was vector-only: CheckVector is due after the synchronisation
  bool by_components = false;
};

// Makes the plane.  The ids are painted on the stream and not waited for (FinishLevelPlane, after the caller's
// first synchronisation); the components' call has ended, its time is in *plane_us.  *launches: the handle's
// count so far, as every family starts its own.
LevelPlane SelectLevelPlane(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness,
                            float* plane_us, int* launches) {
  LevelPlane lp;
  lp.by_components = connectedness != 0;
  if (!lp.by_components) {
    int32_t max_id = 0;
    lp.vector = PaintLevelPlane(h, seg, seg_len, level, &max_id);
    lp.plane = h->d_ids.As<int32_t>();
    lp.max_group = (uint32_t)max_id;
    lp.groups_bound = (uint64_t)h->stats.distinct_ids;
  } else {
    size_t n_components = 0, n_intervals = 0;
    LevelComponents(h, seg, seg_len, level, connectedness, nullptr, 0, &n_components, nullptr, 0, &n_intervals,
                    nullptr, VSG_MEM_DEVICE, true);
    lp.plane = h->comp.labels.As<int32_t>();
    lp.comp_table = h->comp.table.As<int32_t>();
    lp.max_group = n_components ? (uint32_t)(n_components - 1) : 0u;
    lp.groups_bound = n_components;
    const vsg_render_component_stats& cs = h->comp.stats;
    *plane_us = h->stats.clear_us + h->stats.fill_us + cs.runs_us + cs.sort_us + cs.link_us + cs.order_us +
                cs.label_us;
  }
  *launches = h->stats.launches;
  return lp;
}

// After the synchronisation that followed SelectLevelPlane: the times of a painted plane, the vector path's flag.
void FinishLevelPlane(vsg_render* h, const LevelPlane& lp, float* plane_us) {
  if (lp.by_components) return;
  float us[STAGE_COUNT];
  h->clock.Read(us, STAGE_COUNT);
  h->stats.clear_us = us[STAGE_CLEAR];
  h->stats.fill_us = us[STAGE_FILL];
  *plane_us = us[STAGE_CLEAR] + us[STAGE_FILL];
  if (lp.vector) h->CheckVector();
}

}  // namespace

extern "C" {

int vsg_render_level_regions(vsg_render* h, const uint8_t* seg, size_t seg_len, int level,
                             vsg_render_level_region* regions, size_t capacity_regions, size_t* num_regions,
                             int32_t* intervals, size_t capacity_intervals, size_t* num_intervals, int mem_out) {
  return Guard([&] {
    using namespace vsg_render_impl;
    static_assert(sizeof(vsg_render_level_region) == kLevelRegionWords * sizeof(int32_t), "moved as int32 words");
    if (!h) Throw(VSG_ERR_INVALID, "handle is null");
    if (!num_regions || !num_intervals) Throw(VSG_ERR_INVALID, "a count pointer is null");
    *num_regions = *num_intervals = 0;
    CheckMem(mem_out, "outputs");
    const bool count_only = !regions && !intervals && capacity_regions == 0 && capacity_intervals == 0;
    CheckFrameBelow2Pow32(h);
    DeviceGuard guard(h->device);
    std::memset(&h->lvl.stats, 0, sizeof(h->lvl.stats));

    LevelFront f = PaintLevelRuns(h, seg, seg_len, level, &h->lvl.stats);
    const uint32_t n = f.n;
    *num_intervals = n;

    // ---- sort, table, moments, outputs ----
    const uint32_t cap_regions = f.cap_regions;
    const bool intervals_fit = n <= capacity_intervals;
    const bool deliver = !count_only && intervals_fit;
    const size_t region_bytes = (size_t)cap_regions * sizeof(vsg_render_level_region);
    const size_t interval_bytes = (size_t)n * sizeof(Interval);
    if (deliver && n && (!regions || !intervals)) Throw(VSG_ERR_INVALID, "an output is null");
    if (n) {
      SortLevelRuns(h, &f, &h->lvl.stats);
      LevelStatus* status = f.status;
      LevelStatus* seen = h->lvl.seen.As<LevelStatus>();
      int32_t* d_regions = f.regions;
      Interval* d_intervals = f.intervals;
      if (!count_only) {
        LaunchLevelMoments(d_intervals, n, cap_regions, d_regions, status, h->stream);
        VSG_HIP(hipGetLastError());
        h->lvl.clock.Mark(LVL_MOMENTS);
        ++h->lvl.stats.launches;
      }
      if (deliver && mem_out == VSG_MEM_DEVICE) {
        // the number of regions is on the device: the copy decides there whether they fit
        CopyLists lists = {};
        lists.list[0] = {d_regions, reinterpret_cast<int32_t*>(regions), kLevelRegionWords, &status->regions, 0,
                         (uint32_t)std::min<size_t>(capacity_regions, cap_regions)};
        lists.list[1] = {reinterpret_cast<const int32_t*>(d_intervals), intervals, 4, nullptr, n, n};
        LaunchCopyLists(lists, h->stream);
        VSG_HIP(hipGetLastError());
        ++h->lvl.stats.launches;
      } else if (deliver) {
        // through the pinned block; handed to the caller once the number of regions is known
        h->lvl.seen.Reserve(2 * sizeof(LevelStatus) + region_bytes + interval_bytes, &h->allocations);
        seen = h->lvl.seen.As<LevelStatus>();
        char* stage = reinterpret_cast<char*>(seen + 2);
        VSG_HIP(hipMemcpyAsync(stage, d_regions, region_bytes, hipMemcpyDeviceToHost, h->stream));
        VSG_HIP(hipMemcpyAsync(stage + region_bytes, d_intervals, interval_bytes, hipMemcpyDeviceToHost, h->stream));
        h->lvl.stats.launches += 2;
      }
      VSG_HIP(hipMemcpyAsync(&seen[1], status, sizeof(LevelStatus), hipMemcpyDeviceToHost, h->stream));
      ++h->lvl.stats.launches;
      VSG_HIP(hipStreamSynchronize(h->stream));
      if (seen[1].regions == 0 || seen[1].regions > cap_regions) {
        Throw(VSG_ERR_INTERNAL, "the plane has more regions than the desc has ids");
      }
      float us[LVL_COUNT];
      h->lvl.clock.Read(us, LVL_COUNT);
      h->lvl.stats.sort_us = us[LVL_SORT];
      h->lvl.stats.table_us = us[LVL_TABLE];
      h->lvl.stats.moments_us = us[LVL_MOMENTS];
      h->lvl.stats.regions = seen[1].regions;
      h->lvl.stats.largest_region_intervals = seen[1].largest;
    }
    h->stats.launches += h->lvl.stats.launches;
    h->stats.device_allocations = h->allocations;
    const size_t n_regions = (size_t)h->lvl.stats.regions;
    *num_regions = n_regions;
    if (count_only) return;
    if (!intervals_fit || n_regions > capacity_regions) {
      Throw(VSG_ERR_INVALID, "the level has " + std::to_string(n_regions) + " regions and " + std::to_string(n) +
                                 " intervals, the capacities are " + std::to_string(capacity_regions) + " and " +
                                 std::to_string(capacity_intervals));
    }
    if (n && mem_out == VSG_MEM_HOST) {
      const char* stage = reinterpret_cast<const char*>(h->lvl.seen.As<LevelStatus>() + 2);
      std::memcpy(regions, stage, n_regions * sizeof(vsg_render_level_region));
      std::memcpy(intervals, stage + region_bytes, interval_bytes);
    }
  });
}

VSG_RENDER_LAST_STATS(vsg_render_last_level_stats, vsg_render_level_stats, lvl.stats)

int vsg_render_level_components(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness,
                                vsg_render_level_component* components, size_t capacity_components,
                                size_t* num_components, int32_t* intervals, size_t capacity_intervals,
                                size_t* num_intervals, int32_t* label_image, int mem_out) {
  return Guard([&] {
    using namespace vsg_render_impl;
    static_assert(sizeof(vsg_render_level_component) == kLevelComponentWords * sizeof(int32_t), "moved as int32 words");
    CheckConnectedness(connectedness, false);
    if (!h) Throw(VSG_ERR_INVALID, "handle is null");
    if (!num_components || !num_intervals) Throw(VSG_ERR_INVALID, "a count pointer is null");
    *num_components = *num_intervals = 0;
    LevelComponents(h, seg, seg_len, level, connectedness, components, capacity_components, num_components, intervals,
                    capacity_intervals, num_intervals, label_image, mem_out, false);
  });
}

VSG_RENDER_LAST_STATS(vsg_render_last_component_stats, vsg_render_component_stats, comp.stats)

}  // extern "C"
