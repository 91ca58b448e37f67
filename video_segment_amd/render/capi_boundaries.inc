// capi_boundaries.inc -- vsg_render_level_boundaries.  A part of render_capi.cpp.
extern "C" {

int vsg_render_level_boundaries(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness,
                                int which, vsg_render_level_boundary* boundaries, size_t capacity_boundaries,
                                size_t* num_boundaries, int32_t* points, size_t capacity_points, size_t* num_points,
                                int mem_out) {
  return Guard([&] {
    using namespace vsg_render_impl;
    static_assert(sizeof(vsg_render_level_boundary) == kLevelBoundaryWords * sizeof(int32_t), "moved as int32 words");
    CheckConnectedness(connectedness, true);
    if (which != VSG_RENDER_BOUNDARY_INNER && which != VSG_RENDER_BOUNDARY_OUTER) {
      Throw(VSG_ERR_INVALID, "which is neither VSG_RENDER_BOUNDARY_INNER nor VSG_RENDER_BOUNDARY_OUTER");
    }
    if (!h) Throw(VSG_ERR_INVALID, "handle is null");
    if (!num_boundaries || !num_points) Throw(VSG_ERR_INVALID, "a count pointer is null");
    *num_boundaries = *num_points = 0;
    CheckMem(mem_out, "outputs");
    const bool count_only = !boundaries && !points && capacity_boundaries == 0 && capacity_points == 0;
    const bool outer = which == VSG_RENDER_BOUNDARY_OUTER;
    const int W = h->W, H = h->H;
    CheckFrameBelow2Pow32(h);
    DeviceGuard guard(h->device);
    vsg_render_boundary_stats& bs = h->bound.stats;
    std::memset(&bs, 0, sizeof(bs));

    // ---- the plane: the level's ids, or the indices of its regions' components ----
    const LevelPlane lp = SelectLevelPlane(h, seg, seg_len, level, connectedness, &bs.plane_us, &bs.launches);

    // ---- count: the number of points sizes everything below ----
    // seen: [0] after the count, [1] at the end
    auto [status, seen] = ReserveStatusPair<BoundStatus>(h, &h->bound.status, &h->bound.seen);
    VSG_HIP(hipMemsetAsync(status, 0, sizeof(BoundStatus), h->stream));
    h->bound.clock.Begin(h->stream);
    LaunchBoundClassify(lp.plane, W, H, outer, false, 0, nullptr, status, h->stream);
    VSG_HIP(hipGetLastError());
    h->bound.clock.Mark(BND_COUNT);
    VSG_HIP(hipMemcpyAsync(&seen[0], status, sizeof(BoundStatus), hipMemcpyDeviceToHost, h->stream));
    int launches = 3;
    VSG_HIP(hipStreamSynchronize(h->stream));
    {
      float us[BND_STAGES];
      h->bound.clock.Read(us, BND_STAGES);
      bs.count_us = us[BND_COUNT];
    }
    FinishLevelPlane(h, lp, &bs.plane_us);
    auto finish = [&] { CountLaunches(h, &bs.launches, launches); };
    if (seen[0].points > 0x7fffffffull) {
      finish();
      Throw(VSG_ERR_INVALID, "the level has more than 2^31 - 1 boundary points");
    }
    const uint32_t n = (uint32_t)seen[0].points;
    *num_points = n;
    bs.points = n;
    if (n == 0) return finish();   // no group at all: both lists are empty

    // ---- emit, sort, table ----
    const uint32_t cap_records = (uint32_t)std::min<uint64_t>(lp.groups_bound, n);   // every group has a point
    if (cap_records == 0) Throw(VSG_ERR_INTERNAL, "the plane has groups the desc has no ids for");
    const bool points_fit = n <= capacity_points;
    const bool deliver = !count_only && points_fit;
    if (deliver && (!boundaries || !points)) Throw(VSG_ERR_INVALID, "an output is null");
    const int end_bit = 32 + BitsFor(lp.max_group, 32);
    const size_t temp_bytes = MaxBytes({SortKeysU64TempBytes(n, end_bit), LevelTempBytes(n, end_bit)});
    const size_t record_bytes = (size_t)cap_records * sizeof(vsg_render_level_boundary);
    const size_t point_bytes = (size_t)n * 2 * sizeof(int32_t);
    h->d_sort_temp.Reserve(temp_bytes, &h->allocations);
    h->bound.keys.Reserve((size_t)n * 2 * sizeof(unsigned long long), &h->allocations);
    h->bound.rank.Reserve((size_t)n * sizeof(uint32_t), &h->allocations);
    h->bound.points.Reserve(point_bytes, &h->allocations);
    h->bound.records.Reserve(record_bytes, &h->allocations);
    unsigned long long* keys = h->bound.keys.As<unsigned long long>();
    unsigned long long* keys_sorted = keys + n;
    uint32_t* rank = h->bound.rank.As<uint32_t>();
    int32_t* d_points = h->bound.points.As<int32_t>();
    int32_t* d_records = h->bound.records.As<int32_t>();
    h->bound.clock.Begin(h->stream);
    LaunchBoundClassify(lp.plane, W, H, outer, true, n, keys, status, h->stream);
    VSG_HIP(hipGetLastError());
    h->bound.clock.Mark(BND_EMIT);
    VSG_HIP(SortKeysU64(h->d_sort_temp.p, temp_bytes, keys, keys_sorted, n, end_bit, h->stream));
    h->bound.clock.Mark(BND_SORT);
    VSG_HIP(HeadScan(h->d_sort_temp.p, temp_bytes, HeadFlag{keys_sorted}, rank, n, h->stream));
    LaunchBoundTable(keys_sorted, rank, n, W, H, lp.max_group, cap_records, lp.comp_table, d_points, d_records, status,
                     h->stream);
    VSG_HIP(hipGetLastError());
    h->bound.clock.Mark(BND_TABLE);
    launches += 5;   // emit, the sort and the scan counted as one each, table, finish
    if (deliver && mem_out == VSG_MEM_DEVICE) {
      // the number of boundaries is on the device: the copy decides there whether they fit
      CopyLists lists = {};
      lists.list[0] = {d_records, reinterpret_cast<int32_t*>(boundaries), kLevelBoundaryWords, &status->boundaries, 0,
                       (uint32_t)std::min<size_t>(capacity_boundaries, cap_records)};
      lists.list[1] = {d_points, points, 2, nullptr, n, n};
      lists.flags = &status->flags;
      LaunchCopyLists(lists, h->stream);
      VSG_HIP(hipGetLastError());
      ++launches;
    } else if (deliver) {
      // through the pinned block; handed to the caller once the number of boundaries is known
      h->bound.seen.Reserve(2 * sizeof(BoundStatus) + record_bytes + point_bytes, &h->allocations);
      seen = h->bound.seen.As<BoundStatus>();
      char* stage = reinterpret_cast<char*>(seen + 2);
      VSG_HIP(hipMemcpyAsync(stage, d_records, record_bytes, hipMemcpyDeviceToHost, h->stream));
      VSG_HIP(hipMemcpyAsync(stage + record_bytes, d_points, point_bytes, hipMemcpyDeviceToHost, h->stream));
      launches += 2;
    }
    VSG_HIP(hipMemcpyAsync(&seen[1], status, sizeof(BoundStatus), hipMemcpyDeviceToHost, h->stream));
    ++launches;
    VSG_HIP(hipStreamSynchronize(h->stream));
    {
      float us[BND_STAGES];
      h->bound.clock.Read(us, BND_STAGES);
      bs.emit_us = us[BND_EMIT];
      bs.sort_us = us[BND_SORT];
      bs.table_us = us[BND_TABLE];
    }
    finish();
    if ((seen[1].flags & BOUND_FLAG_OVERFLOW) || seen[1].emitted != n) {
      Throw(VSG_ERR_INTERNAL, "the emit pass found other boundary points than the count pass");
    }
    if ((seen[1].flags & BOUND_FLAG_RANGE) || seen[1].boundaries == 0 || seen[1].boundaries > cap_records ||
        (lp.comp_table && seen[1].boundaries != lp.groups_bound)) {
      Throw(VSG_ERR_INTERNAL, "a sorted boundary key or a boundary record is out of range");
    }
    const size_t n_boundaries = seen[1].boundaries;
    *num_boundaries = n_boundaries;
    bs.boundaries = (int64_t)n_boundaries;
    bs.largest_boundary_points = seen[1].largest;
    if (count_only) return;
    if (!points_fit || n_boundaries > capacity_boundaries) {
      Throw(VSG_ERR_INVALID, "the level has " + std::to_string(n_boundaries) + " boundaries and " + std::to_string(n) +
                                 " points, the capacities are " + std::to_string(capacity_boundaries) + " and " +
                                 std::to_string(capacity_points));
    }
    if (mem_out == VSG_MEM_HOST) {
      const char* stage = reinterpret_cast<const char*>(h->bound.seen.As<BoundStatus>() + 2);
      std::memcpy(boundaries, stage, n_boundaries * sizeof(vsg_render_level_boundary));
      std::memcpy(points, stage + record_bytes, point_bytes);
    }
  });
}

VSG_RENDER_LAST_STATS(vsg_render_last_boundary_stats, vsg_render_boundary_stats, bound.stats)

}  // extern "C"
