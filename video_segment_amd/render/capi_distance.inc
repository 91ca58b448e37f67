// capi_distance.inc -- vsg_render_boundary_distance and vsg_render_boundary_benchmark.  A part of render_capi.cpp,
// after capi_persistence.inc.
extern "C" {

int vsg_render_boundary_distance(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int32_t* out,
                                 int mem_out) {
  return Guard([&] {
    using namespace vsg_render_impl;
    static_assert(VSG_RENDER_DISTANCE_NONE == kDistanceNone, "the kernels' none is the header's");
    if (!h) Throw(VSG_ERR_INVALID, "handle is null");
    if (!out) Throw(VSG_ERR_INVALID, "out is null");
    CheckMem(mem_out, "out");
    const int W = h->W, H = h->H;
    const size_t n = (size_t)W * H, bytes = n * sizeof(int32_t);
    DeviceGuard guard(h->device);
    vsg_render_distance_stats& ds = h->dist.stats;
    std::memset(&ds, 0, sizeof(ds));

    // ---- P, as vsg_render_id_image paints it, and its edge set ----
    h->d_ids.Reserve(bytes, &h->allocations);
    const bool vector = PaintIds(h, seg, seg_len, level, h->d_ids.As<uint32_t>(),
                                 [](int mapped) { return (uint32_t)mapped; });
    h->dist.words.Reserve((size_t)DistChunks(H) * W * sizeof(uint32_t), &h->allocations);
    // seen: [0] after the classify pass, [1] at the end
    auto [status, seen] = ReserveStatusPair<DistStatus>(h, &h->dist.status, &h->dist.seen);
    uint32_t* words = h->dist.words.As<uint32_t>();
    VSG_HIP(hipMemsetAsync(status, 0, sizeof(DistStatus), h->stream));
    h->dist.clock.Begin(h->stream);
    LaunchDistClassify(h->d_ids.As<int32_t>(), (size_t)W, W, H, false, words, status, h->stream);
    VSG_HIP(hipGetLastError());
    h->dist.clock.Mark(DST_CLASSIFY);
    VSG_HIP(hipMemcpyAsync(&seen[0], status, sizeof(DistStatus), hipMemcpyDeviceToHost, h->stream));
    int launches = 3;
    h->FinishStats();   // the number of edge pixels decides what runs below
    if (vector) h->CheckVector();
    float us[DST_STAGES];
    h->dist.clock.Read(us, DST_STAGES);
    ds.plane_us = h->stats.clear_us + h->stats.fill_us;
    ds.classify_us = us[DST_CLASSIFY];
    ds.edge_pixels = (int64_t)seen[0].edge_pixels;

    if (ds.edge_pixels == 0) {
      // ---- no edge: none everywhere ----
      if (mem_out == VSG_MEM_HOST) {
        std::fill(out, out + n, (int32_t)VSG_RENDER_DISTANCE_NONE);
      } else {
        VSG_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(out), VSG_RENDER_DISTANCE_NONE, n, h->stream));
        VSG_HIP(hipStreamSynchronize(h->stream));
        ++launches;
      }
    } else {
      // ---- columns, then rows ----
      h->dist.gsq.Reserve(bytes, &h->allocations);
      int32_t* d = out;   // device output: written in place
      if (mem_out == VSG_MEM_HOST) {
        h->dist.out.Reserve(bytes, &h->allocations);
        d = h->dist.out.As<int32_t>();
      }
      h->dist.clock.Begin(h->stream);
      LaunchDistColumns(words, W, H, h->dist.gsq.As<int32_t>(), h->stream);
      VSG_HIP(hipGetLastError());
      h->dist.clock.Mark(DST_COLUMNS);
      VSG_HIP(LaunchDistRows(h->dist.gsq.As<int32_t>(), W, H, d, status, h->stream));
      h->dist.clock.Mark(DST_ROWS);
      launches += 3;
      if (mem_out == VSG_MEM_HOST) {
        VSG_HIP(hipMemcpyAsync(out, d, bytes, hipMemcpyDeviceToHost, h->stream));
        ++launches;
      }
      VSG_HIP(hipMemcpyAsync(&seen[1], status, sizeof(DistStatus), hipMemcpyDeviceToHost, h->stream));
      VSG_HIP(hipStreamSynchronize(h->stream));
      h->dist.clock.Read(us, DST_STAGES);
      ds.columns_us = us[DST_COLUMNS];
      ds.rows_us = us[DST_ROWS];
      ds.max_distance = (int64_t)seen[1].max_distance;
    }
    h->stats.launches += launches;
    h->stats.device_allocations = h->allocations;
    ds.launches = h->stats.launches;
  });
}

int vsg_render_boundary_benchmark(vsg_render* h, const uint8_t* seg, size_t seg_len, const int32_t* other,
                                  size_t other_pitch, int mem_other, int tolerance_sq,
                                  vsg_render_boundary_score* scores, size_t capacity_levels, size_t* num_levels,
                                  int mem_out) {
  return Guard([&] {
    using namespace vsg_render_impl;
    static_assert(sizeof(vsg_render_boundary_score) == kBoundaryScoreWords * sizeof(int64_t), "moved as int64 words");
    if (!h) Throw(VSG_ERR_INVALID, "handle is null");
    if (!num_levels) Throw(VSG_ERR_INVALID, "the count pointer is null");
    CheckOtherPlane(other, mem_other);
    CheckMem(mem_out, "scores");
    if (tolerance_sq < 0 || tolerance_sq > VSG_RENDER_MAX_TOLERANCE_SQ) {
      Throw(VSG_ERR_INVALID, "tolerance_sq " + std::to_string(tolerance_sq) + " is outside [0, " +
                                 std::to_string(VSG_RENDER_MAX_TOLERANCE_SQ) + "]");
    }
    if (!scores && capacity_levels != 0) Throw(VSG_ERR_INVALID, "scores is null");
    const int W = h->W, H = h->H;
    const size_t pitch = CheckOtherPitch(h, other_pitch);
    const size_t n = (size_t)W * H, bytes = n * sizeof(int32_t);
    DeviceGuard guard(h->device);
    vsg_render_distance_stats& ds = h->dist.stats;
    std::memset(&ds, 0, sizeof(ds));
    std::memset(&h->pers.stats, 0, sizeof(h->pers.stats));

    // ---- Q, as vsg_render_persistence_image makes it ----
    h->pers.q.Reserve(bytes, &h->allocations);
    const int32_t* q = h->pers.q.As<int32_t>();
    int launches = 0, levels = 0;
    const bool vector = PaintPersistence(h, seg, seg_len, h->pers.q.As<int32_t>(), (size_t)W, &levels, &launches);
    const size_t L = (size_t)levels, bins = L + 1;

    // ---- B: where it is, or through the pinned block to the device, rows packed; G ----
    h->dist.words.Reserve((size_t)DistChunks(H) * W * sizeof(uint32_t), &h->allocations);
    // seen: [0] after the classify pass, [1] at the end
    auto [status, seen] = ReserveStatusPair<DistStatus>(h, &h->dist.status, &h->dist.seen);
    h->dist.hist.Reserve(3 * bins * sizeof(uint32_t), &h->allocations);
    uint32_t* words = h->dist.words.As<uint32_t>();
    uint32_t* hist = h->dist.hist.As<uint32_t>();   // all, near, disc
    h->dist.clock.Begin(h->stream);
    const OtherPlane b = UploadOtherPlane(h, other, pitch, mem_other, &launches);
    h->dist.clock.Mark(DST_PLANE);
    VSG_HIP(hipMemsetAsync(status, 0, sizeof(DistStatus), h->stream));
    VSG_HIP(hipMemsetAsync(hist, 0, 3 * bins * sizeof(uint32_t), h->stream));
    LaunchDistClassify(b.plane, b.pitch, W, H, true, words, status, h->stream);
    VSG_HIP(hipGetLastError());
    h->dist.clock.Mark(DST_CLASSIFY);
    VSG_HIP(hipMemcpyAsync(&seen[0], status, sizeof(DistStatus), hipMemcpyDeviceToHost, h->stream));
    launches += 4;
    FinishPersistence(h, vector, launches);   // the size of G decides what runs below
    float us[DST_STAGES];
    h->dist.clock.Read(us, DST_STAGES);
    ds.plane_us = h->pers.stats.plane_us + h->pers.stats.persist_us + us[DST_PLANE];
    ds.classify_us = us[DST_CLASSIFY];
    ds.levels = (int64_t)L;
    ds.edge_pixels = h->pers.stats.edge_pixels;
    ds.other_edge_pixels = (int64_t)seen[0].edge_pixels;
    ds.launches = h->stats.launches;
    h->stats.device_allocations = h->allocations;
    *num_levels = L;
    if (!scores && capacity_levels == 0) return;   // the count only
    if (capacity_levels < L) {
      Throw(VSG_ERR_INVALID, "the hierarchy has " + std::to_string(L) + " levels, scores has room for " +
                                 std::to_string(capacity_levels));
    }

    // ---- D_G where G has a pixel; the histograms; the records ----
    const bool any = seen[0].edge_pixels != 0;
    const int32_t* dist = nullptr;
    long long* records = reinterpret_cast<long long*>(scores);   // device output: written in place
    if (mem_out == VSG_MEM_HOST) {
      h->dist.scores.Reserve(L * sizeof(vsg_render_boundary_score), &h->allocations);
      records = h->dist.scores.As<long long>();
    }
    launches = 0;
    h->dist.clock.Begin(h->stream);
    if (any) {
      h->dist.gsq.Reserve(bytes, &h->allocations);
      h->dist.out.Reserve(bytes, &h->allocations);
      LaunchDistColumns(words, W, H, h->dist.gsq.As<int32_t>(), h->stream);
      VSG_HIP(hipGetLastError());
      h->dist.clock.Mark(DST_COLUMNS);
      VSG_HIP(LaunchDistRows(h->dist.gsq.As<int32_t>(), W, H, h->dist.out.As<int32_t>(), status, h->stream));
      h->dist.clock.Mark(DST_ROWS);
      dist = h->dist.out.As<int32_t>();
      launches += 2;
    }
    LaunchDistMatch(q, dist, W, H, levels, tolerance_sq, hist, hist + bins, status, h->stream);
    if (any) LaunchDistDisc(q, words, W, H, levels, tolerance_sq, hist + 2 * bins, status, h->stream);
    LaunchDistScores(hist, hist + bins, hist + 2 * bins, levels, status, records, h->stream);
    VSG_HIP(hipGetLastError());
    h->dist.clock.Mark(DST_MATCH);
    launches += any ? 3 : 2;
    if (mem_out == VSG_MEM_HOST) {
      VSG_HIP(hipMemcpyAsync(scores, records, L * sizeof(vsg_render_boundary_score), hipMemcpyDeviceToHost,
                             h->stream));
      ++launches;
    }
    VSG_HIP(hipMemcpyAsync(&seen[1], status, sizeof(DistStatus), hipMemcpyDeviceToHost, h->stream));
    ++launches;
    VSG_HIP(hipStreamSynchronize(h->stream));
    h->dist.clock.Read(us, DST_STAGES);
    ds.columns_us = us[DST_COLUMNS];
    ds.rows_us = us[DST_ROWS];
    ds.match_us = us[DST_MATCH];
    h->stats.launches += launches;
    h->stats.device_allocations = h->allocations;
    ds.launches = h->stats.launches;
    if (seen[1].flags) Throw(VSG_ERR_INTERNAL, "the persistence plane holds a value outside [0, L]");
  });
}

VSG_RENDER_LAST_STATS(vsg_render_last_distance_stats, vsg_render_distance_stats, dist.stats)

}  // extern "C"
