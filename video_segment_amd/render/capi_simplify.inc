// capi_simplify.inc -- vsg_render_level_mesh_simplified, which goes on from the lists a count-only
// vsg_render_level_mesh leaves on the device.  A part of render_capi.cpp.
extern "C" {

int vsg_render_level_mesh_simplified(vsg_render* h, const uint8_t* seg, size_t seg_len, int level,
                                     int connectedness, float max_error, int min_segment_points,
                                     vsg_render_mesh_segment* segments, size_t capacity_segments,
                                     size_t* num_segments, int32_t* vertices, size_t capacity_vertices,
                                     size_t* num_vertices, vsg_render_mesh_loop* loops, size_t capacity_loops,
                                     size_t* num_loops, int32_t* refs, size_t capacity_refs, size_t* num_refs,
                                     int mem_out) {
  return Guard([&] {
    using namespace vsg_render_impl;
    static_assert(sizeof(vsg_render_simplify_stats) == 80, "documented size");
    CheckConnectedness(connectedness, true);
    if (!h) Throw(VSG_ERR_INVALID, "handle is null");
    if (!num_segments || !num_vertices || !num_loops || !num_refs) Throw(VSG_ERR_INVALID, "a count pointer is null");
    CheckMem(mem_out, "mem_out");
    if (!std::isfinite(max_error) || max_error < 0) Throw(VSG_ERR_INVALID, "max_error is not a finite number >= 0");
    if (min_segment_points < 0) Throw(VSG_ERR_INVALID, "min_segment_points is negative");
    *num_segments = *num_vertices = *num_loops = *num_refs = 0;
    const bool count_only = !segments && !vertices && !loops && !refs && capacity_segments == 0 &&
                            capacity_vertices == 0 && capacity_loops == 0 && capacity_refs == 0;
    vsg_render_simplify_stats& ss = h->simp.stats;
    std::memset(&ss, 0, sizeof(ss));

    // ---- the contour and mesh stages, as a count-only call ----
    MeshRun run;
    size_t n_segments = 0, n_mesh_vertices = 0, n_loops = 0, n_refs = 0;
    struct MeshPart {
      vsg_render* h;
      ~MeshPart() { h->simp.stats.launches = h->mesh.stats.launches; }
    };
    {
      MeshPart part{h};
      LevelMesh(h, seg, seg_len, level, connectedness, nullptr, 0, &n_segments, nullptr, 0, &n_mesh_vertices, nullptr,
                0, &n_loops, nullptr, 0, &n_refs, VSG_MEM_HOST, &run);
    }
    const uint32_t S = run.segments, V = run.vertices, C = run.loops, R = run.refs;
    if (S == 0) return;   // no covered pixel: all four lists are empty
    DeviceGuard guard(h->device);

    // ---- blocks: a segment keeps one vertex more than it has at the most ----
    if ((uint64_t)V + S > 0xffffffffull) Throw(VSG_ERR_INVALID, "the level has more than 2^32 - 1 vertices and segments");
    const uint32_t slots = V + S;
    const size_t temp_bytes = MaxBytes({ExclusiveSumU32TempBytes((int)S)});
    h->d_sort_temp.Reserve(temp_bytes, &h->allocations);
    // seen: [1] at the end
    auto [status, seen] = ReserveStatusPair<SimplifyStatus>(h, &h->simp.status, &h->simp.seen);
    h->simp.work.Reserve((size_t)slots * 36 + (size_t)S * 24, &h->allocations);
    const size_t seg_words = (size_t)S * kMeshSegmentWords;
    h->simp.lists.Reserve((seg_words + (size_t)slots * 2) * 4, &h->allocations);
    SimplifyView m;
    m.segments = run.t.segments;
    m.vertices = reinterpret_cast<const int2*>(run.t.vertices);
    m.n_segments = S;
    m.slots = slots;
    m.eps = (double)max_error * (double)max_error;
    m.threshold = min_segment_points > 0 ? (uint32_t)std::max(3, min_segment_points) : 0u;
    m.best = h->simp.work.As<unsigned long long>();          // 2 per slot
    m.kept = reinterpret_cast<int2*>(m.best + 2 * (size_t)slots);
    m.kseg = reinterpret_cast<uint32_t*>(m.kept + slots);
    m.lo = m.kseg + slots;
    m.hi = m.lo + slots;
    m.kcount = m.hi + slots;
    m.rounds = m.kcount + S;
    m.sflag = m.rounds + S;
    m.long_list = m.sflag + S;
    uint32_t* ncount = m.long_list + S;
    uint32_t* nfirst = ncount + S;
    int32_t* d_segments = h->simp.lists.As<int32_t>();
    int32_t* d_vertices = d_segments + seg_words;

    // ---- the rounds, the joint pass, the tables ----
    int launches = 0;
    VSG_HIP(hipMemsetAsync(status, 0, sizeof(SimplifyStatus), h->stream));
    h->simp.clock.Begin(h->stream);
    VSG_HIP(SimplifyDp(m, status, h->stream));
    h->simp.clock.Mark(SMP_DP);
    VSG_HIP(SimplifyClean(m, ncount, h->stream));
    h->simp.clock.Mark(SMP_CLEAN);
    VSG_HIP(SimplifyTables(h->d_sort_temp.p, temp_bytes, m, ncount, nfirst, d_segments, d_vertices, status, h->stream));
    launches += 8;   // the status' clear, SimplifyDp's 3, the joint pass, SimplifyTables' 3
    const bool fits = S <= capacity_segments && C <= capacity_loops && R <= capacity_refs;
    const bool to_device = !count_only && mem_out == VSG_MEM_DEVICE && segments && vertices && loops && refs;
    if (to_device) {
      // the number of vertices is on the device: the copy decides there whether they fit.  Counted whether or
      // not the other three lists fit
      if (fits) {
        CopyLists lists = {};
        lists.list[0] = {d_segments, reinterpret_cast<int32_t*>(segments), kMeshSegmentWords, nullptr, S, S};
        lists.list[1] = {d_vertices, vertices, 2, &status->vertices_out, 0,
                         (uint32_t)std::min<size_t>(capacity_vertices, slots)};
        lists.list[2] = {run.t.loops, reinterpret_cast<int32_t*>(loops), kMeshLoopWords, nullptr, C, C};
        lists.list[3] = {run.t.refs, refs, 1, nullptr, R, R};
        lists.flags = &status->flags;
        LaunchCopyLists(lists, h->stream);
        VSG_HIP(hipGetLastError());
      }
      ++launches;
    }
    h->simp.clock.Mark(SMP_TABLE);
    VSG_HIP(hipMemcpyAsync(&seen[1], status, sizeof(SimplifyStatus), hipMemcpyDeviceToHost, h->stream));
    ++launches;
    if (!count_only && mem_out == VSG_MEM_HOST) launches += 4;   // counted whether or not the lists fit
    VSG_HIP(hipStreamSynchronize(h->stream));
    {
      float us[SMP_STAGES];
      h->simp.clock.Read(us, SMP_STAGES);
      ss.dp_us = us[SMP_DP];
      ss.clean_us = us[SMP_CLEAN];
      ss.table_us = us[SMP_TABLE];
    }
    CountLaunches(h, &ss.launches, launches);
    const size_t out = seen[1].vertices_out;
    if ((seen[1].flags & SIMPLIFY_FLAG_RANGE) || out > slots || out < S) {
      Throw(VSG_ERR_INTERNAL, "a segment or a vertex of the simplification is out of range");
    }
    *num_segments = S;
    *num_vertices = out;
    *num_loops = C;
    *num_refs = R;
    ss.segments = S;
    ss.collapsed_segments = seen[1].collapsed;
    ss.vertices_in = V;
    ss.vertices_kept = seen[1].vertices_kept;
    ss.vertices_out = (int64_t)out;
    ss.single_vertex_closed = seen[1].single_closed;
    ss.longest_segment_vertices_in = seen[1].longest_in;
    ss.max_rounds = (int)seen[1].max_rounds;
    if (count_only) return;
    if (!fits || out > capacity_vertices) {
      Throw(VSG_ERR_INVALID, "the level has " + std::to_string(S) + " segments, " + std::to_string(out) + " vertices, " +
                                 std::to_string(C) + " loops and " + std::to_string(R) + " refs, the capacities are " +
                                 std::to_string(capacity_segments) + ", " + std::to_string(capacity_vertices) + ", " +
                                 std::to_string(capacity_loops) + " and " + std::to_string(capacity_refs));
    }
    if (!segments || !vertices || !loops || !refs) Throw(VSG_ERR_INVALID, "an output is null");
    if (mem_out == VSG_MEM_HOST) {
      // no list is empty; the four copies were counted above
      DeliverToHost(h, &h->simp.seen, 2 * sizeof(SimplifyStatus),
                    {{d_segments, seg_words * 4, segments},
                     {d_vertices, out * 8, vertices},
                     {run.t.loops, (size_t)C * kMeshLoopWords * 4, loops},
                     {run.t.refs, (size_t)R * 4, refs}});
      h->stats.device_allocations = h->allocations;
    }
  });
}

VSG_RENDER_LAST_STATS(vsg_render_last_simplify_stats, vsg_render_simplify_stats, simp.stats)

}  // extern "C"
