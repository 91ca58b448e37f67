// capi_contours.inc -- vsg_render_level_contours and vsg_render_level_mesh, which goes on from the contours' cracks
// (and capi_simplify.inc from the mesh).
// A part of render_capi.cpp.
namespace {

// What a vsg_render_level_contours call left on the device for vsg_render_level_mesh; in.n == 0: no crack.
struct ContourRun {
  vsg_render_impl::MeshInput in;
  const unsigned long long* ckeys_sorted;
  uint32_t max_group;
  int rounds;
};

// Work space of a contour call: the scan over `pixels` mask bytes, and the sort, both scans and the ranks of
// `contours` contour slots.
size_t ContourTempBytes(uint32_t pixels, int64_t contours, int end_bit) {
  using namespace vsg_render_impl;
  return MaxBytes({ContourClassifyTempBytes(pixels), SortKeysU64TempBytes(contours, end_bit),
                   ExclusiveSumU32TempBytes((int)contours), LevelTempBytes(contours, end_bit)});
}

// vsg_render_level_contours; run: null, or what the mesh call goes on with.
void LevelContours(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness,
                   vsg_render_level_contour* contours, size_t capacity_contours, size_t* num_contours,
                   int32_t* vertices, size_t capacity_vertices, size_t* num_vertices, int mem_out, ContourRun* run) {
  {
    using namespace vsg_render_impl;
    if (run) std::memset(run, 0, sizeof(*run));
    static_assert(sizeof(vsg_render_level_contour) == kLevelContourWords * sizeof(int32_t), "moved as int32 words");
    static_assert(sizeof(vsg_render_contour_stats) == 64, "documented size");
    CheckConnectedness(connectedness, true);
    if (!h) Throw(VSG_ERR_INVALID, "handle is null");
    if (!num_contours || !num_vertices) Throw(VSG_ERR_INVALID, "a count pointer is null");
    *num_contours = *num_vertices = 0;
    CheckMem(mem_out, "mem_out");
    const bool count_only = !contours && !vertices && capacity_contours == 0 && capacity_vertices == 0;
    const int W = h->W, H = h->H;
    if ((uint64_t)W * (uint64_t)H * 4 > (1ull << 31)) {
      Throw(VSG_ERR_INVALID, "the frame has more than 2^31 pixel sides: crack keys do not fit 32 bits");
    }
    const uint32_t pixels = (uint32_t)W * (uint32_t)H;
    DeviceGuard guard(h->device);
    vsg_render_contour_stats& ts = h->cont.stats;
    std::memset(&ts, 0, sizeof(ts));
    // the offsets' scan runs before the first synchronisation: its work space before anything is enqueued
    const size_t scan_bytes = ContourTempBytes(pixels, 1, 64);
    h->d_sort_temp.Reserve(scan_bytes, &h->allocations);

    // ---- the plane: the level's ids, or the indices of its regions' components ----
    const LevelPlane lp = SelectLevelPlane(h, seg, seg_len, level, connectedness, &ts.plane_us, &ts.launches);

    // ---- count: the number of cracks sizes everything below ----
    // seen: [0] after the count, [1] at the end
    auto [status, seen] = ReserveStatusPair<ContourStatus>(h, &h->cont.status, &h->cont.seen);
    h->cont.mask.Reserve(pixels, &h->allocations);
    h->cont.offset.Reserve((size_t)pixels * sizeof(uint32_t), &h->allocations);
    uint8_t* mask = h->cont.mask.As<uint8_t>();
    uint32_t* offset = h->cont.offset.As<uint32_t>();
    VSG_HIP(hipMemsetAsync(status, 0, sizeof(ContourStatus), h->stream));
    h->cont.clock.Begin(h->stream);
    VSG_HIP(ContourClassify(h->d_sort_temp.p, h->d_sort_temp.cap, lp.plane, W, H, mask, offset, status, h->stream));
    VSG_HIP(hipGetLastError());
    h->cont.clock.Mark(CNT_CLASSIFY);
    VSG_HIP(hipMemcpyAsync(&seen[0], status, sizeof(ContourStatus), hipMemcpyDeviceToHost, h->stream));
    int launches = 4;   // the clear, the masks, the scan counted as one, the status
    VSG_HIP(hipStreamSynchronize(h->stream));
    {
      float us[CNT_STAGES];
      h->cont.clock.Read(us, CNT_STAGES);
      ts.classify_us = us[CNT_CLASSIFY];
    }
    FinishLevelPlane(h, lp, &ts.plane_us);
    auto finish = [&] { CountLaunches(h, &ts.launches, launches); };
    if (seen[0].cracks > 4ull * pixels) {
      finish();
      Throw(VSG_ERR_INTERNAL, "more cracks than pixel sides");
    }
    const uint32_t n = (uint32_t)seen[0].cracks;
    ts.cracks = n;
    if (n == 0) return finish();   // no covered pixel: both lists are empty
    if (n < 4) {
      finish();
      Throw(VSG_ERR_INTERNAL, "fewer cracks than one pixel has");
    }

    // ---- emit, trace, table ----
    const int rounds = ContourRounds(n);
    const uint32_t cap = n / 4;   // a contour has four cracks or more
    const int end_bit = 32 + BitsFor(lp.max_group, 32);
    const size_t temp_bytes = ContourTempBytes(pixels, cap, end_bit);
    h->d_sort_temp.Reserve(temp_bytes, &h->allocations);
    h->cont.cracks.Reserve((size_t)n * 36, &h->allocations);
    h->cont.slots.Reserve((size_t)cap * 28, &h->allocations);
    h->cont.records.Reserve((size_t)cap * sizeof(vsg_render_level_contour), &h->allocations);
    uint2* state_a = h->cont.cracks.As<uint2>();
    uint2* state_b = state_a + n;
    uint32_t* key = reinterpret_cast<uint32_t*>(state_b + n);
    uint32_t* succ = key + n;
    uint32_t* leader = succ + n;
    uint32_t* place = leader + n;
    uint32_t* owner = place + n;
    unsigned long long* ckeys = h->cont.slots.As<unsigned long long>();
    unsigned long long* ckeys_sorted = ckeys + cap;
    uint32_t* crank = reinterpret_cast<uint32_t*>(ckeys_sorted + cap);
    uint32_t* count = crank + cap;
    uint32_t* first = count + cap;
    int32_t* d_records = h->cont.records.As<int32_t>();
    h->cont.clock.Begin(h->stream);
    LaunchContourEmit(lp.plane, W, H, mask, offset, n, key, succ, state_a, status, h->stream);
    VSG_HIP(hipGetLastError());
    h->cont.clock.Mark(CNT_CLASSIFY);
    const uint2* ranked = LaunchContourTrace(key, succ, n, rounds, state_a, state_b, leader, status, h->stream);
    // the doubling state that is not the result holds the vertices: n pairs at the most
    int32_t* d_vertices = reinterpret_cast<int32_t*>(ranked == state_a ? state_b : state_a);
    VSG_HIP(hipMemsetAsync(ckeys, 0xff, (size_t)cap * sizeof(unsigned long long), h->stream));   // unused: last
    LaunchContourLeaders(leader, key, lp.plane, n, cap, ckeys, status, h->stream);
    VSG_HIP(hipGetLastError());
    VSG_HIP(SortKeysU64(h->d_sort_temp.p, temp_bytes, ckeys, ckeys_sorted, cap, end_bit, h->stream));
    VSG_HIP(HeadScan(h->d_sort_temp.p, temp_bytes, HeadFlag{ckeys_sorted}, crank, cap, h->stream));
    VSG_HIP(ContourVertices(h->d_sort_temp.p, temp_bytes, ckeys_sorted, key, succ, leader, ranked, n, cap, W, place,
                            count, first, d_vertices, owner, status, h->stream));
    VSG_HIP(hipGetLastError());
    h->cont.clock.Mark(CNT_TRACE);
    LaunchContourTable(ckeys_sorted, crank, count, first, d_vertices, owner, n, cap, lp.max_group, lp.comp_table,
                       d_records, status, h->stream);
    VSG_HIP(hipGetLastError());
    ts.rounds = 2 * rounds;
    // emit, the rounds (two a launch) and the cut between them, the clear, leaders, the sort and the scan
    // counted as one each, heads, the scan, vertices, table, measure, finish
    launches += rounds + 12;
    const bool to_device = !count_only && mem_out == VSG_MEM_DEVICE && contours && vertices;
    if (to_device) {
      // the lengths of both lists are on the device: the copy decides there whether they fit
      CopyLists lists = {};
      lists.list[0] = {d_records, reinterpret_cast<int32_t*>(contours), kLevelContourWords, &status->contours, 0,
                       (uint32_t)std::min<size_t>(capacity_contours, cap)};
      lists.list[1] = {d_vertices, vertices, 2, &status->vertices, 0, (uint32_t)std::min<size_t>(capacity_vertices, n)};
      lists.flags = &status->flags;
      LaunchCopyLists(lists, h->stream);
      VSG_HIP(hipGetLastError());
      ++launches;
    }
    h->cont.clock.Mark(CNT_TABLE);
    VSG_HIP(hipMemcpyAsync(&seen[1], status, sizeof(ContourStatus), hipMemcpyDeviceToHost, h->stream));
    ++launches;
    if (!count_only && mem_out == VSG_MEM_HOST) launches += 2;   // counted whether or not the lists fit
    VSG_HIP(hipStreamSynchronize(h->stream));
    {
      float us[CNT_STAGES];
      h->cont.clock.Read(us, CNT_STAGES);
      ts.classify_us += us[CNT_CLASSIFY];
      ts.trace_us = us[CNT_TRACE];
      ts.table_us = us[CNT_TABLE];
    }
    finish();
    if (seen[1].flags & CONTOUR_FLAG_OVERFLOW) Throw(VSG_ERR_INTERNAL, "more contours than a quarter of the cracks");
    if ((seen[1].flags & CONTOUR_FLAG_RANGE) || seen[1].contours == 0 || seen[1].contours > cap ||
        seen[1].vertices > n || (uint64_t)seen[1].vertices < 4ull * seen[1].contours) {
      Throw(VSG_ERR_INTERNAL, "a crack, a contour or a vertex is out of range");
    }
    const size_t n_contours = seen[1].contours, n_vertices = seen[1].vertices;
    *num_contours = n_contours;
    *num_vertices = n_vertices;
    ts.contours = (int64_t)n_contours;
    ts.vertices = (int64_t)n_vertices;
    ts.holes = seen[1].holes;
    ts.largest_contour_cracks = seen[1].largest;
    if (run) {
      MeshInput& in = run->in;
      in.plane = lp.plane;
      in.width = W;
      in.height = H;
      in.mask = mask;
      in.offset = offset;
      in.n = n;
      in.key = key;
      in.succ = succ;
      in.leader = leader;
      in.place = place;
      in.ranked = ranked;
      in.contours = (uint32_t)n_contours;
      in.count = count;
      in.records = d_records;
      run->ckeys_sorted = ckeys_sorted;
      run->max_group = lp.max_group;
      run->rounds = rounds;
    }
    if (count_only) return;
    if (n_contours > capacity_contours || n_vertices > capacity_vertices) {
      Throw(VSG_ERR_INVALID, "the level has " + std::to_string(n_contours) + " contours and " +
                                 std::to_string(n_vertices) + " vertices, the capacities are " +
                                 std::to_string(capacity_contours) + " and " + std::to_string(capacity_vertices));
    }
    if (!contours || !vertices) Throw(VSG_ERR_INVALID, "an output is null");
    if (mem_out == VSG_MEM_HOST) {
      // neither list is empty; the two copies were counted above
      DeliverToHost(h, &h->cont.seen, 2 * sizeof(ContourStatus),
                    {{d_records, n_contours * sizeof(vsg_render_level_contour), contours},
                     {d_vertices, n_vertices * 2 * sizeof(int32_t), vertices}});
      h->stats.device_allocations = h->allocations;
    }
  }
}

}  // namespace

extern "C" {

int vsg_render_level_contours(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness,
                              vsg_render_level_contour* contours, size_t capacity_contours, size_t* num_contours,
                              int32_t* vertices, size_t capacity_vertices, size_t* num_vertices, int mem_out) {
  return Guard([&] {
    LevelContours(h, seg, seg_len, level, connectedness, contours, capacity_contours, num_contours, vertices,
                  capacity_vertices, num_vertices, mem_out, nullptr);
  });
}

VSG_RENDER_LAST_STATS(vsg_render_last_contour_stats, vsg_render_contour_stats, cont.stats)

}  // extern "C"

namespace {

// What a vsg_render_level_mesh call left on the device for vsg_render_level_mesh_simplified: the four lists
// and their lengths; segments == 0: no crack.
struct MeshRun {
  vsg_render_impl::MeshSegmentSpace t;
  uint32_t segments, vertices, loops, refs;
};

// Work space of the sort of `items` segment keys and of a scan over as many counts.
size_t MeshTempBytes(int64_t items, int end_bit) {
  using namespace vsg_render_impl;
  return MaxBytes({SortKeysU64TempBytes(items, end_bit), ExclusiveSumU32TempBytes((int)items)});
}

// vsg_render_level_mesh; left: null, or what the simplified call goes on with.
void LevelMesh(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness,
               vsg_render_mesh_segment* segments, size_t capacity_segments, size_t* num_segments, int32_t* vertices,
               size_t capacity_vertices, size_t* num_vertices, vsg_render_mesh_loop* loops, size_t capacity_loops,
               size_t* num_loops, int32_t* refs, size_t capacity_refs, size_t* num_refs, int mem_out, MeshRun* left) {
  {
    using namespace vsg_render_impl;
    if (left) std::memset(left, 0, sizeof(*left));
    static_assert(sizeof(vsg_render_mesh_segment) == kMeshSegmentWords * sizeof(int32_t), "moved as int32 words");
    static_assert(sizeof(vsg_render_mesh_loop) == kMeshLoopWords * sizeof(int32_t), "moved as int32 words");
    static_assert(sizeof(vsg_render_mesh_stats) == 104, "documented size");
    CheckConnectedness(connectedness, true);
    if (!h) Throw(VSG_ERR_INVALID, "handle is null");
    if (!num_segments || !num_vertices || !num_loops || !num_refs) Throw(VSG_ERR_INVALID, "a count pointer is null");
    CheckMem(mem_out, "mem_out");
    *num_segments = *num_vertices = *num_loops = *num_refs = 0;
    const bool count_only = !segments && !vertices && !loops && !refs && capacity_segments == 0 &&
                            capacity_vertices == 0 && capacity_loops == 0 && capacity_refs == 0;
    vsg_render_mesh_stats& ms = h->mesh.stats;
    std::memset(&ms, 0, sizeof(ms));

    // ---- the contour stages, as a count-only call ----
    ContourRun run;
    size_t n_contours = 0, n_contour_vertices = 0;
    struct ContourPart {
      vsg_render* h;
      ~ContourPart() {
        const vsg_render_contour_stats& ts = h->cont.stats;
        vsg_render_mesh_stats& ms = h->mesh.stats;
        ms.cracks = ts.cracks;
        ms.plane_us = ts.plane_us;
        ms.classify_us = ts.classify_us;
        ms.trace_us = ts.trace_us + ts.table_us;
        ms.rounds = ts.rounds;
        ms.launches = ts.launches;
      }
    };
    {
      ContourPart part{h};
      LevelContours(h, seg, seg_len, level, connectedness, nullptr, 0, &n_contours, nullptr, 0, &n_contour_vertices,
                    VSG_MEM_HOST, &run);
    }
    const uint32_t n = run.in.n;
    if (n == 0) return;   // no covered pixel: all four lists are empty
    DeviceGuard guard(h->device);
    const uint32_t C = run.in.contours;
    const int end_bit = 32 + BitsFor(run.max_group, 32);

    // ---- split: junctions, the third doubling, halves, owners ----
    // sized for every crack and for what is scanned here: the library's need is not promised to grow with the
    // number of items
    size_t temp_bytes = std::max(MeshTempBytes(n, end_bit), MeshTempBytes(C, end_bit));
    h->d_sort_temp.Reserve(temp_bytes, &h->allocations);
    // seen: [0] after the split, [1] at the end
    auto [status, seen] = ReserveStatusPair<MeshStatus>(h, &h->mesh.status, &h->mesh.seen);
    h->mesh.cracks.Reserve((size_t)n * 40 + (size_t)C * 12 + n, &h->allocations);
    MeshCrackSpace w;
    w.state_a = h->mesh.cracks.As<uint2>();
    w.state_b = w.state_a + n;
    w.skeys = reinterpret_cast<unsigned long long*>(w.state_b + n);
    w.half = reinterpret_cast<uint32_t*>(w.skeys + n);
    w.head_of = w.half + n;            // and last_of behind it
    w.seg_of = w.head_of + 2 * (size_t)n;
    w.hasj = w.seg_of + n;
    w.nrefs = w.hasj + C;
    w.first_ref = w.nrefs + C;
    w.sides = reinterpret_cast<uint8_t*>(w.first_ref + C);
    w.heads = nullptr;
    int launches = 0;
    auto finish = [&] { CountLaunches(h, &ms.launches, launches); };
    VSG_HIP(hipMemsetAsync(status, 0, sizeof(MeshStatus), h->stream));
    h->mesh.clock.Begin(h->stream);
    VSG_HIP(MeshSplit(h->d_sort_temp.p, temp_bytes, run.in, run.ckeys_sorted, run.rounds, &w, status, h->stream));
    h->mesh.clock.Mark(MSH_SPLIT);
    VSG_HIP(hipMemcpyAsync(&seen[0], status, sizeof(MeshStatus), hipMemcpyDeviceToHost, h->stream));
    // the clear, MeshSplit's 7 and a launch for two rounds, the status
    launches += 9 + run.rounds / 2;
    VSG_HIP(hipStreamSynchronize(h->stream));
    ms.rounds += run.rounds;
    ms.junctions = seen[0].junctions;
    const uint32_t S = seen[0].segments, R = seen[0].refs;
    if ((seen[0].flags & MESH_FLAG_RANGE) || S == 0 || S > n || R < C || R > n || S > R) {
      finish();
      Throw(VSG_ERR_INTERNAL, "a crack, a contour or a half is out of range");
    }

    // ---- tables: the segments' order, vertices, records, loops, refs, lengths ----
    if ((uint64_t)n + S > 0xffffffffull) {
      finish();
      Throw(VSG_ERR_INVALID, "the level has more than 2^32 - 1 cracks and segments");
    }
    const uint32_t slots = n + S;      // a vertex per crack of an owner half and an end corner per segment
    temp_bytes = std::max(temp_bytes, MeshTempBytes(S, end_bit));
    h->d_sort_temp.Reserve(temp_bytes, &h->allocations);
    const size_t seg_words = (size_t)S * kMeshSegmentWords, loop_words = (size_t)C * kMeshLoopWords;
    h->mesh.lists.Reserve((size_t)S * 16 + (seg_words + (size_t)slots * 3 + loop_words + R) * 4, &h->allocations);
    MeshSegmentSpace t;
    t.skeys_sorted = h->mesh.lists.As<unsigned long long>();
    t.scount = reinterpret_cast<uint32_t*>(t.skeys_sorted + S);
    t.sfirst = t.scount + S;
    t.segments = reinterpret_cast<int32_t*>(t.sfirst + S);
    t.vertex_slots = slots;
    t.vertices = t.segments + seg_words;
    t.vseg = reinterpret_cast<uint32_t*>(t.vertices + (size_t)slots * 2);
    t.loops = reinterpret_cast<int32_t*>(t.vseg + slots);
    t.refs = t.loops + loop_words;
    VSG_HIP(MeshTables(h->d_sort_temp.p, temp_bytes, run.in, w, t, S, R, end_bit, status, h->stream));
    launches += 11;
    const bool fits = S <= capacity_segments && C <= capacity_loops && R <= capacity_refs;
    const bool to_device = !count_only && mem_out == VSG_MEM_DEVICE && segments && vertices && loops && refs;
    if (to_device) {
      // the number of vertices is on the device: the copy decides there whether they fit.  Counted whether or
      // not the other three lists fit
      if (fits) {
        CopyLists lists = {};
        lists.list[0] = {t.segments, reinterpret_cast<int32_t*>(segments), kMeshSegmentWords, nullptr, S, S};
        lists.list[1] = {t.vertices, vertices, 2, &status->vertices, 0,
                         (uint32_t)std::min<size_t>(capacity_vertices, slots)};
        lists.list[2] = {t.loops, reinterpret_cast<int32_t*>(loops), kMeshLoopWords, nullptr, C, C};
        lists.list[3] = {t.refs, refs, 1, nullptr, R, R};
        lists.flags = &status->flags;
        LaunchCopyLists(lists, h->stream);
        VSG_HIP(hipGetLastError());
      }
      ++launches;
    }
    h->mesh.clock.Mark(MSH_TABLE);
    VSG_HIP(hipMemcpyAsync(&seen[1], status, sizeof(MeshStatus), hipMemcpyDeviceToHost, h->stream));
    ++launches;
    if (!count_only && mem_out == VSG_MEM_HOST) launches += 4;   // counted whether or not the lists fit
    VSG_HIP(hipStreamSynchronize(h->stream));
    {
      float us[MSH_STAGES];
      h->mesh.clock.Read(us, MSH_STAGES);
      ms.split_us = us[MSH_SPLIT];
      ms.table_us = us[MSH_TABLE];
    }
    finish();
    const size_t V = seen[1].vertices;
    if ((seen[1].flags & MESH_FLAG_RANGE) || V > slots || V < 2ull * S) {
      Throw(VSG_ERR_INTERNAL, "a segment, a vertex or a ref is out of range");
    }
    *num_segments = S;
    *num_vertices = V;
    *num_loops = C;
    *num_refs = R;
    ms.segments = S;
    ms.closed_segments = seen[1].closed;
    ms.shared_segments = seen[1].shared;
    ms.vertices = (int64_t)V;
    ms.loops = C;
    ms.refs = R;
    ms.longest_segment_cracks = seen[1].longest;
    if (left) {
      left->t = t;
      left->segments = S;
      left->vertices = (uint32_t)V;
      left->loops = C;
      left->refs = R;
    }
    if (count_only) return;
    if (!fits || V > capacity_vertices) {
      Throw(VSG_ERR_INVALID, "the level has " + std::to_string(S) + " segments, " + std::to_string(V) + " vertices, " +
                                 std::to_string(C) + " loops and " + std::to_string(R) + " refs, the capacities are " +
                                 std::to_string(capacity_segments) + ", " + std::to_string(capacity_vertices) + ", " +
                                 std::to_string(capacity_loops) + " and " + std::to_string(capacity_refs));
    }
    if (!segments || !vertices || !loops || !refs) Throw(VSG_ERR_INVALID, "an output is null");
    if (mem_out == VSG_MEM_HOST) {
      // no list is empty; the four copies were counted above
      DeliverToHost(h, &h->mesh.seen, 2 * sizeof(MeshStatus),
                    {{t.segments, seg_words * 4, segments},
                     {t.vertices, V * 8, vertices},
                     {t.loops, loop_words * 4, loops},
                     {t.refs, (size_t)R * 4, refs}});
      h->stats.device_allocations = h->allocations;
    }
  }
}

}  // namespace

extern "C" {

int vsg_render_level_mesh(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness,
                          vsg_render_mesh_segment* segments, size_t capacity_segments, size_t* num_segments,
                          int32_t* vertices, size_t capacity_vertices, size_t* num_vertices,
                          vsg_render_mesh_loop* loops, size_t capacity_loops, size_t* num_loops, int32_t* refs,
                          size_t capacity_refs, size_t* num_refs, int mem_out) {
  return Guard([&] {
    LevelMesh(h, seg, seg_len, level, connectedness, segments, capacity_segments, num_segments, vertices,
              capacity_vertices, num_vertices, loops, capacity_loops, num_loops, refs, capacity_refs, num_refs, mem_out,
              nullptr);
  });
}

VSG_RENDER_LAST_STATS(vsg_render_last_mesh_stats, vsg_render_mesh_stats, mesh.stats)

}  // extern "C"
