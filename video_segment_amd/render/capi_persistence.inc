// capi_persistence.inc -- vsg_render_persistence_image, vsg_render_persistence_frame and
// vsg_render_persistence_graph.  A part of render_capi.cpp, after capi_adjacency.inc.
namespace {

// The hierarchy's height and the ancestor table of h->pers.ids in h->pers.table, or the refusals of
// vsg_render_id_image at the top level.  Host work only.
int BuildPersistenceTable(vsg_render* h) {
  const size_t L = vsg_render_impl::PersistenceHeight(h->kept.size());
  if (L > 65535) Throw(VSG_ERR_INVALID, "the hierarchy has " + std::to_string(L) + " levels, more than 65535");
  if (h->pers.ids.size() > (1u << 30)) Throw(VSG_ERR_INVALID, "too many regions");
  int bad_level = 0;
  int32_t bad_id = 0;
  if (!vsg_render_impl::BuildAncestorTable(h->kept, h->pers.ids.data(), h->pers.ids.size(), &h->pers.table,
                                           &bad_level, &bad_id)) {
    Throw(VSG_ERR_INVALID,
          "region " + std::to_string(bad_id) + " is not in hierarchy level " + std::to_string(bad_level));
  }
  return (int)L;
}

// Region ids, then the table's rows, to h->pers.anc in one copy on the stream; returns the table (null
// when there is none: one level, or no region).  The pinned block gets room for at least pinned_bytes, what
// the call reads back through it later: it must not grow while the copy is in flight.
const int32_t* UploadPersistenceTable(vsg_render* h, size_t pinned_bytes, int* launches) {
  const size_t n = h->pers.ids.size() + h->pers.table.size();
  h->pers.anc.Reserve(std::max<size_t>(n, 1) * sizeof(int32_t), &h->allocations);
  h->pers.seen.Reserve(std::max(n * sizeof(int32_t), pinned_bytes), &h->allocations);
  if (n == 0) return nullptr;
  int32_t* stage = h->pers.seen.As<int32_t>();
  std::copy(h->pers.ids.begin(), h->pers.ids.end(), stage);
  std::copy(h->pers.table.begin(), h->pers.table.end(), stage + h->pers.ids.size());
  VSG_HIP(hipMemcpyAsync(h->pers.anc.p, stage, n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  ++*launches;
  return h->pers.table.empty() ? nullptr : h->pers.anc.As<int32_t>() + h->pers.ids.size();
}

// The front half of the image and the frame call: the level-0 plane in h->d_plane painted with a dense
// number per distinct region id (so that sparse ids cost nothing), the ancestor table on the device, and
// Q written to q.  Leaves the family's clock after PRS_PERSIST and the status in flight.  Returns whether the desc was
// vector-only; *levels = L.
bool PaintPersistence(vsg_render* h, const uint8_t* seg, size_t seg_len, int32_t* q, size_t q_pitch, int* levels,
                      int* launches) {
  const int W = h->W, H = h->H;
  vsg_render_persistence_stats& ps = h->pers.stats;
  h->pers.ids.clear();
  int L = 1;
  uint32_t* plane = h->d_plane.As<uint32_t>();
  const bool vector = PaintIdsAt(
      h, seg, seg_len, 0, plane, h->pitch,
      [&](int mapped) {
        if (mapped < 0) Throw(VSG_ERR_INVALID, "region id " + std::to_string(mapped) + " is negative");
        h->pers.ids.push_back(mapped);
        return (uint32_t)(h->pers.ids.size() - 1);
      },
      [&] { L = BuildPersistenceTable(h); });
  *levels = L;
  ps.levels = L;
  ps.regions = (int64_t)h->pers.ids.size();
  const int32_t* table = UploadPersistenceTable(h, sizeof(PersStatus), launches);
  h->pers.status.Reserve(sizeof(PersStatus), &h->allocations);
  PersStatus* status = h->pers.status.As<PersStatus>();
  VSG_HIP(hipMemsetAsync(status, 0, sizeof(PersStatus), h->stream));
  h->pers.clock.Begin(h->stream);
  vsg_render_impl::LaunchPersistPlane(reinterpret_cast<const int32_t*>(plane), h->pitch, W, H, table,
                                      (uint32_t)h->pers.ids.size(), L, q, q_pitch, status, h->stream);
  VSG_HIP(hipGetLastError());
  h->pers.clock.Mark(PRS_PERSIST);
  *launches += 2;
  return vector;
}

// The back half: the status back, the one synchronisation, the stats, the device's flag.
void FinishPersistence(vsg_render* h, bool vector, int launches) {
  vsg_render_persistence_stats& ps = h->pers.stats;
  // the table went through the pinned block before the plane kernel ran; the status may follow it
  PersStatus* seen = h->pers.seen.As<PersStatus>();
  VSG_HIP(hipMemcpyAsync(seen, h->pers.status.p, sizeof(PersStatus), hipMemcpyDeviceToHost, h->stream));
  ++launches;
  h->FinishStats();
  float us[PRS_STAGES];
  h->pers.clock.Read(us, PRS_STAGES);
  ps.plane_us = h->stats.clear_us + h->stats.fill_us;
  ps.persist_us = us[PRS_PERSIST];
  ps.compose_us = us[PRS_COMPOSE];
  h->stats.launches += launches;
  ps.launches = h->stats.launches;
  if (vector) h->CheckVector();
  if (seen->flags) Throw(VSG_ERR_INTERNAL, "the plane holds a region number the host did not give out");
  ps.edge_pixels = (int64_t)seen->edge_pixels;
  ps.top_pixels = (int64_t)seen->top_pixels;
}

}  // namespace

extern "C" {

int vsg_render_persistence_image(vsg_render* h, const uint8_t* seg, size_t seg_len, int32_t* out, int* num_levels,
                                 int mem_out) {
  return Guard([&] {
    if (!h) Throw(VSG_ERR_INVALID, "handle is null");
    if (!out) Throw(VSG_ERR_INVALID, "out is null");
    if (!num_levels) Throw(VSG_ERR_INVALID, "the count pointer is null");
    CheckMem(mem_out, "out");
    *num_levels = 0;
    const int W = h->W, H = h->H;
    const size_t bytes = (size_t)W * H * sizeof(int32_t);
    DeviceGuard guard(h->device);
    std::memset(&h->pers.stats, 0, sizeof(h->pers.stats));
    int32_t* q = out;   // device output: written in place
    if (mem_out == VSG_MEM_HOST) {
      h->pers.q.Reserve(bytes, &h->allocations);
      q = h->pers.q.As<int32_t>();
    }
    int launches = 0, levels = 0;
    const bool vector = PaintPersistence(h, seg, seg_len, q, (size_t)W, &levels, &launches);
    if (mem_out == VSG_MEM_HOST) {
      VSG_HIP(hipMemcpyAsync(out, q, bytes, hipMemcpyDeviceToHost, h->stream));
      ++launches;
    }
    FinishPersistence(h, vector, launches);
    *num_levels = levels;
  });
}

int vsg_render_persistence_frame(vsg_render* h, const uint8_t* seg, size_t seg_len, const uint8_t* bgr, size_t stride,
                                 int mem_in, uint8_t* out, size_t out_stride, int mem_out, int* num_levels) {
  return Guard([&] {
    if (!h) Throw(VSG_ERR_INVALID, "handle is null");
    if (!out) Throw(VSG_ERR_INVALID, "out is null");
    if (!num_levels) Throw(VSG_ERR_INVALID, "the count pointer is null");
    CheckMem(mem_in, "bgr");
    CheckMem(mem_out, "out");
    *num_levels = 0;
    const int W = h->W, H = h->H;
    const size_t row_bytes = (size_t)W * 3;
    const bool video = h->opt.has_video != 0;
    if (video && !bgr) Throw(VSG_ERR_INVALID, "the handle was created with has_video: bgr is null");
    if (video && stride < row_bytes) Throw(VSG_ERR_INVALID, "stride is smaller than 3 * width");
    if (out_stride == 0) out_stride = vsg_render_default_stride(W);
    if (out_stride < row_bytes) Throw(VSG_ERR_INVALID, "out_stride is smaller than 3 * width");
    DeviceGuard guard(h->device);
    std::memset(&h->pers.stats, 0, sizeof(h->pers.stats));
    // Q has the plane's pitch: every tile row of it is 16-byte aligned
    h->pers.q.Reserve((size_t)h->pitch * H * sizeof(int32_t), &h->allocations);
    int32_t* q = h->pers.q.As<int32_t>();
    int launches = 0, levels = 0;
    const bool vector = PaintPersistence(h, seg, seg_len, q, (size_t)h->pitch, &levels, &launches);
    SourceFrame src{nullptr, 0};
    if (video) src = UploadSource(h, bgr, stride, mem_in, &launches);
    const PictureOut dst = StagePicture(h, out, out_stride, H, mem_out);
    h->pers.clock.Mark(PRS_WAIT);
    vsg_render_impl::LaunchPersistCompose(q, (size_t)h->pitch, W, H, levels, src.p, src.stride, dst.p, dst.stride,
                                          h->stream);
    VSG_HIP(hipGetLastError());
    h->pers.clock.Mark(PRS_COMPOSE);
    ++launches;
    if (mem_out == VSG_MEM_HOST) {
      VSG_HIP(hipMemcpy2DAsync(out, out_stride, dst.p, dst.stride, row_bytes, H, hipMemcpyDeviceToHost, h->stream));
      ++launches;
    }
    FinishPersistence(h, vector, launches);
    *num_levels = levels;
  });
}

int vsg_render_persistence_graph(vsg_render* h, const uint8_t* seg, size_t seg_len, int neighbourhood,
                                 vsg_render_level_node* nodes, size_t capacity_nodes, size_t* num_nodes,
                                 vsg_render_level_edge* edges, size_t capacity_edges, size_t* num_edges,
                                 int32_t* persistence, int64_t* level_sides, size_t capacity_levels,
                                 size_t* num_levels, int mem_out) {
  return Guard([&] {
    using namespace vsg_render_impl;
    if (neighbourhood != VSG_RENDER_ADJACENT_N4 && neighbourhood != VSG_RENDER_ADJACENT_N8) {
      Throw(VSG_ERR_INVALID, "neighbourhood is neither VSG_RENDER_ADJACENT_N4 nor VSG_RENDER_ADJACENT_N8");
    }
    if (!h) Throw(VSG_ERR_INVALID, "handle is null");
    if (!num_nodes || !num_edges || !num_levels) Throw(VSG_ERR_INVALID, "a count pointer is null");
    *num_nodes = *num_edges = *num_levels = 0;
    CheckMem(mem_out, "outputs");
    const bool count_only = !nodes && !edges && !persistence && !level_sides && capacity_nodes == 0 &&
                            capacity_edges == 0 && capacity_levels == 0;
    DeviceGuard guard(h->device);
    vsg_render_persistence_stats& ps = h->pers.stats;
    std::memset(&ps, 0, sizeof(ps));

    // ---- the level-0 graph, left on the device ----
    size_t n_nodes = 0, n_edges = 0;
    LevelAdjacency(h, seg, seg_len, 0, 0, neighbourhood, nullptr, 0, &n_nodes, nullptr, 0, &n_edges, VSG_MEM_DEVICE);
    const vsg_render_adjacency_stats& as = h->adj.stats;
    ps.nodes = (int64_t)n_nodes;
    ps.edges = (int64_t)n_edges;
    ps.plane_us = as.plane_us;
    ps.graph_us = as.count_us + as.emit_us + as.sort_us + as.table_us;
    int launches = 0;
    auto finish = [&] {
      h->stats.launches += launches;
      ps.launches = h->stats.launches;
      h->stats.device_allocations = h->allocations;
    };

    // ---- the ancestors of every region that paints, by ascending id ----
    const ParsedDesc& d = h->desc;
    const bool vector = d.rasterization_removed && d.has_mesh;
    h->pers.ids.clear();
    for (size_t r = 0; r < d.region_ids.size(); ++r) {
      const bool paints = vector ? d.region_poly_begin[r] != d.region_poly_begin[r + 1]
                                 : d.region_begin[r] != d.region_begin[r + 1];
      if (paints) h->pers.ids.push_back(d.region_ids[r]);   // none is negative: the adjacency call refused those
    }
    std::sort(h->pers.ids.begin(), h->pers.ids.end());
    h->pers.ids.erase(std::unique(h->pers.ids.begin(), h->pers.ids.end()), h->pers.ids.end());
    int L = 1;
    try {
      L = BuildPersistenceTable(h);
    } catch (...) {
      finish();
      throw;
    }
    ps.levels = L;
    ps.regions = (int64_t)h->pers.ids.size();
    *num_nodes = n_nodes;
    *num_edges = n_edges;
    *num_levels = (size_t)L;

    // ---- one thread per edge, then the levels' sums ----
    const size_t hist_bytes = ((size_t)L + 1) * sizeof(unsigned long long);
    const size_t sides_bytes = (size_t)L * sizeof(int64_t);
    const size_t pers_bytes = n_edges * sizeof(int32_t);
    h->pers.out.Reserve(hist_bytes + sides_bytes + pers_bytes, &h->allocations);
    h->pers.status.Reserve(sizeof(PersStatus), &h->allocations);
    unsigned long long* hist = h->pers.out.As<unsigned long long>();
    long long* d_sides = reinterpret_cast<long long*>(hist + L + 1);
    int32_t* d_pers = reinterpret_cast<int32_t*>(d_sides + L);
    PersStatus* status = h->pers.status.As<PersStatus>();
    // the table has left the pinned block by the time the status and the lists arrive in it
    const size_t nb = n_nodes * sizeof(vsg_render_level_node), eb = n_edges * sizeof(vsg_render_level_edge);
    const bool fits = n_nodes <= capacity_nodes && n_edges <= capacity_edges && (size_t)L <= capacity_levels;
    const bool have = (n_nodes == 0 || nodes) && level_sides && (n_edges == 0 || (edges && persistence));
    const bool to_host = !count_only && fits && have && mem_out == VSG_MEM_HOST;
    const int32_t* table = UploadPersistenceTable(
        h, sizeof(PersStatus) + (to_host ? sides_bytes + nb + eb + pers_bytes : 0), &launches);
    VSG_HIP(hipMemsetAsync(status, 0, sizeof(PersStatus), h->stream));
    VSG_HIP(hipMemsetAsync(hist, 0, hist_bytes, h->stream));
    h->pers.clock.Begin(h->stream);
    LaunchPersistEdges(h->adj.nodes.As<int32_t>(), (uint32_t)n_nodes, h->adj.edges.As<int32_t>(),
                       (uint32_t)n_edges, h->pers.anc.As<int32_t>(), (uint32_t)h->pers.ids.size(), table, L, d_pers,
                       hist, status, h->stream);
    LaunchPersistSides(hist, L, d_sides, h->stream);
    VSG_HIP(hipGetLastError());
    h->pers.clock.Mark(PRS_PERSIST);
    launches += 3 + (n_edges ? 1 : 0);
    char* stage = h->pers.seen.As<char>();
    VSG_HIP(hipMemcpyAsync(stage, status, sizeof(PersStatus), hipMemcpyDeviceToHost, h->stream));
    ++launches;
    VSG_HIP(hipStreamSynchronize(h->stream));
    {
      float us[PRS_STAGES];
      h->pers.clock.Read(us, PRS_STAGES);
      ps.persist_us = us[PRS_PERSIST];
    }
    if (reinterpret_cast<const PersStatus*>(stage)->flags) {
      finish();
      Throw(VSG_ERR_INTERNAL, "an edge of the level-0 graph, its node or a region id is out of range");
    }
    if (count_only) return finish();
    if (!fits) {
      finish();
      Throw(VSG_ERR_INVALID, "the graph has " + std::to_string(n_nodes) + " nodes and " + std::to_string(n_edges) +
                                 " edges, the hierarchy " + std::to_string(L) + " levels; the capacities are " +
                                 std::to_string(capacity_nodes) + ", " + std::to_string(capacity_edges) + " and " +
                                 std::to_string(capacity_levels));
    }
    if (!have) {
      finish();
      Throw(VSG_ERR_INVALID, "an output is null");
    }
    // the lengths are known: four copies, through the pinned block (it has the room since the table's upload)
    // for host outputs
    const std::initializer_list<Delivery> lists = {{d_sides, sides_bytes, level_sides},
                                                   {h->adj.nodes.p, nb, nodes},
                                                   {h->adj.edges.p, eb, edges},
                                                   {d_pers, pers_bytes, persistence}};
    if (to_host) {
      launches += DeliverToHost(h, &h->pers.seen, sizeof(PersStatus), lists);
    } else {
      for (const Delivery& l : lists) {
        if (!l.bytes) continue;
        VSG_HIP(hipMemcpyAsync(l.to, l.from, l.bytes, hipMemcpyDeviceToDevice, h->stream));
        ++launches;
      }
      VSG_HIP(hipStreamSynchronize(h->stream));
    }
    finish();
  });
}

VSG_RENDER_LAST_STATS(vsg_render_last_persistence_stats, vsg_render_persistence_stats, pers.stats)

}  // extern "C"
