// capi_adjacency.inc -- vsg_render_level_adjacency.  A part of render_capi.cpp.
namespace {

// The body of vsg_render_level_adjacency; vsg_render_persistence_graph runs it for the counts alone and
// takes the lists from h->adj.nodes and h->adj.edges.
void LevelAdjacency(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness,
                    int neighbourhood, vsg_render_level_node* nodes, size_t capacity_nodes, size_t* num_nodes,
                    vsg_render_level_edge* edges, size_t capacity_edges, size_t* num_edges, int mem_out) {
  using namespace vsg_render_impl;
  static_assert(sizeof(vsg_render_level_node) == kLevelNodeWords * sizeof(int32_t), "moved as int32 words");
  static_assert(sizeof(vsg_render_level_edge) == kLevelEdgeWords * sizeof(int32_t), "moved as int32 words");
  CheckConnectedness(connectedness, true);
  if (neighbourhood != VSG_RENDER_ADJACENT_N4 && neighbourhood != VSG_RENDER_ADJACENT_N8) {
    Throw(VSG_ERR_INVALID, "neighbourhood is neither VSG_RENDER_ADJACENT_N4 nor VSG_RENDER_ADJACENT_N8");
  }
  if (!h) Throw(VSG_ERR_INVALID, "handle is null");
  if (!num_nodes || !num_edges) Throw(VSG_ERR_INVALID, "a count pointer is null");
  *num_nodes = *num_edges = 0;
  CheckMem(mem_out, "outputs");
  const bool count_only = !nodes && !edges && capacity_nodes == 0 && capacity_edges == 0;
  const bool diagonal = neighbourhood == VSG_RENDER_ADJACENT_N8;
  const int W = h->W, H = h->H;
  CheckFrameBelow2Pow32(h);
  DeviceGuard guard(h->device);
  vsg_render_adjacency_stats& as = h->adj.stats;
  std::memset(&as, 0, sizeof(as));

  // ---- the plane: the level's ids, or the indices of its regions' components ----
  const LevelPlane lp = SelectLevelPlane(h, seg, seg_len, level, connectedness, &as.plane_us, &as.launches);
  const int group_bits = BitsFor(lp.max_group, 31);

  // ---- count: the number of keys sizes everything below ----
  // seen: [0] after the count, [1] at the end
  auto [status, seen] = ReserveStatusPair<AdjStatus>(h, &h->adj.status, &h->adj.seen);
  VSG_HIP(hipMemsetAsync(status, 0, sizeof(AdjStatus), h->stream));
  h->adj.clock.Begin(h->stream);
  LaunchAdjClassify(lp.plane, W, H, group_bits, diagonal, false, 0, nullptr, status, h->stream);
  VSG_HIP(hipGetLastError());
  h->adj.clock.Mark(ADJ_COUNT);
  VSG_HIP(hipMemcpyAsync(&seen[0], status, sizeof(AdjStatus), hipMemcpyDeviceToHost, h->stream));
  int launches = 3;
  VSG_HIP(hipStreamSynchronize(h->stream));
  {
    float us[ADJ_STAGES];
    h->adj.clock.Read(us, ADJ_STAGES);
    as.count_us = us[ADJ_COUNT];
  }
  FinishLevelPlane(h, lp, &as.plane_us);
  auto finish = [&] { CountLaunches(h, &as.launches, launches); };
  if (seen[0].keys > 0x7fffffffull) {
    finish();
    Throw(VSG_ERR_INVALID, "the level has more than 2^31 - 1 bordering sides and diagonal contacts");
  }
  const uint32_t n = (uint32_t)seen[0].keys;
  as.sides = as.keys = n;
  if (n == 0) return finish();   // no covered pixel: both lists are empty

  // ---- emit, sort, table ----
  const uint32_t cap_nodes = (uint32_t)std::min<uint64_t>(lp.groups_bound, n);   // every group has a key
  if (cap_nodes == 0) Throw(VSG_ERR_INTERNAL, "the plane has groups the desc has no ids for");
  const uint32_t cap_edges = n;                                               // every edge has a key
  const int end_bit = 2 * group_bits + 2;
  const size_t temp_bytes = MaxBytes({SortKeysU64TempBytes(n, end_bit), HeadScanTempBytes<AdjHeads>(n)});
  const size_t node_bytes = (size_t)cap_nodes * sizeof(vsg_render_level_node);
  const size_t edge_bytes = (size_t)cap_edges * sizeof(vsg_render_level_edge);
  h->d_sort_temp.Reserve(temp_bytes, &h->allocations);
  h->adj.keys.Reserve((size_t)n * 2 * sizeof(unsigned long long), &h->allocations);
  h->adj.heads.Reserve((size_t)n * sizeof(unsigned long long), &h->allocations);
  h->adj.nodes.Reserve(node_bytes, &h->allocations);
  h->adj.edges.Reserve(edge_bytes, &h->allocations);
  unsigned long long* keys = h->adj.keys.As<unsigned long long>();
  unsigned long long* keys_sorted = keys + n;
  unsigned long long* heads = h->adj.heads.As<unsigned long long>();
  int32_t* d_nodes = h->adj.nodes.As<int32_t>();
  int32_t* d_edges = h->adj.edges.As<int32_t>();
  h->adj.clock.Begin(h->stream);
  LaunchAdjClassify(lp.plane, W, H, group_bits, diagonal, true, n, keys, status, h->stream);
  VSG_HIP(hipGetLastError());
  h->adj.clock.Mark(ADJ_EMIT);
  VSG_HIP(SortKeysU64(h->d_sort_temp.p, temp_bytes, keys, keys_sorted, n, end_bit, h->stream));
  h->adj.clock.Mark(ADJ_SORT);
  VSG_HIP(hipMemsetAsync(d_nodes, 0, node_bytes, h->stream));   // the counts are summed into them
  VSG_HIP(hipMemsetAsync(d_edges, 0, edge_bytes, h->stream));
  VSG_HIP(HeadScan(h->d_sort_temp.p, temp_bytes, AdjHeads{keys_sorted, group_bits}, heads, n, h->stream));
  LaunchAdjTable(keys_sorted, heads, n, group_bits, lp.max_group, cap_nodes, cap_edges, lp.comp_table, d_nodes, d_edges,
                 status, h->stream);
  VSG_HIP(hipGetLastError());
  h->adj.clock.Mark(ADJ_TABLE);
  // emit, the sort and the scan counted as one each, two clears, table, finish, resolve
  launches += 7 + (lp.comp_table ? 0 : 1);
  const bool to_device = !count_only && mem_out == VSG_MEM_DEVICE && nodes && edges;
  if (to_device) {
    // the lengths of both lists are on the device: the copy decides there whether they fit
    CopyLists lists = {};
    lists.list[0] = {d_nodes, reinterpret_cast<int32_t*>(nodes), kLevelNodeWords, &status->nodes, 0,
                     (uint32_t)std::min<size_t>(capacity_nodes, cap_nodes)};
    lists.list[1] = {d_edges, reinterpret_cast<int32_t*>(edges), kLevelEdgeWords, &status->edges, 0,
                     (uint32_t)std::min<size_t>(capacity_edges, cap_edges)};
    lists.flags = &status->flags;
    LaunchCopyLists(lists, h->stream);
    VSG_HIP(hipGetLastError());
    ++launches;
  }
  VSG_HIP(hipMemcpyAsync(&seen[1], status, sizeof(AdjStatus), hipMemcpyDeviceToHost, h->stream));
  ++launches;
  VSG_HIP(hipStreamSynchronize(h->stream));
  {
    float us[ADJ_STAGES];
    h->adj.clock.Read(us, ADJ_STAGES);
    as.emit_us = us[ADJ_EMIT];
    as.sort_us = us[ADJ_SORT];
    as.table_us = us[ADJ_TABLE];
  }
  if ((seen[1].flags & ADJ_FLAG_OVERFLOW) || seen[1].emitted != n) {
    finish();
    Throw(VSG_ERR_INTERNAL, "the emit pass found other adjacency keys than the count pass");
  }
  if ((seen[1].flags & ADJ_FLAG_RANGE) || seen[1].nodes == 0 || seen[1].nodes > cap_nodes ||
      seen[1].edges > cap_edges || (lp.comp_table && seen[1].nodes != lp.groups_bound)) {
    finish();
    Throw(VSG_ERR_INTERNAL, "a sorted adjacency key, a node or an edge is out of range");
  }
  const size_t n_nodes = seen[1].nodes, n_edges = seen[1].edges;
  *num_nodes = n_nodes;
  *num_edges = n_edges;
  as.nodes = (int64_t)n_nodes;
  as.edges = (int64_t)n_edges;
  as.largest_node_edges = seen[1].largest;
  if (count_only) return finish();
  if (n_nodes > capacity_nodes || n_edges > capacity_edges) {
    finish();
    Throw(VSG_ERR_INVALID, "the level has " + std::to_string(n_nodes) + " nodes and " + std::to_string(n_edges) +
                               " edges, the capacities are " + std::to_string(capacity_nodes) + " and " +
                               std::to_string(capacity_edges));
  }
  if (!nodes || (n_edges && !edges)) {
    finish();
    Throw(VSG_ERR_INVALID, "an output is null");
  }
  if (mem_out == VSG_MEM_HOST) {
    // there is a node, there may be no edge
    launches += DeliverToHost(h, &h->adj.seen, 2 * sizeof(AdjStatus),
                              {{d_nodes, n_nodes * sizeof(vsg_render_level_node), nodes},
                               {d_edges, n_edges * sizeof(vsg_render_level_edge), edges}});
  } else if (!to_device) {
    // edges was null with no edge to deliver: the copy kernel was not launched
    VSG_HIP(hipMemcpyAsync(nodes, d_nodes, n_nodes * sizeof(vsg_render_level_node), hipMemcpyDeviceToDevice,
                           h->stream));
    ++launches;
    VSG_HIP(hipStreamSynchronize(h->stream));
  }
  finish();
}

}  // namespace

extern "C" {

int vsg_render_level_adjacency(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness,
                               int neighbourhood, vsg_render_level_node* nodes, size_t capacity_nodes,
                               size_t* num_nodes, vsg_render_level_edge* edges, size_t capacity_edges,
                               size_t* num_edges, int mem_out) {
  return Guard([&] {
    LevelAdjacency(h, seg, seg_len, level, connectedness, neighbourhood, nodes, capacity_nodes, num_nodes, edges,
                   capacity_edges, num_edges, mem_out);
  });
}

VSG_RENDER_LAST_STATS(vsg_render_last_adjacency_stats, vsg_render_adjacency_stats, adj.stats)

}  // extern "C"
