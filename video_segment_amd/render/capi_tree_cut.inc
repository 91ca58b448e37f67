// capi_tree_cut.inc -- vsg_render_tree_cut, vsg_render_tree_cut_tuning and vsg_render_last_cut_stats.  A part
// of render_capi.cpp, after capi_persistence.inc, whose ancestor table it takes.
namespace {

constexpr int64_t kCutMaxGain = 1ll << 32;         // of a penalty and of a table's gain
constexpr uint64_t kCutMaxEntries = 1ull << 27;    // L * R + L * P
constexpr int64_t kCutDefaultBlockNodes = 32768;   // unmeasured: see DESIGN 5t

// The node table's arrays in one block of T nodes; the first kCutZeroBytes * T bytes have to be zero before the
// node table is made.
constexpr size_t kCutZeroBytes = 32, kCutNodeBytes = 76;
struct CutArrays {
  vsg_render_impl::CutNodes nodes;
  unsigned long long* best;
  uint32_t *selected, *place;
};
CutArrays CarveCutNodes(void* block, size_t T) {
  CutArrays a;
  unsigned long long* q = static_cast<unsigned long long*>(block);
  a.nodes.sum = q;
  a.best = q + T;
  uint32_t* w = reinterpret_cast<uint32_t*>(q + 2 * T);
  a.nodes.area = w;
  a.nodes.leaves = w + T;
  a.nodes.children = w + 2 * T;
  a.selected = w + 3 * T;
  long long* g = reinterpret_cast<long long*>(w + 4 * T);
  a.nodes.gain = g;
  a.nodes.split = g + T;
  int32_t* i = reinterpret_cast<int32_t*>(g + 2 * T);
  a.nodes.level = i;
  a.nodes.id = i + T;
  a.nodes.parent = i + 2 * T;
  a.nodes.best_label = i + 3 * T;
  a.nodes.best_count = i + 4 * T;
  a.nodes.keep = reinterpret_cast<uint32_t*>(i + 5 * T);
  a.place = reinterpret_cast<uint32_t*>(i + 6 * T);
  return a;
}

}  // namespace

extern "C" {

int vsg_render_tree_cut(vsg_render* h, const uint8_t* seg, size_t seg_len, const int32_t* labels,
                        size_t labels_pitch, int mem_labels, int64_t penalty, const vsg_render_cut_gain* gains,
                        size_t num_gains, int mem_gains, vsg_render_cut_node* nodes, size_t capacity_nodes,
                        size_t* num_nodes, int32_t* plane, int64_t* total, int mem_out) {
  return Guard([&] {
    using namespace vsg_render_impl;
    static_assert(sizeof(vsg_render_cut_node) == kCutNodeWords * sizeof(int32_t), "moved as int32 words");
    static_assert(sizeof(vsg_render_cut_gain) == sizeof(CutGain), "read as is");
    if (penalty < 0 || penalty > kCutMaxGain) {
      Throw(VSG_ERR_INVALID, "penalty " + std::to_string(penalty) + " is not in [0, 2^32]");
    }
    if (labels && gains) Throw(VSG_ERR_INVALID, "both labels and a gain table are given");
    if (!labels && !gains) Throw(VSG_ERR_INVALID, "neither labels nor a gain table is given");
    if (!h) Throw(VSG_ERR_INVALID, "handle is null");
    if (!num_nodes || !total) Throw(VSG_ERR_INVALID, "a count pointer is null");
    *num_nodes = 0;
    *total = 0;
    if (labels) CheckMem(mem_labels, "labels");
    if (gains) CheckMem(mem_gains, "gains");
    CheckMem(mem_out, "outputs");
    if (labels) (void)CheckOtherPitch(h, labels_pitch);
    const bool count_only = !nodes && !plane && capacity_nodes == 0;
    CheckFrameBelow2Pow32(h);
    const int W = h->W, H = h->H;
    DeviceGuard guard(h->device);
    vsg_render_cut_stats& cs = h->cut.stats;
    std::memset(&cs, 0, sizeof(cs));
    cs.block_nodes = h->cut.block_nodes;

    // ---- level 0: the regions of the id image with their areas and, with labels, their pairs; on the device ----
    size_t n_leaves = 0, n_pairs = 0;
    const int32_t* list = nullptr;
    uint32_t list_words = 0, area_word = 0;
    int launches = 0;
    if (labels) {
      size_t n_cols = 0;
      const int rc = vsg_render_level_overlap(h, seg, seg_len, 0, 0, labels, labels_pitch, mem_labels, nullptr, 0,
                                              &n_leaves, nullptr, 0, &n_cols, nullptr, 0, &n_pairs, VSG_MEM_DEVICE);
      if (rc != VSG_OK) Throw(rc, g_last_error);
      const vsg_render_overlap_stats& os = h->ovl.stats;
      cs.plane_us = os.plane_us;
      cs.table_us = os.count_us + os.emit_us + os.sort_us + os.table_us;
      list = h->ovl.rows.As<int32_t>();
      list_words = kOverlapRowWords;
      area_word = 4;
    } else {
      size_t n_intervals = 0;
      const int rc = vsg_render_level_regions(h, seg, seg_len, 0, nullptr, 0, &n_leaves, nullptr, 0, &n_intervals,
                                              VSG_MEM_DEVICE);
      if (rc != VSG_OK) Throw(rc, g_last_error);
      const vsg_render_level_stats& ls = h->lvl.stats;
      cs.plane_us = h->stats.clear_us + h->stats.fill_us;
      cs.table_us = ls.runs_us + ls.sort_us + ls.table_us;
      list = h->lvl.regions.As<int32_t>();
      list_words = kLevelRegionWords;
      area_word = 3;
      if (n_leaves) {
        // a count-only call leaves the areas out: the moments' kernel, on the lists it left on the device
        LaunchLevelMoments(h->lvl.intervals.As<Interval>(), (uint32_t)n_intervals, (uint32_t)n_leaves,
                           h->lvl.regions.As<int32_t>(), h->lvl.status.As<LevelStatus>(), h->stream);
        VSG_HIP(hipGetLastError());
        ++launches;
      }
    }
    auto finish = [&] {
      h->stats.launches += launches;
      launches = 0;
      cs.launches = h->stats.launches;
      h->stats.device_allocations = h->allocations;
    };
    auto fail = [&](int code, const std::string& text) {
      finish();
      Throw(code, text);
    };

    // ---- the ancestors of every region that paints, by ascending id ----
    const ParsedDesc& d = h->desc;
    const bool vector = d.rasterization_removed && d.has_mesh;
    h->pers.ids.clear();
    for (size_t r = 0; r < d.region_ids.size(); ++r) {
      const bool paints = vector ? d.region_poly_begin[r] != d.region_poly_begin[r + 1]
                                 : d.region_begin[r] != d.region_begin[r + 1];
      if (paints) h->pers.ids.push_back(d.region_ids[r]);   // none is negative: the level-0 call refused those
    }
    std::sort(h->pers.ids.begin(), h->pers.ids.end());
    h->pers.ids.erase(std::unique(h->pers.ids.begin(), h->pers.ids.end()), h->pers.ids.end());
    const uint64_t height = PersistenceHeight(h->kept.size());
    if (height <= 65535 && height * ((uint64_t)n_leaves + n_pairs) > kCutMaxEntries) {
      fail(VSG_ERR_INVALID, "the hierarchy has L = " + std::to_string(height) + " levels, the frame R = " +
                                std::to_string(n_leaves) + " regions and P = " + std::to_string(n_pairs) +
                                " pairs: L * R + L * P is above 2^27");
    }
    int levels = 1;
    try {
      levels = BuildPersistenceTable(h);
    } catch (...) {
      finish();
      throw;
    }
    const uint32_t L = (uint32_t)levels, R = (uint32_t)n_leaves, P = (uint32_t)n_pairs;
    const uint32_t n_ids = (uint32_t)h->pers.ids.size();
    const uint32_t N = L * R, M = L * P;
    cs.levels = L;
    cs.leaves = R;
    cs.pairs = P;
    cs.entries = (int64_t)N + M;

    // ---- the lift, up to the number of nodes ----
    const CutGain* d_gains = reinterpret_cast<const CutGain*>(gains);
    if (gains && num_gains && mem_gains == VSG_MEM_HOST) {
      h->cut.gains.Reserve(num_gains * sizeof(CutGain), &h->allocations);
      VSG_HIP(hipMemcpyAsync(h->cut.gains.p, gains, num_gains * sizeof(CutGain), hipMemcpyHostToDevice, h->stream));
      ++launches;
      d_gains = h->cut.gains.As<CutGain>();
    }
    const StatusPair<CutStatus> words = ReserveStatusPair<CutStatus>(h, &h->cut.status, &h->cut.seen);
    CutStatus* const status = words.status;
    CutStatus* seen = words.seen;   // [0] after the lift, [1] after the records and at the end
    const size_t level_bytes = ((size_t)L + 1) * sizeof(uint32_t);
    h->cut.levels.Reserve(level_bytes, &h->allocations);
    h->cut.levels_seen.Reserve(level_bytes, &h->allocations);
    h->cut.leaves.Reserve(std::max<size_t>(R, 1) * 4 * sizeof(uint32_t), &h->allocations);
    h->cut.lift.Reserve(std::max<size_t>(N, 1) * 32, &h->allocations);
    const int node_end_bit = 32 + BitsFor(L - 1, 16);
    size_t temp_bytes = MaxBytes({SortPairsU64U32TempBytes(N, node_end_bit), HeadScanTempBytes<CutKeyHead>(N),
                                  HeadScanTempBytes<CutMark>(N)});
    h->d_sort_temp.Reserve(temp_bytes, &h->allocations);
    int32_t* leaf_id = h->cut.leaves.As<int32_t>();
    uint32_t* leaf_area = reinterpret_cast<uint32_t*>(leaf_id) + R;
    uint32_t* leaf_col = leaf_area + R;
    uint32_t* leaf_node = leaf_col + R;
    unsigned long long* keys = h->cut.lift.As<unsigned long long>();
    unsigned long long* keys_sorted = keys + N;
    uint32_t* vals = reinterpret_cast<uint32_t*>(keys + 2 * (size_t)N);
    uint32_t* vals_sorted = vals + N;
    uint32_t* rank = vals + 2 * (size_t)N;
    uint32_t* map = vals + 3 * (size_t)N;
    uint32_t* level_first = h->cut.levels.As<uint32_t>();
    const int32_t* table = UploadPersistenceTable(h, 0, &launches);
    VSG_HIP(hipMemsetAsync(status, 0, sizeof(CutStatus), h->stream));
    VSG_HIP(hipMemsetAsync(level_first, 0, level_bytes, h->stream));
    launches += 2;
    h->cut.clock.Begin(h->stream);
    if (gains && num_gains) {
      LaunchCutGainCheck(d_gains, num_gains, status, h->stream);
      ++launches;
    }
    if (N) {
      LaunchCutLeaves(list, list_words, area_word, R, h->pers.anc.As<int32_t>(), n_ids, leaf_id, leaf_area, leaf_col,
                      status, h->stream);
      LaunchCutNodeKeys(leaf_id, leaf_col, R, table, n_ids, L, keys, vals, h->stream);
      VSG_HIP(hipGetLastError());
      VSG_HIP(SortPairsU64U32(h->d_sort_temp.p, temp_bytes, keys, keys_sorted, vals, vals_sorted, N, node_end_bit,
                              h->stream));
      VSG_HIP(HeadScan(h->d_sort_temp.p, temp_bytes, CutKeyHead{keys_sorted}, rank, N, h->stream));
      LaunchCutNodeMap(vals_sorted, rank, R, L, map, level_first, status, h->stream);
      launches += 5;   // the sort and the scan count as one each
    }
    VSG_HIP(hipGetLastError());
    h->cut.clock.Mark(CUT_LIFT);
    uint32_t* first_seen = h->cut.levels_seen.As<uint32_t>();
    VSG_HIP(hipMemcpyAsync(&seen[0], status, sizeof(CutStatus), hipMemcpyDeviceToHost, h->stream));
    VSG_HIP(hipMemcpyAsync(first_seen, level_first, level_bytes, hipMemcpyDeviceToHost, h->stream));
    launches += 2;
    VSG_HIP(hipStreamSynchronize(h->stream));
    auto read_clock = [&] {
      float us[CUT_STAGES];
      h->cut.clock.Read(us, CUT_STAGES);
      cs.lift_us = us[CUT_LIFT];
      cs.dp_us = us[CUT_DP];
      cs.paint_us = us[CUT_PAINT];
    };
    if (seen[0].flags & CUT_FLAG_GAIN_ORDER) {
      fail(VSG_ERR_INVALID, "the gain table is not strictly ascending by (level, id)");
    }
    if (seen[0].flags & CUT_FLAG_GAIN_RANGE) fail(VSG_ERR_INVALID, "a gain of the table is not in [-2^32, 2^32]");
    const uint32_t T = seen[0].tree_nodes;
    if ((seen[0].flags & CUT_FLAG_RANGE) || (N != 0) != (T != 0) || T > N || (T && T < L)) {
      fail(VSG_ERR_INTERNAL, "a region of the level-0 list has no ancestors, or the lifted keys are out of range");
    }
    cs.tree_nodes = T;
    const size_t plane_bytes = (size_t)W * H * sizeof(int32_t);
    if (T == 0) {
      // no region in the frame: no record, and -1 everywhere
      read_clock();
      if (plane && mem_out == VSG_MEM_DEVICE) {
        VSG_HIP(hipMemsetAsync(plane, 0xff, plane_bytes, h->stream));
        ++launches;
        VSG_HIP(hipStreamSynchronize(h->stream));
      } else if (plane) {
        std::memset(plane, 0xff, plane_bytes);
      }
      return finish();
    }

    // ---- the node table and the gains ----
    h->cut.nodes.Reserve((size_t)T * kCutNodeBytes, &h->allocations);
    const CutArrays a = CarveCutNodes(h->cut.nodes.p, T);
    const uint32_t cap_records = std::min(T, R);   // the selected nodes partition the leaves
    h->cut.records.Reserve((size_t)cap_records * sizeof(vsg_render_cut_node), &h->allocations);
    int32_t* d_records = h->cut.records.As<int32_t>();
    h->cut.clock.Mark(CUT_WAIT);
    VSG_HIP(hipMemsetAsync(h->cut.nodes.p, 0, (size_t)T * kCutZeroBytes, h->stream));
    LaunchCutNodeTable(keys_sorted, vals_sorted, rank, map, leaf_area, R, L, T, a.nodes, h->stream);
    VSG_HIP(hipGetLastError());
    launches += 2;
    if (labels) {
      if (M) {
        const int label_bits = BitsFor(h->ovl.seen.As<OvlStatus>()[0].max_label, 31);
        const int pair_end_bit = label_bits + BitsFor(T - 1, 31);
        temp_bytes = MaxBytes({temp_bytes, SortPairsU64U32TempBytes(M, pair_end_bit),
                               HeadScanTempBytes<CutKeyHead>(M)});
        h->d_sort_temp.Reserve(temp_bytes, &h->allocations);
        h->cut.pairs.Reserve((size_t)M * 32, &h->allocations);
        unsigned long long* pkeys = h->cut.pairs.As<unsigned long long>();
        unsigned long long* pkeys_sorted = pkeys + M;
        uint32_t* counts = reinterpret_cast<uint32_t*>(pkeys + 2 * (size_t)M);
        uint32_t* counts_sorted = counts + M;
        uint32_t* prank = counts + 2 * (size_t)M;
        uint32_t* sums = counts + 3 * (size_t)M;
        VSG_HIP(hipMemsetAsync(sums, 0, (size_t)M * sizeof(uint32_t), h->stream));
        LaunchCutPairKeys(h->ovl.pairs.As<int32_t>(), P, map, R, L, label_bits, pkeys, counts, h->stream);
        VSG_HIP(hipGetLastError());
        VSG_HIP(SortPairsU64U32(h->d_sort_temp.p, temp_bytes, pkeys, pkeys_sorted, counts, counts_sorted, M,
                                pair_end_bit, h->stream));
        VSG_HIP(HeadScan(h->d_sort_temp.p, temp_bytes, CutKeyHead{pkeys_sorted}, prank, M, h->stream));
        LaunchCutBest(pkeys_sorted, counts_sorted, prank, M, label_bits, T, sums, a.best, status, h->stream);
        launches += 6;
      }
      LaunchCutGainLabels(a.best, T, penalty, a.nodes, h->stream);
    } else {
      LaunchCutGainLookup(d_gains, num_gains, T, a.nodes, h->stream);
    }
    VSG_HIP(hipGetLastError());
    ++launches;
    h->cut.clock.Mark(CUT_LIFT);

    // ---- the dynamic programme: one workgroup, or a launch per level ----
    if ((int64_t)T <= h->cut.block_nodes) {
      LaunchCutDpBlock(level_first, L, a.nodes, h->stream);
      cs.dp_path = 1;
      cs.dp_launches = 1;
    } else {
      for (uint32_t l = 0; l < L; ++l) {
        if (first_seen[l + 1] <= first_seen[l] || first_seen[l + 1] > T) {
          fail(VSG_ERR_INTERNAL, "a level of the hierarchy has no node");
        }
        LaunchCutDpLevel(first_seen[l], first_seen[l + 1], a.nodes, h->stream);
      }
      cs.dp_path = 2;
      cs.dp_launches = (int)L;
    }
    VSG_HIP(hipGetLastError());
    launches += cs.dp_launches;
    h->cut.clock.Mark(CUT_DP);

    // ---- select, order, records ----
    LaunchCutSelect(map, R, L, T, a.nodes.keep, leaf_node, a.selected, status, h->stream);
    VSG_HIP(hipGetLastError());
    VSG_HIP(HeadScan(h->d_sort_temp.p, temp_bytes, CutMark{a.selected}, a.place, T, h->stream));
    LaunchCutRecords(a.selected, a.place, T, cap_records, a.nodes, d_records, status, h->stream);
    VSG_HIP(hipGetLastError());
    h->cut.clock.Mark(CUT_PAINT);
    VSG_HIP(hipMemcpyAsync(&seen[1], status, sizeof(CutStatus), hipMemcpyDeviceToHost, h->stream));
    launches += 4;
    VSG_HIP(hipStreamSynchronize(h->stream));
    if ((seen[1].flags & CUT_FLAG_RANGE) || seen[1].cut_nodes == 0 || seen[1].cut_nodes > cap_records) {
      fail(VSG_ERR_INTERNAL, "a node, a pair key or a record of the cut is out of range");
    }
    const size_t n_cut = seen[1].cut_nodes;
    *num_nodes = n_cut;
    *total = (int64_t)seen[1].total;
    cs.cut_nodes = (int64_t)n_cut;
    cs.total = (int64_t)seen[1].total;
    cs.covered = (int64_t)seen[1].covered;
    if (count_only) {
      read_clock();
      return finish();
    }
    if (n_cut > capacity_nodes) {
      read_clock();
      fail(VSG_ERR_INVALID, "the cut has " + std::to_string(n_cut) + " nodes, the capacity is " +
                                std::to_string(capacity_nodes));
    }
    if (!nodes) {
      read_clock();
      fail(VSG_ERR_INVALID, "an output is null");
    }

    // ---- the plane and the outputs, now that they fit ----
    const size_t record_bytes = n_cut * sizeof(vsg_render_cut_node);
    const bool to_host = mem_out == VSG_MEM_HOST;
    if (to_host) {
      // the pinned block may move: nothing is in flight, and what was read of the status words is used
      h->cut.seen.Reserve(2 * sizeof(CutStatus) + record_bytes + (plane ? plane_bytes : 0), &h->allocations);
      seen = h->cut.seen.As<CutStatus>();
      if (plane) h->cut.plane.Reserve(plane_bytes, &h->allocations);
    }
    int32_t* d_plane = to_host ? h->cut.plane.As<int32_t>() : plane;
    h->cut.clock.Mark(CUT_WAIT);
    if (plane) {
      LaunchCutPaint(h->d_ids.As<int32_t>(), W, H, leaf_id, R, leaf_node, a.place, d_plane, status, h->stream);
      VSG_HIP(hipGetLastError());
      ++launches;
    }
    h->cut.clock.Mark(CUT_PAINT);
    VSG_HIP(hipMemcpyAsync(&seen[1], status, sizeof(CutStatus), hipMemcpyDeviceToHost, h->stream));
    ++launches;
    if (to_host) {
      launches += DeliverToHost(h, &h->cut.seen, 2 * sizeof(CutStatus),
                                {{d_records, record_bytes, nodes}, {d_plane, plane ? plane_bytes : 0, plane}});
    } else {
      VSG_HIP(hipMemcpyAsync(nodes, d_records, record_bytes, hipMemcpyDeviceToDevice, h->stream));
      ++launches;
      VSG_HIP(hipStreamSynchronize(h->stream));
    }
    read_clock();
    finish();
    if (h->cut.seen.As<CutStatus>()[1].flags & CUT_FLAG_RANGE) {
      Throw(VSG_ERR_INTERNAL, "the plane holds an id the level-0 list does not");
    }
  });
}

int vsg_render_tree_cut_tuning(vsg_render* h, int64_t block_nodes) {
  return Guard([&] {
    if (!h) Throw(VSG_ERR_INVALID, "handle is null");
    if (block_nodes < -1) Throw(VSG_ERR_INVALID, "block_nodes is below -1");
    h->cut.block_nodes = block_nodes == -1 ? kCutDefaultBlockNodes : block_nodes;
  });
}

VSG_RENDER_LAST_STATS(vsg_render_last_cut_stats, vsg_render_cut_stats, cut.stats)

}  // extern "C"
