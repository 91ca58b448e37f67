// capi_overlap.inc -- vsg_render_level_overlap.  A part of render_capi.cpp.
extern "C" {

int vsg_render_level_overlap(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, int connectedness,
                             const int32_t* other, size_t other_pitch, int mem_other,
                             vsg_render_overlap_row* rows, size_t capacity_rows, size_t* num_rows,
                             vsg_render_overlap_col* cols, size_t capacity_cols, size_t* num_cols,
                             vsg_render_overlap_pair* pairs, size_t capacity_pairs, size_t* num_pairs,
                             int mem_out) {
  return Guard([&] {
    using namespace vsg_render_impl;
    static_assert(sizeof(vsg_render_overlap_row) == kOverlapRowWords * sizeof(int32_t), "moved as int32 words");
    static_assert(sizeof(vsg_render_overlap_col) == kOverlapColWords * sizeof(int32_t), "moved as int32 words");
    static_assert(sizeof(vsg_render_overlap_pair) == kOverlapPairWords * sizeof(int32_t), "moved as int32 words");
    if (!h) Throw(VSG_ERR_INVALID, "handle is null");
    if (!num_rows || !num_cols || !num_pairs) Throw(VSG_ERR_INVALID, "a count pointer is null");
    *num_rows = *num_cols = *num_pairs = 0;
    CheckOtherPlane(other, mem_other);
    CheckConnectedness(connectedness, true);
    CheckMem(mem_out, "outputs");
    const int W = h->W, H = h->H;
    const size_t pitch = CheckOtherPitch(h, other_pitch);
    const bool count_only =
        !rows && !cols && !pairs && capacity_rows == 0 && capacity_cols == 0 && capacity_pairs == 0;
    CheckFrameBelow2Pow32(h);
    DeviceGuard guard(h->device);
    vsg_render_overlap_stats& os = h->ovl.stats;
    std::memset(&os, 0, sizeof(os));

    // ---- P: the level's ids, or the indices of its regions' components ----
    const LevelPlane lp = SelectLevelPlane(h, seg, seg_len, level, connectedness, &os.plane_us, &os.launches);
    const int group_bits = BitsFor(lp.max_group, 31);

    // ---- B: where it is, or through the pinned block to the device, rows packed ----
    // seen: [0] after the count, [1] at the end
    auto [status, seen] = ReserveStatusPair<OvlStatus>(h, &h->ovl.status, &h->ovl.seen);
    h->ovl.totals.Reserve((size_t)H * kOverlapRowTotals * sizeof(uint32_t), &h->allocations);
    int launches = 0;
    h->ovl.clock.Begin(h->stream);
    const OtherPlane b = UploadOtherPlane(h, other, pitch, mem_other, &launches);
    h->ovl.clock.Mark(OVL_UPLOAD);

    // ---- count: the number of runs sizes everything below ----
    VSG_HIP(hipMemsetAsync(status, 0, sizeof(OvlStatus), h->stream));
    LaunchOverlapRuns(lp.plane, b.plane, b.pitch, W, H, 1, 1, false, 0, nullptr, nullptr,
                      h->ovl.totals.As<uint32_t>(), status, h->stream);
    VSG_HIP(hipGetLastError());
    h->ovl.clock.Mark(OVL_COUNT);
    VSG_HIP(hipMemcpyAsync(&seen[0], status, sizeof(OvlStatus), hipMemcpyDeviceToHost, h->stream));
    launches += 4;
    VSG_HIP(hipStreamSynchronize(h->stream));
    {
      float us[OVL_STAGES];
      h->ovl.clock.Read(us, OVL_STAGES);
      os.count_us = us[OVL_COUNT];
      os.plane_us += us[OVL_UPLOAD];
    }
    float painted_us = 0;
    FinishLevelPlane(h, lp, &painted_us);
    os.plane_us += painted_us;
    auto finish = [&] { CountLaunches(h, &os.launches, launches); };
    os.covered = seen[0].covered;
    os.labelled = seen[0].labelled;
    os.both = seen[0].both;
    os.runs = seen[0].runs;
    if (seen[0].runs > 0x7fffffffu) {
      finish();
      Throw(VSG_ERR_INVALID, "the two planes have more than 2^31 - 1 runs");
    }
    const uint32_t n = seen[0].runs;
    if (n == 0) return finish();   // nothing covered and nothing labelled: all three lists are empty

    // ---- emit, sort, table ----
    const uint32_t max_label = seen[0].max_label;
    const int label_bits = BitsFor(max_label, 31);
    const int end_bit = group_bits + label_bits + 2;
    // distinct keys: no more than runs, and no more than (groups or none) x (labels or none)
    const uint32_t m = (uint32_t)std::min<uint64_t>(n, (lp.groups_bound + 1) * ((uint64_t)max_label + 2));
    const uint32_t cap_rows = (uint32_t)std::min<uint64_t>(lp.groups_bound, n);   // every group has a run
    if (seen[0].covered && cap_rows == 0) Throw(VSG_ERR_INTERNAL, "the plane has groups the desc has no ids for");
    const size_t temp_bytes = MaxBytes({LevelTempBytes(n, end_bit), HeadScanTempBytes<OvlRowHeads>(n),
                                        HeadScanTempBytes<OvlKeyHeads>(n), HeadScanTempBytes<OvlColHeads>(n)});
    const size_t row_bytes = (size_t)cap_rows * sizeof(vsg_render_overlap_row);
    h->d_sort_temp.Reserve(temp_bytes, &h->allocations);
    h->ovl.runs.Reserve((size_t)n * 2 * 12, &h->allocations);
    h->ovl.heads.Reserve((size_t)n * 2 * sizeof(unsigned long long), &h->allocations);
    h->ovl.keys.Reserve((size_t)m * 24 + 8, &h->allocations);
    h->ovl.rows.Reserve(std::max<size_t>(row_bytes, 16), &h->allocations);
    h->ovl.cols.Reserve((size_t)m * sizeof(vsg_render_overlap_col), &h->allocations);
    h->ovl.pairs.Reserve((size_t)m * sizeof(vsg_render_overlap_pair), &h->allocations);
    // runs: keys, sorted keys, lengths, sorted lengths
    unsigned long long* keys = h->ovl.runs.As<unsigned long long>();
    unsigned long long* keys_sorted = keys + n;
    uint32_t* lengths = reinterpret_cast<uint32_t*>(keys + 2 * (size_t)n);
    uint32_t* lengths_sorted = lengths + n;
    unsigned long long* row_heads = h->ovl.heads.As<unsigned long long>();
    unsigned long long* key_heads = row_heads + n;
    // distinct keys: key, rank, start (m + 1), the columns' first keys (m + 1)
    unsigned long long* dkey = h->ovl.keys.As<unsigned long long>();
    unsigned long long* drank = dkey + m;
    uint32_t* dstart = reinterpret_cast<uint32_t*>(dkey + 2 * (size_t)m);
    uint32_t* cfirst = dstart + m + 1;
    // the column sort: its operands where the unsorted runs were, its results and the labels' ranks where
    // the scans were; m <= n, and both are read for the last time before they are written again
    unsigned long long* ckeys = keys;
    uint32_t* cvals = lengths;
    unsigned long long* ckeys_sorted = row_heads;
    uint32_t* cvals_sorted = reinterpret_cast<uint32_t*>(key_heads);
    uint32_t* col_rank = cvals_sorted + n;
    int32_t* d_rows = h->ovl.rows.As<int32_t>();
    int32_t* d_cols = h->ovl.cols.As<int32_t>();
    int32_t* d_pairs = h->ovl.pairs.As<int32_t>();
    h->ovl.clock.Begin(h->stream);
    LaunchOverlapRuns(lp.plane, b.plane, b.pitch, W, H, group_bits, label_bits, true, n, keys, lengths, nullptr,
                      status, h->stream);
    VSG_HIP(hipGetLastError());
    h->ovl.clock.Mark(OVL_EMIT);
    VSG_HIP(SortPairsU64U32(h->d_sort_temp.p, temp_bytes, keys, keys_sorted, lengths, lengths_sorted, n, end_bit,
                            h->stream));
    h->ovl.clock.Mark(OVL_SORT);
    if (row_bytes) VSG_HIP(hipMemsetAsync(d_rows, 0, row_bytes, h->stream));   // `unlabelled` of a row without any
    const OvlBits bits{group_bits, label_bits};
    VSG_HIP(HeadScan(h->d_sort_temp.p, temp_bytes, OvlRowHeads{keys_sorted, bits}, row_heads, n, h->stream));
    VSG_HIP(HeadScan(h->d_sort_temp.p, temp_bytes, OvlKeyHeads{keys_sorted, lengths_sorted}, key_heads, n, h->stream));
    LaunchOverlapTable(keys_sorted, lengths_sorted, row_heads, key_heads, n, m, group_bits, label_bits, lp.max_group,
                       cap_rows, lp.comp_table, dkey, dstart, drank, d_rows, d_pairs, ckeys, cvals, status, h->stream);
    VSG_HIP(hipGetLastError());
    VSG_HIP(SortPairsU64U32(h->d_sort_temp.p, temp_bytes, ckeys, ckeys_sorted, cvals, cvals_sorted, m, end_bit,
                            h->stream));
    VSG_HIP(HeadScan(h->d_sort_temp.p, temp_bytes, OvlColHeads{ckeys_sorted, bits}, col_rank, m, h->stream));
    LaunchOverlapCols(ckeys_sorted, cvals_sorted, col_rank, dstart, drank, m, group_bits, label_bits, cfirst, d_cols,
                      d_pairs, status, h->stream);
    VSG_HIP(hipGetLastError());
    h->ovl.clock.Mark(OVL_TABLE);
    // emit, a clear, table, pairs, rows, column heads, columns; two sorts and three scans counted as one each
    launches += 12;
    const bool to_device = !count_only && mem_out == VSG_MEM_DEVICE;
    if (to_device) {
      // the lengths of the lists are on the device: the copy decides there whether they fit
      CopyLists lists = {};
      lists.list[0] = {d_rows, reinterpret_cast<int32_t*>(rows), kOverlapRowWords, &status->rows, 0,
                       rows ? (uint32_t)std::min<size_t>(capacity_rows, cap_rows) : 0u};
      lists.list[1] = {d_cols, reinterpret_cast<int32_t*>(cols), kOverlapColWords, &status->cols, 0,
                       cols ? (uint32_t)std::min<size_t>(capacity_cols, m) : 0u};
      lists.list[2] = {d_pairs, reinterpret_cast<int32_t*>(pairs), kOverlapPairWords, &status->pairs, 0,
                       pairs ? (uint32_t)std::min<size_t>(capacity_pairs, m) : 0u};
      lists.flags = &status->flags;
      LaunchCopyLists(lists, h->stream);
      VSG_HIP(hipGetLastError());
      ++launches;
    }
    VSG_HIP(hipMemcpyAsync(&seen[1], status, sizeof(OvlStatus), hipMemcpyDeviceToHost, h->stream));
    ++launches;
    VSG_HIP(hipStreamSynchronize(h->stream));
    {
      float us[OVL_STAGES];
      h->ovl.clock.Read(us, OVL_STAGES);
      os.emit_us = us[OVL_EMIT];
      os.sort_us = us[OVL_SORT];
      os.table_us = us[OVL_TABLE];
    }
    if ((seen[1].flags & OVL_FLAG_OVERFLOW) || seen[1].emitted != n) {
      finish();
      Throw(VSG_ERR_INTERNAL, "the emit pass found other runs than the count pass");
    }
    if ((seen[1].flags & OVL_FLAG_RANGE) || seen[1].distinct == 0 || seen[1].distinct > m ||
        seen[1].rows > cap_rows || seen[1].pairs > m || seen[1].cols > m ||
        (lp.comp_table && seen[1].rows != lp.groups_bound)) {
      finish();
      Throw(VSG_ERR_INTERNAL, "a sorted overlap key, a row, a column or a pair is out of range");
    }
    const size_t n_rows = seen[1].rows, n_cols = seen[1].cols, n_pairs = seen[1].pairs;
    *num_rows = n_rows;
    *num_cols = n_cols;
    *num_pairs = n_pairs;
    os.rows = (int64_t)n_rows;
    os.cols = (int64_t)n_cols;
    os.pairs = (int64_t)n_pairs;
    os.largest_row_pairs = seen[1].largest;
    if (count_only) return finish();
    if (n_rows > capacity_rows || n_cols > capacity_cols || n_pairs > capacity_pairs) {
      finish();
      Throw(VSG_ERR_INVALID, "the table has " + std::to_string(n_rows) + " rows, " + std::to_string(n_cols) +
                                 " columns and " + std::to_string(n_pairs) + " pairs, the capacities are " +
                                 std::to_string(capacity_rows) + ", " + std::to_string(capacity_cols) + " and " +
                                 std::to_string(capacity_pairs));
    }
    if ((n_rows && !rows) || (n_cols && !cols) || (n_pairs && !pairs)) {
      finish();
      Throw(VSG_ERR_INVALID, "an output is null");
    }
    if (mem_out == VSG_MEM_HOST) {
      launches += DeliverToHost(h, &h->ovl.seen, 2 * sizeof(OvlStatus),
                                {{d_rows, n_rows * sizeof(vsg_render_overlap_row), rows},
                                 {d_cols, n_cols * sizeof(vsg_render_overlap_col), cols},
                                 {d_pairs, n_pairs * sizeof(vsg_render_overlap_pair), pairs}});
    }
    finish();
  });
}

VSG_RENDER_LAST_STATS(vsg_render_last_overlap_stats, vsg_render_overlap_stats, ovl.stats)

}  // extern "C"
