// capi_volume.inc -- the volume session: vsg_render_volume_begin, _add, _table.  A part of render_capi.cpp.
namespace {

static_assert(sizeof(vsg_render_volume_row) == vsg_render_impl::kVolumeRowBytes, "as the header says");
static_assert(sizeof(vsg_render_volume_col) == vsg_render_impl::kVolumeColBytes, "as the header says");
static_assert(sizeof(vsg_render_volume_pair) == vsg_render_impl::kVolumePairBytes, "as the header says");
static_assert(sizeof(vsg_render_volume_stats) == 112, "as the header says");

// Grows a block of the session and keeps its first `used` bytes.  The stream is idle: every call ends with a
// synchronisation.
void ReserveKeeping(vsg_render* h, Block* b, size_t bytes, size_t used) {
  if (bytes <= b->cap) return;
  Block bigger;
  bigger.pinned = b->pinned;
  bigger.Reserve(std::max(bytes, 2 * b->cap), &h->allocations);
  if (used) {
    VSG_HIP(hipMemcpyAsync(bigger.p, b->p, used, hipMemcpyDeviceToDevice, h->stream));
    VSG_HIP(hipStreamSynchronize(h->stream));
  }
  std::swap(b->p, bigger.p);
  std::swap(b->cap, bigger.cap);
}

// The session's tables as the kernels take them.
vsg_render_impl::VolumeTables VolumeTablesOf(const VolumeState& v) {
  // the entries both blocks of a table have room for
  auto room = [](const Block& keys, const Block& records, size_t record_bytes) {
    return (uint32_t)std::min<size_t>(std::min(keys.cap / 8, records.cap / record_bytes), 0x7fffffffu);
  };
  vsg_render_impl::VolumeTables t;
  t.row_keys = v.row_keys[v.rows_at].As<unsigned long long>();
  t.rows = v.rows[v.rows_at].p;
  t.n_rows = v.n_rows;
  t.cap_rows = room(v.row_keys[v.rows_at], v.rows[v.rows_at], sizeof(vsg_render_volume_row));
  t.col_keys = v.col_keys[v.cols_at].As<unsigned long long>();
  t.cols = v.cols[v.cols_at].p;
  t.n_cols = v.n_cols;
  t.cap_cols = room(v.col_keys[v.cols_at], v.cols[v.cols_at], sizeof(vsg_render_volume_col));
  t.pair_keys = v.pair_keys[v.pairs_at].As<unsigned long long>();
  t.pairs = v.pairs[v.pairs_at].p;
  t.n_pairs = v.n_pairs;
  t.cap_pairs = room(v.pair_keys[v.pairs_at], v.pairs[v.pairs_at], sizeof(vsg_render_volume_pair));
  return t;
}

// Room for `n` entries in the twin that holds a table, its first `used` entries kept.
void GrowVolumeTable(vsg_render* h, Block* keys, Block* records, size_t record_bytes, uint64_t n, uint32_t used) {
  if (n > 0x7fffffffull) Throw(VSG_ERR_INVALID, "a table of the volume session would have more than 2^31 - 1 entries");
  ReserveKeeping(h, keys, std::max<size_t>((size_t)n * 8, 16), (size_t)used * 8);
  ReserveKeeping(h, records, std::max<size_t>((size_t)n * record_bytes, 16), (size_t)used * record_bytes);
}

// A table that got new keys behind its sorted part: one radix sort of the n keys with a permutation, the records
// gathered into the twin, the twins swapped.  Returns the launches, the sort counted as one.
int ResortVolumeTable(vsg_render* h, Block (&keys)[2], Block (&records)[2], int* at, size_t record_bytes, uint32_t n,
                      int end_bit) {
  using namespace vsg_render_impl;
  VolumeState& v = h->vol;
  const int from = *at, to = 1 - from;
  const size_t temp_bytes = LevelTempBytes(n, end_bit);
  h->d_sort_temp.Reserve(temp_bytes, &h->allocations);
  keys[to].Reserve(keys[from].cap, &h->allocations);
  records[to].Reserve(records[from].cap, &h->allocations);
  v.perm.Reserve((size_t)n * 2 * sizeof(uint32_t), &h->allocations);
  uint32_t* perm_in = v.perm.As<uint32_t>();
  uint32_t* perm_out = perm_in + n;
  LaunchVolumeIota(perm_in, n, h->stream);
  VSG_HIP(SortPairsU64U32(h->d_sort_temp.p, temp_bytes, keys[from].As<unsigned long long>(),
                          keys[to].As<unsigned long long>(), perm_in, perm_out, n, end_bit, h->stream));
  LaunchVolumeGather(records[from].p, records[to].p, perm_out, n, record_bytes, h->stream);
  VSG_HIP(hipGetLastError());
  *at = to;
  return 3;
}

}  // namespace

extern "C" {

int vsg_render_volume_begin(vsg_render* h, int level, int with_colors, int with_labels) {
  return Guard([&] {
    if (!h) Throw(VSG_ERR_INVALID, "handle is null");
    if (level < 0) Throw(VSG_ERR_INVALID, "level is negative");
    if (with_colors != 0 && with_colors != 1) Throw(VSG_ERR_INVALID, "with_colors is neither 0 nor 1");
    if (with_labels != 0 && with_labels != 1) Throw(VSG_ERR_INVALID, "with_labels is neither 0 nor 1");
    VolumeState& v = h->vol;
    v.active = true;
    v.level = level;
    v.with_colors = with_colors != 0;
    v.with_labels = with_labels != 0;
    v.n_rows = v.n_cols = v.n_pairs = 0;
    v.max_id = v.max_label = 0;
    std::memset(&v.stats, 0, sizeof(v.stats));
  });
}

int vsg_render_volume_add(vsg_render* h, const uint8_t* seg, size_t seg_len, int frame, const uint8_t* bgr,
                          size_t stride, int mem_in, const int32_t* other, size_t other_pitch, int mem_other) {
  return Guard([&] {
    using namespace vsg_render_impl;
    if (!h) Throw(VSG_ERR_INVALID, "handle is null");
    if (frame < 0) Throw(VSG_ERR_INVALID, "frame is negative");
    VolumeState& v = h->vol;
    if (!v.active) Throw(VSG_ERR_STATE, "no volume session: call vsg_render_volume_begin first");
    if (v.with_colors) {
      if (!bgr) Throw(VSG_ERR_INVALID, "bgr is null");
      if (mem_in != VSG_MEM_HOST && mem_in != VSG_MEM_DEVICE) {
        Throw(VSG_ERR_INVALID, "mem_in is neither VSG_MEM_HOST nor VSG_MEM_DEVICE");
      }
      if (stride < (size_t)h->W * 3) Throw(VSG_ERR_INVALID, "stride is smaller than 3 * width");
    }
    if (v.with_labels) {
      CheckOtherPlane(other, mem_other);
      CheckOtherPitch(h, other_pitch);
    }
    CheckFrameBelow2Pow32(h);
    DeviceGuard guard(h->device);
    vsg_render_volume_stats& vs = v.stats;
    int launches = 0;
    float frame_us = 0;

    // ---- the frame's lists, each left on the device by the call that makes it; nothing is merged yet ----
    size_t n_ovl_rows = 0, n_ovl_cols = 0, n_ovl_pairs = 0;
    uint32_t frame_max_label = 0;
    int64_t labelled = 0, both = 0;
    if (v.with_labels) {
      const int rc = vsg_render_level_overlap(h, seg, seg_len, v.level, 0, other, other_pitch, mem_other, nullptr, 0,
                                              &n_ovl_rows, nullptr, 0, &n_ovl_cols, nullptr, 0, &n_ovl_pairs,
                                              VSG_MEM_DEVICE);
      if (rc != VSG_OK) Throw(rc, g_last_error);
      const vsg_render_overlap_stats& os = h->ovl.stats;
      frame_max_label = h->ovl.seen.As<OvlStatus>()[0].max_label;
      labelled = os.labelled;
      both = os.both;
      launches += os.launches;
      frame_us += os.plane_us + os.count_us + os.emit_us + os.sort_us + os.table_us;
    }
    LevelFront f;
    uint32_t n_regions = 0;
    if (v.with_colors) {
      size_t n_colors = 0;
      LevelColors(h, seg, seg_len, v.level, 0, bgr, stride, mem_in, nullptr, 0, &n_colors, nullptr, 0, VSG_MEM_DEVICE,
                  &f);
      n_regions = (uint32_t)n_colors;
      const vsg_render_color_stats& ks = h->color.stats;
      launches += ks.launches;
      frame_us += ks.plane_us + ks.sums_us + ks.table_us;
    } else {
      vsg_render_level_stats ls;   // of the shared front half; the last level_regions call's stay
      std::memset(&ls, 0, sizeof(ls));
      f = PaintLevelRuns(h, seg, seg_len, v.level, &ls);
      frame_us += h->stats.clear_us + h->stats.fill_us + ls.runs_us;
      if (f.n) {
        SortLevelRuns(h, &f, &ls);
        LevelStatus* seen = h->lvl.seen.As<LevelStatus>();
        VSG_HIP(hipMemcpyAsync(&seen[1], f.status, sizeof(LevelStatus), hipMemcpyDeviceToHost, h->stream));
        ++ls.launches;
        VSG_HIP(hipStreamSynchronize(h->stream));
        float lus[LVL_COUNT];
        h->lvl.clock.Read(lus, LVL_COUNT);
        frame_us += lus[LVL_SORT] + lus[LVL_TABLE];
        n_regions = seen[1].regions;
        if (n_regions == 0 || n_regions > f.cap_regions) {
          Throw(VSG_ERR_INTERNAL, "the plane has more regions than the desc has ids");
        }
      }
      h->stats.launches += ls.launches;
      launches += h->stats.launches;
    }
    if (v.with_labels && n_ovl_rows != n_regions) {
      Throw(VSG_ERR_INTERNAL, "the overlap table has other rows than the level has regions");
    }
    if (n_regions > f.cap_regions) Throw(VSG_ERR_INTERNAL, "the level has more regions than the desc has ids for");

    // ---- room for every key the frame can bring, what is there kept ----
    GrowVolumeTable(h, &v.row_keys[v.rows_at], &v.rows[v.rows_at], sizeof(vsg_render_volume_row),
                    (uint64_t)v.n_rows + n_regions, v.n_rows);
    GrowVolumeTable(h, &v.col_keys[v.cols_at], &v.cols[v.cols_at], sizeof(vsg_render_volume_col),
                    (uint64_t)v.n_cols + n_ovl_cols, v.n_cols);
    GrowVolumeTable(h, &v.pair_keys[v.pairs_at], &v.pairs[v.pairs_at], sizeof(vsg_render_volume_pair),
                    (uint64_t)v.n_pairs + n_ovl_pairs, v.n_pairs);
    v.geo.Reserve(std::max<size_t>((size_t)n_regions * kVolumeGeoBytes, 16), &h->allocations);
    auto [status, seen] = ReserveStatusPair<VolumeStatus>(h, &v.status, &v.seen);

    // ---- geometry, merge ----
    VolumeFrame fr;
    fr.frame = frame;
    fr.regions = f.regions;
    fr.geo = v.geo.p;
    fr.colors = v.with_colors ? h->color.records.As<int32_t>() : nullptr;
    fr.overlap_rows = v.with_labels ? h->ovl.rows.As<int32_t>() : nullptr;
    fr.n_rows = n_regions;
    fr.overlap_cols = h->ovl.cols.As<int32_t>();
    fr.n_cols = (uint32_t)n_ovl_cols;
    fr.overlap_pairs = h->ovl.pairs.As<int32_t>();
    fr.n_pairs = (uint32_t)n_ovl_pairs;
    const VolumeTables tables = VolumeTablesOf(v);
    VSG_HIP(hipMemsetAsync(status, 0, sizeof(VolumeStatus), h->stream));
    v.clock.Begin(h->stream);
    if (n_regions) {
      VSG_HIP(hipMemsetAsync(v.geo.p, 0, (size_t)n_regions * kVolumeGeoBytes, h->stream));
      LaunchVolumeGeometry(f.intervals, f.rank, f.n, n_regions, v.geo.p, status, h->stream);
      VSG_HIP(hipGetLastError());
    }
    v.clock.Mark(VOL_GEOMETRY);
    // From here on the tables change.  Whatever fails behind this line (a launch, a copy, an allocation or the sort
    // of a table that got keys) leaves a part of the frame merged, or an unsorted tail counted as sorted: the
    // session ends with the failure, so that no later call bisects such a table.
    int own = 2 + (n_regions ? 2 : 0);   // the status' clear and copy; the clear of geo and its kernel
    int resorts = 0;
    VolumeStatus st = {};
    float us[VOL_STAGES], sort_us[VOL_STAGES];
    try {
      own += LaunchVolumeMerge(fr, tables, status, h->stream);
      VSG_HIP(hipGetLastError());
      v.clock.Mark(VOL_MERGE);
      VSG_HIP(hipMemcpyAsync(&seen[0], status, sizeof(VolumeStatus), hipMemcpyDeviceToHost, h->stream));
      VSG_HIP(hipStreamSynchronize(h->stream));   // the number of new keys decides which tables are sorted again
      v.clock.Read(us, VOL_STAGES);
      st = seen[0];
      if ((st.flags & VOLUME_FLAG_RANGE) || st.new_rows > n_regions || st.new_cols > n_ovl_cols ||
          st.new_pairs > n_ovl_pairs) {
        Throw(VSG_ERR_INTERNAL, "the frame's lists disagree, or a key of the volume session had no slot");
      }

      // ---- new keys: the table sorted again; the clock starts anew, the wait for the status words is no stage ----
      v.n_rows += st.new_rows;
      v.n_cols += st.new_cols;
      v.n_pairs += st.new_pairs;
      if (n_regions) v.max_id = std::max(v.max_id, (uint32_t)f.max_id);
      v.max_label = std::max(v.max_label, frame_max_label);
      std::fill(sort_us, sort_us + VOL_STAGES, 0.0f);
      if (st.new_rows || st.new_cols || st.new_pairs) {
        v.clock.Begin(h->stream);
        if (st.new_rows) {
          own += ResortVolumeTable(h, v.row_keys, v.rows, &v.rows_at, sizeof(vsg_render_volume_row), v.n_rows,
                                   BitsFor(v.max_id, 31));
          ++resorts;
        }
        if (st.new_cols) {
          own += ResortVolumeTable(h, v.col_keys, v.cols, &v.cols_at, sizeof(vsg_render_volume_col), v.n_cols,
                                   BitsFor(v.max_label, 31));
          ++resorts;
        }
        if (st.new_pairs) {
          own += ResortVolumeTable(h, v.pair_keys, v.pairs, &v.pairs_at, sizeof(vsg_render_volume_pair), v.n_pairs,
                                   32 + BitsFor(v.max_id, 31));
          ++resorts;
        }
        v.clock.Mark(VOL_SORT);
        VSG_HIP(hipStreamSynchronize(h->stream));
        v.clock.Read(sort_us, VOL_STAGES);
      }
    } catch (const Error& e) {
      v.active = false;
      Throw(e.code, std::string(e.what()) + "; the volume session has ended");
    }
    vs.frames += 1;
    vs.rows = v.n_rows;
    vs.cols = v.n_cols;
    vs.pairs = v.n_pairs;
    vs.new_rows = st.new_rows;
    vs.new_cols = st.new_cols;
    vs.new_pairs = st.new_pairs;
    vs.resorts = resorts;
    vs.covered += (int64_t)st.covered;
    vs.labelled += labelled;
    vs.both += both;
    vs.frame_us = frame_us;
    vs.geometry_us = us[VOL_GEOMETRY];
    vs.merge_us = us[VOL_MERGE];
    vs.sort_us = sort_us[VOL_SORT];
    vs.launches = launches + own;
    h->stats.launches += own;
    h->stats.device_allocations = h->allocations;
  });
}

int vsg_render_volume_table(vsg_render* h, vsg_render_volume_row* rows, size_t capacity_rows, size_t* num_rows,
                            vsg_render_volume_col* cols, size_t capacity_cols, size_t* num_cols,
                            vsg_render_volume_pair* pairs, size_t capacity_pairs, size_t* num_pairs, int mem_out) {
  return Guard([&] {
    using namespace vsg_render_impl;
    if (!h) Throw(VSG_ERR_INVALID, "handle is null");
    if (!num_rows || !num_cols || !num_pairs) Throw(VSG_ERR_INVALID, "a count pointer is null");
    *num_rows = *num_cols = *num_pairs = 0;
    CheckMem(mem_out, "outputs");
    VolumeState& v = h->vol;
    if (!v.active) Throw(VSG_ERR_STATE, "no volume session: call vsg_render_volume_begin first");
    const size_t n_rows = v.n_rows, n_cols = v.n_cols, n_pairs = v.n_pairs;
    *num_rows = n_rows;
    *num_cols = n_cols;
    *num_pairs = n_pairs;
    const bool count_only =
        !rows && !cols && !pairs && capacity_rows == 0 && capacity_cols == 0 && capacity_pairs == 0;
    if (count_only) return;
    if (n_rows > capacity_rows || n_cols > capacity_cols || n_pairs > capacity_pairs) {
      Throw(VSG_ERR_INVALID, "the table has " + std::to_string(n_rows) + " rows, " + std::to_string(n_cols) +
                                 " columns and " + std::to_string(n_pairs) + " pairs, the capacities are " +
                                 std::to_string(capacity_rows) + ", " + std::to_string(capacity_cols) + " and " +
                                 std::to_string(capacity_pairs));
    }
    if ((n_rows && !rows) || (n_cols && !cols) || (n_pairs && !pairs)) Throw(VSG_ERR_INVALID, "an output is null");
    v.stats.table_us = 0;
    if (n_rows == 0 && n_cols == 0) return;
    DeviceGuard guard(h->device);
    const size_t row_bytes = n_rows * sizeof(vsg_render_volume_row);
    const size_t col_bytes = n_cols * sizeof(vsg_render_volume_col);
    const size_t pair_bytes = n_pairs * sizeof(vsg_render_volume_pair);
    // The session's records are the caller's records but for what the read-out fills in, so it works on copies: in
    // the caller's own memory for device outputs (the capacities are known to hold them), in the session's blocks
    // for host outputs.
    const bool host = mem_out == VSG_MEM_HOST;
    if (host) {
      v.out_rows.Reserve(std::max<size_t>(row_bytes, 16), &h->allocations);
      v.out_cols.Reserve(std::max<size_t>(col_bytes, 16), &h->allocations);
      v.out_pairs.Reserve(std::max<size_t>(pair_bytes, 16), &h->allocations);
    }
    void* const d_rows = host ? v.out_rows.p : static_cast<void*>(rows);
    void* const d_cols = host ? v.out_cols.p : static_cast<void*>(cols);
    void* const d_pairs = host ? v.out_pairs.p : static_cast<void*>(pairs);
    auto [status, seen] = ReserveStatusPair<VolumeStatus>(h, &v.status, &v.seen);
    const VolumeTables t = VolumeTablesOf(v);
    int launches = 2;
    VSG_HIP(hipMemsetAsync(status, 0, sizeof(VolumeStatus), h->stream));
    v.clock.Begin(h->stream);
    if (row_bytes) VSG_HIP(hipMemcpyAsync(d_rows, t.rows, row_bytes, hipMemcpyDeviceToDevice, h->stream));
    if (col_bytes) VSG_HIP(hipMemcpyAsync(d_cols, t.cols, col_bytes, hipMemcpyDeviceToDevice, h->stream));
    if (pair_bytes) VSG_HIP(hipMemcpyAsync(d_pairs, t.pairs, pair_bytes, hipMemcpyDeviceToDevice, h->stream));
    launches += (row_bytes ? 1 : 0) + (col_bytes ? 1 : 0) + (pair_bytes ? 1 : 0);
    launches += LaunchVolumeReadout(t, d_rows, d_cols, d_pairs, status, h->stream);
    VSG_HIP(hipGetLastError());
    v.clock.Mark(VOL_TABLE);
    VSG_HIP(hipMemcpyAsync(&seen[1], status, sizeof(VolumeStatus), hipMemcpyDeviceToHost, h->stream));
    VSG_HIP(hipStreamSynchronize(h->stream));
    float us[VOL_STAGES];
    v.clock.Read(us, VOL_STAGES);
    v.stats.table_us = us[VOL_TABLE];
    if (seen[1].flags & VOLUME_FLAG_RANGE) {
      Throw(VSG_ERR_INTERNAL, "a pair of the volume session has no row or no column");
    }
    if (host) {
      launches += DeliverToHost(h, &v.seen, 2 * sizeof(VolumeStatus),
                                {{d_rows, row_bytes, rows}, {d_cols, col_bytes, cols}, {d_pairs, pair_bytes, pairs}});
    }
    h->stats.launches += launches;
    h->stats.device_allocations = h->allocations;
  });
}

VSG_RENDER_LAST_STATS(vsg_render_last_volume_stats, vsg_render_volume_stats, vol.stats)

}  // extern "C"
