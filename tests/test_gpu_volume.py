"""The volume session on the MI355X (libvsg_render.so: the level, colour and overlap pipelines per frame, then
k_volume_geometry, the k_volume_merge kernels, the re-sort and the read-out kernels) against volume_model.py.
Every sequence is read out after every add, and the tables are compared as raw bytes: there is no tolerance
anywhere in this file."""
import copy
import os
import re
import subprocess

import numpy as np
import pytest

import level_boundaries_cases as bc
import level_regions_cases as lc
import level_overlap_cases as oc
import render_model as rm
import synth
import vector_cases as vc
import vector_raster_model as vrm
import volume_cases as vcs
import volume_model as vm

pytestmark = pytest.mark.gpu

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "video_segment_amd", "host")
NAMES = ("rows", "cols", "pairs")
DTYPES = (vm.ROW_DTYPE, vm.COL_DTYPE, vm.PAIR_DTYPE)
FILL = 0x5A5A5A5A
STAT_KEYS = ("frames", "rows", "cols", "pairs", "new_rows", "new_cols", "new_pairs", "covered", "labelled", "both")


@pytest.fixture(scope="module")
def vsg():
    import video_segment_amd as v
    from video_segment_amd import _lib, render
    _lib.build()
    render.build()
    assert _lib.lib().vsg_device_count() > 0
    assert (render.VOLUME_ROW_DTYPE, render.VOLUME_COL_DTYPE, render.VOLUME_PAIR_DTYPE) == DTYPES
    return v


def assert_same(got, want, what):
    for name, g, w, dtype in zip(NAMES, got, want, DTYPES):
        assert g.dtype == dtype and g.shape == w.shape, (what, name, g.shape, w.shape)
        if not vm.same_bits(g, w):
            bad = [n for n in dtype.names if not np.array_equal(g[n], w[n])]
            k = int(np.flatnonzero([g[i].tobytes() != w[i].tobytes() for i in range(len(g))])[0])
            raise AssertionError((what, name, bad, k, g[k], w[k]))


def add(r, a, colors=True, labels=True):
    r.volume_add(a.msg.SerializeToString(), a.frame, a.F if colors else None, a.B if labels else None)


def run(vsg, s, colors=True, labels=True, r=None):
    """The sequence added frame by frame, the table and the stats compared with the model after every add.
    Returns the stats of every add."""
    own = r is None
    if own:
        r = vsg.SegmentationRenderer(s.W, s.H)
    r.volume_begin(s.level, colors, labels)
    assert_same(r.volume_table(), vm.volume([], colors, labels), (s.name, "empty"))
    stats = []
    for k, a in enumerate(s.adds):
        add(r, a, colors, labels)
        adds = vcs.model_adds(s, k + 1)
        assert_same(r.volume_table(), vm.volume(adds, colors, labels), (s.name, colors, labels, k))
        st = r.last_volume_stats()
        want = vm.stats_of(adds, colors, labels)
        assert {n: st[n] for n in STAT_KEYS} == {n: want[n] for n in STAT_KEYS}, (s.name, k, st)
        assert st["resorts"] == sum(1 for n in ("new_rows", "new_cols", "new_pairs") if want[n]), (s.name, k, st)
        stats.append(st)
    if own:
        r.close()
    return stats


@pytest.mark.parametrize("s", vcs.life_span(), ids=lambda s: s.name)
def test_life_span(vsg, s):
    run(vsg, s)
    r = vsg.SegmentationRenderer(s.W, s.H)
    r.volume_begin(0, True, True)
    for a in s.adds:
        add(r, a)
    rows = r.volume_table()[0]
    if s.name == "gap":
        three = rows[rows["id"] == 3][0]
        assert (three["first_frame"], three["last_frame"], three["frames"]) == (0, 2, 2)
    if s.name == "out_of_order":
        assert rows["first_frame"].tolist() == [5, 2] and rows["last_frame"].tolist() == [9, 9]
    if s.name == "late":
        five = rows[rows["id"] == 5][0]
        assert five["sum_t"] == 94 * 7 + 200 * vcs.MAX > 1 << 32
    r.close()


def test_search_and_resort_edges(vsg):
    s = vcs.search_edges()
    stats = run(vsg, s)
    assert [st["new_rows"] for st in stats] == [3, 4, 0, 8]          # into an empty table; below, between, above;
    assert [st["new_cols"] for st in stats] == [3, 4, 0, 8]          # no new key; new keys only
    assert stats[2]["new_pairs"] == 0 and stats[2]["resorts"] == 0
    assert stats[0]["resorts"] == stats[1]["resorts"] == stats[3]["resorts"] == 3
    run(vsg, s, labels=False)
    run(vsg, s, colors=False)


def test_widths_and_growth(vsg):
    """300 ids under one label, one id under 300 labels, then 5 000 new keys in every table: the blocks grow, and
    what the first two adds left in them is still there (the model's table holds it)."""
    s = vcs.widths()
    stats = run(vsg, s)
    assert stats[0]["rows"] == vcs.MANY and stats[0]["cols"] == 1 and stats[0]["pairs"] == vcs.MANY
    assert stats[1]["new_rows"] == 1 and stats[1]["new_cols"] == vcs.MANY and stats[1]["new_pairs"] == vcs.MANY
    assert stats[2]["new_rows"] == stats[2]["new_cols"] == stats[2]["new_pairs"] == vcs.GROWN
    # the same as 5000 x 1: every key in one frame row
    flat = vcs.Seq("widths_flat", s.W * s.H, 1, 0,
                   [vcs.Add(a.frame, bc.case("flat", a.P.reshape(1, -1)).msg, a.P.reshape(1, -1),
                            a.F.reshape(1, -1, 3), a.B.reshape(1, -1)) for a in s.adds])
    run(vsg, flat)


def test_empty_sides(vsg):
    s = vcs.empty_sides()
    stats = run(vsg, s)
    assert stats[1]["new_rows"] == 0 and stats[1]["rows"] == stats[0]["rows"]        # no covered pixel
    assert stats[2]["new_cols"] == 0 and stats[2]["new_pairs"] == 0                  # B all void
    # an uncovered frame first: the columns are there before any row
    first = vcs.Seq("uncovered_first", s.W, s.H, 0, [s.adds[1], s.adds[0]])
    run(vsg, first)
    # without labels, without colours, without either: the fields at their documented defaults
    for colors, labels in ((True, False), (False, True), (False, False)):
        run(vsg, s, colors, labels)
        r = vsg.SegmentationRenderer(s.W, s.H)
        r.volume_begin(0, colors, labels)
        for a in s.adds:
            add(r, a, colors, labels)
        rows, cols, pairs = r.volume_table()
        if not labels:
            assert len(cols) == 0 and len(pairs) == 0 and not rows["unlabelled"].any()
            assert (rows["best_label"] == -1).all() and not rows["best_count"].any()
            assert not rows["first_pair"].any() and not rows["num_pairs"].any()
        if not colors:
            assert not any(rows[n].any() for n in ("sum", "sum_sq", "min", "max"))
        assert not rows["reserved0"].any() and not rows["reserved1"].any()
        r.close()


def test_extremes(vsg):
    stats = run(vsg, vcs.extremes())
    assert stats[1]["resorts"] == 0


def test_64_bit_sums(vsg):
    """One region covering a 4096 x 4096 frame of constant 255 in device memory, 129 adds: the volume passes 2^31
    and the sums of squares 2^47.  (The full frame and 129 adds are used: nothing was halved.)"""
    import torch
    W = H = 4096
    ADDS = 129
    seg = bc.case("full", np.full((H, W), 8, np.int32)).msg.SerializeToString()
    F = torch.full((H, W, 3), 255, dtype=torch.uint8, device=torch.device("cuda", 0))
    r = vsg.SegmentationRenderer(W, H)
    r.volume_begin(0, True, False)
    r.volume_add(seg, 0, F)
    rows, cols, pairs = r.volume_table()
    assert len(rows) == 1 and len(cols) == 0 and len(pairs) == 0
    assert rows[0]["sum_x"] == H * (W * (W - 1) // 2) > 1 << 34
    assert rows[0]["sum_y"] == W * (H * (H - 1) // 2) and rows[0]["volume"] == W * H
    for k in range(1, ADDS):
        r.volume_add(seg, k, F)
    row = r.volume_table()[0][0]
    assert row["volume"] == ADDS * (1 << 24) > 1 << 31
    assert row["sum_sq"].tolist() == [255 * 255 * ADDS * (1 << 24)] * 3
    assert row["sum"].tolist() == [255 * ADDS * (1 << 24)] * 3
    assert row["sum_x"] == ADDS * H * (W * (W - 1) // 2)
    assert row["sum_t"] == (1 << 24) * (ADDS * (ADDS - 1) // 2)
    assert (row["min_x"], row["min_y"], row["max_x"], row["max_y"]) == (0, 0, W - 1, H - 1)
    assert (row["first_frame"], row["last_frame"], row["frames"]) == (0, ADDS - 1, ADDS)
    assert row["min"].tolist() == [255] * 3 and row["max"].tolist() == [255] * 3
    st = r.last_volume_stats()
    assert st["frames"] == ADDS and st["covered"] == ADDS * (1 << 24) and st["rows"] == 1
    r.close()


@pytest.mark.parametrize("level", (0, 1, 2))
def test_levels_and_kept_hierarchy(vsg, level):
    """Frame 0 carries the hierarchy; the later frames are the same desc without one and use the kept one."""
    s = vcs.three_levels(level)
    assert len(s.adds[0].msg.hierarchy) == 3 and all(len(a.msg.hierarchy) == 0 for a in s.adds[1:])
    stats = run(vsg, s)
    assert stats[-1]["rows"] == len(np.unique(s.adds[0].P))


def test_vector_only_desc_as_one_frame(vsg):
    W, H = 64, 48
    ids = vc.l1_voronoi(11, W, H, 12)
    vector = vc.vector_only(ids)
    r = vsg.SegmentationRenderer(W, H)
    seg = vector.SerializeToString()
    P = vrm.id_plane(r.rasterize(seg), W, H)
    raster = vcs.seq("vector", (0, 2), [np.asarray(ids, np.int32)] * 2, [oc.stripes(W, H)] * 2)
    a, b = raster.adds
    s = vcs.Seq("vector", W, H, 0, [a, vcs.Add(1, vector, P, a.F, np.roll(a.B, 3, axis=0)), b])
    run(vsg, s, r=r)
    assert r.last_vector_stats()["lines"] == 0                    # the last add was a raster desc again
    r.close()


@pytest.mark.parametrize("W", bc.WIDTHS)
def test_geometry_edges(vsg, W):
    for H in bc.HEIGHTS:
        s = vcs.geometry(W, H)
        r = vsg.SegmentationRenderer(W, H)
        run(vsg, s, colors=False, labels=False, r=r)
        rows = r.volume_table()[0]
        want = vm.volume(vcs.model_adds(s), False, False)[0]
        for name in ("sum_x", "sum_y", "min_x", "min_y", "max_x", "max_y", "volume"):
            assert np.array_equal(rows[name], want[name]), (W, H, name)
        run(vsg, s, r=r)
        r.close()


def test_session_rules(vsg):
    import torch
    from video_segment_amd import render
    from video_segment_amd._lib import VSG_ERR_INVALID, VSG_ERR_STATE, VsgError
    s = vcs.three_levels(1)
    r = vsg.SegmentationRenderer(s.W, s.H)
    a = s.adds[0]
    seg = a.msg.SerializeToString()
    # no session yet
    for call in (lambda: add(r, a), r.volume_table):
        with pytest.raises(VsgError) as e:
            call()
        assert e.value.code == VSG_ERR_STATE
    r.volume_begin(1, True, True)
    add(r, a)
    before = r.volume_table()
    before_stats = {n: r.last_volume_stats()[n] for n in STAT_KEYS}
    # a required plane that is missing, a bad stride or pitch, a level the hierarchy does not have: refused, and
    # the table is what it was
    L = render.lib()
    d_B = torch.from_numpy(a.B).cuda()
    assert L.vsg_render_volume_add(r.h, seg, len(seg), 1, None, 3 * s.W, 0, d_B.data_ptr(), 0, 1) == VSG_ERR_INVALID
    assert L.vsg_render_volume_add(r.h, seg, len(seg), 1, a.F.ctypes.data, 3 * s.W, 0, None, 0, 1) == VSG_ERR_INVALID
    assert L.vsg_render_volume_add(r.h, seg, len(seg), 1, a.F.ctypes.data, 3 * s.W - 1, 0, d_B.data_ptr(), 0,
                                   1) == VSG_ERR_INVALID
    assert L.vsg_render_volume_add(r.h, seg, len(seg), 1, a.F.ctypes.data, 3 * s.W, 0, d_B.data_ptr(), s.W - 1,
                                   1) == VSG_ERR_INVALID
    assert L.vsg_render_volume_add(r.h, seg, len(seg), 1, a.F.ctypes.data, 3 * s.W, 2, d_B.data_ptr(), 0,
                                   1) == VSG_ERR_INVALID
    for mem_other in (2, -1, 7):
        assert L.vsg_render_volume_add(r.h, seg, len(seg), 1, a.F.ctypes.data, 3 * s.W, 0, d_B.data_ptr(), 0,
                                       mem_other) == VSG_ERR_INVALID
        assert b"mem_other" in L.vsg_render_last_error()
    assert_same(r.volume_table(), before, "after refused arguments")
    r.volume_begin(7, True, True)                  # the level is checked by the add, against the kept hierarchy
    with pytest.raises(VsgError) as e:
        add(r, a)
    assert e.value.code == VSG_ERR_INVALID
    assert all(len(t) == 0 for t in r.volume_table())
    # a failed add in the middle of a session leaves the table byte-identical
    r.volume_begin(1, True, True)
    add(r, a)
    with pytest.raises(VsgError):
        r.volume_add(b"\x12\x03\x08", 1, a.F, a.B)       # a truncated message
    assert_same(r.volume_table(), before, "after a failed add")
    assert {n: r.last_volume_stats()[n] for n in STAT_KEYS} == before_stats
    # a bad level in the middle of a session: a desc whose own hierarchy does not reach the session's level
    short = copy.deepcopy(a.msg)
    del short.hierarchy[1:]
    with pytest.raises(VsgError) as e:
        r.volume_add(short.SerializeToString(), 1, a.F, a.B)
    assert e.value.code == VSG_ERR_INVALID
    assert_same(r.volume_table(), before, "after a bad level")
    assert {n: r.last_volume_stats()[n] for n in STAT_KEYS} == before_stats
    r.id_image(seg, 0)                                   # the whole hierarchy is the kept one again
    # other calls between two adds change nothing
    r.render(seg, a.F)
    r.level_overlap(seg, 2, np.roll(a.B, 7))
    r.level_colors(s.adds[1].msg.SerializeToString(), 0, a.F)
    r.level_regions(seg, 0)
    assert_same(r.volume_table(), before, "after other calls")
    add(r, s.adds[1])
    add(r, s.adds[2])
    want = vm.volume(vcs.model_adds(s))
    assert_same(r.volume_table(), want, "the whole sequence")
    # host and device outputs give equal bytes; a capacity that is too small touches nothing
    dev = torch.device("cuda", 0)
    words = (render.VOLUME_ROW_WORDS, render.VOLUME_COL_WORDS, render.VOLUME_PAIR_WORDS)
    sizes = [len(t) for t in want]
    outs = [torch.full((k + 3, w), FILL, dtype=torch.int32, device=dev) for k, w in zip(sizes, words)]
    got = r.volume_table(rows_out=outs[0], cols_out=outs[1], pairs_out=outs[2])
    for g, w_, o, k, w in zip(got, want, outs, sizes, words):
        assert g.is_cuda and g.shape == (k, w) and g.cpu().numpy().tobytes() == w_.tobytes()
        assert bool((o[k:] == FILL).all())
    for cut in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        for o in outs:
            o.fill_(FILL)
        with pytest.raises(VsgError) as e:
            r.volume_table(rows_out=outs[0][:sizes[0] - cut[0]], cols_out=outs[1][:sizes[1] - cut[1]],
                           pairs_out=outs[2][:sizes[2] - cut[2]])
        assert e.value.code == VSG_ERR_INVALID
        assert all(bool((o == FILL).all()) for o in outs), cut
        host = [np.frombuffer(bytes([0x5A]) * (d.itemsize * (k - c)), d).copy()
                for d, k, c in zip(DTYPES, sizes, cut)]
        nr, nc, npairs = (render.C.c_size_t() for _ in range(3))
        rc = L.vsg_render_volume_table(r.h, host[0].ctypes.data, len(host[0]), render.C.byref(nr), host[1].ctypes.data,
                                       len(host[1]), render.C.byref(nc), host[2].ctypes.data, len(host[2]),
                                       render.C.byref(npairs), 0)
        assert rc == VSG_ERR_INVALID and [nr.value, nc.value, npairs.value] == sizes      # the counts are set
        assert all(set(h.tobytes()) <= {0x5A} for h in host), cut
    # the session goes on after a table call and after refusals; a begin in the middle empties it
    add(r, s.adds[0])
    assert r.last_volume_stats()["frames"] == 4
    r.volume_begin(1, False, False)
    assert all(len(t) == 0 for t in r.volume_table()) and r.last_volume_stats()["frames"] == 0
    add(r, s.adds[2], False, False)
    assert_same(r.volume_table(), vm.volume(vcs.model_adds(s)[2:], False, False), "after a restart")
    r.close()


def test_one_frame_session_equals_the_sibling_calls(vsg):
    for s in (vcs.three_levels(1), vcs.empty_sides(), vcs.geometry(257, 5)):
        a = s.adds[0]
        seg = a.msg.SerializeToString()
        r = vsg.SegmentationRenderer(s.W, s.H)
        r.volume_begin(s.level, True, True)
        add(r, a)
        rows, cols, pairs = r.volume_table()
        regions, _ = r.level_regions(seg, s.level)
        colors = r.level_colors(seg, s.level, a.F)
        orows, ocols, opairs = r.level_overlap(seg, s.level, a.B)
        for name in ("id", "min_x", "min_y", "max_x", "max_y"):
            assert np.array_equal(rows[name], regions[name]), (s.name, name)
        assert np.array_equal(rows["volume"], regions["area"])
        for name in ("sum", "sum_sq", "min", "max"):
            assert np.array_equal(rows[name], colors[name]), (s.name, name)
        for name in ("first_pair", "num_pairs", "unlabelled", "best_label", "best_count"):
            assert np.array_equal(rows[name], orows[name]), (s.name, name)
        assert np.array_equal(cols["label"], ocols["label"]) and np.array_equal(cols["volume"], ocols["area"])
        for name in ("uncovered", "num_pairs", "best_row", "best_count"):
            assert np.array_equal(cols[name], ocols[name]), (s.name, name)
        for name in ("row", "col", "label", "count"):
            assert np.array_equal(pairs[name], opairs[name]), (s.name, name)
        assert (rows["frames"] == 1).all() and (pairs["frames"] == 1).all() and (cols["frames"] == 1).all()
        assert (rows["first_frame"] == a.frame).all() and (rows["sum_t"] == a.frame * rows["volume"]).all()
        r.close()


def test_stats_and_launches(vsg):
    """The totals are checked after every add of every sequence (run); here the number of launches: it is the same
    for H = 1 and H = 257, and for frame 1 and frame 20 of a steady sequence."""
    launches = {}
    for H in (1, 257):
        s = vcs.geometry(65, H)
        for flags in ((True, True), (False, False)):
            launches[H, flags] = run(vsg, s, *flags)[0]["launches"]
    assert launches[1, (True, True)] == launches[257, (True, True)] > 0
    assert launches[1, (False, False)] == launches[257, (False, False)] > 0
    steady = run(vsg, vcs.steady(21))
    assert steady[1]["launches"] == steady[20]["launches"] > 0
    assert steady[0]["resorts"] == 3 and all(st["resorts"] == 0 for st in steady[1:])
    assert steady[0]["launches"] > steady[1]["launches"]          # the first add sorted its three tables
    assert all(st[n] >= 0 for st in steady for n in ("frame_us", "geometry_us", "merge_us", "sort_us", "table_us"))
    assert steady[-1]["table_us"] > 0 and steady[-1]["merge_us"] > 0
    # sort_us is the sorts' alone: nothing when no table was sorted again
    assert steady[0]["sort_us"] > 0 and all(st["sort_us"] == 0 for st in steady[1:])


def test_scores_of_a_session(vsg):
    from video_segment_amd import render
    s = vcs.three_levels(1)
    r = vsg.SegmentationRenderer(s.W, s.H)
    r.volume_begin(1, True, True)
    for a in s.adds:
        add(r, a)
    got = render.volume_scores(*r.volume_table())
    n, ue_sum, duration = vm.scores_direct(vcs.model_adds(s))
    assert (got["n"], got["ue_sum"], got["mean_duration"]) == (n, ue_sum, duration)
    assert got == render.volume_scores(*vm.volume(vcs.model_adds(s)))
    r.close()


STREAM = (96, 64, 16, 8)   # W, H, frames, chunk size


def test_driver_accumulates_the_session_in_its_render_unit(vsg, tmp_path):
    """seg_tree_synth --volume_level: the C++ SegmentationRenderUnit's session over the frames it renders equals a
    Python session over the same stream, and the driver writes one line per supervoxel."""
    subprocess.check_call(["make", "-C", HOST, "-s"])
    W, H, N, chunk = STREAM
    fl = synth.const_flow(W, H)
    frames = [synth.soft_frame(W, H, k) for k in range(N)]
    d = vsg.DenseSegmentation(W, H, vsg.default_options(chunk_size=chunk), has_flow=True)
    reg = vsg.RegionSegmentation(W, H, vsg.default_region_options(chunk_set_size=3, chunk_set_overlap=1,
                                                                  constraint_chunks=1, min_region_num=3))
    over, segs = [], []
    for k in range(N):
        n = d.process_frame(frames[k], fl if k > 0 else None, flush=(k == N - 1))
        over += [d.result_bytes(i) for i in range(n)]
    for k, seg in enumerate(over):
        n = reg.process_frame(seg, frames[k], fl if k > 0 else None, flush=(k == N - 1))
        segs += [reg.result_bytes(i) for i in range(n)]
    d.close()
    reg.close()
    assert len(segs) == N
    r = vsg.SegmentationRenderer(W, H)
    r.volume_begin(0, True, False)
    adds = []
    for k, (seg, F) in enumerate(zip(segs, frames)):
        r.volume_add(seg, k, F)
        adds.append((k, r.id_image(seg, 0), F, None))
    rows, cols, pairs = r.volume_table()
    assert_same((rows, cols, pairs), vm.volume(adds, True, False), "stream")
    assert rows["volume"].sum() == N * W * H and rows["frames"].max() > 1      # supervoxels live longer than a frame
    r.close()
    out = str(tmp_path / "supervoxels.txt")
    p = subprocess.run([os.path.join(HOST, "seg_tree_synth"), "--width", str(W), "--height", str(H), "--frames", str(N),
                        "--chunk_size", str(chunk), "--input", "soft", "--flow", "--region_segmentation",
                        "--chunk_set_size", "3", "--chunk_set_overlap", "1", "--min_region_num", "3",
                        "--nouse_pipeline", "--volume_level", "0", "--volume_out", out],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    m = re.search(r"volume_level=0 volume_frames=(\d+) volume_supervoxels=(\d+) volume_voxels=(\d+) "
                  r"volume_fnv1a32=(\w+)", p.stdout)
    assert m, p.stdout
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (N, len(rows), N * W * H)
    assert int(m.group(4), 16) == rm.fnv1a32([rows])
    lines = np.loadtxt(out, dtype=np.int64, ndmin=2)
    want = np.stack([rows[n] for n in ("id", "first_frame", "last_frame", "frames", "volume", "min_x", "min_y",
                                       "max_x", "max_y", "sum_x", "sum_y", "sum_t")] +
                    [rows["sum"][:, c] for c in range(3)], axis=1).astype(np.int64)
    assert np.array_equal(lines, want)
