"""The tree cut on the device: every case of tree_cut_cases, with both gain sources and under both DP paths,
against the numpy model as raw bytes, in host and in device memory; the launch rule; the cross-checks with the
handle's own level_regions, level_overlap and id_image; nesting; the search for a node count; the refusals; a
real stream and the driver's line."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import level_regions_cases as lc
import persistence_cases as pc
import render_model as rm
import synth
import tree_cut_cases as tc
import tree_cut_model as tm
import vector_cases as vc
import vector_raster_model as vm

pytestmark = pytest.mark.gpu

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "video_segment_amd", "host")
CASES = tc.all_cases()
BY_NAME = {c.name: c for c in CASES}
FILL = 0x5A5A5A5A
PER_LEVEL, ONE_BLOCK = 0, (1 << 63) - 1
PATHS = ((PER_LEVEL, 2), (ONE_BLOCK, 1))


@pytest.fixture(scope="module")
def vsg():
    import video_segment_amd as v
    from video_segment_amd import _lib, render
    _lib.build()
    render.build()
    assert _lib.lib().vsg_device_count() > 0
    assert render.CUT_NODE_DTYPE == tm.NODE_DTYPE and render.CUT_GAIN_DTYPE == tm.GAIN_DTYPE
    assert render.CUT_BLOCK_ALWAYS == ONE_BLOCK
    return v


class Expected:
    """The model's tree of one frame, and its cuts, each computed once."""

    def __init__(self, ids0, hierarchy):
        self.ids0, self.hierarchy = ids0, hierarchy
        self.tree = tm.Tree(ids0, hierarchy)
        self.cuts = {}

    def cut(self, key, **source):
        if key not in self.cuts:
            self.cuts[key] = tm.cut(self.ids0, self.hierarchy, tree=self.tree, **source)
        return self.cuts[key]


_expected = {}


def expected_of(case):
    if case.name not in _expected:
        _expected[case.name] = Expected(tc.ids_of(case.msg), rm.hierarchy_of(case.msg))
    return _expected[case.name]


def sources_of(case):
    return [(("labels", p), dict(labels=case.labels, penalty=p)) for p in case.penalties] + \
        [(("gains",), dict(gains=case.gains))]


def on_device(x):
    import torch
    if x.dtype == tm.GAIN_DTYPE:
        return torch.from_numpy(np.frombuffer(x.tobytes(), np.int32).reshape(-1, 4).copy()).to("cuda:0")
    return torch.from_numpy(x).to("cuda:0")


def check_cut(r, seg, want, key, source, path, what, device):
    """One call against the model: records, plane and total as raw bytes, and the stats."""
    import torch
    from video_segment_amd import render
    records, plane, total = want.cut(key, **source)
    tree = want.tree
    H, W = plane.shape
    if not device:
        nodes, got_plane, got_total = r.tree_cut(seg, **source)
        assert nodes.dtype == tm.NODE_DTYPE and got_plane.dtype == np.int32, what
    else:
        kw = {k: (on_device(v) if isinstance(v, np.ndarray) else v) for k, v in source.items()}
        d_nodes = torch.full((len(records) + 1, render.CUT_NODE_WORDS), FILL, dtype=torch.int32, device="cuda:0")
        d_plane = torch.full((H + 1, W), FILL, dtype=torch.int32, device="cuda:0")
        nodes, got_plane, got_total = r.tree_cut(seg, nodes_out=d_nodes, plane_out=d_plane[:H], **kw)
        assert nodes.is_cuda and got_plane.is_cuda, what
        nodes, got_plane = nodes.cpu().numpy(), got_plane.cpu().numpy()
        assert bool((d_nodes[len(records):] == FILL).all()) and bool((d_plane[H] == FILL).all()), what
    assert got_total == total, (what, got_total, total)
    assert np.ascontiguousarray(nodes).tobytes() == records.tobytes(), what
    assert np.ascontiguousarray(got_plane).tobytes() == plane.tobytes(), what
    st = r.last_cut_stats()
    assert st["levels"] == tree.L and st["leaves"] == len(tree.ids) and st["tree_nodes"] == len(tree.nodes), (what, st)
    assert st["cut_nodes"] == len(records) and st["total"] == total, (what, st)
    assert st["covered"] == int((want.ids0 >= 0).sum()), (what, st)
    assert st["dp_path"] == (path if len(tree.nodes) else 0), (what, st)
    assert st["dp_launches"] == ((tree.L if path == 2 else 1) if len(tree.nodes) else 0), (what, st)
    assert st["entries"] == tree.L * (st["leaves"] + st["pairs"]), (what, st)
    assert (st["pairs"] > 0) == ("labels" in source and bool(((want.ids0 >= 0) & (source["labels"] >= 0)).any()))
    return st


def check_case(vsg, case, r=None):
    want = expected_of(case)
    seg = case.msg.SerializeToString()
    own = r is None
    r = r or vsg.SegmentationRenderer(case.W, case.H, has_video=False)
    for block_nodes, path in PATHS:
        r.tree_cut_tuning(block_nodes)
        for n, (key, source) in enumerate(sources_of(case)):
            check_cut(r, seg, want, key, source, path, (case.name, key, path), False)
            if n == 0 or "gains" in source:
                check_cut(r, seg, want, key, source, path, (case.name, key, path, "device"), True)
    r.tree_cut_tuning(-1)
    if own:
        r.close()


@pytest.mark.parametrize("L", pc.LADDER_HEIGHTS)
def test_ladders(vsg, L):
    for k in tc.ladder_splits(L):
        check_case(vsg, BY_NAME["ladder_%d_split_%d" % (L, k)])


@pytest.mark.parametrize("W", pc.bc.WIDTHS)
def test_widths_around_tile_and_block_edges(vsg, W):
    for H in pc.bc.HEIGHTS:
        check_case(vsg, BY_NAME["width_%dx%d" % (W, H)])


@pytest.mark.parametrize("name", ["chain_4", "narrow_5", "narrow_7", "max_id", "out_of_order", "three_levels",
                                  "checker", "uncovered", "uncovered_frame", "uncovered_unlabelled", "dense_64",
                                  "big_gains"])
def test_named_case(vsg, name):
    check_case(vsg, BY_NAME[name])


def test_every_case_is_run():
    named = {"chain_4", "narrow_5", "narrow_7", "max_id", "out_of_order", "three_levels", "checker", "uncovered",
             "uncovered_frame", "uncovered_unlabelled", "dense_64", "big_gains", "reuse_small", "reuse_large"}
    rest = [c.name for c in CASES if c.name not in named and not c.name.startswith(("ladder_", "width_"))]
    assert rest == []


def test_handle_reuse_small_large_small_allocates_once(vsg):
    small, large = BY_NAME["reuse_small"], BY_NAME["reuse_large"]
    r = vsg.SegmentationRenderer(small.W, small.H, has_video=False)
    allocs = []
    for _ in range(2):
        for case in (small, large, small):
            check_case(vsg, case, r)
            allocs.append(r.last_stats()["device_allocations"])
    assert allocs[1] > allocs[0] > 0 and allocs[3:] == [allocs[2]] * 3, allocs
    # a second identical call allocates nothing
    seg = large.msg.SerializeToString()
    r.tree_cut(seg, labels=large.labels, penalty=1)
    before = r.last_stats()["device_allocations"]
    r.tree_cut(seg, labels=large.labels, penalty=1)
    assert r.last_stats()["device_allocations"] == before
    r.close()


def test_launch_rule(vsg):
    """One workgroup: the launches do not depend on L.  Per level: dp_launches is L, and the call has L - 1
    launches more than on the other path."""
    block, level = {}, {}
    for L in (1, 2, 5, 20):
        case = BY_NAME["ladder_%d_split_1" % L]
        seg = case.msg.SerializeToString()
        r = vsg.SegmentationRenderer(case.W, case.H, has_video=False)
        for _ in range(2):                                  # the second round has nothing left to allocate
            for block_nodes, out in ((ONE_BLOCK, block), (PER_LEVEL, level)):
                r.tree_cut_tuning(block_nodes)
                r.tree_cut(seg, labels=case.labels, penalty=1)
                a = r.last_cut_stats()
                r.tree_cut(seg, gains=case.gains)
                b = r.last_cut_stats()
                out[L] = (a["launches"], b["launches"], a["dp_launches"], b["dp_launches"])
        r.close()
    assert len(set(block.values())) == 1 and block[1][2:] == (1, 1) and min(block[1]) > 0, block
    for L, (a, b, da, db) in level.items():
        assert (da, db) == (L, L) and (a, b) == (block[L][0] + L - 1, block[L][1] + L - 1), (L, level, block)


@pytest.mark.parametrize("name", ["three_levels", "out_of_order", "narrow_7", "dense_64", "ladder_5_split_2"])
def test_cross_checks_with_the_siblings(vsg, name):
    from video_segment_amd import render
    case = BY_NAME[name]
    seg = case.msg.SerializeToString()
    L = expected_of(case).tree.L
    r = vsg.SegmentationRenderer(case.W, case.H, has_video=False)
    regions = {l: r.level_regions(seg, l)[0] for l in range(L)}
    rows = {l: r.level_overlap(seg, l, case.labels)[0] for l in range(L)}
    rows0, _, pairs0 = r.level_overlap(seg, 0, case.labels)
    for p in case.penalties:
        nodes, plane, total = r.tree_cut(seg, labels=case.labels, penalty=p)
        for n in nodes:
            reg = regions[int(n["level"])]
            k = int(np.searchsorted(reg["id"], n["id"]))
            assert reg["id"][k] == n["id"] and reg["area"][k] == n["area"], (name, p, n)
            row = rows[int(n["level"])][k]
            assert (row["id"], row["best_label"], row["best_count"]) == (n["id"], n["best_label"], n["best_count"])
            assert n["gain"] == int(n["best_count"]) - p
        assert total == int(nodes["gain"].sum())
        if p == 0:
            assert render.cut_scores(nodes)["best_sum"] == render.overlap_scores(rows0, pairs0)["asa_sum"]
    above = int(max(rows[l]["best_count"].max() for l in range(L))) + 1
    nodes, plane, _ = r.tree_cut(seg, labels=case.labels, penalty=above)
    assert (nodes["level"] == L - 1).all()
    top = r.id_image(seg, L - 1)
    assert np.array_equal(np.where(plane >= 0, nodes["id"][np.maximum(plane, 0)], -1), top)
    assert render.cut_scores(nodes)["per_level"] == {L - 1: len(nodes)}
    r.close()


def test_cuts_are_nested_on_the_device(vsg):
    case = BY_NAME["dense_64"]
    seg = case.msg.SerializeToString()
    r = vsg.SegmentationRenderer(case.W, case.H, has_video=False)
    counts, levels = [], []
    for p in (0, 1, 2, 3, 4, 6, 9, 14, 22, 40, 100, 1 << 32):
        nodes, plane, _ = r.tree_cut(seg, labels=case.labels, penalty=p)
        counts.append(len(nodes))
        levels.append(tm.level_plane(nodes, plane))
    assert all(a >= b for a, b in zip(counts, counts[1:])), counts
    assert all((a <= b).all() for a, b in zip(levels, levels[1:]))
    assert counts[0] > counts[-1] == 16 and len(set(counts)) >= 4, counts      # the top level has 4 x 4 blocks
    r.close()


def test_tree_cut_for_count(vsg):
    from video_segment_amd import render
    case = BY_NAME["dense_64"]
    seg = case.msg.SerializeToString()
    r = vsg.SegmentationRenderer(case.W, case.H, has_video=False)
    finest = len(r.tree_cut(seg, labels=case.labels, plane=False)[0])
    for max_nodes in (finest, finest - 1, 100, 17, 16):
        penalty, nodes, plane, total = render.tree_cut_for_count(r, seg, case.labels, max_nodes)
        assert len(nodes) <= max_nodes and plane.shape == (case.H, case.W), (max_nodes, penalty, len(nodes))
        if penalty > 0:
            more, _, _ = r.tree_cut(seg, labels=case.labels, penalty=penalty - 1, plane=False)
            assert len(more) > max_nodes, (max_nodes, penalty)
        else:
            assert max_nodes >= finest
    # two top-level nodes: even the top has more than one node
    ladder = BY_NAME["ladder_5_split_2"]
    r2 = vsg.SegmentationRenderer(ladder.W, ladder.H, has_video=False)
    penalty, nodes, _, _ = render.tree_cut_for_count(r2, ladder.msg.SerializeToString(), ladder.labels, 1)
    assert penalty == 1 << 32 and len(nodes) == 2 and (nodes["level"] == 4).all()
    r.close()
    r2.close()


def test_vector_only_desc(vsg):
    W, H = 64, 48
    ids = vc.l1_voronoi(11, W, H, 12)
    m = vc.vector_only(ids)
    present = sorted(int(i) for i in np.unique(ids))
    lc.add_hierarchy(m, [{i: 100 + i % 4 for i in present}, {100 + k: 200 + k // 2 for k in range(4)}])
    seg = m.SerializeToString()
    for w, h in ((W, H), (96, 72)):                    # at the desc's size, and scan converted at another
        r = vsg.SegmentationRenderer(w, h, has_video=False)
        ids0 = vm.id_plane(r.rasterize(seg), w, h)
        want = Expected(ids0, rm.hierarchy_of(m))
        labels = tc.shifted_labels(ids0, 3)
        for block_nodes, path in PATHS:
            r.tree_cut_tuning(block_nodes)
            for p in (0, 2, 50):
                check_cut(r, seg, want, ("labels", p), dict(labels=labels, penalty=p), path, ("vector", w, p), p == 2)
        r.close()


def test_hierarchy_bookkeeping(vsg):
    """A frame with a hierarchy, then one without uses the kept one, then one of another height replaces it."""
    with_4 = BY_NAME["ladder_4_split_2"]
    ids = tc.ids_of(with_4.msg)
    without = lc.desc_from_ids(ids)
    with_2 = lc.desc_from_ids(ids, [{k: 70 + k // 2 for k in range(5)}])
    r = vsg.SegmentationRenderer(5, 2, has_video=False)
    want_4 = Expected(ids, rm.hierarchy_of(with_4.msg))
    want_2 = Expected(ids, rm.hierarchy_of(with_2))
    assert (want_4.tree.L, want_2.tree.L) == (4, 2)
    for msg, want, what in ((with_4.msg, want_4, "own"), (without, want_4, "kept"), (with_2, want_2, "replaced"),
                            (without, want_2, "kept again")):
        for p in (0, 2):
            check_cut(r, msg.SerializeToString(), want, ("labels", p), dict(labels=with_4.labels, penalty=p), 1, what,
                      False)
    r.close()


def _filled(n, dtype):
    return np.frombuffer(bytes([0x5A]) * (n * np.dtype(dtype).itemsize), dtype).copy()


def _untouched(*arrays):
    return all((np.frombuffer(np.ascontiguousarray(x).tobytes(), np.uint8) == 0x5A).all() for x in arrays)


def test_refusals_leave_the_outputs_untouched(vsg):
    import torch
    from video_segment_amd._lib import VSG_ERR_INVALID, VsgError
    from video_segment_amd import render
    case = BY_NAME["big_gains"]
    seg = case.msg.SerializeToString()
    W, H = case.W, case.H
    r = vsg.SegmentationRenderer(W, H, has_video=False)
    lib = render.lib()
    want_n = len(tm.cut(tc.ids_of(case.msg), rm.hierarchy_of(case.msg), labels=case.labels)[0])
    nodes, plane = _filled(8, tm.NODE_DTYPE), _filled(W * H, np.int32).reshape(H, W)

    def refused(**kw):
        with pytest.raises(VsgError) as e:
            r.tree_cut(seg, nodes_out=nodes, plane_out=plane, **kw)
        assert e.value.code == VSG_ERR_INVALID, kw
        assert _untouched(nodes, plane), kw
        return str(e.value)

    refused(labels=case.labels, gains=case.gains)
    refused()
    refused(labels=case.labels, penalty=-1)
    refused(labels=case.labels, penalty=(1 << 32) + 1)
    for what, bad in tc.bad_tables():
        refused(gains=bad)
        with pytest.raises(VsgError) as e:
            r.tree_cut(seg, gains=on_device(bad))          # count only
        assert e.value.code == VSG_ERR_INVALID, what
        d_nodes = torch.full((8, render.CUT_NODE_WORDS), FILL, dtype=torch.int32, device="cuda:0")
        d_plane = torch.full((H, W), FILL, dtype=torch.int32, device="cuda:0")
        with pytest.raises(VsgError) as e:
            r.tree_cut(seg, gains=on_device(bad), nodes_out=d_nodes, plane_out=d_plane)
        assert e.value.code == VSG_ERR_INVALID, what
        assert bool((d_nodes == FILL).all()) and bool((d_plane == FILL).all()), what

    # raw calls: a bad memory kind, a pitch below W, a capacity one too small, count only
    def ptr(x):
        return x.ctypes.data_as(C.c_void_p) if x is not None else None

    def call(out_nodes, capacity, out_plane, pitch=0, mem_labels=0, mem_out=0):
        n, total = C.c_size_t(77), C.c_int64(77)
        rc = lib.vsg_render_tree_cut(r.h, seg, len(seg), ptr(case.labels), pitch, mem_labels, 0, None, 0, 0,
                                     ptr(out_nodes), capacity, C.byref(n), ptr(out_plane), C.byref(total), mem_out)
        return rc, n.value, total.value

    total_ = tm.cut(tc.ids_of(case.msg), rm.hierarchy_of(case.msg), labels=case.labels)[2]
    assert call(None, 0, None) == (0, want_n, total_)                                    # count only
    assert call(nodes, want_n, plane, mem_labels=2)[0] == -1 and _untouched(nodes, plane)
    assert call(nodes, want_n, plane, mem_out=3)[0] == -1 and _untouched(nodes, plane)
    assert call(nodes, want_n, plane, pitch=W - 1)[0] == -1 and _untouched(nodes, plane)
    assert call(nodes, want_n - 1, plane) == (-1, want_n, total_) and _untouched(nodes, plane)
    assert call(nodes, 0, plane) == (-1, want_n, total_) and _untouched(nodes, plane)
    assert call(nodes, want_n, plane) == (0, want_n, total_)
    assert _untouched(nodes[want_n:]) and not _untouched(plane)
    assert lib.vsg_render_tree_cut_tuning(r.h, -2) == -1
    r.close()


def test_size_refusal_with_a_tall_hierarchy_on_a_small_frame(vsg):
    """64 x 64 one-pixel regions under 32769 levels: L * R is 4096 above 2^27."""
    from video_segment_amd._lib import VSG_ERR_INVALID, VsgError
    W = H = 64
    ids = np.arange(W * H, dtype=np.int32).reshape(H, W)
    tall = 32769
    msg = lc.desc_from_ids(ids, [{int(i): 1 for i in ids.ravel()}] + [{1: 1}] * (tall - 2))
    assert len(msg.hierarchy) == tall
    seg = msg.SerializeToString()
    r = vsg.SegmentationRenderer(W, H, has_video=False)
    nodes, plane = _filled(8, tm.NODE_DTYPE), _filled(W * H, np.int32).reshape(H, W)
    labels = np.zeros((H, W), np.int32)
    for source in (dict(labels=labels), dict(gains=np.zeros(0, tm.GAIN_DTYPE))):
        with pytest.raises(VsgError) as e:
            r.tree_cut(seg, nodes_out=nodes, plane_out=plane, **source)
        assert e.value.code == VSG_ERR_INVALID
        text = str(e.value)
        assert "L = 32769" in text and "R = 4096" in text, text
        assert ("P = 4096" if "labels" in source else "P = 0") in text, text
        assert _untouched(nodes, plane)
    r.close()


STREAM = (64, 48, 16, 8)   # W, H, frames, chunk size


@pytest.fixture(scope="module")
def stream(vsg):
    """A synth stream through the dense unit and the region stage: the serialized descs."""
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
    return segs


PENALTY = 5


def test_stream_end_to_end_and_the_drivers_line(vsg, stream):
    W, H, N, chunk = STREAM
    r = vsg.SegmentationRenderer(W, H, has_video=False)
    model_ = rm.RenderModel(W, H)
    arrays, n_nodes, sum_total, previous, heights = [], 0, 0, None, []
    for k, seg in enumerate(stream):
        m = lc.Msg()
        m.ParseFromString(seg)
        hier = model_._ingest(m)             # a desc without a hierarchy uses the kept one, as the handle does
        heights.append(len(hier))
        ids0 = model_.id_image(m, 0)
        if previous is not None:
            nodes, plane, total = r.tree_cut(seg, labels=previous, penalty=PENALTY)
            if k % 5 == 0 or k == N - 1:     # every frame is cut, a few are compared with the model
                want = tm.cut(ids0, hier, labels=previous, penalty=PENALTY)
                assert tm.same_bits(nodes, want[0]) and tm.same_bits(plane, want[1]) and total == want[2], k
            arrays += [nodes, plane]
            n_nodes += len(nodes)
            sum_total += total
        previous = r.id_image(seg, 0)
        assert np.array_equal(previous, ids0)
    assert max(heights) >= 2, heights
    r.close()
    subprocess.check_call(["make", "-C", HOST, "-s"])
    p = subprocess.run([os.path.join(HOST, "seg_tree_synth"), "--width", str(W), "--height", str(H), "--frames",
                        str(N), "--chunk_size", str(chunk), "--input", "soft", "--flow", "--region_segmentation",
                        "--chunk_set_size", "3", "--chunk_set_overlap", "1", "--min_region_num", "3",
                        "--nouse_pipeline", "--tree_cut", str(PENALTY)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    found = re.search(r"tree_cut_nodes=(\d+) tree_cut_total=(-?\d+) tree_cut_fnv1a32=(\w+)", p.stdout)
    assert found, p.stdout
    assert (int(found.group(1)), int(found.group(2))) == (n_nodes, sum_total)
    assert int(found.group(3), 16) == rm.fnv1a32(arrays)
