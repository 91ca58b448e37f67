"""vsg_render_level_mesh_simplified on the MI355X (libvsg_render.so: the contour and mesh stages, then
k_simplify_dp_wave, k_simplify_dp_block, k_simplify_clean, the scan, k_simplify_compact, k_simplify_records,
k_copy_lists) against level_mesh_simplify_model.py, which applies boundary_oracle.approx_poly_dp to every
segment's full lattice point list, and against the mesh and rasterize calls of the same handle.  All four lists
are compared as raw bytes: there is no tolerance anywhere in this file.  The device takes a fraction of a second
on every case; the slowest case, comb_8192, spends its time in the Python model, whose recursion on 49 146 lattice
points is as deep as the comb has teeth."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import level_components_model as cm
import level_contours_model as tm
import level_mesh_model as mm
import level_mesh_simplify_cases as sc
import level_mesh_simplify_model as sm
import level_regions_cases as lc
import render_model as rm
import synth
import vector_raster_model as vm

pytestmark = pytest.mark.gpu

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "video_segment_amd", "host")
CASES = sc.all_cases()
BY_NAME = {c.name: c for c in CASES}
MODES = (0, cm.N4, cm.N8)
NAMES = ("segments", "vertices", "loops", "refs")
PARAMS = sc.PARAMS


@pytest.fixture(scope="module")
def vsg():
    import video_segment_amd as v
    from video_segment_amd import _lib, render
    _lib.build()
    render.build()
    assert _lib.lib().vsg_device_count() > 0
    assert (render.N4, render.N8) == (cm.N4, cm.N8)
    return v


def assert_same(got, want, what):
    assert len(got) == len(want) == 4
    for name, a, b in zip(NAMES, got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.shape, b.shape)
        assert mm.same_bits(a, b), (what, name)


def plane_of(ids, connect):
    if connect == 0:
        return ids, None
    comps, _, labels = cm.sweep(ids, connect)
    return labels, comps


def check_ids(r, seg, ids, level, what, modes=MODES, params=PARAMS):
    """Every mode and parameter pair of one level against the model, with the counts, and against level_mesh."""
    for connect in modes:
        plane, comps = plane_of(ids, connect)
        mesh = mm.mesh(plane, comps)
        plain = r.level_mesh(seg, level, connect)
        assert_same(plain, mesh, (what, level, connect, "mesh"))
        for e, msp in params:
            key = (what, level, connect, e, msp)
            want = sm.simplified(plane, comps, e, msp, result=mesh)
            got = r.level_mesh_simplified(seg, level, connect, e, msp)
            assert_same(got, want, key)
            assert mm.same_bits(got[2], plain[2]) and mm.same_bits(got[3], plain[3]), key
            st = r.last_simplify_stats()
            assert {k: st[k] for k in sm.COUNTS} == sm.stats_of(mesh, e, msp), key
            ms = r.last_mesh_stats()
            assert ms["segments"] == len(mesh[0]) and ms["vertices"] == st["vertices_in"], key
            assert r.last_contour_stats()["cracks"] == ms["cracks"], key
            if (e, msp) == (0.0, 0):
                for a, b in zip(got[0], plain[0]):
                    assert a["num_vertices"] == b["num_vertices"], key
                    if not a["closed"]:
                        assert np.array_equal(got[1][a["first_vertex"]:a["first_vertex"] + a["num_vertices"]],
                                              plain[1][b["first_vertex"]:b["first_vertex"] + b["num_vertices"]]), key


def check_case(vsg, case, modes=MODES, params=PARAMS):
    r = vsg.SegmentationRenderer(case.W, case.H, has_video=False)
    seg = case.msg.SerializeToString()
    for level in case.levels:
        check_ids(r, seg, np.array(lc.id_image(case.msg, level), np.int32), level, case.name, modes, params)
    r.close()


@pytest.mark.parametrize("name", sorted(BY_NAME))
def test_every_case_in_every_mode_at_every_level(vsg, name):
    check_case(vsg, BY_NAME[name])


def test_a_frame_without_a_covered_pixel(vsg):
    c = BY_NAME["uncovered_frame"]
    r = vsg.SegmentationRenderer(c.W, c.H)
    for connect in MODES:
        segments, vertices, loops, refs = r.level_mesh_simplified(c.msg.SerializeToString(), 0, connect)
        assert segments.shape == (0,) and segments.dtype == mm.SEGMENT_DTYPE
        assert vertices.shape == (0, 2) and vertices.dtype == np.int32
        assert loops.shape == (0,) and loops.dtype == mm.LOOP_DTYPE and refs.shape == (0,) and refs.dtype == np.int32
        st = r.last_simplify_stats()
        assert all(st[k] == 0 for k in sm.COUNTS)
    r.close()


def test_a_desc_made_of_the_simplified_mesh_rasterizes(vsg):
    """At (0, 0) back to the id plane, bit for bit; at (1, 4) without a refusal, to a plane of the same ids."""
    from video_segment_amd import render
    for name, levels in (("three_levels", None), ("euclidean_voronoi_200x150", (0,))):
        c = BY_NAME[name]
        r = vsg.SegmentationRenderer(c.W, c.H)
        seg = c.msg.SerializeToString()
        for level in levels or (0, max(c.levels)):
            ids = r.id_image(seg, level)
            for connect in (0, cm.N4):
                if connect == 0:
                    group_ids = r.level_regions(seg, level)[0]["id"]
                else:
                    group_ids = r.level_components(seg, level, connect)[0]["id"]
                exact = r.level_mesh_simplified(seg, level, connect, 0.0, 0)
                rows = r.rasterize(render.simplified_mesh_desc(c.W, c.H, group_ids, *exact))
                assert r.last_vector_stats()["lines"] > 0
                assert np.array_equal(vm.id_plane(rows, c.W, c.H), ids), (name, level, connect)
                coarse = r.level_mesh_simplified(seg, level, connect, 1.0, 4)
                rows = r.rasterize(render.simplified_mesh_desc(c.W, c.H, group_ids, *coarse))
                back = vm.id_plane(rows, c.W, c.H)
                assert set(np.unique(back).tolist()) <= set(np.unique(ids).tolist()) | {-1}, (name, level, connect)
        r.close()


def test_bad_levels_and_bad_arguments(vsg):
    from video_segment_amd._lib import VSG_ERR_INVALID, VsgError
    c = BY_NAME["three_levels"]
    r = vsg.SegmentationRenderer(c.W, c.H)
    seg = c.msg.SerializeToString()
    bad = [dict(level=3), dict(level=-1), dict(connectedness=3), dict(max_error=-0.5), dict(max_error=float("nan")),
           dict(max_error=float("inf")), dict(min_segment_points=-1)]
    for kwargs in bad:
        with pytest.raises(VsgError) as e:
            r.level_mesh_simplified(seg, **kwargs)
        assert e.value.code == VSG_ERR_INVALID, kwargs
    ids = np.array(lc.id_image(c.msg, 2), np.int32)
    plane, comps = plane_of(ids, cm.N8)
    assert_same(r.level_mesh_simplified(seg, 2, cm.N8), sm.simplified(plane, comps), "after the refusals")
    r.close()


def test_capacities_and_count_only(vsg):
    from video_segment_amd import render
    c = BY_NAME["euclidean_voronoi_200x150"]
    seg = c.msg.SerializeToString()
    L = render.lib()
    r = vsg.SegmentationRenderer(c.W, c.H)
    ids = np.array(lc.id_image(c.msg, 0), np.int32)
    for connect in (0, cm.N4):
        plane, comps = plane_of(ids, connect)
        want = sm.simplified(plane, comps, 1.0, 4)
        sizes = tuple(len(a) for a in want)

        def call(outs, caps):
            counts = [C.c_size_t(77) for _ in range(4)]
            args = []
            for o, cap, n in zip(outs, caps, counts):
                args += [o.ctypes.data_as(C.c_void_p) if o is not None else None, cap, C.byref(n)]
            rc = L.vsg_render_level_mesh_simplified(r.h, seg, len(seg), 0, connect, 1.0, 4, *args, 0)
            return (rc,) + tuple(n.value for n in counts)

        assert call([None] * 4, [0] * 4) == (0,) + sizes                      # count only
        outs = [np.zeros(sizes[0] + 2, mm.SEGMENT_DTYPE), np.zeros((sizes[1] + 2, 2), np.int32),
                np.zeros(sizes[2] + 2, mm.LOOP_DTYPE), np.zeros(sizes[3] + 2, np.int32)]

        def fill():
            for o in outs:
                o.view(np.uint8).reshape(-1)[:] = 0x5A

        def untouched(o, start=0):
            return (o[start:].view(np.uint8) == 0x5A).all()

        for k in range(4):                                                    # each capacity one too small
            caps = list(sizes)
            caps[k] -= 1
            fill()
            assert call(outs, caps) == (-1,) + sizes, k
            assert all(untouched(o) for o in outs), k
        fill()
        assert call(outs, [0] * 4) == (-1,) + sizes and all(untouched(o) for o in outs)
        fill()
        assert call(outs, list(sizes)) == (0,) + sizes                        # exact capacities
        assert_same([o[:n] for o, n in zip(outs, sizes)], want, "exact")
        assert all(untouched(o, n) for o, n in zip(outs, sizes))
    r.close()


def test_device_outputs_equal_host_outputs(vsg):
    import torch
    from video_segment_amd import render
    c = BY_NAME["three_levels"]
    seg = c.msg.SerializeToString()
    dev = torch.device("cuda", 0)
    r = vsg.SegmentationRenderer(c.W, c.H)
    widths = (render.MESH_SEGMENT_WORDS, 2, render.MESH_LOOP_WORDS, 0)
    guard = 0x5A5A5A5A
    for level in c.levels:
        for connect in MODES:
            for e, msp in ((0.0, 0), (1.0, 4)):
                host = r.level_mesh_simplified(seg, level, connect, e, msp)
                sizes = [len(a) for a in host]
                outs = [torch.full((n + 3, w) if w else (n + 3,), guard, dtype=torch.int32, device=dev)
                        for n, w in zip(sizes, widths)]
                got = r.level_mesh_simplified(seg, level, connect, e, msp, *outs)
                for name, g, h, n, w in zip(NAMES, got, host, sizes, widths):
                    assert g.is_cuda and tuple(g.shape) == ((n, w) if w else (n,)), name
                    assert g.cpu().numpy().tobytes() == h.tobytes(), (name, level, connect)
                assert all(bool((o[n:] == guard).all()) for o, n in zip(outs, sizes))
                # each list one entry too short: refused, nothing written
                for k in range(4):
                    for o in outs:
                        o.fill_(guard)
                    cut = [o[:n - (1 if j == k else 0)] for j, (o, n) in enumerate(zip(outs, sizes))]
                    with pytest.raises(render.VsgError):
                        r.level_mesh_simplified(seg, level, connect, e, msp, *cut)
                    assert all(bool((o == guard).all()) for o in outs), (k, level, connect)
    r.close()


def test_handle_reuse_with_the_other_level_calls_before_and_after(vsg):
    small, large = lc.reuse_sequence()
    r = vsg.SegmentationRenderer(small.W, small.H)
    segs = {c.name: c.msg.SerializeToString() for c in (small, large)}

    def siblings(s):
        return (r.level_mesh(s, 0, cm.N8), r.level_contours(s, 0, cm.N4), r.level_boundaries(s, 0, cm.N4))

    before = {n: siblings(s) for n, s in segs.items()}
    want = {}
    for c in (small, large):
        for k in (0, cm.N8):
            plane, comps = plane_of(np.array(lc.id_image(c.msg, 0), np.int32), k)
            want[c.name, k] = sm.simplified(plane, comps, 1.0, 4)
    allocs = []
    for _ in range(2):
        for c in (small, large, small):
            for k in (0, cm.N8):
                assert_same(r.level_mesh_simplified(segs[c.name], 0, k), want[c.name, k], (c.name, k))
                r.level_mesh(segs[c.name], 0, k)               # interleaved: shares the mesh stages' blocks
                r.level_contours(segs[c.name], 0, k)
                r.level_boundaries(segs[c.name], 0, k)         # and the sort's work space
            allocs.append(r.last_stats()["device_allocations"])
    # the second round of identical calls allocates nothing
    assert allocs[1] > allocs[0] > 0 and allocs[3:] == [allocs[2]] * 3, allocs
    for n, s in segs.items():
        for a, b in zip(siblings(s), before[n]):
            assert all(tm.same_bits(x, y) for x, y in zip(a, b)), n
    r.close()


def test_the_level_of_render_is_neither_resolved_nor_changed(vsg):
    c = BY_NAME["three_levels"]
    seg = c.msg.SerializeToString()
    r = vsg.SegmentationRenderer(c.W, c.H, hierarchy_level=1, has_video=False)
    assert r.level is None
    for level in c.levels:
        r.level_mesh_simplified(seg, level, cm.N4)
        assert r.level is None
    first = r.render(seg)
    assert r.level == 1
    for level in c.levels:
        r.level_mesh_simplified(seg, level)
        assert r.level == 1
    assert tm.same_bits(r.render(seg), first)
    r.close()


def test_launches_are_a_function_of_the_mode_and_the_rounds(vsg):
    """Over every case at level 0 and every parameter pair, host outputs: one value per (connectedness, rounds of
    the doublings), whatever the recursion's depth."""
    seen = {}
    depths = set()
    for c in CASES:
        r = vsg.SegmentationRenderer(c.W, c.H, has_video=False)
        seg = c.msg.SerializeToString()
        for connect in MODES:
            for e, msp in PARAMS:
                r.level_mesh_simplified(seg, 0, connect, e, msp)
                st, ms = r.last_simplify_stats(), r.last_mesh_stats()
                if ms["cracks"]:
                    seen.setdefault((connect, ms["rounds"]), set()).add(st["launches"])
                    depths.add(st["max_rounds"])
                    assert st["launches"] > ms["launches"]
        r.close()
    assert all(len(v) == 1 for v in seen.values()), {k: v for k, v in seen.items() if len(v) > 1}
    assert min(depths) == 0 and max(depths) >= 64


STREAM = (96, 64, 16, 8)   # W, H, frames, chunk size


@pytest.fixture(scope="module")
def stream(vsg):
    """The synth stream through the dense unit and the hierarchical stage: the serialized descs."""
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


def test_a_real_stream_every_frame_at_every_level(vsg, stream):
    """Every frame at every level in the regions' mode at (1.0, 4), the reference's parameters.  All three modes
    at all five parameter pairs on the frames with k % 5 == 1 and on the last frame only."""
    W, H, N, _ = STREAM
    r = vsg.SegmentationRenderer(W, H)
    model_ = rm.RenderModel(W, H)
    for k, seg in enumerate(stream):
        m = lc.Msg()
        m.ParseFromString(seg)
        hier = model_._ingest(m)                 # a desc without a hierarchy uses the kept one, as the handle does
        for level in range(max(len(hier), 1)):
            # every frame and level at the reference's parameters, a few frames in all modes at all of them
            full = k % 5 == 1 or k == N - 1
            check_ids(r, seg, np.array(model_.id_image(m, level), np.int32), level, ("stream", k),
                      MODES if full else (0,), PARAMS if full else ((1.0, 4),))
    r.close()


def test_driver_prints_the_python_paths_sums(vsg, stream):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    W, H, N, chunk = STREAM
    r = vsg.SegmentationRenderer(W, H)
    base = [os.path.join(HOST, "seg_tree_synth"), "--width", str(W), "--height", str(H), "--frames", str(N),
            "--chunk_size", str(chunk), "--input", "soft", "--flow", "--region_segmentation",
            "--chunk_set_size", "3", "--chunk_set_overlap", "1", "--min_region_num", "3", "--nouse_pipeline"]
    for flags, connect, e, msp in (
            (["--level_mesh", "0", "--mesh_max_error", "1.0"], 0, 1.0, 4),
            (["--level_mesh", "0", "--mesh_components", "--components_n8", "--mesh_max_error", "1.5",
              "--mesh_min_segment_points", "3"], cm.N8, 1.5, 3)):
        lists = [r.level_mesh_simplified(seg, 0, connect, e, msp) for seg in stream]
        p = subprocess.run(base + flags, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        assert "level_mesh_count=" not in p.stdout
        m = re.search(r"level_mesh_simplified_count=(\d+) level_mesh_simplified_fnv1a32=(\w+)", p.stdout)
        assert m, p.stdout
        assert int(m.group(1)) == sum(len(four[0]) for four in lists)
        assert int(m.group(2), 16) == rm.fnv1a32(a for four in lists for a in four)
    r.close()
    # a flag without the one it belongs to, and values the call would refuse, end the driver before any frame
    for flags, word in ((["--mesh_max_error", "1.0"], "--level_mesh"),
                        (["--level_mesh", "0", "--mesh_min_segment_points", "3"], "--mesh_max_error"),
                        (["--level_mesh", "0", "--mesh_max_error", "-1"], ">= 0"),
                        (["--level_mesh", "0", "--mesh_max_error", "nan"], ">= 0"),
                        (["--level_mesh", "0", "--mesh_max_error", "1", "--mesh_min_segment_points", "-2"], ">= 0")):
        p = subprocess.run(base + flags, capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and word in p.stderr and "level_mesh" not in p.stdout, (flags, p.stderr)
