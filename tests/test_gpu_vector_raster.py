"""Vector-only descs on the MI355X (libvsg_render.so: k_vec_walk, radix sort, k_vec_pairs, then the
renderer's own two kernels) against the numpy model of the reference's RasterVectorization
(vector_raster_model.py): int32 and byte equality, no tolerance anywhere.

Every input's model run has to report zero `unspecified` rows before anything is compared (the cases
that are meant to be refused assert the opposite).  Seeds: 11 for the 64 x 48 partition, 12 for the
1920 x 1080 one; neither trips that assertion."""
import ctypes as C

import numpy as np
import pytest

import render_model as rm
import vector_cases as vc
import vector_raster_model as vm
from test_boundary import CASES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vsg():
    import video_segment_amd as v
    from video_segment_amd import _lib, render
    _lib.build()
    render.build()
    assert _lib.lib().vsg_device_count() > 0
    return v


def model_rows(msg, W, H):
    rows, unspecified = vm.rasterize_desc(msg, W, H)
    assert unspecified == 0, "the model does not define %d rows of this input" % unspecified
    return rows


def check_all(vsg, msg, W, H, frame_seed=1):
    """rasterize(), id_image(level 0) and render() of a vector-only desc at W x H against the model."""
    assert msg.rasterization_removed and all(len(r.raster.scan_inter) == 0 for r in msg.region)
    seg = msg.SerializeToString()
    want = model_rows(msg, W, H)
    r = vsg.SegmentationRenderer(W, H)
    got = r.rasterize(seg)
    assert got.dtype == np.int32 and got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want)
    st = r.last_vector_stats()
    assert st["crossings"] == 2 * len(want) and st["launches"] > 0
    groups = {(int(rid), int(y)) for y, _, _, rid in want}
    assert st["groups"] == len(groups)
    assert np.array_equal(r.id_image(seg, 0), vm.id_plane(want, W, H))
    frame = np.random.RandomState(frame_seed).randint(0, 256, (H, W, 3)).astype(np.uint8)
    fed = vm.with_intervals(msg, want, W, H)
    assert np.array_equal(r.render(seg, frame), rm.RenderModel(W, H).render(fed, frame))
    assert r.last_stats()["intervals"] == len(want)
    r.close()
    return want, st


@pytest.fixture(scope="module")
def voronoi_desc(vsg):
    ids = vc.l1_voronoi(11, 64, 48, 12)
    assert len(np.unique(ids)) == 12
    return vc.vector_only(ids)


def test_voronoi_64x48(vsg, voronoi_desc):
    want, _ = check_all(vsg, voronoi_desc, 64, 48)
    assert (want[:, 1] > want[:, 2]).any()      # it has empty intervals, and they are exported


@pytest.mark.parametrize("name", ["hole", "nested", "four_corner", "diagonal_touch"])
def test_boundary_cases(vsg, name):
    ids = CASES[name]
    want, _ = check_all(vsg, vc.vector_only(ids), ids.shape[1], ids.shape[0])
    assert np.array_equal(vm.id_plane(want, ids.shape[1], ids.shape[0]), ids)


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (5, 9)])
def test_smallest_frames_and_one_region(vsg, shape):
    check_all(vsg, vc.vector_only(np.zeros(shape, np.int32)), shape[1], shape[0])


def test_one_pixel_regions_in_a_row(vsg):
    check_all(vsg, vc.vector_only(np.arange(7, dtype=np.int32).reshape(1, 7)), 7, 1)


def test_comb_is_one_large_group(vsg):
    m = vc.comb(40)
    _, st = check_all(vsg, m, 80, 3)
    assert st["largest_group"] == 80 and st["groups"] == 3


def test_hand_made_apex_pinch_hole_and_empty_region(vsg):
    check_all(vsg, vc.hourglass(), 10, 10)
    check_all(vsg, vc.make_desc(10, 8, [(1, [[(5, 2), (8, 6), (2, 6), (5, 2)]])]), 10, 8)
    check_all(vsg, vc.make_desc(10, 9, [(4, []), (2, [vc.rect(1, 1, 9, 8), vc.rect(3, 3, 6, 5)[::-1]]), (9, [])]),
              10, 9)
    check_all(vsg, vc.make_desc(7, 3, [(1, [[(7, 0), (7, 3), (4, 3), (7, 0)]]), (2, [vc.rect(0, 0, 4.5, 1)])]), 7, 3)
    # no polygon anywhere: an empty list, an empty picture
    m = vc.make_desc(6, 4, [(1, []), (2, [])])
    r = vsg.SegmentationRenderer(6, 4, has_video=False)
    assert r.rasterize(m.SerializeToString()).shape == (0, 4)
    assert (r.render(m.SerializeToString()) == 0).all()
    assert (r.id_image(m.SerializeToString()) == -1).all()
    r.close()


def test_300_two_line_regions(vsg):
    m = vc.two_line_regions(300)
    _, st = check_all(vsg, m, m.frame_width, m.frame_height)
    assert st["lines"] == 600 and st["groups"] == 600 and st["largest_group"] == 2


@pytest.mark.parametrize("size", [(96, 72), (100, 75)])
def test_scaled_to_the_handles_size(vsg, voronoi_desc, size):
    W, H = size
    assert (voronoi_desc.frame_width, voronoi_desc.frame_height) == (64, 48)
    check_all(vsg, voronoi_desc, W, H)


def test_device_output_with_a_canary_and_capacity(vsg, voronoi_desc):
    import torch
    from video_segment_amd._lib import VSG_ERR_INVALID, VsgError
    from video_segment_amd import render
    W, H = 64, 48
    seg = voronoi_desc.SerializeToString()
    want = model_rows(voronoi_desc, W, H)
    n = len(want)
    dev = torch.device("cuda", 0)
    r = vsg.SegmentationRenderer(W, H)
    buf = torch.full((n + 8, 4), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    got = r.rasterize(seg, out=buf[:n])
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    assert bool((buf[n:] == 0x5A5A5A5A).all())
    # capacity one short: refused, the count reported, the buffer untouched, the handle usable
    host = np.full((n - 1, 4), -7, np.int32)
    count = C.c_size_t()
    rc = render.lib().vsg_render_rasterize(r.h, seg, len(seg), host.ctypes.data_as(C.c_void_p), n - 1,
                                           C.byref(count), 0)
    assert rc == VSG_ERR_INVALID and count.value == n and (host == -7).all()
    with pytest.raises(VsgError):
        r.rasterize(seg, out=host)
    assert np.array_equal(r.rasterize(seg), want)
    r.close()


def test_undefined_rows_and_bad_indices_are_refused(vsg, voronoi_desc):
    from video_segment_amd._lib import VSG_ERR_INVALID, VsgError
    good_seg = voronoi_desc.SerializeToString()
    want = model_rows(voronoi_desc, 64, 48)
    bad = {"bow_tie": vc.bow_tie(),
           "open polylines": vc.make_desc(8, 8, [(1, [[(2, 1), (2, 5), (6, 5)]]), (2, [[(3, 1), (3, 5)]])]),
           "leaves the row": vc.make_desc(8, 8, [(1, [vc.rect(2, 1, 9, 3)])]),
           "indistinguishable": vc.make_desc(8, 2, [(1, [[(2, 0), (2, 2)], [(2.0005, 0), (2.0005, 2)]])])}
    for name, m in bad.items():
        assert vm.rasterize_desc(m)[1] > 0, name
    idx = vc.make_desc(8, 8, [(1, [vc.rect(1, 1, 5, 5)])])
    idx.region[0].vectorization.polygon[0].coord_idx[2] = len(idx.vector_mesh.coord) - 1
    bad["coord_idx"] = idx
    rows = vc.make_desc(8, 8, [(1, [vc.rect(1, 1, 5, 9)])])
    bad["below the frame"] = rows
    for name, m in bad.items():
        W, H = m.frame_width, m.frame_height
        r = vsg.SegmentationRenderer(W, H, has_video=False)
        for call in (r.rasterize, r.render, r.id_image):
            with pytest.raises(VsgError) as e:
                call(m.SerializeToString())
            assert e.value.code == VSG_ERR_INVALID, (name, call)
        # the handle is usable afterwards
        ok = vc.make_desc(W, H, [(3, [vc.rect(0, 0, 2, 2)])])
        assert r.rasterize(ok.SerializeToString()).tolist() == [[0, 0, 1, 3], [1, 0, 1, 3]]
        r.close()
    r = vsg.SegmentationRenderer(64, 48)
    with pytest.raises(VsgError):
        r.rasterize(vc.bow_tie(64, 48).SerializeToString())
    assert np.array_equal(r.rasterize(good_seg), want)
    r.close()


def test_desc_with_rasters_is_rendered_as_before(vsg, voronoi_desc):
    """rasterization_removed = false: the rasters are painted, the vectorization is not looked at, and
    another frame size is still refused."""
    from video_segment_amd._lib import VSG_ERR_INVALID, VsgError
    W, H = 64, 48
    ids = vc.l1_voronoi(11, W, H, 12)
    full = vc.vectorize(ids)
    assert not full.rasterization_removed and len(full.vector_mesh.coord) > 0
    bare = vc.Msg()
    bare.CopyFrom(full)
    bare.ClearField("vector_mesh")
    for reg in bare.region:
        reg.ClearField("vectorization")
    frame = np.random.RandomState(2).randint(0, 256, (H, W, 3)).astype(np.uint8)
    r = vsg.SegmentationRenderer(W, H)
    got = r.render(full.SerializeToString(), frame)
    assert r.last_vector_stats()["crossings"] == 0
    assert np.array_equal(got, r.render(bare.SerializeToString(), frame))
    assert np.array_equal(got, rm.RenderModel(W, H).render(full, frame))
    assert np.array_equal(r.id_image(full.SerializeToString(), 0), ids)
    r.close()
    full.frame_width, full.frame_height = W, H
    r = vsg.SegmentationRenderer(96, 72, has_video=False)
    with pytest.raises(VsgError) as e:
        r.render(full.SerializeToString())
    assert e.value.code == VSG_ERR_INVALID
    r.close()


def test_thirty_frames_allocate_only_on_the_first(vsg, voronoi_desc):
    W, H = 64, 48
    seg = voronoi_desc.SerializeToString()
    frame = np.zeros((H, W, 3), np.uint8)
    r = vsg.SegmentationRenderer(W, H)
    allocs = []
    for _ in range(30):
        r.render(seg, frame)
        r.id_image(seg, 0)
        r.rasterize(seg)
        allocs.append(r.last_stats()["device_allocations"])
    assert allocs[0] > 0 and len(set(allocs)) == 1, allocs
    r.close()


def test_full_hd_frame_with_300_seeds(vsg):
    W, H = 1920, 1080
    m = vc.vector_only(vc.l1_voronoi(12, W, H, 300))
    seg = m.SerializeToString()
    want = model_rows(m, W, H)
    r = vsg.SegmentationRenderer(W, H, has_video=False)
    got = r.rasterize(seg)
    assert rm.fnv1a32([got]) == rm.fnv1a32([want])
    assert np.array_equal(got, want)
    # the picture: equality of all bytes, of which the hash the issue names is a function
    picture = r.render(seg)
    assert np.array_equal(picture, rm.RenderModel(W, H, has_video=False).render(vm.with_intervals(m, want, W, H)))
    st = r.last_vector_stats()
    assert st["crossings"] == 2 * len(want) and st["walk_us"] > 0 and st["sort_us"] > 0 and st["pairs_us"] > 0
    r.close()


def test_unit_tree_writes_and_renders_vector_only_descs(vsg, tmp_path):
    """seg_tree_synth --over_segment --write_to_file --remove_rasterization --render_level 0: the
    container's descs carry no scan_inter, SegmentationRenderUnit renders the same vector-only descs,
    and the hash over its frames equals the model's.  With an original size the writer scales."""
    import os
    import re
    import subprocess
    import synth
    from video_segment_amd import segmentation_io as sio
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    host = os.path.join(root, "video_segment_amd", "host")
    subprocess.check_call(["make", "-C", host, "-s"])
    W, H, N = 64, 48, 12
    out = str(tmp_path / "vector.pb")
    base = [os.path.join(host, "seg_tree_synth"), "--width", str(W), "--height", str(H), "--frames", str(N),
            "--chunk_size", "8", "--input", "soft", "--flow", "--over_segment"]

    def first_line(stdout):
        return re.sub(r" seconds=\S+ fps=\S+ pipeline=\d", "", stdout.splitlines()[0])

    plain = subprocess.run(base + ["--nouse_pipeline"], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stderr
    want_hash = None
    for extra in (["--use_pipeline"], ["--nouse_pipeline"]):
        p = subprocess.run(base + extra + ["--write_to_file", "--output_file", out, "--remove_rasterization",
                                           "--render_level", "0"], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        assert first_line(p.stdout) == first_line(plain.stdout)     # labels and bytes of the stream: unchanged
        flags, frames, _ = sio.read_segmentation_file(out)
        assert flags == [1, 0] and len(frames) == N
        if want_hash is None:
            model = rm.RenderModel(W, H, hierarchy_level=0)
            pictures = []
            for k, (_, seg) in enumerate(frames):
                m = vc.Msg()
                m.ParseFromString(seg)
                assert m.rasterization_removed and len(m.vector_mesh.coord) > 0
                assert all(len(r.raster.scan_inter) == 0 for r in m.region)
                assert (m.frame_width, m.frame_height) == (W, H)
                rows = model_rows(m, W, H)
                pictures.append(model.render(vm.with_intervals(m, rows, W, H), synth.soft_frame(W, H, k)))
            want_hash = rm.fnv1a32(pictures)
        got = re.search(r"render_frames=(\d+) render_fnv1a32=(\w+)", p.stdout)
        assert got, p.stdout
        assert int(got.group(1)) == N and int(got.group(2), 16) == want_hash
    # a video that was downscaled from 96 x 72: the written descs have that size
    p = subprocess.run(base + ["--write_to_file", "--output_file", out, "--remove_rasterization", "--original_width",
                               "96", "--original_height", "72"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    _, scaled, _ = sio.read_segmentation_file(out)
    for (_, a), (_, b) in zip(scaled, frames):
        ma, mb = vc.Msg(), vc.Msg()
        ma.ParseFromString(a)
        mb.ParseFromString(b)
        assert (ma.frame_width, ma.frame_height) == (96, 72) and ma.rasterization_removed
        want = vm.scale_vectorization(np.asarray(mb.vector_mesh.coord, np.float32), W, H, 96, 72)
        assert np.array_equal(np.asarray(ma.vector_mesh.coord, np.float32), want)
    r = vsg.SegmentationRenderer(96, 72, has_video=False)
    m0 = vc.Msg()
    m0.ParseFromString(frames[0][1])
    assert np.array_equal(r.rasterize(scaled[0][1]), model_rows(m0, 96, 72))
    r.close()
