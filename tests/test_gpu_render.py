"""The renderer on the MI355X (libvsg_render.so: k_render_fill, k_render_compose) against the numpy
model of the reference (render_model.py), byte for byte: nothing about a rendered frame or an id image
is approximate, so there is no tolerance anywhere in this file."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import render_model as rm
import synth
from test_proto_wire import build_schema

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "video_segment_amd", "host")
Msg = build_schema()


@pytest.fixture(scope="module")
def vsg():
    import video_segment_amd as v
    from video_segment_amd import _lib, render
    _lib.build()
    render.build()
    assert _lib.lib().vsg_device_count() > 0
    return v


def parse(seg):
    m = Msg()
    m.ParseFromString(seg)
    return m


def overseg(vsg, W, H, N, chunk, frame_fn=synth.soft_frame, with_ids=False):
    """Dense over-segmentation on the GPU: (frames, serialized descs[, id images])."""
    fl = synth.const_flow(W, H)
    frames = [frame_fn(W, H, k) for k in range(N)]
    d = vsg.DenseSegmentation(W, H, vsg.default_options(chunk_size=chunk), has_flow=True)
    segs, ids = [], []
    for k in range(N):
        n = d.process_frame(frames[k], fl if k > 0 else None, flush=(k == N - 1))
        for i in range(n):
            segs.append(d.result_bytes(i))
            if with_ids:
                ids.append(d.result_id_image(i))
    d.close()
    assert len(segs) == N
    return (frames, segs, ids) if with_ids else (frames, segs)


def hierarchical(vsg, W, H, N, chunk, opts):
    """Dense on the GPU, RegionSegmentation on the host: (frames, over-segmentation descs and id
    images, hierarchical descs)."""
    frames, segs, ids = overseg(vsg, W, H, N, chunk, with_ids=True)
    fl = synth.const_flow(W, H)
    r = vsg.RegionSegmentation(W, H, vsg.default_region_options(**opts))
    out = []
    for k, seg in enumerate(segs):
        m = r.process_frame(seg, frames[k], fl if k > 0 else None, flush=(k == N - 1))
        out += [r.result_bytes(i) for i in range(m)]
    r.close()
    assert len(out) == N
    return frames, segs, ids, out


HIER_CASE = (96, 64, 60, 8, dict(chunk_set_size=3, chunk_set_overlap=1, constraint_chunks=1, min_region_num=3))


@pytest.fixture(scope="module")
def hier_case(vsg):
    W, H, N, chunk, opts = HIER_CASE
    return hierarchical(vsg, W, H, N, chunk, opts)


def option_combinations():
    for he, alpha in itertools.product((True, False), (0.5, 0.9, 1.0)):
        yield dict(highlight_edges=he, blend_alpha=alpha, has_video=True, concat_with_source=False)
        yield dict(highlight_edges=he, blend_alpha=alpha, has_video=True, concat_with_source=True)
        yield dict(highlight_edges=he, blend_alpha=alpha, has_video=False, concat_with_source=False)


def test_oversegmentation_level_0_every_option_combination(vsg):
    W, H, N, chunk = 320, 240, 20, 8
    frames, segs = overseg(vsg, W, H, N, chunk)
    msgs = [parse(s) for s in segs]
    assert len({m.chunk_id for m in msgs}) >= 3
    combos = list(option_combinations())
    assert len(combos) == 18
    for o in combos:
        r = vsg.SegmentationRenderer(W, H, **o)
        model = rm.RenderModel(W, H, **o)
        for k in range(N):
            got = r.render(segs[k], frames[k] if o["has_video"] else None)
            want = model.render(msgs[k], frames[k])
            assert got.shape == want.shape and got.dtype == np.uint8
            assert np.array_equal(got, want), (o, k)
        assert r.level == model.level
        r.close()
    # without video concatenation is refused
    from video_segment_amd._lib import VSG_ERR_INVALID, VsgError
    with pytest.raises(VsgError) as e:
        vsg.SegmentationRenderer(W, H, has_video=False, concat_with_source=True)
    assert e.value.code == VSG_ERR_INVALID


def test_hierarchy_levels_across_chunk_sets(vsg, hier_case):
    from video_segment_amd._lib import VSG_ERR_INVALID, VsgError
    W, H, N, chunk, _ = HIER_CASE
    frames, over_segs, over_ids, segs = hier_case
    msgs = [parse(s) for s in segs]
    heights = [len(m.hierarchy) for m in msgs]
    assert heights[0] >= 2 and sum(1 for h in heights if h > 0) >= 3   # the kept hierarchy is replaced
    for level in (0, 1, 2, 0.1, 0.4, 0.75, 50):
        r = vsg.SegmentationRenderer(W, H, hierarchy_level=level)
        model = rm.RenderModel(W, H, hierarchy_level=level)
        assert r.level is None
        for k in range(N):
            got = r.render(segs[k], frames[k])
            assert np.array_equal(got, model.render(msgs[k], frames[k])), (level, k)
        assert r.level == model.level
        r.close()
    # id images at every level of the current hierarchy
    r = vsg.SegmentationRenderer(W, H)
    model = rm.RenderModel(W, H)
    for k in range(N):
        current = len(model._ingest(msgs[k]))
        for level in range(current):
            assert np.array_equal(r.id_image(segs[k], level), model.id_image(msgs[k], level)), (k, level)
        with pytest.raises(VsgError) as e:
            r.id_image(segs[k], current)
        assert e.value.code == VSG_ERR_INVALID
    with pytest.raises(VsgError):
        r.id_image(segs[0], -1)
    # level 0 of the over-segmentation: what the dense stage itself reports
    for k in range(N):
        assert np.array_equal(r.id_image(over_segs[k], 0), over_ids[k]), k
    r.close()


def test_stride_padding_is_left_alone(vsg):
    import torch
    W, H = 322, 200
    assert (3 * W) % 4 != 0
    frames, segs = overseg(vsg, W, H, 3, 8)
    msgs = [parse(s) for s in segs]
    want = [rm.RenderModel(W, H).render(msgs[k], frames[k]) for k in range(3)]
    from video_segment_amd import render
    for stride in (render.default_stride(W), 1000, 971):   # default, larger, and one that is not dword aligned
        assert stride >= 3 * W
        buf = np.full((H, stride), 0xAB, np.uint8)
        view = buf[:, :3 * W].reshape(H, W, 3)
        r = vsg.SegmentationRenderer(W, H)
        for k in range(3):
            buf[:] = 0xAB
            out = r.render(segs[k], frames[k], out=view)
            assert out is view
            assert np.array_equal(view, want[k]), (stride, k)
            assert (buf[:, 3 * W:] == 0xAB).all(), (stride, k)
        r.close()
        # the same in device memory, with the source frame at that stride too
        dev = torch.device("cuda", 0)
        r = vsg.SegmentationRenderer(W, H)
        dbuf = torch.full((H, stride), 0xAB, dtype=torch.uint8, device=dev)
        dview = dbuf[:, :3 * W].view(H, W, 3)
        sbuf = torch.zeros((H, stride), dtype=torch.uint8, device=dev)
        sview = sbuf[:, :3 * W].view(H, W, 3)
        sview.copy_(torch.from_numpy(frames[1]))
        r.render(segs[1], sview, out=dview)
        assert np.array_equal(dview.cpu().numpy(), want[1]), stride
        assert bool((dbuf[:, 3 * W:] == 0xAB).all()), stride
        r.close()


def test_device_memory_in_and_out_equals_host_path(vsg):
    import torch
    W, H, N, chunk = 320, 240, 9, 8
    frames, segs = overseg(vsg, W, H, N, chunk)
    dev = torch.device("cuda", 0)
    for o in (dict(), dict(concat_with_source=True), dict(blend_alpha=0.9, highlight_edges=False)):
        rh = vsg.SegmentationRenderer(W, H, **o)
        rd = vsg.SegmentationRenderer(W, H, **o)
        for k in range(N):
            host = rh.render(segs[k], frames[k])
            got = rd.render(segs[k], torch.from_numpy(frames[k]).to(dev))
            assert got.is_cuda and got.dtype == torch.uint8
            assert np.array_equal(got.cpu().numpy(), host), (o, k)
            ids = torch.empty((H, W), dtype=torch.int32, device=dev)
            assert rd.id_image(segs[k], 0, out=ids) is ids
            assert np.array_equal(ids.cpu().numpy(), rh.id_image(segs[k], 0))
        rh.close()
        rd.close()


@pytest.mark.parametrize("W,H", [(1920, 1080), (3840, 2160)])
def test_full_size_chunk_result(vsg, W, H):
    N = 4
    frames, segs = overseg(vsg, W, H, N, 20)
    r = vsg.SegmentationRenderer(W, H)
    model = rm.RenderModel(W, H)
    for k in range(N):
        got = r.render(segs[k], frames[k])
        if k in (0, N - 1):    # first and last frame of the chunk
            m = parse(segs[k])
            want = model.render(m, frames[k])
            assert np.array_equal(got, want), k
            assert np.array_equal(r.id_image(segs[k], 0), model.id_image(m, 0)), k
    st = r.last_stats()
    assert st["launches"] <= 6 and st["intervals"] > 0
    r.close()


def pixel_regions_desc(W, H):
    """Every pixel a region of its own: W * H regions and intervals."""
    m = Msg()
    m.frame_width, m.frame_height = W, H
    for y in range(H):
        for x in range(W):
            r = m.region.add()
            r.id = y * W + x
            s = r.raster.scan_inter.add()
            s.y, s.left_x, s.right_x = y, x, x
    return m


def test_handle_reuse_allocates_nothing_in_steady_state(vsg):
    W, H = 160, 120
    rng = np.random.RandomState(5)
    frame = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    small = Msg()
    small.frame_width, small.frame_height = W, H
    reg = small.region.add()
    reg.id = 9
    for y in range(10, 20):
        s = reg.raster.scan_inter.add()
        s.y, s.left_x, s.right_x = y, 5, 100
    many = pixel_regions_desc(W, H)
    descs = [small, many, small]
    r = vsg.SegmentationRenderer(W, H)
    model = rm.RenderModel(W, H)
    allocs = []
    for _ in range(3):
        for d in descs:
            got = r.render(d.SerializeToString(), frame)
            assert np.array_equal(got, model.render(d, frame))
            assert np.array_equal(r.id_image(d.SerializeToString(), 0), model.id_image(d, 0))
            st = r.last_stats()
            assert st["launches"] <= 6
        allocs.append(r.last_stats()["device_allocations"])
    assert allocs[0] > 0 and allocs[1] == allocs[0] and allocs[2] == allocs[0], allocs
    assert r.last_stats()["intervals"] == 10
    r.close()


def test_intervals_outside_the_frame_are_refused(vsg):
    from video_segment_amd._lib import VSG_ERR_INVALID, VsgError
    W, H = 32, 16
    r = vsg.SegmentationRenderer(W, H, has_video=False)
    for y, lx, rx in ((16, 0, 3), (-1, 0, 3), (2, -1, 3), (2, 30, 32)):
        m = Msg()
        reg = m.region.add()
        reg.id = 1
        s = reg.raster.scan_inter.add()
        s.y, s.left_x, s.right_x = y, lx, rx
        with pytest.raises(VsgError) as e:
            r.render(m.SerializeToString())
        assert e.value.code == VSG_ERR_INVALID
    with pytest.raises(VsgError):
        r.render(b"\x12\x7f\x01")   # truncated message
    r.close()


@pytest.mark.parametrize("flags,model_options", [
    (["--render_level", "0.4"], dict(hierarchy_level=0.4)),
    (["--render_level", "0", "--render_concat"], dict(hierarchy_level=0, concat_with_source=True)),
    (["--render_level=2", "--render_blend_alpha=0.9"], dict(hierarchy_level=2, blend_alpha=0.9)),
])
def test_unit_tree_with_render_unit(vsg, hier_case, flags, model_options):
    """seg_tree_synth ... -> RegionSegmentationUnit -> SegmentationRenderUnit -> sinks: the hash over
    the rendered frames equals the model's, and the line the driver printed before is unchanged."""
    subprocess.check_call(["make", "-C", HOST, "-s"])
    W, H, N, chunk, _ = HIER_CASE
    frames, _, _, segs = hier_case
    model = rm.RenderModel(W, H, **model_options)
    want = rm.fnv1a32(model.render(parse(segs[k]), frames[k]) for k in range(N))
    base = [os.path.join(HOST, "seg_tree_synth"), "--width", str(W), "--height", str(H), "--frames", str(N),
            "--chunk_size", str(chunk), "--input", "soft", "--flow", "--region_segmentation",
            "--chunk_set_size", "3", "--chunk_set_overlap", "1", "--min_region_num", "3"]

    def first_line(stdout):
        return re.sub(r" seconds=\S+ fps=\S+", "", stdout.splitlines()[0])

    for extra in (["--use_pipeline"], ["--nouse_pipeline"]):
        plain = subprocess.run(base + extra, capture_output=True, text=True, timeout=300)
        assert plain.returncode == 0, plain.stderr
        assert "render_" not in plain.stdout
        p = subprocess.run(base + extra + flags, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        assert first_line(p.stdout) == first_line(plain.stdout)
        m = re.search(r"render_frames=(\d+) render_fnv1a32=(\w+) render_level=(-?\d+)", p.stdout)
        assert m, p.stdout
        assert int(m.group(1)) == N
        assert int(m.group(2), 16) == want
        assert int(m.group(3)) == model.level
