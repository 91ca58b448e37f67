"""The host writer's edits of a serialized SegmentationDesc (video_segment_amd/host/segmentation_io.cpp:
RemoveRasterization, ScaleVectorization, PrepareDescForWriting, the reference's
segmentation_unit.cpp:379-395) through `seg_tree_synth --rewrite_pb`, against the model's
remove_rasterization and scale_vectorization.  Needs no device."""
import os
import subprocess

import numpy as np
import pytest

import vector_cases as vc
import vector_raster_model as vm
from video_segment_amd import segmentation_io as sio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "video_segment_amd", "host")
EXE = os.path.join(HOST, "seg_tree_synth")


@pytest.fixture(scope="module")
def container(tmp_path_factory):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "video_segment_amd", "csrc"), "-j8", "-s"])
    subprocess.check_call(["make", "-C", HOST, "-s"])
    descs = [vc.vectorize(vc.l1_voronoi(seed, 64, 48, 12)) for seed in (11, 13)]
    assert all(m.frame_width == 64 and len(m.vector_mesh.coord) > 0 for m in descs)
    path = str(tmp_path_factory.mktemp("pb") / "in.pb")
    w = sio.SegmentationWriter(path)
    w.open_file([1, 0])
    for k, m in enumerate(descs):
        w.add_segmentation_data_to_chunk(m.SerializeToString(), 40000 * k)
    w.write_term_header_and_close()
    return path, descs


def rewrite(path, *flags):
    out = path + ".out"
    p = subprocess.run([EXE, "--rewrite_pb", path, "--output_file", out] + list(flags), capture_output=True,
                       text=True, timeout=60)
    return p, out


def parsed(frame_bytes):
    m = vc.Msg()
    m.ParseFromString(frame_bytes)
    return m


def test_default_writes_the_same_bytes(container):
    path, descs = container
    p, out = rewrite(path)
    assert p.returncode == 0, p.stderr
    assert open(out, "rb").read() == open(path, "rb").read()


def test_remove_rasterization_clears_rasters_and_sets_the_flag(container):
    path, descs = container
    p, out = rewrite(path, "--remove_rasterization")
    assert p.returncode == 0, p.stderr
    flags, frames, _ = sio.read_segmentation_file(out)
    assert flags == [1, 0] and [pts for pts, _ in frames] == [0, 40000]
    for (_, got), m in zip(frames, descs):
        want = vm.remove_rasterization(m)
        assert got == want.SerializeToString()
        g = parsed(got)
        assert g.rasterization_removed and all(not r.HasField("raster") for r in g.region)
        assert [list(q.coord_idx) for r in g.region for q in r.vectorization.polygon] == \
               [list(q.coord_idx) for r in m.region for q in r.vectorization.polygon]


@pytest.mark.parametrize("size", [(96, 72), (100, 75)])
def test_scaling_branch(container, size):
    path, descs = container
    W, H = size
    p, out = rewrite(path, "--remove_rasterization", "--original_width", str(W), "--original_height", str(H))
    assert p.returncode == 0, p.stderr
    _, frames, _ = sio.read_segmentation_file(out)
    for (_, got), m in zip(frames, descs):
        g = parsed(got)
        assert (g.frame_width, g.frame_height) == (W, H) and g.rasterization_removed
        assert all(not r.HasField("raster") for r in g.region)
        want = vm.scale_vectorization(np.asarray(m.vector_mesh.coord, np.float32), 64, 48, W, H)
        assert np.array_equal(np.asarray(g.vector_mesh.coord, np.float32), want)
        # the written desc rasterizes at its own size to what the unscaled one gives at that size
        a, ua = vm.rasterize_desc(g)
        b, ub = vm.rasterize_desc(vm.remove_rasterization(m), W, H)
        assert ua == 0 and ub == 0 and np.array_equal(a, b)
    # without remove_rasterization the reference re-rasterizes on the host; this layer says it cannot
    p, _ = rewrite(path, "--original_width", str(W), "--original_height", str(H))
    assert p.returncode != 0 and "remove_rasterization" in p.stderr


def test_desc_without_a_mesh_is_left_alone(tmp_path):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    m = vc.Msg()
    m.frame_width, m.frame_height = 8, 4
    r = m.region.add()
    r.id = 3
    s = r.raster.scan_inter.add()
    s.y, s.left_x, s.right_x = 1, 2, 5
    path = str(tmp_path / "plain.pb")
    w = sio.SegmentationWriter(path)
    w.open_file([1, 0])
    w.add_segmentation_data_to_chunk(m.SerializeToString(), 0)
    w.write_term_header_and_close()
    p, out = rewrite(path, "--remove_rasterization", "--original_width", "16", "--original_height", "8")
    assert p.returncode == 0, p.stderr
    assert sio.read_segmentation_file(out)[1][0][1] == m.SerializeToString()
