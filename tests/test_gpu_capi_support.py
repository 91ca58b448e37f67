"""What libvsg_resize, libvsg_flow and libvsg_render take from video_segment_amd/common/capi_support.h,
seen through their statistics on the MI355X: the stage clock times exactly the stages a call ran, the
blocks of a handle stop growing after the first call of a kind, and a handle of another device leaves
the caller's current device alone.  What the libraries compute is checked by test_gpu_resize.py,
test_gpu_flow.py, test_gpu_render.py and test_gpu_vector_raster.py."""
import numpy as np
import pytest

import render_model
from test_render_model import make_desc

pytestmark = pytest.mark.gpu

RESIZE_STAGES = ("upload_us", "horizontal_us", "vertical_us", "download_us", "copy_us")


@pytest.fixture(scope="module")
def libs():
    from video_segment_amd import _lib, flow, render, resize
    for m in (_lib, flow, render, resize):
        m.build()
    assert _lib.lib().vsg_device_count() > 0
    return flow, render, resize


def noise(w, h, seed, channels=3):
    return np.random.default_rng(seed).integers(0, 256, (h, w, channels), dtype=np.uint8)


def raster_desc():
    """5 x 9: two regions, the second of two intervals; the last column and row 8 stay unpainted."""
    return make_desc(5, 9, {3: [(0, 0, 3), (1, 0, 1)], 7: [(1, 2, 3), (4, 1, 2)]})


def test_resize_times_the_stages_that_ran(libs):
    import torch
    _, _, resize = libs
    img = noise(96, 72, 1)
    d = resize.Downscaler(96, 72, mode=resize.DOWNSCALE_TO_MAX_SIZE, size=48)
    assert d.out_size == (48, 36)
    on_device = d.process_frame_device(torch.from_numpy(img).cuda()).cpu().numpy()   # device in, device out
    st = d.last_stats()
    assert st["upload_us"] == 0 and st["download_us"] == 0 and st["copy_us"] == 0, st
    assert st["horizontal_us"] > 0 and st["vertical_us"] > 0, st
    on_host = d.process_frame(img)                                                   # host in, host out
    st = d.last_stats()
    assert all(st[k] > 0 for k in RESIZE_STAGES[:4]) and st["copy_us"] == 0, st
    assert np.array_equal(on_host, on_device)
    d.process_frame(img)
    again = d.last_stats()
    assert again["device_allocations"] == st["device_allocations"] > 0
    assert (again["launches"], again["host_syncs"]) == (st["launches"], st["host_syncs"]) == (4, 1)
    d.close()


def test_resize_identity_reports_only_the_copy(libs):
    import torch
    _, _, resize = libs
    img = noise(96, 72, 2)
    d = resize.Downscaler(96, 72, mode=resize.DOWNSCALE_NONE)
    assert d.out_size == (96, 72)
    out = d.process_frame(torch.from_numpy(img).cuda())    # one device-to-host copy
    st = d.last_stats()
    assert np.array_equal(out, img)
    assert st["copy_us"] > 0 and all(st[k] == 0 for k in RESIZE_STAGES[:4]), st
    assert st["device_allocations"] == 0 and st["launches"] == 1
    d.close()


def test_flow_times_the_stages_that_ran(libs):
    flow, _, _ = libs
    d = flow.DenseFlow(33, 31)
    assert d.process_frame(noise(33, 31, 3)) is None
    first = d.last_stats()
    assert first["pyramid_us"] > 0, first
    assert first["warp_us"] == 0 and first["iterate_us"] == 0 and first["export_us"] == 0, first
    assert d.process_frame(noise(33, 31, 4)) is not None
    second = d.last_stats()
    assert all(second[k] > 0 for k in ("pyramid_us", "warp_us", "iterate_us", "export_us")), second
    assert second["device_allocations"] == first["device_allocations"] > 0
    assert first["host_syncs"] == second["host_syncs"] == 1
    d.close()


def test_render_then_id_image_on_one_handle(libs):
    _, render, _ = libs
    desc, frame = raster_desc(), noise(5, 9, 5)
    seg = desc.SerializeToString()
    model = render_model.RenderModel(5, 9)
    want, want_ids = model.render(desc, frame), model.id_image(desc, 0)
    r = render.SegmentationRenderer(5, 9)
    allocs = []
    for _ in range(2):
        assert np.array_equal(r.render(seg, frame), want)
        st = r.last_stats()
        assert st["clear_us"] >= 0 and st["fill_us"] >= 0 and st["compose_us"] >= 0, st
        assert np.array_equal(r.id_image(seg, 0), want_ids)
        st = r.last_stats()
        assert st["clear_us"] >= 0 and st["fill_us"] >= 0 and st["compose_us"] >= 0, st
        allocs.append(st["device_allocations"])
    assert allocs[1] == allocs[0] > 0, allocs
    r.close()


def test_a_handle_of_another_device_restores_the_callers(libs):
    import torch
    from video_segment_amd import _lib
    if _lib.lib().vsg_device_count() < 2:
        pytest.skip("one HIP device")
    flow, render, resize = libs
    img, frames = noise(96, 72, 6), [noise(33, 31, 7), noise(33, 31, 8)]
    desc, frame = raster_desc(), noise(5, 9, 9)
    seg = desc.SerializeToString()

    def run(device):
        torch.cuda.set_device(0)
        d = resize.Downscaler(96, 72, mode=resize.DOWNSCALE_TO_MAX_SIZE, size=48, device=device)
        f = flow.DenseFlow(33, 31, device=device)
        r = render.SegmentationRenderer(5, 9, device=device)
        assert torch.cuda.current_device() == 0
        f.process_frame(frames[0])
        got = d.process_frame(img), f.process_frame(frames[1]), r.render(seg, frame)
        assert torch.cuda.current_device() == 0
        for handle in (d, f, r):
            handle.close()
        assert torch.cuda.current_device() == 0
        return got

    for on_1, on_0 in zip(run(1), run(0)):
        assert np.array_equal(on_1, on_0)
