"""The graph-build kernels (build_kernels.hip, edge_sort.hip) against the CPU oracle at the sizes
where they change path: frames smaller than the bilateral window, tiles that end 1 px into the
frame, more tiles than the persistent grid has workgroups, rows whose first and last bytes are the
only extremes next to padding that is more extreme, pixel counts on and one past a key tile, flow
that leaves the frame by less than a pixel.  Every comparison is of integers or f32 words."""
import numpy as np
import pytest

import edge_shape_cases as ec
import node_states as ns
from test_gpu_parity import bits, canon_partition

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vsg():
    import video_segment_amd as v
    from video_segment_amd import _lib
    _lib.build()
    assert _lib.lib().vsg_device_count() > 0, "GPU tests need a HIP device"
    return v


@pytest.mark.parametrize("case", ec.BILATERAL_CASES, ids=ec.bilateral_id)
def test_smoothed_bit_exact(vsg, case):
    """k_minmax_u8 + k_bilateral / k_gaussian3 / k_convert_planar on padded rows."""
    W, H, kind, pad, presmoothing = case
    view, _ = ec.padded_frame(W, H, kind, pad)
    g = vsg.DenseSegGraph(W, H, 1)
    g.add_frame_bgr(view, presmoothing=presmoothing)
    got = g.smoothed(0)
    g.close()
    want = ec.oracle_smoothed(*case)
    diff = bits(got) != bits(want)
    assert not diff.any(), "%d of %d words differ, first at (y, x, c) = %s" % (
        int(diff.sum()), diff.size, tuple(np.argwhere(diff)[0]))


@pytest.mark.parametrize("with_flow", [False, True], ids=["noflow", "flow"])
@pytest.mark.parametrize("l1", [False, True], ids=["l2", "l1"])
@pytest.mark.parametrize("W,H", ec.KEY_SIZES)
def test_edge_keys_bit_exact(vsg, W, H, l1, with_flow):
    """k_spatial_keys and k_temporal_keys (+ prev_idx) on and one past a tile, H = 1, W = 2, and flow
    that leaves the frame on every side (by half a pixel, by infinity, as NaN)."""
    f0, f1, flow, _ = ec.key_inputs(W, H)
    want_s0, want_s1, want_tb, want_pidx = ec.oracle_keys(W, H, l1, with_flow)
    g = vsg.DenseSegGraph(W, H, 2, l1=l1)
    g.add_frame_features(f0)
    g.add_frame_features(f1)
    g.add_temporal(flow if with_flow else None)
    assert np.array_equal(g.spatial_buckets(0), want_s0)
    assert np.array_equal(g.spatial_buckets(1), want_s1)
    tb, pidx = g.temporal_buckets(1)
    g.close()
    assert np.array_equal(pidx, want_pidx)
    assert np.array_equal(tb, want_tb)


@pytest.mark.parametrize("min_size", [0, 3])
@pytest.mark.parametrize("W,H", ec.TILE_EDGE_SIZES)
def test_slot_order_through_the_merge(vsg, W, H, min_size):
    """k_scatter_slots<4> and <9>: the order of the slots inside a bucket is only visible in what the
    ordered merge makes of it."""
    f0, f1, flow, _ = ec.key_inputs(W, H)
    want_stats, want_roots = ec.oracle_merge(W, H, min_size)
    g = vsg.DenseSegGraph(W, H, 2)
    g.add_frame_features(f0)
    g.add_frame_features(f1)
    g.add_temporal(flow)
    g.segment(min_size, False)
    stats, roots, states = g.merge_stats(), g.node_roots(), g.node_states()
    g.close()
    assert np.array_equal(stats, want_stats)
    assert np.array_equal(canon_partition(roots), canon_partition(want_roots))
    ns.assert_states_equal(states, ec.oracle_merge_states(W, H, min_size), "%dx%d min %d" % (W, H, min_size), W, H)
