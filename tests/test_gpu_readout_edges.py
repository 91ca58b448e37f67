"""The read-out kernels (readout_kernels.hip) against the CPU oracle on regions that hang together
by diagonals only -- what the N4 pass rewrites -- at the widths where its kernels change path: the
64-lane steps of the run kernels, the 256 and 1024 column strides of the N4 kernels, a row whose
fixed point takes a thousand trips, H = 1, the unhashed pair list, all four combinations of the
read-out flags, and both sides of the widest accepted frame."""
import numpy as np
import pytest

import edge_shape_cases as ec
import node_states as ns
import oracle_lib as ol
import synth
from test_gpu_parity import assert_region_lists_equal

pytestmark = pytest.mark.gpu

MAX_WIDTH = 10224     # include/vsg.h


@pytest.fixture(scope="module")
def vsg():
    import video_segment_amd as v
    from video_segment_amd import _lib
    _lib.build()
    assert _lib.lib().vsg_device_count() > 0, "GPU tests need a HIP device"
    return v


def assert_readout_equal(gg, og, F):
    assert gg.num_regions() == og.num_regions()
    for t in range(F):
        assert np.array_equal(gg.index_image(t), og.index_image(t)), t
    gs, gc = gg.region_sizes()
    os_, oc = og.region_sizes()
    assert np.array_equal(gs, os_) and np.array_equal(gc, oc)
    assert gg.num_neighbor_links() == og.num_neighbor_links()
    assert_region_lists_equal(gg, og, F)


def gpu_readout(vsg, case, use_flows=False, enforce_n4=True, enforce_connected=True):
    _, W, H, F, min_size = case
    gg = vsg.DenseSegGraph(W, H, F)
    ec.build_graph(gg, case, use_flows)
    gg.segment(min_size, False)
    gg.obtain_results(use_flows=use_flows, enforce_n4=enforce_n4,
                      enforce_spatial_connectedness=enforce_connected)
    return gg


@pytest.mark.parametrize("case", ec.READOUT_CASES, ids=ec.readout_id)
def test_readout_matches_oracle(vsg, case):
    gg = gpu_readout(vsg, case)
    assert_readout_equal(gg, ec.oracle_readout(case), case[3])
    gg.close()


@pytest.mark.parametrize("enforce_connected", [True, False], ids=["conn", "noconn"])
@pytest.mark.parametrize("enforce_n4", [True, False], ids=["n4", "non4"])
@pytest.mark.parametrize("case", ec.FLAG_CASES, ids=ec.readout_id)
def test_readout_flags(vsg, case, enforce_n4, enforce_connected):
    gg = gpu_readout(vsg, case, False, enforce_n4, enforce_connected)
    assert_readout_equal(gg, ec.oracle_readout(case, False, enforce_n4, enforce_connected), case[3])
    gg.close()


@pytest.mark.parametrize("case", ec.FLOW_CASES, ids=ec.readout_id)
def test_readout_with_flows(vsg, case):
    gg = gpu_readout(vsg, case, use_flows=True)
    assert_readout_equal(gg, ec.oracle_readout(case, True), case[3])
    gg.close()


@pytest.mark.parametrize("case", ec.UNHASHED_CASES, ids=ec.readout_id)
def test_unhashed_pair_list(vsg, monkeypatch, case):
    """VSG_PAIR_TABLE=0 (read at the call): every pair of every kept edge is listed, sorted and made
    unique, as when a chunk has more distinct pairs than the hash table takes."""
    F = case[3]
    monkeypatch.delenv("VSG_PAIR_TABLE", raising=False)
    hashed = gpu_readout(vsg, case)
    monkeypatch.setenv("VSG_PAIR_TABLE", "0")
    listed = gpu_readout(vsg, case)
    for a, b in zip(hashed.get_regions(), listed.get_regions()):
        assert np.array_equal(a, b)
    assert hashed.num_neighbor_links() == listed.num_neighbor_links()
    for t in range(F):
        assert np.array_equal(hashed.get_intervals(t), listed.get_intervals(t))
    assert_readout_equal(listed, ec.oracle_readout(case), F)
    hashed.close()
    listed.close()


def test_readout_constrained_chunk(vsg):
    """A second-chunk graph (virtual slice, constrained slice, virtual temporal edges) at 65 x 9 with
    checker frames: constrained slices are swept, the virtual slice is skipped."""
    W, H, real = 65, 9, 3
    x, y = np.arange(W)[None, :], np.arange(H)[:, None]
    labels_v = ((y // 5) * 5 + x // 16).astype(np.int32)
    labels_c = np.roll(labels_v, 2, axis=1).astype(np.int32)
    gg = vsg.DenseSegGraph(W, H, real + 1)
    og = ol.OracleGraph(W, H, real + 1)
    gg.add_virtual_frame(labels_v)
    og.add_virtual_frame(labels_v)
    fl = synth.const_flow(W, H)
    prev = None
    for t in range(real):
        feat = ec.features("checker", W, H, t)
        gg.add_frame_features(feat, constraint_ids=labels_c if t == 0 else None)
        og.add_frame(feat, labels_c if t == 0 else None)
        gg.add_temporal(fl, is_virtual=(t == 0))
        og.add_temporal(feat if t else None, prev, fl, is_virtual=(t == 0))
        prev = feat
    gg.segment(4, True)
    og.segment(4, True)
    assert np.array_equal(gg.merge_stats(), og.merge_stats())
    ns.assert_states_equal(gg.node_states(), og.node_states(), "constrained 65x9 chunk", W, H)
    gg.obtain_results(use_flows=True)
    og.obtain_results([None] + [fl] * real)
    assert_region_lists_equal(gg, og, real + 1)
    assert gg.num_regions() == og.num_regions()
    for t in range(1, real + 1):
        assert np.array_equal(gg.index_image(t), og.index_image(t)), t
    regs, _, _ = gg.get_regions()
    assert (regs[:, 2] >= 0).any()
    assert len(gg.get_intervals(0)) == 0
    gg.close()


@pytest.mark.parametrize("W", [ec.WIDE_CASE[1], MAX_WIDTH])
def test_rows_past_64k_of_lds(vsg, W):
    """k_enforce_n4 holds 16 W bytes of a row in LDS: 4100 px is just past the 64 KiB a kernel gets
    unasked, 10224 px the widest accepted frame (160 KiB).  diag3 makes the row's fixed point a chain
    of about W trips."""
    case = ("diag3", W) + ec.WIDE_CASE[2:]
    assert 16 * W > 64 * 1024
    gg = gpu_readout(vsg, case)
    assert_readout_equal(gg, ec.oracle_readout(case), case[3])
    gg.close()


def test_wider_frame_is_rejected_at_creation(vsg):
    from video_segment_amd import _lib
    before = _lib.memory_stats()
    with pytest.raises(_lib.VsgError) as e:
        vsg.DenseSegGraph(MAX_WIDTH + 1, 3, 1)
    assert e.value.code == _lib.VSG_ERR_INVALID and str(MAX_WIDTH) in str(e.value)
    with pytest.raises(_lib.VsgError) as e:
        vsg.DenseSegmentation(MAX_WIDTH + 1, 3)
    assert e.value.code == _lib.VSG_ERR_INVALID and str(MAX_WIDTH) in str(e.value)
    after = _lib.memory_stats()
    for k in ("bytes_in_use", "runtime_mallocs", "cache_hits"):   # nothing was allocated, let alone launched
        assert after[k] == before[k], k
