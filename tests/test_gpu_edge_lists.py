"""The edge lists edge_sort.hip builds (vsg_graph_list_slots: sorted slots and bucket offsets as the
device holds them) against the lists derived from the oracle's bucket planes (edge_list_cases.py),
word for word.  Every case is built twice: a frame and its temporal list through the separate calls
(add_frame_features, add_temporal) and through the combined entry that a stream uses for every frame
after a chunk's first (add_frame_features(..., temporal=True): one chain, one scan over both
histogram matrices, one scatter grid over the tiles of both lists)."""
import numpy as np
import pytest

import edge_list_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vsg():
    import video_segment_amd as v
    from video_segment_amd import _lib
    _lib.build()
    assert _lib.lib().vsg_device_count() > 0, "GPU tests need a HIP device"
    return v


def _build(vsg, case, combined):
    _, W, H, l1, _ = case
    frames, temporal = lc.inputs(case)
    g = vsg.DenseSegGraph(W, H, len(frames), l1=l1)
    try:
        for t, f in enumerate(frames):
            if t == 0:
                g.add_frame_features(f)
                continue
            flow, is_virtual = temporal[t - 1]
            if combined:
                g.add_frame_features(f, temporal=True, flow=flow, is_virtual=is_virtual)
            else:
                g.add_frame_features(f)
                g.add_temporal(flow, is_virtual=is_virtual)
        return {index: g.list_slots(index) for index in range(2 * len(frames) - 1)}
    finally:
        g.close()


def _first_difference(got, want):
    n = min(got.size, want.size)
    d = np.nonzero(got[:n] != want[:n])[0]
    return "sizes %d / %d, first difference at %s" % (got.size, want.size, int(d[0]) if d.size else None)


@pytest.mark.parametrize("combined", [False, True], ids=["separate", "combined"])
@pytest.mark.parametrize("case", lc.CASES, ids=lc.case_id)
def test_lists_equal_the_model(vsg, case, combined):
    want = lc.expected_lists(case)
    got = _build(vsg, case, combined)
    assert set(got) == set(want)
    for index in sorted(want):
        slots, offsets = got[index]
        assert np.array_equal(offsets, want[index][1]), "list %d offsets: %s" % (
            index, _first_difference(offsets, want[index][1]))
        assert np.array_equal(slots, want[index][0]), "list %d slots: %s" % (
            index, _first_difference(slots, want[index][0]))


def test_prev_idx_of_the_combined_entry(vsg):
    """The combined entry fills prev_idx like add_temporal does (the merge reads it with the list)."""
    import edge_shape_cases as ec
    W, H = 5, 205
    f0, f1, flow, _ = ec.key_inputs(W, H)
    want_pidx = ec.oracle_keys(W, H, False, True)[3]
    g = vsg.DenseSegGraph(W, H, 2)
    g.add_frame_features(f0)
    g.add_frame_features(f1, temporal=True, flow=flow)
    tb, pidx = g.temporal_buckets(1)
    g.close()
    assert np.array_equal(pidx, want_pidx)
    assert np.array_equal(tb, ec.oracle_keys(W, H, False, True)[2])


def test_list_slots_rejects_a_list_that_is_not_there(vsg):
    from video_segment_amd._lib import VsgError
    g = vsg.DenseSegGraph(4, 4, 2)
    g.add_frame_features(np.zeros((4, 4, 3), np.float32))
    with pytest.raises(VsgError):
        g.list_slots(1)
    with pytest.raises(VsgError):
        g.list_slots(7)
    g.close()
