"""Exact comparison of the state the ordered merge computes -- per node: representative, f32 mean
colour, size, constraint id, flags -- between the HIP library and the CPU oracle
(vsg_graph_node_states / vsg_stream_last_node_states and their vso_ mirrors).

A state is the tuple (root, mean [n,3] f32, size, constraint, flags u8) the accessors return.
No tolerance anywhere: the workers of the merge are required to leave the words the sequential
replay leaves."""
import numpy as np

# The comparison runs on chunk graphs of at most this many nodes (100 MB of state on each side).
NODE_CAP = 4194304

FLAG_FINALIZED = 1
FLAG_NO_DESC = 2
# kFlagTentative, kFlagHubBroken, kFlagHubExcluded (device_graph.h) and the unused bits: marks of a
# merge stage, taken off again when the stage is through -- clear on every representative after
# a segment call (k_clear_tentative, k_hub_clear, ResetHubExclusions).
TRANSIENT_FLAGS = 0xFC


def canon_partition(labels):
    """Relabels by first occurrence so that two partitions can be compared exactly."""
    _, first, inv = np.unique(labels, return_index=True, return_inverse=True)
    order = np.argsort(np.argsort(first))
    return order[inv]


def words(mean):
    return np.ascontiguousarray(mean, np.float32).view(np.uint32)


def _describe(state, i):
    root, mean, size, cons, flags = state
    return "root %d size %d constraint %d flags 0x%02x mean %s (words %s)" % (
        root[i], size[i], cons[i], flags[i], mean[i].tolist(), ["0x%08x" % w for w in words(mean[i])])


def differing_nodes(got, want):
    """Boolean mask of the nodes whose state differs (partition, size, constraint, flags & 3, mean
    words where 'no descriptor' is clear on both sides)."""
    g_root, g_mean, g_size, g_cons, g_flags = got
    w_root, w_mean, w_size, w_cons, w_flags = want
    # the same partition: both roots are node ids, so node i's two representatives have to lie in
    # each other's region (two gathers; canon_partition sorts, which takes seconds on 4 M nodes)
    n = len(w_root)
    for r in (g_root, w_root):
        assert r.min(initial=0) >= 0 and r.max(initial=0) < max(n, 1), "a representative is no node id"
    bad = (w_root[g_root] != w_root) | (g_root[w_root] != g_root)
    bad |= g_size != w_size
    bad |= g_cons != w_cons
    bad |= (g_flags & 3) != (w_flags & 3)
    with_desc = ((g_flags | w_flags) & FLAG_NO_DESC) == 0
    bad |= with_desc & (words(g_mean) != words(w_mean)).any(axis=1)
    return bad


def assert_states_equal(got, want, what, W=None, H=None, transient_clear=True):
    """got: the library's state, want: the oracle's.  transient_clear: also require the stage marks
    to be clear in `got` (the oracle has none)."""
    n = len(want[0])
    assert len(got[0]) == n, "%s: %d nodes against %d" % (what, len(got[0]), n)
    for a, b in zip(got, want):
        assert a.shape == b.shape and a.dtype == b.dtype, what
    bad = differing_nodes(got, want)
    if transient_clear:
        bad |= (got[4] & TRANSIENT_FLAGS) != 0
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        if W and H:
            where = "(slice %d, y %d, x %d)" % (i // (W * H), (i % (W * H)) // W, i % W)
        else:
            where = "node %d" % i
        raise AssertionError("%s: the state of %d of %d nodes differs; first at %s\n  library: %s\n  oracle:  %s" % (
            what, int(bad.sum()), n, where, _describe(got, i), _describe(want, i)))


def compare_stream_chunk(gs, os_, what):
    """After a call that segmented a chunk in both streams (keeping on in both): compares the chunk
    graph's states, unless the graph is above the node cap.  Returns whether it compared."""
    want = os_.last_node_states()
    n = len(want[0])
    if n > NODE_CAP:
        print("node states: %s skipped, %d nodes are above the cap of %d" % (what, n, NODE_CAP))
        return False
    assert_states_equal(gs.last_node_states(), want, what, gs.W, gs.H)
    return True


def region_table(state):
    """One row per region (by representative): used by the mutant test to count changed regions."""
    root = state[0]
    reps, first = np.unique(root, return_index=True)
    return reps, first
