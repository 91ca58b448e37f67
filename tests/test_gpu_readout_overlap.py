"""The chunk boundary beside the merge: the run-length intervals of all slices in one launch, the halo
planes rendered inside the encode pool.

Every case streams against the CPU oracle byte for byte (test_gpu_parity.run_streams: result counts,
SegmentationDesc bytes, merge statistics, node states); the halo case also asserts, from the library's own
host counter (vsg_stream_last_boundary_paths), that the pool rendered the planes.
"""
import pytest

import synth
from test_gpu_parity import run_streams, vsg  # noqa: F401  (vsg: the module fixture)

pytestmark = pytest.mark.gpu


def stream_paths(vsg, W, H, N, kind, flow, chunk, **options):  # noqa: F811
    """run_streams, returning the boundary paths of every segmented chunk in order."""
    seen = []
    frames = [synth.FRAME_FNS[kind](W, H, k) for k in range(N)] if kind in synth.FRAME_FNS else None
    run_streams(vsg, W, H, N, kind, flow, chunk, frames=frames,
                on_chunk=lambda s: seen.append(s.last_boundary_paths()), **options)
    return seen


# ---- run-length intervals of all slices in one launch ----------------------------------------------

@pytest.mark.parametrize("W,H", [(2, 5), (63, 3), (64, 3), (65, 3), (4100, 3)])
def test_intervals_of_all_slices_at_row_widths(vsg, W, H):  # noqa: F811
    """One wavefront per row walks it 64 pixels at a time: a row shorter than, equal to, one longer
    than a step, and one of many steps; 2 is the narrowest frame the library accepts (see below).
    Three chunks: from the second on the first slice is virtual and the slice list skips it (9 slices,
    8 of them rasterised); the last one is flushed (all of its 9 buffered slices but the virtual one)."""
    seen = stream_paths(vsg, W, H, 22, "noise", True, 8)
    assert len(seen) == 3


def test_width_one_is_refused(vsg):  # noqa: F811
    """vsg_stream_create: width in [2, 10224].  A one pixel wide frame never reaches the read-out."""
    from video_segment_amd._lib import VsgError
    with pytest.raises(VsgError) as e:
        vsg.DenseSegmentation(1, 5, vsg.default_options(chunk_size=4), has_flow=True)
    assert e.value.code == -1


# ---- halo planes -----------------------------------------------------------------------------------

def test_halo_planes_rendered_in_the_pool(vsg):  # noqa: F811
    """Both overlap frames' id planes are rendered by the encode pool at a constrained boundary, none at
    a flush; the next chunk's constraints are those planes, so three chunks equal to the oracle's prove
    them right."""
    seen = stream_paths(vsg, 161, 97, 22, "bench", True, 8)   # 8 + 7 + 7 frames, the last call flushes
    assert [p["halo_planes_in_pool"] for p in seen] == [2, 2, 0], seen
