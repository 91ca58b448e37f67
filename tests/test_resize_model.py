"""The downscale model (tests/resize_model.py) on its own: the reference's size rule against the
values worked out from its text in numpy f32, and the sanity of the resampling definition."""
import numpy as np
import pytest

import resize_model as rm
from resize_cases import FILTER_CASES, SIZE_TABLE


@pytest.mark.parametrize("in_w,in_h,mode,size,out_w,out_h", SIZE_TABLE)
def test_output_size_table(in_w, in_h, mode, size, out_w, out_h):
    w, h, step = rm.output_size(mode, in_w, in_h, size=size)
    assert (w, h) == (out_w, out_h)
    assert step % 4 == 0 and 0 <= step - 3 * w < 4


def test_output_size_by_factor_and_none():
    assert rm.output_size(rm.BY_FACTOR, 97, 61, factor=0.5)[:2] == (50, 31)
    assert rm.output_size(rm.NONE, 96, 72) == (96, 72, 288)
    assert rm.output_size(rm.NONE, 97, 61) == (98, 61, 296)


@pytest.mark.parametrize("kw", [
    dict(mode=rm.BY_FACTOR, factor=1.5), dict(mode=rm.TO_MIN_SIZE, size=0), dict(mode=rm.TO_MAX_SIZE, size=-3),
    dict(mode=rm.BY_FACTOR, factor=0.0), dict(mode=rm.BY_FACTOR, factor=-0.5), dict(mode=7),
])
def test_output_size_rejects(kw):
    with pytest.raises(ValueError):
        rm.output_size(kw.pop("mode"), 97, 61, **kw)


def test_tap_counts():
    """A window of 2 R = 4 max(1, r) source pixels holds floor(2 R) or floor(2 R) + 1 of them."""
    cases = [(3840, 640), (70, 26), (97, 78), (61, 48), (97, 98), (768, 64), (4096, 16)]
    taps = {c: int(rm.filter_tables(*c)[1].max()) for c in cases}
    assert taps == {(3840, 640): 24, (70, 26): 11, (97, 78): 5, (61, 48): 6, (97, 98): 4, (768, 64): 48,
                    (4096, 16): 1024}


@pytest.mark.parametrize("n_in,n_out", FILTER_CASES)
def test_weights_sum_to_one(n_in, n_out):
    first, count, weights = rm.filter_tables(n_in, n_out)
    assert weights.dtype == np.float32 and first.dtype == np.int32 and count.dtype == np.int32
    assert (count >= 1).all() and (np.diff(first) >= 0).all()
    for o in range(n_out):
        assert not weights[o, count[o]:].any()
        # f32 rounding of at most 48 normalised taps: 48 * 2^-25 relative, weights below 1.2 in size
        assert abs(float(weights[o].astype(np.float64).sum()) - 1.0) < 2.0 ** -22
        # the taps cover the centre
        c = (o + 0.5) * n_in / n_out - 0.5
        assert first[o] <= c <= first[o] + count[o] - 1


@pytest.mark.parametrize("value", [0, 1, 128, 255])
def test_constant_stays_constant(value):
    img = np.full((61, 97, 3), value, np.uint8)
    for w, h in [(78, 48), (98, 61), (26, 17)]:
        assert (rm.resize(img, w, h) == value).all()


def test_step_edge_saturates():
    img = np.zeros((20, 64, 3), np.uint8)
    img[:, 32:] = 255
    raw = rm.resize_f32(img, 24, 10)
    assert raw.min() < 0.0 and raw.max() > 255.0
    out = rm.resize(img, 24, 10)
    assert out.min() == 0 and out.max() == 255
    assert (out[raw < 0] == 0).all() and (out[raw > 255] == 255).all()


def test_identity_returns_input():
    img = np.random.default_rng(5).integers(0, 256, (72, 96, 3), dtype=np.uint8)
    out = rm.resize(img, 96, 72)
    assert out is not img and (out == img).all()
    assert (rm.downscale(img, rm.BY_FACTOR, factor=1.0) == img).all()


def test_identity_axis_reproduces_values():
    """97 x 61 -> 98 x 61: the vertical filter still runs and its taps of weight 1 and 0 change nothing."""
    img = np.random.default_rng(6).integers(0, 256, (61, 97, 3), dtype=np.uint8)
    h_only = rm.filter_axis0(np.ascontiguousarray(img.astype(np.float32).transpose(1, 0, 2)), 98).transpose(1, 0, 2)
    assert (rm.resize_f32(img, 98, 61) == h_only).all()


def test_mean_is_kept():
    img = np.random.default_rng(7).integers(0, 256, (61, 97, 3), dtype=np.uint8)
    out = rm.downscale(img, rm.TO_MIN_SIZE, size=48)
    assert out.shape == (48, 78, 3)
    assert abs(float(out.mean()) - float(img.mean())) < 0.5
