"""level_pool_model.py against a plain Python double loop in exact rational arithmetic and against closed forms.
Needs no device."""
import math

import numpy as np
import pytest

import level_colors_cases as kc
import level_colors_model as km
import level_components_model as cm
import level_pool_model as pm
import level_regions_cases as lc

SMALL = [c for c in kc.small() if c.case.W * c.case.H <= 700]


def features(W, H, C, seed, integers):
    rng = np.random.RandomState(seed)
    if integers:
        return rng.randint(-(1 << 15), (1 << 15) + 1, (C, H, W)).astype(np.float32)
    return rng.standard_normal((C, H, W)).astype(np.float32)


@pytest.mark.parametrize("c", SMALL, ids=lambda c: c.name)
@pytest.mark.parametrize("integers", [True, False])
def test_the_vectorised_form_equals_the_double_loop(c, integers):
    X = features(c.case.W, c.case.H, 3, 7, integers).astype(np.float64)
    for level in c.case.levels:
        ids = lc.id_image(c.case.msg, level)
        for connect in (0, cm.N4, cm.N8):
            if connect:
                comps, _, P = cm.sweep(ids, connect)
            else:
                comps, P = None, ids
            g, out = pm.pool(P, X, comps)
            g2, out2 = pm.pool_literal(P, X, comps)
            assert pm.same_bits(g, g2), (c.name, level, connect)
            for s in pm.STATS:
                assert pm.same_bits(out[s], out2[s]), (c.name, level, connect, s)


def test_groups_and_byte_sums_equal_the_colour_model():
    for c in SMALL:
        ids = lc.id_image(c.case.msg, 0)
        want = km.colors(ids, c.F)
        g, out = pm.pool(ids, c.F.transpose(2, 0, 1).astype(np.float64))
        assert np.array_equal(g["id"], want["id"]) and np.array_equal(g["area"], want["area"])
        assert (g["component"] == -1).all() and (g["reserved"] == 0).all()
        assert np.array_equal(out["sum"], want["sum"]) and np.array_equal(out["sum_sq"], want["sum_sq"])
        assert np.array_equal(out["min"], want["min"]) and np.array_equal(out["max"], want["max"])


def test_closed_forms():
    H, W = 5, 9
    P = np.zeros((H, W), np.int32)
    P[:, 5:] = 3
    P[0, 0] = -1
    yy, xx = np.mgrid[0:H, 0:W]
    X = np.stack([xx, yy, np.full((H, W), 0.5)]).astype(np.float64)
    g, out = pm.pool(P, X)
    assert g["id"].tolist() == [0, 3] and g["area"].tolist() == [24, 20]
    assert out["sum"].tolist() == [[5 * 10, 5 * 10, 12.0], [5 * (5 + 6 + 7 + 8), 4 * 10, 10.0]]
    assert out["sum_sq"][1].tolist() == [5 * (25 + 36 + 49 + 64), 4 * 30, 5.0]
    assert out["min"].tolist() == [[0, 0, 0.5], [5, 0, 0.5]] and out["max"].tolist() == [[4, 4, 0.5], [8, 4, 0.5]]
    mean, var = pm.moments(g, out["sum"], out["sum_sq"])
    assert mean[1].tolist() == [6.5, 2.0, 0.5] and var[1].tolist() == [1.25, 2.0, 0.0]


def test_the_sum_is_correctly_rounded_where_a_running_sum_is_not():
    P = np.zeros((1, 3), np.int32)
    X = np.array([[[1e30, 1.0, -1e30]]], np.float32).astype(np.float64)
    _, out = pm.pool(P, X)
    assert out["sum"][0, 0] == 1.0 and float(np.sum(X)) == 0.0


def test_nan_and_infinities():
    P = np.array([[0, 0, 1, 1, 2, 2]], np.int32)
    X = np.array([[[1, np.nan, np.inf, -np.inf, np.nan, np.nan]],
                  [[1, 2, 3, 4, 5, 6]]], np.float32).astype(np.float64)
    _, out = pm.pool(P, X)
    assert math.isnan(out["sum"][0, 0]) and math.isnan(out["sum_sq"][0, 0])
    assert out["min"][0, 0] == 1 and out["max"][0, 0] == 1
    assert math.isnan(out["sum"][1, 0]) and out["sum_sq"][1, 0] == np.inf
    assert out["min"][1, 0] == -np.inf and out["max"][1, 0] == np.inf
    assert math.isnan(out["sum"][2, 0]) and out["min"][2, 0] == np.inf and out["max"][2, 0] == -np.inf
    assert out["sum"][:, 1].tolist() == [3, 7, 11] and out["max"][:, 1].tolist() == [2, 4, 6]


def test_bfloat16_round_to_nearest_even():
    x = np.array([1.0, 1.00390625, 1.01171875, 1.0078125, -2.5, np.inf, 3.4028235e38], np.float32)
    # 1 + 2^-8 is a tie: to even (down); 1 + 3 * 2^-8 is a tie: to even (up); 1 + 2^-7 is representable
    assert pm.to_bf16(x).tolist() == [0x3f80, 0x3f80, 0x3f82, 0x3f81, 0xc020, 0x7f80, 0x7f80]
    assert np.isnan(pm.from_bf16(pm.to_bf16(np.array([np.nan], np.float32)))).all()
    bits = np.arange(0, 1 << 16, dtype=np.uint16)
    finite = np.isfinite(pm.from_bf16(bits))
    assert np.array_equal(pm.to_bf16(pm.from_bf16(bits))[finite], bits[finite])
    assert np.array_equal(pm.widen(bits[finite], pm.BF16), pm.from_bf16(bits[finite]).astype(np.float64))


def test_unpool():
    P = np.array([[4, 4, -1], [9, 4, 9]], np.int32)
    values = np.array([[1.5, -2.0], [0.1, 65520.0]], np.float32)
    out = pm.unpool(P, values, fill=7.0)
    assert out.dtype == np.float32 and out.shape == (2, 2, 3)
    assert out[0].tolist() == [[1.5, 1.5, 7.0], [np.float32(0.1), 1.5, np.float32(0.1)]]
    half = pm.unpool(P, values, fill=7.0, dtype=pm.F16)
    assert half.dtype == np.float16 and half[1, 1, 0] == np.inf and half[0, 1, 0] == np.float16(0.1)
    b = pm.unpool(P, values, fill=7.0, dtype=pm.BF16)
    assert b.dtype == np.uint16 and pm.from_bf16(b)[0, 0, 2] == 7.0
    assert np.array_equal(b, pm.to_bf16(out))
    # pooling the unpooled planes of integer values returns area * value
    ints = np.array([[3, -5], [70, 11]], np.float32)
    g, back = pm.pool(P, pm.unpool(P, ints).astype(np.float64))
    assert np.array_equal(back["sum"], g["area"][:, None] * ints.astype(np.float64))
