"""The definition of what libvsg_resize.so (include/vsg_resize.h) computes.

Two parts:

* ``output_size``: the size rule of the reference's reader (video_reader_unit.cpp:155-206), in f32
  where the reference is in f32.  This part is pinned by the reference's text.
* ``filter_tables`` / ``resize``: a separable Keys bicubic (a = -0.6, the default of swscale's
  SWS_BICUBIC) whose support widens with the downscale ratio.  The reference calls swscale on a
  decoded YUV frame; neither swscale nor a codec is part of the reference tree, so this arithmetic
  is NOT pinned by it ("parity unpinned").  The library equals this model byte for byte.

Per axis, n_in -> n_out, in f64: r = n_in / n_out, s = max(1, r), R = 2 s.  Output o has its
centre at c = (o + 0.5) r - 0.5 and the taps i = ceil(c - R) .. floor(c + R) with weight
k(|i - c| / s); the weights are summed in tap order, divided by that sum and rounded to f32.  A tap
outside [0, n_in - 1] reads the clamped index but stays a tap of its own.  A frame is filtered
horizontally into f32 (not rounded to 8 bits), then vertically; each pass is
``acc = 0; for taps in order: acc = acc + w * v`` with every operation a correctly rounded f32
operation (no fused multiply-add).  The result is rint (half to even), saturated to [0, 255].  A
frame whose size does not change on either axis is copied.
"""
import math

import numpy as np

NONE, BY_FACTOR, TO_MIN_SIZE, TO_MAX_SIZE = 0, 1, 2, 3
A = -0.6


def output_size(mode, in_w, in_h, size=0, factor=1.0):
    """(out_w, out_h, width_step) of OpenStreams' rule; ValueError where the library refuses."""
    f32 = np.float32
    if not (1 <= in_w <= 65535 and 1 <= in_h <= 65535):
        raise ValueError("bad frame size")
    if mode == NONE:
        fac = f32(1.0)
    elif mode == BY_FACTOR:
        fac = f32(factor)
        if fac > f32(1.0):
            raise ValueError("Only downscaling is supported")
    elif mode in (TO_MIN_SIZE, TO_MAX_SIZE):
        if size <= 0:
            raise ValueError("size has to be positive")
        a = f32(size) * (f32(1.0) / f32(in_w))
        b = f32(size) * (f32(1.0) / f32(in_h))
        fac = max(a, b) if mode == TO_MIN_SIZE else min(a, b)
        fac = min(f32(1.0), fac)
    else:
        raise ValueError("unknown mode")
    if not fac > 0:
        raise ValueError("the output would be empty")
    out_w = int(np.ceil(f32(in_w) * fac))
    out_h = int(np.ceil(f32(in_h) * fac))
    out_w += out_w % 2
    if out_w < 1 or out_h < 1:
        raise ValueError("the output would be empty")
    step = out_w * 3
    if step % 4:
        step += 4 - step % 4
    return out_w, out_h, step


def keys(t):
    """The Keys cubic at a = -0.6 for t >= 0 (f64)."""
    if t <= 1.0:
        return ((A + 2.0) * t - (A + 3.0)) * t * t + 1.0
    if t < 2.0:
        return ((A * t - 5.0 * A) * t + 8.0 * A) * t - 4.0 * A
    return 0.0


_tables = {}


def filter_tables(n_in, n_out):
    """(first int32[n_out], count int32[n_out], weights f32[n_out, max_taps]) of one axis.  first
    may be negative and first + count may pass n_in: tap j reads clamp(first + j, 0, n_in - 1).
    Rows are zero beyond their count."""
    key = (n_in, n_out)
    if key in _tables:
        return _tables[key]
    r = n_in / n_out
    s = max(1.0, r)
    R = 2.0 * s
    first = np.zeros(n_out, np.int32)
    count = np.zeros(n_out, np.int32)
    rows = []
    for o in range(n_out):
        c = (o + 0.5) * r - 0.5
        lo, hi = math.ceil(c - R), math.floor(c + R)
        w = [keys(abs((i - c) / s)) for i in range(lo, hi + 1)]
        total = 0.0
        for v in w:          # in tap order: numpy's sum is pairwise
            total = total + v
        rows.append(np.array([v / total for v in w], np.float64).astype(np.float32))
        first[o], count[o] = lo, hi - lo + 1
    weights = np.zeros((n_out, int(count.max())), np.float32)
    for o, row in enumerate(rows):
        weights[o, :len(row)] = row
    _tables[key] = (first, count, weights)
    return _tables[key]


def filter_axis0(x, n_out):
    """Filters axis 0 of an f32 array (n_in, ...) to (n_out, ...), unrounded f32."""
    n_in = x.shape[0]
    first, count, weights = filter_tables(n_in, n_out)
    out = np.zeros((n_out,) + x.shape[1:], np.float32)
    for o in range(n_out):
        acc = np.zeros(x.shape[1:], np.float32)
        for j in range(int(count[o])):
            i = min(max(int(first[o]) + j, 0), n_in - 1)
            acc = acc + weights[o, j] * x[i]     # two f32 operations, each rounded on its own
        out[o] = acc
    return out


def resize_f32(img, out_w, out_h):
    """The unsaturated, unrounded f32 result (out_h, out_w, 3) of both passes."""
    x = np.ascontiguousarray(img, np.uint8).astype(np.float32)
    h = filter_axis0(np.ascontiguousarray(x.transpose(1, 0, 2)), out_w).transpose(1, 0, 2)
    return filter_axis0(np.ascontiguousarray(h), out_h)


def resize(img, out_w, out_h):
    """H x W x 3 uint8 -> out_h x out_w x 3 uint8."""
    in_h, in_w = img.shape[:2]
    if (out_w, out_h) == (in_w, in_h):
        return np.array(img, np.uint8)
    return np.clip(np.rint(resize_f32(img, out_w, out_h)), 0, 255).astype(np.uint8)


def downscale(img, mode, size=0, factor=1.0):
    in_h, in_w = img.shape[:2]
    out_w, out_h, _ = output_size(mode, in_w, in_h, size, factor)
    return resize(img, out_w, out_h)
