"""numpy f32 model of the dense flow unit (include/vsg_flow.h): the DEFINITION of what libvsg_flow
computes.  The library has to equal it bit for bit.

The reference's DenseFlowUnit (video_framework/flow_reader.cpp:226-371) feeds 8-bit luminance frames
(LuminanceUnit, conversion_units.cpp:75-105) to OpenCV's OpticalFlowDual_TVL1 with warps = 2 and
iterations = 10 (flow_reader.h:143-144, flow_reader.cpp:246-250) and everything else at OpenCV's
defaults; backward flow is calc(current, previous) (flow_reader.cpp:291-294), the first frame has
none (flow_reader.cpp:283-288).  OpenCV is not part of the reference tree, so the arithmetic below
is written from the published algorithm -- C. Zach, T. Pock, H. Bischof, "A Duality Based Approach
for Realtime TV-L1 Optical Flow", DAGM 2007, as laid out in J. Sanchez, E. Meinhardt-Llopis,
G. Facciolo, "TV-L1 Optical Flow Estimation", IPOL 2013 -- in the structure of OpenCV 2.4's
OpticalFlowDual_TVL1 (calc / procOneScale / estimateV / divergence / estimateU / forwardGradient /
estimateDualVariables).

Every operation is one correctly rounded IEEE f32 operation in the order written here; there are no
fused multiply-adds.  The only f64 value is the per-iteration error sum and its threshold.

Choices that are OURS and not verifiable against OpenCV:
  * the association order of every sum (pyrDown taps, bicubic taps, divergence, rho);
  * bicubic sampling uses the exact f32 fraction of x + u (OpenCV's remap quantises it to 1/32 and
    takes weights from a table); weights are the a = -0.75 cubic in Horner form, the fourth as
    1 - w0 - w1 - w2; four row sums are combined vertically; taps outside the image contribute 0;
  * the bilinear upsampling computes its pixel-centre coordinate (d + 0.5) * (src / dst) - 0.5 in
    f32 (OpenCV: in f64, then cast) and clamps the two taps of an axis instead of zeroing the
    fraction; horizontal interpolation first, a * (1 - t) + b * t;
  * |grad u| is sqrt(ux * ux + uy * uy) in f32 (OpenCV: a double hypot, cast);
  * l_t = lambda * theta and taut = tau / theta are f32 operations on the f32 parameters;
  * the stop threshold is the f64 product 0.01 * 0.01 * (W_s * H_s); the error of one iteration is
    the f64 sum of the f32 per-pixel terms (its summation order is free: test_flow_model.py shows
    that no decision of the tested inputs is within 1e-6 relative of its threshold);
  * the pyramid level that OpenCV computes and then discards (the first with a side below 16) is
    not computed.
"""
import numpy as np

F = np.float32
TAU, LAMBDA, THETA, NSCALES, EPSILON = F(0.25), F(0.15), F(0.3), 5, 0.01
FLT_EPSILON = F(1.1920929e-07)


def luminance(bgr):
    """cvtColor(BGR2GRAY), 8 bit: (1868 B + 9617 G + 4899 R + 8192) >> 14."""
    b = bgr[..., 0].astype(np.int32)
    g = bgr[..., 1].astype(np.int32)
    r = bgr[..., 2].astype(np.int32)
    return ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(np.uint8)


def pyramid_sizes(W, H):
    """[(W_s, H_s)] from the finest level on; stops before the first level with a side below 16."""
    sizes = [(W, H)]
    while len(sizes) < NSCALES:
        w, h = (sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2
        if w < 16 or h < 16:
            break
        sizes.append((w, h))
    return sizes


def _reflect101(i, n):
    i = np.abs(i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def pyr_down(src):
    """Separable [1 4 6 4 1], reflect-101, ((W + 1) / 2, (H + 1) / 2), scale 1 / 256."""
    H, W = src.shape
    xs = 2 * np.arange((W + 1) // 2)
    c = [src[:, _reflect101(xs + k, W)] for k in (-2, -1, 0, 1, 2)]
    row = c[2] * F(6) + (c[1] + c[3]) * F(4) + c[0] + c[4]
    ys = 2 * np.arange((H + 1) // 2)
    r = [row[_reflect101(ys + k, H), :] for k in (-2, -1, 0, 1, 2)]
    return ((r[2] * F(6) + (r[1] + r[3]) * F(4) + r[0] + r[4]) * F(1.0 / 256.0)).astype(F)


def pyramid(lum_u8):
    levels = [lum_u8.astype(F)]
    for _ in pyramid_sizes(lum_u8.shape[1], lum_u8.shape[0])[1:]:
        levels.append(pyr_down(levels[-1]))
    return levels


def centered_gradient(I):
    H, W = I.shape
    xp, xm = np.minimum(np.arange(W) + 1, W - 1), np.maximum(np.arange(W) - 1, 0)
    yp, ym = np.minimum(np.arange(H) + 1, H - 1), np.maximum(np.arange(H) - 1, 0)
    return F(0.5) * (I[:, xp] - I[:, xm]), F(0.5) * (I[yp, :] - I[ym, :])


def _cubic_weights(t):
    A = F(-0.75)
    t1 = t + F(1)
    w0 = ((A * t1 + F(3.75)) * t1 - F(6)) * t1 + F(3)
    w1 = ((F(1.25) * t - F(2.25)) * t) * t + F(1)
    s = F(1) - t
    w2 = ((F(1.25) * s - F(2.25)) * s) * s + F(1)
    w3 = ((F(1) - w0) - w1) - w2
    return w0, w1, w2, w3


def warp3(planes, u1, u2, counters=None):
    """Bicubic samples of each plane at (x + u1, y + u2); the planes share addresses and weights.
    counters, if given, receives "outside_taps" (taps of the 4 x 4 footprints that fell outside the
    plane) and "clamped" (pixels whose gather index the [-4, W + 4] / [-4, H + 4] clamp changed)."""
    H, W = u1.shape
    fx = np.arange(W, dtype=F)[None, :] + u1
    fy = np.arange(H, dtype=F)[:, None] + u2
    fxf, fyf = np.floor(fx), np.floor(fy)
    wx, wy = _cubic_weights(fx - fxf), _cubic_weights(fy - fyf)
    ix = np.minimum(np.maximum(fxf, F(-4)), F(W + 4)).astype(np.int64)
    iy = np.minimum(np.maximum(fyf, F(-4)), F(H + 4)).astype(np.int64)
    if counters is not None:
        xs, ys = ix[..., None] + np.arange(-1, 3), iy[..., None] + np.arange(-1, 3)
        xin, yin = ((xs >= 0) & (xs < W)).sum(-1), ((ys >= 0) & (ys < H)).sum(-1)
        counters["outside_taps"] = int(16 * W * H - (xin * yin).sum())
        counters["clamped"] = int(((ix != fxf) | (iy != fyf)).sum())
    out = []
    for I in planes:
        rows = []
        for r in range(4):
            y = iy + (r - 1)
            yok = (y >= 0) & (y < H)
            yc = np.clip(y, 0, H - 1)
            acc = None
            for c in range(4):
                x = ix + (c - 1)
                ok = yok & (x >= 0) & (x < W)
                v = np.where(ok, I[yc, np.clip(x, 0, W - 1)], F(0)) * wx[c]
                acc = v if acc is None else acc + v
            rows.append(acc)
        out.append(((rows[0] * wy[0] + rows[1] * wy[1]) + rows[2] * wy[2]) + rows[3] * wy[3])
    return out


def upsample2(u, W, H):
    """Bilinear to W x H with pixel-centre mapping and clamped taps, times 2."""
    h, w = u.shape
    def axis(n_dst, n_src):
        f = (np.arange(n_dst, dtype=F) + F(0.5)) * (F(n_src) / F(n_dst)) - F(0.5)
        ff = np.floor(f)
        i = ff.astype(np.int64)
        return np.clip(i, 0, n_src - 1), np.clip(i + 1, 0, n_src - 1), f - ff
    x0, x1, tx = axis(W, w)
    y0, y1, ty = axis(H, h)
    tx, ty = tx[None, :], ty[:, None]
    top = u[y0][:, x0] * (F(1) - tx) + u[y0][:, x1] * tx
    bot = u[y1][:, x0] * (F(1) - tx) + u[y1][:, x1] * tx
    return ((top * (F(1) - ty) + bot * ty) * F(2)).astype(F)


def _shift_left0(a):    # a[y, x - 1], 0 at x = 0
    return np.concatenate([np.zeros_like(a[:, :1]), a[:, :-1]], axis=1)


def _shift_up0(a):      # a[y - 1, x], 0 at y = 0
    return np.concatenate([np.zeros_like(a[:1, :]), a[:-1, :]], axis=0)


def _fwd_x(a):          # a[y, x + 1] - a[y, x], 0 at the last column
    d = np.zeros_like(a)
    d[:, :-1] = a[:, 1:] - a[:, :-1]
    return d


def _fwd_y(a):
    d = np.zeros_like(a)
    d[:-1, :] = a[1:, :] - a[:-1, :]
    return d


TILE_W, TILE_H = 32, 8     # the tile of the library's iteration kernel


def tile_sums(err):
    """The f64 sum of err over each TILE_W x TILE_H tile, tiles in row-major order."""
    H, W = err.shape
    tw, th = -(-W // TILE_W), -(-H // TILE_H)
    e = np.zeros((th * TILE_H, tw * TILE_W), np.float64)
    e[:H, :W] = err
    return e.reshape(th, TILE_H, tw, TILE_W).sum(axis=(1, 3)).ravel()


def one_scale(I0, I1, u1, u2, iterations, warps, info):
    H, W = I0.shape
    thr = 0.01 * 0.01 * float(W * H)
    l_t = LAMBDA * THETA
    taut = TAU / THETA
    I1x, I1y = centered_gradient(I1)
    p11, p12, p21, p22 = (np.zeros((H, W), F) for _ in range(4))
    for _ in range(warps):
        wc = {"size": (W, H)}
        I1w, I1wx, I1wy = warp3((I1, I1x, I1y), u1, u2, wc)
        info["warps"].append(wc)
        grad = I1wx * I1wx + I1wy * I1wy
        rho_c = ((I1w - I1wx * u1) - I1wy * u2) - I0
        n = 0
        while n < iterations:
            rho = rho_c + (I1wx * u1 + I1wy * u2)
            lo, hi = rho < (-l_t) * grad, rho > l_t * grad
            mid = ~lo & ~hi & (grad > FLT_EPSILON)
            with np.errstate(divide="ignore", invalid="ignore"):   # unselected lanes of the where()s
                fi = (-rho) / grad
                d1 = np.where(lo, l_t * I1wx, np.where(hi, (-l_t) * I1wx, np.where(mid, fi * I1wx, F(0))))
                d2 = np.where(lo, l_t * I1wy, np.where(hi, (-l_t) * I1wy, np.where(mid, fi * I1wy, F(0))))
            v1, v2 = u1 + d1, u2 + d2
            div1 = (p11 - _shift_left0(p11)) + (p12 - _shift_up0(p12))
            div2 = (p21 - _shift_left0(p21)) + (p22 - _shift_up0(p22))
            n1, n2 = v1 + THETA * div1, v2 + THETA * div2
            e1, e2 = n1 - u1, n2 - u2
            err = e1 * e1 + e2 * e2
            u1, u2 = n1, n2
            u1x, u1y, u2x, u2y = _fwd_x(u1), _fwd_y(u1), _fwd_x(u2), _fwd_y(u2)
            ng1 = F(1) + taut * np.sqrt(u1x * u1x + u1y * u1y)
            ng2 = F(1) + taut * np.sqrt(u2x * u2x + u2y * u2y)
            p11, p12 = (p11 + taut * u1x) / ng1, (p12 + taut * u1y) / ng1
            p21, p22 = (p21 + taut * u2x) / ng2, (p22 + taut * u2y) / ng2
            n += 1
            info["iterations_run"] += 1
            error = float(np.sum(err, dtype=np.float64))
            info["margin"] = min(info["margin"], abs(error - thr) / thr)
            info["tests"].append({"size": (W, H), "threshold": thr, "error": error, "tiles": tile_sums(err),
                                  "lo": int(lo.sum()), "hi": int((hi & ~lo).sum()), "mid": int(mid.sum()),
                                  "flat": int((~lo & ~hi & ~mid).sum()),
                                  "gradless": int((~(grad > FLT_EPSILON)).sum())})
            if not error > thr:
                break
    assert u1.dtype == F and u2.dtype == F and p11.dtype == F
    return u1, u2


def tvl1(I0_u8, I1_u8, iterations=10, warps=2):
    """OpticalFlowDual_TVL1::calc(I0, I1): H x W x 2 f32 (x, y) flow and
    {"scales", "iterations_run", "margin", "tests", "warps"}; margin is the smallest
    |error - thr| / thr over all stop tests evaluated.  tests and warps are counters beside the
    arithmetic, in execution order: one entry per evaluated stop test (level size, threshold, error,
    the error per tile, and how many pixels took each branch of the thresholding step: lo, else hi,
    else mid, else flat; gradless counts the pixels with grad <= FLT_EPSILON whichever branch they
    took: lo and hi come first, and with grad = 0 their step is as zero as flat's) and one per warp
    (level size, outside_taps, clamped: see warp3)."""
    p0, p1 = pyramid(I0_u8), pyramid(I1_u8)
    info = {"scales": len(p0), "iterations_run": 0, "margin": float("inf"), "tests": [], "warps": []}
    s = len(p0) - 1
    u1, u2 = np.zeros(p0[s].shape, F), np.zeros(p0[s].shape, F)
    while True:
        u1, u2 = one_scale(p0[s], p1[s], u1, u2, iterations, warps, info)
        if s == 0:
            break
        s -= 1
        H, W = p0[s].shape
        u1, u2 = upsample2(u1, W, H), upsample2(u2, W, H)
    return np.stack([u1, u2], axis=-1), info


def backward_flows(lums, iterations=10, warps=2):
    """[None, calc(l1, l0), calc(l2, l1), ...] and the matching info dicts."""
    flows, infos = [None], [None]
    for prev, cur in zip(lums[:-1], lums[1:]):
        f, i = tvl1(cur, prev, iterations, warps)
        flows.append(f)
        infos.append(i)
    return flows, infos


# ---- test inputs ---------------------------------------------------------------------------------
def value_noise(W, H, seed, cell=12):
    """Smooth 8-bit value noise: a random lattice of period `cell`, cubic-smoothstep interpolated."""
    rng = np.random.RandomState(seed)
    gw, gh = W // cell + 3, H // cell + 3
    lat = rng.uniform(0.0, 255.0, (gh, gw))
    x, y = np.arange(W) / float(cell), np.arange(H) / float(cell)
    x0, y0 = x.astype(int), y.astype(int)
    tx, ty = x - x0, y - y0
    tx, ty = tx * tx * (3 - 2 * tx), ty * ty * (3 - 2 * ty)
    tx, ty = tx[None, :], ty[:, None]
    a, b = lat[y0][:, x0], lat[y0][:, x0 + 1]
    c, d = lat[y0 + 1][:, x0], lat[y0 + 1][:, x0 + 1]
    return np.clip(np.rint((a * (1 - tx) + b * tx) * (1 - ty) + (c * (1 - tx) + d * tx) * ty), 0, 255).astype(np.uint8)


def translated_pattern(W, H, n, seed, dx=3, dy=-2):
    """n gray frames: one value-noise canvas whose content moves by (dx, dy) pixels per frame."""
    m = n * max(abs(dx), abs(dy)) + 1
    canvas = value_noise(W + 2 * m, H + 2 * m, seed)
    return [np.ascontiguousarray(canvas[m - k * dy:m - k * dy + H, m - k * dx:m - k * dx + W]) for k in range(n)]


def split_pattern(W, H, n, seed):
    """n gray frames: the left half moves left and the right half moves right by 1 pixel per frame
    over a static background."""
    bg = value_noise(W, H, seed + 1000, cell=9)
    fg = translated_pattern(W, H, 2 * n, seed, dx=1, dy=0)
    out = []
    for k in range(n):
        f = bg.copy()
        hw, y0, y1 = W // 2, H // 4, H - H // 4
        f[y0:y1, :hw] = fg[n - k][y0:y1, :hw]
        f[y0:y1, hw:] = fg[n + k][y0:y1, hw:]
        out.append(f)
    return out


def block_pattern(W, H, n, seed, row=None, col=None):
    """n nearly static gray frames: frame k differs from frame 0 in one small block only, 4 rows from
    `row` (H / 3) and 5 columns from `col` (W / 3) + k, cut off at the frame's border."""
    base = value_noise(W, H, seed)
    row = H // 3 if row is None else row
    col = W // 3 if col is None else col
    out = []
    for k in range(n):
        f = base.copy()
        if k:
            f[row:row + 4, col + k:col + k + 5] = 255 - f[row:row + 4, col + k:col + k + 5]
        out.append(f)
    return out


def letterbox_pattern(W, H, n, seed, bar=12, level=16):
    """translated_pattern with the top and bottom `bar` rows set to `level`: exactly flat areas."""
    out = []
    for f in translated_pattern(W, H, n, seed):
        f[:bar, :] = level
        f[H - bar:, :] = level
        out.append(f)
    return out


def checker_pattern(W, H, n, cell=6, shift=2):
    """n gray frames of a 0 / 255 checkerboard of `cell` pixels that moves left by `shift` per frame."""
    y = np.arange(H)[:, None] // cell
    return [(((np.arange(W)[None, :] + shift * k) // cell + y) % 2 * 255).astype(np.uint8) for k in range(n)]


def constant_pattern(W, H, values):
    return [np.full((H, W), v, np.uint8) for v in values]


def gray_to_bgr(g):
    """A BGR frame whose luminance is g exactly (B = G = R = g: 16384 g + 8192 >> 14 = g)."""
    return np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2))
