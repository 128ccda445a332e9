"""Small numpy helpers shared by the GPU parity tests."""
import numpy as np


def _master(dy, dx, variant):
    if variant == 0:
        return dy, dx
    if variant == 1:
        return dx, dy
    return dx, 1 - dy


def variant_filter(w, variant, inverse=False):
    """w_v[..., dy, dx] = w[..., master(dy, dx)] (or its inverse scatter for gradients)."""
    out = np.empty_like(w)
    for dy in range(2):
        for dx in range(2):
            sy, sx = _master(dy, dx, variant)
            if inverse:
                out[..., sy, sx] = w[..., dy, dx]
            else:
                out[..., dy, dx] = w[..., sy, sx]
    return out


# ------------------------------------------------------------------ 3x3 ("same", pad 1) float64 references on the grid layout
# A grid tensor viewed as (B, H + 2, W + 2, C) is the zero-padded NHWC image: the 3x3 kernels read q + dy*P + dx and write
# q + P + 1, so out[b, r, c] = sum_{dy, dx} xg[b, r + dy, c + dx] @ w_v[:, :, dy, dx].T for r < H, c < W.  Plain per-tap
# matmuls in whatever dtype / device the operands have (float64 for the tests); no convolution library is involved.

def master9(variant):
    """packed tap t = dy*3 + dx -> tap of the OIHW master filter (csrc/common.h master_tap<3>)"""
    taps = []
    for t in range(9):
        dy, dx = divmod(t, 3)
        taps.append(dy * 3 + dx if variant == 0 else dx * 3 + dy if variant == 1 else dx * 3 + (2 - dy))
    return taps


def filter9(w, variant):
    """the filter the kernels apply on the grid for a stream variant: w_v[..., dy, dx] = w[..., master9(dy*3 + dx)]"""
    return w.reshape(*w.shape[:2], 9)[:, :, master9(variant)].reshape(w.shape)


def unfilter9(gv, variant):
    """a gradient with respect to filter9(w, variant), scattered back to the master filter's taps"""
    g = gv.new_zeros(gv.shape).reshape(*gv.shape[:2], 9)
    g[:, :, master9(variant)] = gv.reshape(*gv.shape[:2], 9)
    return g.reshape(gv.shape)


def conv9_ref(xg, wv, bias=None):
    """xg (B, H+2, W+2, K) with a zero frame, wv (N, K, 3, 3) -> (B, H, W, N)"""
    B, R, P, _ = xg.shape
    H, W = R - 2, P - 2
    out = xg.new_zeros((B, H, W, wv.shape[0]))
    for dy in range(3):
        for dx in range(3):
            out += xg[:, dy:dy + H, dx:dx + W, :] @ wv[:, :, dy, dx].t()
    return out if bias is None else out + bias


def dgrad9_ref(gg, wv):
    """data gradient of conv9_ref: gg (B, H+2, W+2, N) with a zero frame -> (B, H, W, K); the same correlation with the
    taps rotated by 180 degrees and the channel roles swapped"""
    return conv9_ref(gg, wv.flip(-1, -2).transpose(0, 1))


def wgrad9_ref(xg, gg):
    """weight gradient (N, K, 3, 3) of conv9_ref and bias gradient (N,): xg (B, H+2, W+2, K), gg (B, H+2, W+2, N)"""
    B, R, P, K = xg.shape
    H, W = R - 2, P - 2
    gv = gg[:, 1:H + 1, 1:W + 1, :].reshape(-1, gg.shape[-1])
    gw = xg.new_zeros((gg.shape[-1], K, 3, 3))
    for dy in range(3):
        for dx in range(3):
            gw[:, :, dy, dx] = gv.t() @ xg[:, dy:dy + H, dx:dx + W, :].reshape(-1, K)
    return gw, gv.sum(0)


# ------------------------------------------------------------------ 2x2 float64 references on the grid layout
# The 2x2 kernels read q + dy*P + dx and write q + out_shift (include/mmlf_hip.h).  On the grid view (B, H + 2, W + 2, C):
#   pad 1: input extent (H, W) at (1, 1)       -> output extent (H + 1, W + 1) at (0, 0), out_shift = 0
#   pad 0: input extent (H + 1, W + 1) at (0, 0) -> output extent (H, W) at (1, 1),       out_shift = P + 1
# Either way out[b, r, c] = sum_{dy, dx} xg[b, r + dy, c + dx] @ w_v[:, :, dy, dx].T over the output's extent (h, w); the
# references return that extent alone, the caller places it.  Plain per-tap matmuls, as conv9_ref.

def filter4(w, variant):
    """the filter the kernels apply on the grid for a stream variant: w_v[..., dy, dx] = w[..., master(dy, dx)]"""
    out = w.new_zeros(w.shape)
    for dy in range(2):
        for dx in range(2):
            sy, sx = _master(dy, dx, variant)
            out[..., dy, dx] = w[..., sy, sx]
    return out


def unfilter4(gv, variant):
    """a gradient with respect to filter4(w, variant), scattered back to the master filter's taps"""
    out = gv.new_zeros(gv.shape)
    for dy in range(2):
        for dx in range(2):
            sy, sx = _master(dy, dx, variant)
            out[..., sy, sx] = gv[..., dy, dx]
    return out


def extent4(xg, pad):
    """(h, w) of the OUTPUT of a pad-`pad` 2x2 convolution whose input lives on the grid view xg (B, H + 2, W + 2, C)"""
    H, W = xg.shape[1] - 2, xg.shape[2] - 2
    return (H + 1, W + 1) if pad else (H, W)


def conv4_ref(xg, wv, bias=None, pad=1):
    """xg (B, H+2, W+2, K) zero outside the input's extent, wv (N, K, 2, 2) -> (B, h, w, N), (h, w) = extent4(xg, pad)"""
    h, w = extent4(xg, pad)
    out = xg.new_zeros((xg.shape[0], h, w, wv.shape[0]))
    for dy in range(2):
        for dx in range(2):
            out += xg[:, dy:dy + h, dx:dx + w, :] @ wv[:, :, dy, dx].t()
    return out if bias is None else out + bias


def dgrad4_ref(gg, wv, pad=1):
    """data gradient of conv4_ref(., wv, pad): gg (B, H+2, W+2, N) holds the output gradient where the forward stored its
    output ((0, 0) for pad 1, (1, 1) for pad 0) -> (B, h, w, K) on the forward INPUT's extent.  The same correlation in the
    other placement, taps rotated by 180 degrees, channel roles swapped."""
    return conv4_ref(gg, wv.flip(-1, -2).transpose(0, 1), None, 1 - pad)


def wgrad4_ref(xg, gg, pad=1):
    """weight gradient (N, K, 2, 2) of conv4_ref(xg, ., pad) and bias gradient (N,); gg as in dgrad4_ref"""
    h, w = extent4(xg, pad)
    o = 0 if pad else 1
    gv = gg[:, o:o + h, o:o + w, :].reshape(-1, gg.shape[-1])
    K = xg.shape[-1]
    gw = xg.new_zeros((gg.shape[-1], K, 2, 2))
    for dy in range(2):
        for dx in range(2):
            gw[:, :, dy, dx] = gv.t() @ xg[:, dy:dy + h, dx:dx + w, :].reshape(-1, K)
    return gw, gv.sum(0)


def check_sum_bar(got, ref, bound, what, tol=2e-5):
    """|got - ref| <= tol * sum|a||b| + 1e-6 * max: the bar every float64 comparison of a convolution kernel here uses
    (`bound` = the same sum over absolute values)"""
    err = (got - ref).abs()
    lim = tol * bound + 1e-6 * float(bound.max()) + 1e-30
    assert bool((err <= lim).all()), (what, float((err / lim).max()))


# ------------------------------------------------------------------ BatchNorm2d + ReLU float64 references on the grid layout
# nn.BatchNorm2d (training statistics, running update, affine) and nn.ReLU with their gradients, over the interior
# [1, H] x [1, W] of the grid view (B, H + 2, W + 2, C), as plain tensor expressions in whatever dtype / device the operands
# have (float64 for the tests); no batch_norm call is involved.  Border positions of the operands are never used (they may hold
# anything); the element-wise results are returned for the whole view, the caller takes the positions it wants.

def _interior(g):
    return g[:, 1:g.shape[1] - 1, 1:g.shape[2] - 1, :]


def bn_stats_ref(zg, gamma, beta, rm, rv, momentum, eps):
    """zg (B, H+2, W+2, C) -> (mean, invstd, scale, shift, new running mean, new running variance), each (C,).  Biased
    variance as E[z^2] - E[z]^2 (the order bn_stats_finalize_kernel takes: the inputs keep mean^2 small against it), exactly
    0 for one element; the running variance takes the unbiased form (the biased one for one element, as the kernel does).
    gamma / beta / rm / rv may be None (1 / 0 / no running update)."""
    zi = _interior(zg)
    n = zi.shape[0] * zi.shape[1] * zi.shape[2]
    mean = zi.sum((0, 1, 2)) / n
    var = ((zi * zi).sum((0, 1, 2)) / n - mean * mean).clamp_min(0) if n > 1 else mean * 0
    invstd = 1 / (var + eps).sqrt()
    scale = invstd if gamma is None else gamma * invstd
    shift = -mean * scale if beta is None else beta - mean * scale
    unb = var * n / (n - 1) if n > 1 else var
    new_rm = None if rm is None else (1 - momentum) * rm + momentum * mean
    new_rv = None if rv is None else (1 - momentum) * rv + momentum * unb
    return mean, invstd, scale, shift, new_rm, new_rv


def bn_apply_ref(zg, scale, shift):
    """u = z * scale + shift (ReLU is the caller's clamp) and the absolute terms |z * scale| + |shift| a rounding bar scales by"""
    t = zg * scale
    return t + shift, t.abs() + shift.abs()


class BnBwd:
    """what bn_bwd_ref returns: mask, dgamma, dbeta, k1, k2, k3, dz, and the sums of absolute terms sum_abs_g = sum |g|,
    sum_abs_gz = sum |g| |zhat|, dz_abs = |k1 g| + |k2| + |k3| |z - mean|"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def bn_bwd_ref(zg, gyg, scale, shift, gamma, mean, invstd):
    """gradient of relu(batch_norm(z)) in training mode, from the forward's coefficients: g = gy * (u > 0) with
    u = z * scale + shift; dbeta = sum g, dgamma = sum g * zhat, zhat = (z - mean) * invstd; k1 = gamma * invstd,
    k2 = k1 * dbeta / n, k3 = k1 * invstd * dgamma / n; dz = k1 * g - k2 - k3 * (z - mean).  mask, dz and dz_abs cover the
    interior (B, H, W, C); gamma may be None (1)."""
    z, gy = _interior(zg), _interior(gyg)
    n = z.shape[0] * z.shape[1] * z.shape[2]
    mask = z * scale + shift > 0
    g = gy * mask
    zc = z - mean
    zhat = zc * invstd
    dbeta, dgamma = g.sum((0, 1, 2)), (g * zhat).sum((0, 1, 2))
    k1 = invstd if gamma is None else gamma * invstd
    k2, k3 = k1 * dbeta / n, k1 * invstd * dgamma / n
    return BnBwd(mask=mask, dgamma=dgamma, dbeta=dbeta, k1=k1, k2=k2, k3=k3, dz=k1 * g - k2 - k3 * zc,
                 sum_abs_g=g.abs().sum((0, 1, 2)), sum_abs_gz=(g.abs() * zhat.abs()).sum((0, 1, 2)),
                 dz_abs=(k1 * g).abs() + k2.abs() + k3.abs() * zc.abs())
