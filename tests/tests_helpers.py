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
