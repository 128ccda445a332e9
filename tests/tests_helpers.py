"""Small numpy helpers shared by the GPU parity tests."""
import contextlib

import numpy as np
import torch


@contextlib.contextmanager
def dry_engine(extents=False, mode='f16x3'):
    """The host code of mmlf_amd.engine without a GPU, as `tools/launch_trace.py --dry` runs it: engine.call records
    (name, args) into the list this yields and launches nothing (the host-only mmlf_audit_* entries still run), the stream
    pointer is 0, the side-stream weight gradient is off.  The caller keeps its tensors on the CPU.  extents:
    MMLF_CHECK_EXTENTS, with engine.EXTENT_CHECKS reset to 0."""
    from mmlf_amd import _lib, engine
    calls = []
    real = engine.call

    def record(name, *args):
        calls.append((name, args))
        if name.startswith('mmlf_audit_'):
            real(name, *args)

    names = ('call', 'CONV_MODE', 'OVERLAP_WGRAD', 'CHECK_EXTENTS', 'EXTENT_CHECKS')
    saved, stream_ptr = [getattr(engine, n) for n in names], _lib.stream_ptr
    engine.call, engine.CONV_MODE, engine.OVERLAP_WGRAD, engine.CHECK_EXTENTS, engine.EXTENT_CHECKS = record, mode, False, extents, 0
    _lib.stream_ptr = lambda: 0
    try:
        yield calls
    finally:
        _lib.stream_ptr = stream_ptr
        for n, v in zip(names, saved):
            if n != 'EXTENT_CHECKS':             # (the count stays readable behind the block)
                setattr(engine, n, v)


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


# ------------------------------------------------------------------ helpers of the direct-call GPU modules
# (tests/test_gpu_elementwise.py, tests/test_gpu_losses.py, tests/test_gpu_heads.py)
GUARDVAL, NGUARD = -4321.0, 64
RATIOS = {}                                  # bar -> largest error / bar seen (each module prints and clears it when done)


class _Pool:
    """output buffers between guard bands"""

    def __init__(self, dev):
        self.dev, self.items = dev, []

    def new(self, n, fill, dtype=torch.float32):
        full = torch.full((n + 2 * NGUARD,), GUARDVAL, dtype=dtype, device=self.dev)
        inner = full[NGUARD:NGUARD + n]
        inner.fill_(fill)
        self.items.append((full, n))
        return inner

    def of(self, t):
        inner = self.new(t.numel(), 0.0, t.dtype)
        inner.copy_(t.reshape(-1))
        return inner

    def check(self, what):
        for k, (full, n) in enumerate(self.items):
            assert bool((full[:NGUARD] == GUARDVAL).all()) and bool((full[NGUARD + n:] == GUARDVAL).all()), \
                (what, f'guard band of buffer {k} ({n} elements) overwritten')


def _pick(values, shape, gen):
    v = torch.tensor(values, dtype=torch.float32, device=gen.device)
    return v[torch.randint(0, len(values), shape, device=gen.device, generator=gen)]


def _ints(lo, hi, shape, gen):
    return torch.randint(lo, hi + 1, shape, device=gen.device, generator=gen).float()


def _bar(err, bar, key, what):
    """err <= bar element-wise (a NaN fails); the largest ratio is kept for the headroom report"""
    ratio = err / bar.clamp_min(1e-300)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    RATIOS[key] = max(RATIOS.get(key, 0.0), worst if worst == worst else float('inf'))
    ok = err <= bar
    assert bool(ok.all()), (what, key, f'{int((~ok).sum())} of {ok.numel()} over the bar, worst ratio {worst}',
                            f'first at flat index {int((~ok).reshape(-1).to(torch.uint8).argmax())}')


def _ulp(got, ref, key, what, ulps=1.0):
    """|got - ref| <= ulps float32 units in the last place (of the larger of the two magnitudes)"""
    g = got.double()
    mag = torch.maximum(g.abs(), ref.abs()).clamp_min(2.0 ** -126)
    _bar((g - ref).abs(), ulps * torch.exp2(torch.floor(torch.log2(mag)) - 23), key, what)


def _same(got, want, what):
    """equal values, element for element (float32 against the float64 reference, which must itself be a float32 number)"""
    assert bool((want.float().double() == want).all()), (what, 'precondition: the exact result is a float32 number')
    bad = ~(got.double() == want)
    if bool(bad.any()):
        k = int(bad.reshape(-1).to(torch.uint8).argmax())
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} elements differ from the exact result; flat index {k} '
                             f'holds {float(got.reshape(-1)[k])!r}, exact {float(want.reshape(-1)[k])!r}')


def _close(got, ref, bar, key, what):
    """|got - ref| <= bar wherever the reference is finite; where it is not (the documented NaN of loss kind 4, the -inf logvar
    of the DPP head) `got` must be the same non-finite value.  No element is left out."""
    g = got.double().reshape(ref.shape)
    fin = torch.isfinite(ref)
    same = (g == ref) | (torch.isnan(g) & torch.isnan(ref))
    assert bool(same[~fin].all()), (what, key, 'differs from the non-finite value of the reference')
    assert bool(torch.isfinite(bar[fin]).all()), (what, key, 'precondition: a finite bar wherever the reference is finite')
    zero = torch.zeros_like(ref)
    _bar(torch.where(fin, (g - ref).abs(), zero), torch.where(fin, bar, zero), key, what)


# ------------------------------------------------------------------ losses, heads and Adam: float64 references
# Plain torch expressions of the mathematics, in float64, on whatever device the operands have.  The operands arrive as the
# float32 tensors the kernels read.  DECISIONS the kernels specify as float32 expressions are taken here from the same float32
# torch expression, and everything after the decision is float64:
#   * |grid_k - gt| < half_step: a float32 subtraction against the float32 half_step;
#   * tot < 0.01f on the sequential float32 sum of the alphas (loss_ref asserts that every total lies outside [0.005, 0.02]
#     or is a float32 sum that equals the float64 one exactly, so the float64 sum the mathematics uses agrees);
#   * raw > 0 and v == max: the same in either precision;
#   * the sign of a float32 difference.
class Ref:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _sign32(a, b):
    """sign of the float32 difference a - b, as float64 (0 where they are equal)"""
    return torch.sign(a.float() - b.float()).double()


def _bins32(grid, x, half_step):
    """[|grid_k - x| < half_step] in float32: grid (K,), x (B, ..., H, W) -> (B, K, ..., H, W) float64"""
    g = grid.float().view(1, -1, *([1] * (x.dim() - 1)))
    half = torch.tensor(half_step, dtype=torch.float64).float().to(x.device)
    return (torch.abs(g - x.float().unsqueeze(1)) < half).double()


def loss_ref(kind, out, target, mask, mask_padding=None, grid=None, half_step=0.0, den_override=None, aux_override=None):
    """The seven training losses on the raw output `out` (B, oc, H, W), float32: 0 masked L1, 1 Laplace NLL (mean, logvar),
    2 cross entropy on relu(scores) against the one-hot of gt, 3 alpha-weighted L1 to every plane of target (B, P, 5, H, W),
    4 its Laplace NLL normalised by the mean total alpha with a -logvar term on pixels without a surface, 5 cross entropy
    against the alpha-weighted more-hot target, 6 the Laplace NLL with mask_padding.  loss = sum(l mask) / den with
    den = den_override, or the number of mask pixels, or 1 where that is 0; aux_override = (s0, s1) replaces the whole-batch
    sums of kind 4 (sum of the total alpha, number of surface-less pixels) and kind 6 (number of in-range pixels, unused).
    Returns Ref(l, g, loss, grad, count, sum, den, aux, parts): l (B, H, W) the per-pixel loss, g (B, c, H, W) its derivative
    with respect to the channels the loss uses, grad = g mask / den, parts the absolute terms the rounding bars are built of."""
    o = out.double()
    B, oc, H, W = o.shape
    n = B * H * W
    mk = mask.double()
    parts, aux = {}, None
    if kind in (0, 1, 6):
        d, s = (o[:, 0] - target.double()).abs(), _sign32(out[:, 0], target)
    if kind == 0:
        l, g = d, s.unsqueeze(1)
    elif kind == 1:
        lv = o[:, 1]
        e = torch.exp(-lv)
        l, g = e * d + lv, torch.stack([e * s, 1 - e * d], 1)
        parts = dict(ed=e * d)
    elif kind in (2, 5):
        if kind == 2:
            t = _bins32(grid, target, half_step)
        else:
            t = (_bins32(grid, target[:, :, 4], half_step) * target[:, :, 3].double().unsqueeze(1)).sum(2)
        v = o.clamp_min(0)
        dot, z = (v * t).sum(1), torch.exp(v).sum(1)
        l = -torch.log(torch.exp(dot) / z)
        pk = torch.exp(o) / z.unsqueeze(1)
        g = torch.where(out > 0, pk - t, torch.zeros_like(pk))
        parts = dict(dot=dot, pk=pk, t=t)
    elif kind in (3, 4):
        w, tg = target[:, :, 3].double(), target[:, :, 4].double()
        d, s = (o[:, 0].unsqueeze(1) - tg).abs(), _sign32(out[:, 0].unsqueeze(1), target[:, :, 4])
        if kind == 3:
            l, g = (d * w).sum(1), (s * w).sum(1, keepdim=True)
            parts = dict(sw=w.abs().sum(1))
        else:
            lv = o[:, 1]
            e = torch.exp(-lv)
            tot32 = torch.zeros_like(target[:, 0, 3])
            for k in range(target.shape[1]):
                tot32 = tot32 + target[:, k, 3]
            tot = w.sum(1)
            assert bool(((tot < 0.005) | (tot > 0.02) | (tot32.double() == tot)).all()), \
                'precondition: a total alpha in [0.005, 0.02] whose float32 sum is not exact'
            oor = (tot32 < torch.tensor(0.01, dtype=torch.float32)).double()
            s0, s1 = (tot.sum(), oor.sum()) if aux_override is None else (aux_override[0].double(), aux_override[1].double())
            aux = (s0, s1)
            f0, f1 = s0 / n, n / s1                          # f1 = inf where no pixel lacks a surface: 0 * inf = NaN below
            term = (e.unsqueeze(1) * d + lv.unsqueeze(1)) * w
            acc, gm, glv = term.sum(1), (e.unsqueeze(1) * s * w).sum(1), ((1 - e.unsqueeze(1) * d) * w).sum(1)
            l_oor = -lv * oor * f1
            l = (acc / f0 + l_oor) / 2
            g = torch.stack([gm / f0 / 2, (glv / f0 - oor * f1) / 2], 1)
            parts = dict(sE=(e.unsqueeze(1) * d * w).sum(1), sT=term.abs().sum(1), acc=acc, f0=f0, f1=f1, l_oor=l_oor,
                         sew=(e.unsqueeze(1) * w).sum(1), sG=((1 - e.unsqueeze(1) * d).abs() * w).sum(1), glv=glv, oor=oor)
    else:
        lv = o[:, 1]
        e = torch.exp(-lv)
        mp = mask_padding.double()
        oor = 1 - mp
        s0 = mp.sum() if aux_override is None else aux_override[0].double()
        aux = (s0, None)
        f0 = n / s0 if float(s0) > 0 else torch.ones_like(s0)
        f1 = n / (n - s0) if float(n - s0) > 0 else torch.ones_like(s0)
        l_in, l_oor = (e * d + lv) * mp * f0, -lv * oor * f1
        l = (l_in + l_oor) / 2
        g = torch.stack([e * s * mp * f0 / 2, ((1 - e * d) * mp * f0 - oor * f1) / 2], 1)
        parts = dict(ed=e * d, f0=f0, f1=f1, mp=mp, oor=oor, l_in=l_in, l_oor=l_oor, nll=e * d + lv)
    count = mk.sum()
    den = count if den_override is None else den_override.double().reshape(())
    den_used = torch.where(den == 0, torch.ones_like(den), den)
    total = (l * mk).sum()
    return Ref(l=l, g=g, loss=total / den_used, grad=g * (mk / den_used).unsqueeze(1), count=count, den=den, den_used=den_used,
               sum=total, aux=aux, parts=parts)


def upr_ref(out, grid, grad_posterior=None):
    """The UPR head: posterior_k = exp(-|grid_k - mu| / b) / (2 b), b = exp(logvar), on out (B, 2, H, W); with grad_posterior
    (B, K, H, W) also the gradient with respect to out: d post_k / d mu = post_k sign(grid_k - mu) / b (0 where they are
    equal), d post_k / d logvar = post_k (|grid_k - mu| / b - 1).  Returns Ref(post, gout, t, b, tm, tl): t = |grid_k - mu| / b,
    tm / tl the per-bin terms of the two sums."""
    o = out.double()
    mu, b = o[:, 0].unsqueeze(1), torch.exp(o[:, 1]).unsqueeze(1)
    gk = grid.double().view(1, -1, 1, 1)
    t = (gk - mu).abs() / b
    post = 1.0 / (2.0 * b) * torch.exp(-t)
    r = Ref(post=post, t=t, b=b, gout=None)
    if grad_posterior is not None:
        go = grad_posterior.double()
        s = _sign32(grid.view(1, -1, 1, 1), out[:, 0].unsqueeze(1))
        r.tm, r.tl = go * post * s / b, go * post * (t - 1)
        r.gout = torch.stack([r.tm.sum(1), r.tl.sum(1)], 1)
    return r


def dpp_ref(scores, grid_torch, grid_np):
    """The DPP head on scores (B, K, H, W): one_hot = [s == max s] (every maximum), posterior = softmax, mean =
    sum grid_torch one_hot, logvar = log sum (grid_np - mean)^2 posterior (-inf where the posterior sits on the arg-max bin
    alone)."""
    s = scores.double()
    one_hot = (torch.max(s, 1, keepdim=True)[0] == s).double()
    e = torch.exp(s)
    post = e / e.sum(1, keepdim=True)
    mean = (grid_torch.double().view(1, -1, 1, 1) * one_hot).sum(1)
    d = grid_np.double().view(1, -1, 1, 1) - mean.unsqueeze(1)
    V = (d * d * post).sum(1)
    return Ref(one_hot=one_hot, post=post, mean=mean, logvar=torch.log(V), V=V, d=d)


def dpp_bwd_ref(scores, grid_np, mean, grad_posterior=None, grad_logvar=None):
    """Gradient of dpp_ref's posterior and logvar with respect to the scores, `mean` (B, H, W) a constant of the graph:
    dL/dp_k = grad_posterior_k + grad_logvar (grid_np_k - mean)^2 / V, dL/ds_i = p_i (dL/dp_i - sum_j dL/dp_j p_j); either
    gradient may be None (it is left out).  Returns Ref(gs, post, d, V, gl, dp, dot)."""
    s = scores.double()
    e = torch.exp(s)
    post = e / e.sum(1, keepdim=True)
    d = grid_np.double().view(1, -1, 1, 1) - mean.double().unsqueeze(1)
    V = (d * d * post).sum(1)
    dp = torch.zeros_like(s) if grad_posterior is None else grad_posterior.double()
    gl = None
    if grad_logvar is not None:
        gl = (grad_logvar.double() / V).unsqueeze(1)
        dp = dp + gl * d * d
    dot = (dp * post).sum(1, keepdim=True)
    return Ref(gs=post * (dp - dot), post=post, d=d, V=V, gl=gl, dp=dp, dot=dot)


def adam_ref(p, g, m, v, lr, beta1, beta2, eps, step, grad_scale=1.0):
    """One step of torch.optim.Adam (no weight decay, no amsgrad) on the gradient g * grad_scale -> (p, m, v)"""
    gi = g.double() * grad_scale
    m2 = m.double() + (gi - m.double()) * (1 - beta1)
    v2 = v.double() * beta2 + gi * gi * (1 - beta2)
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    denom = v2.sqrt() / bc2 ** 0.5 + eps
    return p.double() - lr / bc1 * (m2 / denom), m2, v2


# shape lists of tests/test_gpu_losses.py and of the direct-call tests of tests/test_gpu_heads.py (held to their classes by
# tests/test_loss_head_cpu.py): (B, H, W) with a total of 1 | 255, 256, 257: one block short, exact, one over | B > 1 and an odd
# HW | two batches of 300; the stride frame: more than 8192 * 256 pixels, so a thread of the capped launch takes a second turn
LOSS_FRAMES = [(1, 1, 1), (1, 1, 255), (1, 1, 256), (1, 1, 257), (3, 5, 7), (2, 1, 300)]
LOSS_STRIDE_FRAME = (1, 1024, 2049)
LOSS_NBLOCKS = [1, 3, 63, 64, 65, 1024, 4096]
LOSS_NBLOCKS_FRAMES = [(3, 5, 7), (2, 1, 300)]
ADAM_N = [1, 255, 256, 257, 2097153]


# ------------------------------------------------------------------ data side and validation side: numpy references
# (tests/test_data_refs_cpu.py pins them to the goldens; tests/test_gpu_data_kernels.py holds the kernels to them.)  The shear,
# the patch chain and Contrast are float32 restatements, operation for operation: the kernels must give these BITS.  The
# ensemble posterior and the discretised mixture are float64 with a per-element bound that counts the float32 roundings on the
# kernel's path, under the assumption that the device expf is good to 1 ulp (U32 = 2^-24 is half an ulp).
U32 = 2.0 ** -24
PATCH_NAMES = ('h', 'v', 'i', 'd', 'center', 'gt', 'mpi', 'mask')


def _oracle():
    from oracle import oracle as orc
    return orc


def shift_table_ref(disps, views):
    """hci4d.py:934-938 per (member, view): integer shifts (s0, s1) int32 and weights (1 - alpha, alpha) float32, from
    math.modf / copysign on doubles: what mmlf_shift_views takes as tab_s / tab_w"""
    import math
    half = int(views / 2)
    tab_s, tab_w = np.zeros((len(disps), views, 2), np.int32), np.zeros((len(disps), views, 2), np.float32)
    for s, disp in enumerate(disps):
        for k in range(views):
            alpha, s0 = math.modf(float(disp) * (k - half))
            s1 = s0 + math.copysign(1.0, s0)
            tab_s[s, k] = (int(s0), int(s1))
            tab_w[s, k] = (1.0 - abs(alpha), abs(alpha))
    return tab_s, tab_w


def shift_ref(stacks, disps):
    """four stacks (views, 3, H, W) -> four arrays (S, views, 3, H, W) float32: oracle.shift_views per disparity"""
    orc = _oracle()
    per = [orc.shift_views(stacks, float(d)) for d in disps]
    return [np.stack([p[i] for p in per]).astype(np.float32) for i in range(4)]


def patch_ref(scene, params):
    """One sample of the training patch chain with every parameter given: params = dict(ps, f, disp, y0, x0, rot, flags, mat,
    bright); flags: 1 shift | 2 colour | 4 brightness.  The kernel's documented order (include/mmlf_hip.h): tf_downsample(f),
    tf_shift(disp) under flag 1, ONE crop of ps x ps at (y0, x0) of the down-sampled frame, rot x tf_rotate90 (the mask is not
    rotated), tf_redist_color under flag 2, tf_brightness under flag 4; gt and mpi[:, 4] take / f always and - disp under flag 1.
    Returns (h, v, i, d, center, gt, mpi) float32 and the mask as int64."""
    orc = _oracle()
    p = params
    data = tuple(np.array(a, copy=True) for a in scene[:8])
    data = orc.tf_downsample(data, int(p['f']))
    if p['flags'] & 1:
        data = orc.tf_shift(data, p['disp'])
    data = orc.tf_crop(data, (p['ps'], p['ps']), (p['y0'], p['x0']))
    for _ in range(p['rot']):
        data = orc.tf_rotate90(data)
    if p['flags'] & 2:
        data = orc.tf_redist_color(data, np.asarray(p['mat'], np.float64))
    if p['flags'] & 4:
        data = orc.tf_brightness(data, p['bright'])
    for a in data[:7]:
        assert a.dtype == np.float32, 'precondition: the chain stays in float32'
    return (*[np.ascontiguousarray(a) for a in data[:7]], np.ascontiguousarray(data[7]).astype(np.int64))


def contrast_ref(stacks4, center, alpha, mean32):
    """Contrast (hci4d.py:740-751) for a GIVEN float32 mean: x * float32(alpha) + mean32 * float32(1 - alpha), each operation
    rounded to float32.  stacks4: the four stacks of one sample; returns ([four stacks], center)."""
    a, b, m = np.float32(alpha), np.float32(1.0 - alpha), np.float32(mean32)
    off = np.float32(m * b)
    f = lambda x: (np.asarray(x, np.float32) * a).astype(np.float32) + off   # noqa: E731
    return [f(x) for x in stacks4], f(center)


def ensamble_reduce_ref(means, logvars, grid):
    """means, logvars (S, B, H, W) float32, grid (K,) float32 -> (idx, mean, logvar, ref, bound): idx (B, H, W) the FIRST
    minimum of logvars over the members (np.argmin: the reference's rule on the CPU and that of the kernel's strict <), mean
    and logvar gathered there (exact), ref (B, K, H, W) float64 = (1/S) sum_j exp(t_j) / (2 b_j) with b_j = exp(logvar_j),
    t_j = -|grid_k - mean_j| / b_j, and the bound of the float32 kernel's error: per term (6 + 4 |t_j|) U32 -- the subtraction
    U32, b 2 U32, the division U32 make t off by 4 U32, so exp(t) by 4 |t| U32 plus 2 U32 of its own, 1 / (2 b) adds 3 U32 and
    the product U32 -- plus (S + 1) U32 of the sum for S sequential additions of positive terms and the division, plus 1e-37
    for underflow."""
    S = means.shape[0]
    idx = np.argmin(logvars, 0)
    mean = np.take_along_axis(means, idx[None], 0)[0]
    logvar = np.take_along_axis(logvars, idx[None], 0)[0]
    gk = np.asarray(grid, np.float32).astype(np.float64).reshape(1, -1, 1, 1)
    ref = np.zeros((means.shape[1], gk.size, *means.shape[2:]), np.float64)
    werr = np.zeros_like(ref)
    for j in range(S):
        b = np.exp(logvars[j].astype(np.float64))[:, None]
        t = -np.abs(gk - means[j].astype(np.float64)[:, None]) / b
        term = np.exp(t) / (2.0 * b)
        ref += term
        werr += (6.0 + 4.0 * np.abs(t)) * term
    ref /= S
    bound = U32 / S * werr + (S + 1) * U32 * ref + 1e-37
    return idx, mean, logvar, ref, bound


def ensamble_posterior_f32(means, logvars, grid):
    """the kernel's float32 arithmetic in numpy, operation for operation (laplace_pdf and the sequential sum): what the bound of
    ensamble_reduce_ref is tried against without a GPU"""
    S = means.shape[0]
    gk = np.asarray(grid, np.float32).reshape(1, -1, 1, 1)
    acc = np.zeros((means.shape[1], gk.size, *means.shape[2:]), np.float32)
    for j in range(S):
        b = np.exp(logvars[j].astype(np.float32))[:, None]
        a = np.float32(1.0) / (np.float32(2.0) * b)
        t = -np.abs(gk - means[j][:, None]) / b
        acc = acc + a * np.exp(t)
    return acc / np.float32(S)


def lmm_edges(n_bins, x_min, x_max):
    """validate/cli.py:90-103: the n_bins + 1 float64 bin edges"""
    step = (x_max - x_min) / n_bins
    return np.linspace(x_min - step / 2.0, x_max + step / 2.0, n_bins + 1)


def _cdf_laplace64(x, m, v):
    z = (x - m) / v
    with np.errstate(over='ignore'):
        return np.where(x < m, np.exp(z) / 2.0, 1.0 - np.exp(-z) / 2.0)


def lmm_ref(means, logvars, edges, exp32=None):
    """means, logvars (S, B, H, W) float32, edges (n_bins + 1,) float64 -> (ref, bound), both (B, n_bins, H, W) float64:
    ref = (1/S) sum_s cdf(edge_k+1) - cdf(edge_k) of Laplace(mean_s, v_s) with v = float64(np.exp(float32 logvars)), as
    metrics.laplace_to_discrete states it.  The kernel is float64 except for v = (double)expf(logvar): a 1 ulp expf against
    numpy's float32 exp moves v by at most 2^-22 relative, and each exp(-|z|) / 2 term by w(z) 2^-22, w(z) = |z| exp(-|z|) / 2:
    bound = 2^-22 / S * sum_s (w(z0_s) + w(z1_s)) + 4e-16 (the cancellation in 1 - exp(-z) / 2 and the float64 sum).
    exp32: another float32 exponential (the CPU tests try the bound with it)."""
    S = means.shape[0]
    e = np.asarray(edges, np.float64)
    e0, e1 = e[:-1].reshape(1, -1, 1, 1), e[1:].reshape(1, -1, 1, 1)
    ref = np.zeros((means.shape[1], e.size - 1, *means.shape[2:]), np.float64)
    werr = np.zeros_like(ref)
    w = lambda z: np.abs(z) * np.exp(-np.abs(z)) / 2.0   # noqa: E731
    for s in range(S):
        lv = logvars[s].astype(np.float32)
        v = (np.exp(lv) if exp32 is None else exp32(lv)).astype(np.float32).astype(np.float64)[:, None]
        m = means[s].astype(np.float64)[:, None]
        ref += _cdf_laplace64(e1, m, v) - _cdf_laplace64(e0, m, v)
        werr += w((e0 - m) / v) + w((e1 - m) / v)
    return ref / S, 2.0 ** -22 / S * werr + 4e-16


def lmm_mass_ref(means, logvars, edges):
    """(B, H, W) float64: cdf(last edge) - cdf(first edge) of the mixture: what an image's bin masses add up to"""
    e = np.asarray(edges, np.float64)
    tot = np.zeros(means.shape[1:], np.float64)
    for s in range(means.shape[0]):
        v = np.exp(logvars[s].astype(np.float32)).astype(np.float64)
        m = means[s].astype(np.float64)
        tot += _cdf_laplace64(e[-1], m, v) - _cdf_laplace64(e[0], m, v)
    return tot / means.shape[0]
