"""Multimodal evaluation: what the reference computes in post-hoc scripts over saved files, on the tensors
`validate_scenes` already holds.

    gt_modes               validate/cluster.py:25-64        two ground-truth modes per pixel
    posterior_modes        validate/multimodal.py:44-64     the two strongest modes of a posterior
    mode_proportion        utils/modecnt.py:23-75           mode count and "mode proportion" of the smoothed posterior
    two_mode_error         validate/multimodal.py:51-94     two-mode MSE / BadPix sums, unimodal ones beside them
    sparsification         validate/sparsify.py:101-187     sparsification curves and their AUC
    mode_prediction_curve  validate/mm_prediction.py:43-140 the same for predicting WHERE the ground truth is bimodal

CUDA tensors take the kernels of libmmlf_eval_hip.so (include/mmlf_eval_hip.h states every definition; there is no
fallback: a missing library raises).  CPU tensors take the same arithmetic as vectorised torch, operation by operation
in the same order -- float64, float32 where the header says so -- so both paths give the same integers and, up to the
order of the error sums, the same floats.  The two curve functions are a stable sort and prefix sums on either device.

Where the scripts are arbitrary the definition is fixed: the 2-means split of a neighbourhood is the
global optimum of KMeans' objective (lowest split index on ties), a missing posterior mode is filled with the mode there
is (or the arg-max bin), and pixels of equal key are dropped in pixel order.
"""
import math

import numpy as np
import torch

from ._lib import call_eval, check, ptr

MAX_RADIUS = 4                  # MMLF_EVAL_MAX_RADIUS
FILTER_RADIUS = 8               # int(4 sigma + 0.5) of sigma = 2: the kernel's window is 17 bins
BAD_PIX_T = 0.07
TWO_MODE_FIELDS = ('mm_cnt', 'mm_mse_sum', 'mm_badpix_sum', 'um_mse_sum', 'um_badpix_sum', 'mm_few_modes')
_PARTIALS = 6144                # MMLF_EVAL_PARTIALS


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _check_radius(radius):
    if not 0.0 < float(radius) <= MAX_RADIUS:
        raise ValueError(f'gt_modes: radius {radius} is outside (0, {MAX_RADIUS}]')


def disc_offsets(radius):
    """(dy, dx) with dy^2 + dx^2 <= radius^2, dy outer, dx inner (cluster.py:47-50)"""
    r, r2 = int(math.ceil(radius)), int(math.floor(radius * radius))
    return [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dy * dy + dx * dx <= r2]


def sobel_magnitude(gt):
    """sqrt(sobel_y^2 + sobel_x^2) of (B, H, W) float32 images as scipy.ndimage.sobel defines it (derivative [-1, 0, 1] along
    the axis first, smoothing [1, 2, 1] across it, boundary `reflect`, which at reach 1 is the clamp), in float32"""
    b, h, w = gt.shape
    ys = torch.arange(-1, h + 1, device=gt.device).clamp_(0, h - 1)
    xs = torch.arange(-1, w + 1, device=gt.device).clamp_(0, w - 1)
    g = gt[:, ys][:, :, xs]                                    # (B, H + 2, W + 2)
    n = [[g[:, r:r + h, c:c + w] for c in range(3)] for r in range(3)]
    dy = [n[2][c] - n[0][c] for c in range(3)]
    dx = [n[r][2] - n[r][0] for r in range(3)]
    sy = (dy[0] + dy[2]) + 2.0 * dy[1]
    sx = (dx[0] + dx[2]) + 2.0 * dx[1]
    sq = sy * sy + sx * sx
    # numpy's float32 sqrt is the hardware's, correctly rounded as the kernel's is; torch's vectorised CPU sqrt is not
    # (1268 of the 200 000 values k / 64 come out one ulp off), which would move a pixel across the edge threshold
    return torch.sqrt(sq) if sq.is_cuda else torch.from_numpy(np.sqrt(sq.numpy()))


def _gt_modes_torch(gt, radius, edge_threshold):
    b, h, w = gt.shape
    edges = sobel_magnitude(gt).double() > float(edge_threshold)
    modes = gt.double().unsqueeze(-1).repeat(1, 1, 1, 2)
    bi, yi, xi = torch.nonzero(edges, as_tuple=True)
    if bi.numel():
        offs = disc_offsets(radius)
        vals = torch.stack([gt[bi, (yi + dy).clamp(0, h - 1), (xi + dx).clamp(0, w - 1)] for dy, dx in offs], 1)
        m0, m1 = two_means(torch.sort(vals, 1)[0].double())
        modes[bi, yi, xi, 0] = m0
        modes[bi, yi, xi, 1] = m1
    return modes, edges.to(torch.int32)


def two_means(v):
    """Rows of (N, n) float64, each sorted ascending -> the two group means (ascending) of the split into a lower and an
    upper non-empty group with the smallest summed squared deviation from the group means: the global optimum of 1-D
    2-means, the lowest split index among equal minima ([0, 1, 2] -> 0 and 1.5).  All values equal (n == 1 included):
    that value twice.  Prefix sums left to right, as the kernel accumulates them."""
    n = v.shape[1]
    equal = v[:, 0] == v[:, -1]
    m0, m1 = v[:, 0].clone(), v[:, 0].clone()
    if n > 1:
        c1, c2 = torch.cumsum(v, 1), torch.cumsum(v * v, 1)
        s, q = c1[:, -1:], c2[:, -1:]
        k = torch.arange(1, n, dtype=torch.float64, device=v.device).unsqueeze(0)
        slo, qlo = c1[:, :-1], c2[:, :-1]
        shi, qhi = s - slo, q - qlo
        cost = (qlo - slo * slo / k) + (qhi - shi * shi / (float(n) - k))
        best = cost.min(1, keepdim=True)[0]
        first = torch.argmax((cost == best).to(torch.uint8), 1, keepdim=True)      # the lowest index among equal minima
        a = (slo / k).gather(1, first)[:, 0]
        c = (shi / (float(n) - k)).gather(1, first)[:, 0]
        m0 = torch.where(equal, m0, torch.minimum(a, c))
        m1 = torch.where(equal, m1, torch.maximum(a, c))
    return m0, m1


def gt_modes(gt, radius=2.0, edge_threshold=0.5, return_edges=False):
    """Two ground-truth modes per pixel: (B, H, W) float32 -> (B, H, W, 2) float64 (and the int32 edge map)."""
    _check_radius(radius)
    if gt.dim() != 3 or gt.dtype != torch.float32:
        raise ValueError(f'gt_modes: gt must be (B, H, W) float32, found {gt.dtype} {tuple(gt.shape)}')
    if gt.is_cuda:
        check(gt, 'gt_modes: gt', gt.device)
        b, h, w = gt.shape
        modes = torch.empty((b, h, w, 2), dtype=torch.float64, device=gt.device)
        edges = torch.empty((b, h, w), dtype=torch.int32, device=gt.device)
        with torch.cuda.device(gt.device):
            call_eval('mmlf_eval_gt_modes', ptr(gt), ptr(modes), ptr(edges), b, h, w, float(radius), float(edge_threshold),
                      _stream())
    else:
        modes, edges = _gt_modes_torch(gt.contiguous(), float(radius), float(edge_threshold))
    return (modes, edges) if return_edges else modes


def gaussian_taps(sigma):
    """float64 weights of scipy.ndimage.gaussian_filter1d(sigma) for k = -8..8: exp(-0.5 / sigma^2 * k^2) over their sum,
    with libm's exp and a left-to-right sum (what the entry point computes on the host)"""
    if not (sigma > 0.0 and int(4.0 * sigma + 0.5) == FILTER_RADIUS):
        raise ValueError(f'mode_proportion: sigma {sigma} gives a filter radius other than {FILTER_RADIUS}')
    w = [math.exp(-0.5 / (sigma * sigma) * float(k * k)) for k in range(-FILTER_RADIUS, FILTER_RADIUS + 1)]
    total = 0.0
    for x in w:
        total += x
    return [x / total for x in w]


def reflect_index(i, s):
    """scipy's `reflect` (d c b a | a b c d | d c b a) of period 2s, on an integer tensor"""
    m = torch.remainder(i, 2 * s)
    return torch.where(m < s, m, 2 * s - 1 - m)


def smooth_bins(posterior, sigma=2.0):
    """gaussian_filter1d along the bin axis of (B, S, H, W) float32: float64 accumulation over k = -8..8 ascending, rounded
    to float32 once"""
    s = posterior.shape[1]
    taps = gaussian_taps(float(sigma))
    bins = torch.arange(s, device=posterior.device)
    acc = torch.zeros(posterior.shape, dtype=torch.float64, device=posterior.device)
    for t, wt in enumerate(taps):
        acc = acc + wt * posterior[:, reflect_index(bins + (t - FILTER_RADIUS), s)].double()
    return acc.float()


def _interior(mask_fn, p):
    """mask_fn(centre, left, right) on the bins 1..S-2 of (B, S, H, W); False on the two outer bins"""
    out = torch.zeros(p.shape, dtype=torch.bool, device=p.device)
    if p.shape[1] >= 3:
        out[:, 1:-1] = mask_fn(p[:, 1:-1], p[:, :-2], p[:, 2:])
    return out


def _first_argmax(x):
    return torch.max(x, 1)[1]                                   # (torch: the first of equal maxima)


def _last_argmax(x):
    return x.shape[1] - 1 - torch.max(torch.flip(x, [1]), 1)[1]


def _posterior_modes_torch(p, disp_min, disp_max):
    s = p.shape[1]
    ismax = _interior(lambda c, lft, r: (c > lft) & (c > r), p)
    cnt = ismax.sum(1)
    neg = torch.full_like(p, -math.inf)
    hts = torch.where(ismax, p, neg)
    b1 = _first_argmax(hts)
    hts2 = hts.scatter(1, b1.unsqueeze(1), -math.inf)
    b2 = _first_argmax(hts2)
    amax = _first_argmax(p)
    lo = torch.where(cnt == 0, amax, torch.where(cnt == 1, b1, torch.minimum(b1, b2)))
    hi = torch.where(cnt == 0, amax, torch.where(cnt == 1, b1, torch.maximum(b1, b2)))
    den, rng = float(s - 1 if s > 1 else 1), float(disp_max) - float(disp_min)
    disp = torch.stack([lo, hi], -1).double() / den * rng + float(disp_min)
    return cnt.clamp(max=2).to(torch.int32), disp


def _mode_proportion_torch(p, sigma, outlier):
    sm = smooth_bins(p, sigma)
    s = sm.shape[1]
    bins = torch.arange(s, device=p.device).view(1, -1, 1, 1)
    ismax = _interior(lambda c, lft, r: (lft < c) & (r < c), sm)
    ismin = _interior(lambda c, lft, r: (lft > c) & (r > c), sm)
    nmax = ismax.sum(1)
    hts = torch.where(ismax, sm, torch.full_like(sm, -math.inf))
    b1 = _last_argmax(hts)                                      # last in (height, bin) order
    t1 = hts.gather(1, b1.unsqueeze(1))[:, 0]
    hts2 = hts.scatter(1, b1.unsqueeze(1), -math.inf)
    b2 = _last_argmax(hts2)
    t2 = hts2.gather(1, b2.unsqueeze(1))[:, 0]
    two = (nmax >= 2) & (t2.double() > float(outlier) * t1.double())
    lo, hi = torch.minimum(b1, b2).unsqueeze(1), torch.maximum(b1, b2).unsqueeze(1)
    inside = ismin & (bins > lo) & (bins < hi)
    between = torch.where(inside, sm, torch.full_like(sm, math.inf)).min(1)[0]
    ok = two & inside.any(1)
    prop = torch.where(ok, (t2.double() / between.double()).float(), torch.zeros_like(t2))
    return two.to(torch.int32), prop


def _check_posterior(posterior, who):
    if posterior.dim() != 4 or posterior.dtype != torch.float32 or posterior.shape[1] < 1:
        raise ValueError(f'{who}: posterior must be (B, S >= 1, H, W) float32, found {posterior.dtype} {tuple(posterior.shape)}')


def posterior_analysis(posterior, disp_min, disp_max, sigma=2.0, outlier=0.1):
    """(n_modes, mode_disp, mode_cnt, mode_prop) of one pass over the posterior: both products of
    mmlf_eval_posterior_modes (posterior_modes and mode_proportion return one each)"""
    _check_posterior(posterior, 'posterior_analysis')
    gaussian_taps(float(sigma))                                 # (refuses a sigma the 17-bin window does not serve)
    if not posterior.is_cuda:
        p = posterior.contiguous()
        return (*_posterior_modes_torch(p, disp_min, disp_max), *_mode_proportion_torch(p, float(sigma), float(outlier)))
    check(posterior, 'posterior_analysis: posterior', posterior.device)
    b, s, h, w = posterior.shape
    dev = posterior.device
    n_modes = torch.empty((b, h, w), dtype=torch.int32, device=dev)
    mode_disp = torch.empty((b, h, w, 2), dtype=torch.float64, device=dev)
    mode_cnt = torch.empty((b, h, w), dtype=torch.int32, device=dev)
    mode_prop = torch.empty((b, h, w), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        call_eval('mmlf_eval_posterior_modes', ptr(posterior), ptr(n_modes), ptr(mode_disp), ptr(mode_cnt), ptr(mode_prop),
                  b, s, h, w, float(disp_min), float(disp_max), float(sigma), float(outlier), _stream())
    return n_modes, mode_disp, mode_cnt, mode_prop


def posterior_modes(posterior, disp_min, disp_max):
    """The two strongest modes of (B, S, H, W) float32: n_modes (B, H, W) int32 in {0, 1, 2} and their disparities
    mode_disp (B, H, W, 2) float64, ascending."""
    return posterior_analysis(posterior, disp_min, disp_max)[:2]


def mode_proportion(posterior, sigma=2.0, outlier=0.1):
    """mode_cnt (B, H, W) int32 (more than one kept maximum of the smoothed posterior) and mode_prop (B, H, W) float32 (the
    lower of the two leading maxima over the smallest minimum between them)."""
    return posterior_analysis(posterior, 0.0, 1.0, sigma, outlier)[2:]


def _two_mode_error_torch(mode_disp, n_modes, gt_modes_, gt, pred, margin, lb):
    b, h, w = gt.shape
    ys = torch.arange(h).view(1, -1, 1)
    xs = torch.arange(w).view(1, 1, -1)
    frame = (ys >= margin) & (ys < h - margin) & (xs >= margin) & (xs < w - margin)
    m0, m1 = gt_modes_[..., 0], gt_modes_[..., 1]
    sel = frame & (m0 != m1)
    d0, d1, g = mode_disp[..., 0], mode_disp[..., 1], gt.double()
    if lb:
        e0, e1 = g - d0, g - d1
        mse = torch.minimum(e0 * e0, e1 * e1)
        bad = torch.minimum((e0.abs() > BAD_PIX_T).double(), (e1.abs() > BAD_PIX_T).double())
    else:
        e0, e1 = d0 - m0, d1 - m1
        mse = (e0 * e0 + e1 * e1) * 0.5
        bad = ((e0.abs() > BAD_PIX_T).double() + (e1.abs() > BAD_PIX_T).double()) * 0.5
    eu = g - pred.double()
    cols = [torch.ones_like(g), mse, bad, eu * eu, (eu.abs() > BAD_PIX_T).double(), (n_modes < 2).double()]
    return torch.stack([c[sel].sum() for c in cols])


def two_mode_error(mode_disp, n_modes, gt_modes, gt, pred, margin=15, lb=False):
    """float64 tensor of the six TWO_MODE_FIELDS: the count of pixels inside the frame less `margin` whose two gt modes
    differ, the sums over them of the two-mode MSE / BadPix(0.07) (lb: the lower bound against gt itself) and of the
    unimodal ones of `pred`, and how many of them have n_modes < 2.  Sums, not averages: a count of 0 is a result."""
    b, h, w = gt.shape
    dev = gt.device
    for name, t, dt, shape in (('mode_disp', mode_disp, torch.float64, (b, h, w, 2)), ('n_modes', n_modes, torch.int32, (b, h, w)),
                               ('gt_modes', gt_modes, torch.float64, (b, h, w, 2)), ('gt', gt, torch.float32, (b, h, w)),
                               ('pred', pred, torch.float32, (b, h, w))):
        check(t, f'two_mode_error: {name}', dev, dtype=dt, shape=shape, contiguous=gt.is_cuda)
    if int(margin) < 0:
        raise ValueError(f'two_mode_error: margin {margin} is negative')
    if not gt.is_cuda:
        return _two_mode_error_torch(mode_disp, n_modes, gt_modes, gt, pred, int(margin), bool(lb))
    out = torch.empty(len(TWO_MODE_FIELDS), dtype=torch.float64, device=dev)
    partials = torch.empty(_PARTIALS, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        call_eval('mmlf_eval_two_mode_error', ptr(mode_disp), ptr(n_modes), ptr(gt_modes), ptr(gt), ptr(pred), b, h, w,
                  int(margin), int(bool(lb)), ptr(partials), ptr(out), _stream())
    return out


# ---- the two curves: a stable sort by (key, pixel index) and float64 prefix sums; no kernel of their own ----

def _fractions(step):
    return np.arange(0.0, 1.000000001, step)                    # sparsify.py:125, mm_prediction.py:70


def _prefix_at(values, order, ks):
    """sum of values[order[:k]] for every k of ks (float64 prefix sums of the sorted sequence)"""
    c = torch.cat([torch.zeros(1, dtype=torch.float64, device=values.device), torch.cumsum(values[order].double(), 0)])
    return c[torch.as_tensor(ks, device=values.device)].cpu().numpy()


def _auc(curve, step):
    auc = 0.0
    for i in range(len(curve) - 1):                             # the scripts' trapezoid
        auc += (curve[i] + curve[i + 1]) / 2.0 * step
    return float(auc)


def sparsification(error, uncert, gt, result, step=0.01, metric='mse'):
    """Sparsification curves of one scene (sparsify.py:101-187): the loss over the fraction of pixels with the lowest
    `error` (oracle) and the lowest `uncert`, normalised by the all-pixels entry.  Returns (frac, oracle, uncert,
    sparse_err, auc): the four columns of the script's CSV as float64 numpy arrays, and the area under sparse_err.

    The script selects by argpartition, which is arbitrary among equal keys at the cut: here pixels are ordered by a
    stable sort, (key, pixel index).  It also never clears its masks between fractions; the selections of a sorted order
    are nested prefixes, so that accumulation changes nothing."""
    if metric not in ('mse', 'badpix'):
        raise ValueError(f'sparsification: metric {metric!r} is neither mse nor badpix')
    error, uncert, gt, result = (t.reshape(-1) for t in (error, uncert, gt, result))
    n = gt.numel()
    diff = result - gt                                          # float32, as the script's arrays are
    per_pixel = diff * diff if metric == 'mse' else (diff.abs() > torch.tensor(BAD_PIX_T, dtype=diff.dtype, device=diff.device))
    fracts = _fractions(step)
    ks = [n if f == 1.0 else int(f * n) for f in fracts]
    loss = np.zeros((3, len(fracts)))
    loss[0] = 1.0 - fracts
    with np.errstate(invalid='ignore', divide='ignore'):        # a fraction of no pixel is 0 / 0, as in the script
        for row, key in ((1, error), (2, uncert)):
            order = torch.sort(key, stable=True)[1]
            loss[row] = _prefix_at(per_pixel, order, ks) / np.asarray(ks, dtype=np.float64)
        loss[1:, 0] = 0.0                                       # (the script skips fraction 0)
        loss = loss[:, ::-1].copy()
        loss[1:3] /= loss[1, 0]
    loss = np.delete(loss, -1, axis=1)
    sparse_err = loss[2] - loss[1]
    return loss[0], loss[1], loss[2], sparse_err, _auc(sparse_err, step)


def mode_prediction_curve(mode_prop, gt_modes, step=0.01):
    """How well `mode_prop` predicts where the ground truth is bimodal (mm_prediction.py:43-140): the share of bimodal pixels
    NOT among the fraction with the highest mode_prop, beside the oracle that takes the bimodal pixels first, normalised
    by the first entry.  Returns (frac, oracle, pred, sparse_err, auc).  Equal keys are ordered by pixel index (stable
    sort); the script's masks accumulate over nested prefixes, which changes nothing."""
    mask_gt = (gt_modes[..., 0] != gt_modes[..., 1]).reshape(-1)
    mode_prop = mode_prop.reshape(-1)
    n = mask_gt.numel()
    fracts = _fractions(step)
    ks = [n if f == 1.0 else int(f * n) for f in fracts]
    loss = np.zeros((3, len(fracts)))
    loss[0] = 1.0 - (1.0 - fracts)
    total = float(mask_gt.sum())
    with np.errstate(invalid='ignore', divide='ignore'):
        for row, key in ((1, (~mask_gt).to(torch.uint8)), (2, -mode_prop)):
            order = torch.sort(key, stable=True)[1]
            loss[row] = 1.0 - _prefix_at(mask_gt, order, ks) / total
        loss[1:3] /= loss[1, 0]
    loss = np.delete(loss, -1, axis=1)
    sparse_err = loss[2] - loss[1]
    return loss[0], loss[1], loss[2], sparse_err, _auc(sparse_err, step)
