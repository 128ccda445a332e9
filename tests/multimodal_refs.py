"""Plain pixel-loop restatements of the reference's five multimodal evaluation scripts (numpy, float64), for
tests/test_multimodal_cpu.py.  Each function names the lines it restates (paths relative to the reference repo root).
Where a script is arbitrary (KMeans from a random start, argpartition among equal values) the rule is the one
include/mmlf_eval_hip.h and mmlf_amd/multimodal.py define; it is restated here independently, as loops.

Written for clarity, not speed: use frames of a few pixels."""
import math

import numpy as np

BAD_PIX_T = 0.07


def _clamp(v, hi):
    return max(0, min(hi, v))


def sobel_ref(img, axis):
    """scipy.ndimage.sobel(img, axis) on a 2-D float32 image, float32 arithmetic: derivative [-1, 0, 1] along `axis`, then
    smoothing [1, 2, 1] along the other one, boundary `reflect` (index -1 -> 0, n -> n - 1)"""
    h, w = img.shape
    der = np.zeros((h, w), np.float32)
    for y in range(h):
        for x in range(w):
            if axis == 0:
                der[y, x] = np.float32(img[_clamp(y + 1, h - 1), x]) - np.float32(img[_clamp(y - 1, h - 1), x])
            else:
                der[y, x] = np.float32(img[y, _clamp(x + 1, w - 1)]) - np.float32(img[y, _clamp(x - 1, w - 1)])
    out = np.zeros((h, w), np.float32)
    for y in range(h):
        for x in range(w):
            if axis == 0:
                a, c, b = der[y, _clamp(x - 1, w - 1)], der[y, x], der[y, _clamp(x + 1, w - 1)]
            else:
                a, c, b = der[_clamp(y - 1, h - 1), x], der[y, x], der[_clamp(y + 1, h - 1), x]
            out[y, x] = np.float32(np.float32(a + b) + np.float32(np.float32(2.0) * c))
    return out


def two_means_ref(values):
    """the split of the sorted values into a lower and an upper non-empty group with the smallest summed squared deviation
    from the group means; the lowest split index among equal minima.  Returns (mean_lo, mean_hi, cost)."""
    v = sorted(float(x) for x in values)
    n = len(v)
    best = None
    for k in range(1, n):
        slo = qlo = 0.0
        for x in v[:k]:
            slo += x
            qlo += x * x
        s = q = 0.0
        for x in v:
            s += x
            q += x * x
        shi, qhi = s - slo, q - qlo
        cost = (qlo - slo * slo / k) + (qhi - shi * shi / (n - k))
        if best is None or cost < best[2]:
            best = (slo / k, shi / (n - k), cost)
    return best


def gt_modes_ref(gt, radius=2.0, edge_threshold=0.5):
    """validate/cluster.py:25-64 on one (h, w) float32 image, with the deterministic 2-means in place of KMeans.
    Returns (modes (h, w, 2) float64, edges (h, w) bool)."""
    gt = np.asarray(gt, np.float32)
    h, w = gt.shape
    sy, sx = sobel_ref(gt, 0), sobel_ref(gt, 1)
    der = np.sqrt(sy * sy + sx * sx)                               # cluster.py:29, float32
    edges = der.astype(np.float64) > edge_threshold                # :30
    modes = np.zeros((h, w, 2))
    radius_int = math.ceil(radius)
    for y in range(h):
        for x in range(w):
            if not edges[y, x]:
                modes[y, x, :] = gt[y, x]                          # :38-40
                continue
            disps = []
            for dy in range(-radius_int, radius_int + 1):          # :46-53
                for dx in range(-radius_int, radius_int + 1):
                    if dy * dy + dx * dx <= radius * radius:
                        disps.append(gt[_clamp(y + dy, h - 1), _clamp(x + dx, w - 1)])
            if min(disps) == max(disps):
                modes[y, x, :] = float(disps[0])
            else:
                lo, hi, _ = two_means_ref(disps)
                modes[y, x] = sorted((lo, hi))                     # :60
    return modes, edges


def posterior_modes_ref(posterior, start, stop):
    """validate/multimodal.py:44-49 and :59-64 on one (n, h, w) posterior: the two strongest strict interior maxima (the lower
    bin among equal heights), as disparities, ascending; a missing mode is the one there is, none at all the first arg-max
    bin twice.  Returns (n_modes (h, w) int, disps (h, w, 2) float64)."""
    n, h, w = posterior.shape
    n_modes = np.zeros((h, w), np.int64)
    disps = np.zeros((h, w, 2))
    for y in range(h):
        for x in range(w):
            col = posterior[:, y, x]
            maxs = [j for j in range(1, n - 1) if col[j] > col[j - 1] and col[j] > col[j + 1]]      # :46-49
            maxs.sort(key=lambda j: (-col[j], j))
            n_modes[y, x] = min(len(maxs), 2)
            if not maxs:
                best = [int(np.argmax(col))] * 2
            elif len(maxs) == 1:
                best = [maxs[0]] * 2
            else:
                best = maxs[:2]
            for k, j in enumerate(sorted(best)):                   # :60-64
                disps[y, x, k] = float(j) / float(n - 1 if n > 1 else 1) * (stop - start) + start
    return n_modes, disps


def _reflect(i, n):
    m = i % (2 * n)
    return m if m < n else 2 * n - 1 - m


def gaussian_filter1d_ref(posterior, sigma=2.0):
    """scipy.ndimage.gaussian_filter1d(posterior, sigma, axis=0) on float32 input: float64 accumulation, float32 result"""
    n = posterior.shape[0]
    lw = int(4.0 * sigma + 0.5)
    wts = [math.exp(-0.5 / (sigma * sigma) * k * k) for k in range(-lw, lw + 1)]
    tot = 0.0
    for x in wts:
        tot += x
    wts = [x / tot for x in wts]
    out = np.zeros(posterior.shape, np.float32)
    for i in range(n):
        acc = np.zeros(posterior.shape[1:], np.float64)
        for t, k in enumerate(range(-lw, lw + 1)):
            acc = acc + wts[t] * posterior[_reflect(i + k, n)].astype(np.float64)
        out[i] = acc.astype(np.float32)
    return out


def mode_proportion_ref(posterior, sigma=2.0, outlier=0.1):
    """utils/modecnt.py:23-75 on one (n, h, w) float32 posterior.  Returns (mode_cnt (h, w) int, mode_prop (h, w) float32)."""
    sm = gaussian_filter1d_ref(posterior, sigma)                   # :24
    n, h, w = sm.shape
    mode_prop = np.zeros((h, w), np.float32)
    mode_cnt = np.zeros((h, w), np.int64)
    for y in range(h):
        for x in range(w):
            mins, maxs = [], []
            for i in range(1, n - 1):                              # :37-45
                left, center, right = float(sm[i - 1, y, x]), float(sm[i, y, x]), float(sm[i + 1, y, x])
                if left < center and right < center:
                    maxs.append((i, center))
                elif left > center and right > center:
                    mins.append((i, center))
            maxs = sorted(maxs, key=lambda e: (e[1], e[0]))        # :51 (a stable sort of a list in bin order)
            max_clean = [e for e in maxs if e[1] > maxs[-1][1] * outlier]      # :53-55
            mode_cnt[y, x] = len(max_clean) > 1                    # :61
            if len(max_clean) > 1:
                top_max = max_clean[-2:]                           # :64
                interval = sorted([top_max[0][0], top_max[1][0]])
                top_min = [e[1] for e in mins if interval[0] < e[0] < interval[1]]          # :68-69, all minima
                if top_min:
                    with np.errstate(divide='ignore'):
                        mode_prop[y, x] = np.float32(np.float64(top_max[0][1]) / np.float64(min(top_min)))   # :75
    return mode_cnt, mode_prop


def two_mode_error_ref(disps, n_modes, modes, gt, pred, margin=15, lb=False):
    """validate/multimodal.py:51-94 on one scene: [count, multimodal mse sum, multimodal badpix sum, unimodal mse sum, unimodal
    badpix sum, count with fewer than two modes] over the pixels inside the margin whose two gt modes differ"""
    h, w, _ = modes.shape
    out = [0.0] * 6
    for y in range(margin, h - margin):                            # :54-56
        for x in range(margin, w - margin):
            if modes[y, x, 0] == modes[y, x, 1]:
                continue
            g, d = float(gt[y, x]), disps[y, x]
            if lb:                                                 # :67-71
                mse = min((g - d[0]) ** 2.0, (g - d[1]) ** 2.0)
                bad = min(float(abs(g - d[0]) > BAD_PIX_T), float(abs(g - d[1]) > BAD_PIX_T))
            else:                                                  # :74-77
                mse = float(np.mean((d - modes[y, x]) ** 2.0))
                bad = float(np.mean(np.abs(d - modes[y, x]) > BAD_PIX_T))
            e = g - float(pred[y, x])                              # :80-81
            out[0] += 1.0
            out[1] += mse
            out[2] += bad
            out[3] += e * e
            out[4] += float(abs(e) > BAD_PIX_T)
            out[5] += float(n_modes[y, x] < 2)
    return out


def _auc(curve, step):
    auc = 0.0
    for i in range(len(curve) - 1):                                # sparsify.py:79-83
        auc += (curve[i] + curve[i + 1]) / 2.0 * step
    return auc


def _stable_first(keys, k):
    """the k pixels with the smallest key, equal keys in pixel order"""
    return sorted(range(len(keys)), key=lambda i: (keys[i], i))[:k]


def sparsification_ref(error, uncert, gt, result, step=0.01, badpix=False):
    """validate/sparsify.py:101-187 on one scene (flat float32 arrays).  Returns (frac, oracle, uncert, sparse_err, auc)."""
    n = gt.size
    diff = (np.abs(result - gt) > BAD_PIX_T).astype(float) if badpix else ((result - gt) ** 2.0).astype(float)
    fracts = np.arange(0.0, 1.000000001, step)
    loss = np.zeros((3, len(fracts)))
    mask_o, mask_u = np.zeros(n, bool), np.zeros(n, bool)          # :121-122, never cleared
    for i, fract in enumerate(fracts):
        loss[0, i] = 1.0 - fract
        if i == 0:
            continue
        if fract == 1.0:
            mask_o[...] = True
            mask_u[...] = True
        else:
            k = int(fract * n)
            mask_o[_stable_first(list(error), k)] = True
            mask_u[_stable_first(list(uncert), k)] = True
        with np.errstate(invalid='ignore', divide='ignore'):
            loss[1, i] = np.sum(diff * mask_o) / np.sum(mask_o)
            loss[2, i] = np.sum(diff * mask_u) / np.sum(mask_u)
    loss = loss[:, ::-1].copy()                                    # :164-170
    with np.errstate(invalid='ignore', divide='ignore'):
        loss[1:3] /= loss[1, 0]
    loss = np.delete(loss, -1, axis=1)
    err = loss[2] - loss[1]
    return loss[0], loss[1], loss[2], err, _auc(err, step)


def mode_prediction_ref(mode_prop, gt_modes, step=0.01):
    """validate/mm_prediction.py:43-140 on one scene.  Returns (frac, oracle, pred, sparse_err, auc)."""
    mask_gt = (gt_modes[:, :, 0] != gt_modes[:, :, 1]).flatten()   # :46
    prop = mode_prop.flatten()
    n = mask_gt.size
    error = ~mask_gt                                               # :58
    fracts = np.arange(0.0, 1.000000001, step)
    loss = np.zeros((3, len(fracts)))
    mask_o, mask_p = np.zeros(n, bool), np.zeros(n, bool)
    for i, fract in enumerate(fracts):
        loss[0, i] = 1.0 - fract
        if fract == 1.0:
            mask_o[...] = True
            mask_p[...] = True
        else:
            k = int(fract * n)
            mask_o[_stable_first([int(e) for e in error], k)] = True
            mask_p[_stable_first([-float(p) for p in prop], k)] = True
        with np.errstate(invalid='ignore', divide='ignore'):
            loss[1, i] = 1.0 - np.sum(mask_o.astype(float) * mask_gt.astype(float)) / np.sum(mask_gt.astype(float))   # :12-15
            loss[2, i] = 1.0 - np.sum(mask_p.astype(float) * mask_gt.astype(float)) / np.sum(mask_gt.astype(float))
    loss[0] = 1.0 - loss[0]                                        # :116
    with np.errstate(invalid='ignore', divide='ignore'):
        loss[1:3] /= loss[1, 0]
    loss = np.delete(loss, -1, axis=1)
    err = loss[2] - loss[1]
    return loss[0], loss[1], loss[2], err, _auc(err, step)


# ---- inputs shared by tests/test_multimodal_cpu.py and tests/test_gpu_multimodal.py: no decision sits on a rounding ----

FRAMES = [(1, 1), (1, 5), (2, 3), (5, 7), (33, 65), (3, 130)]
BINS = [1, 2, 3, 4, 9, 17, 18, 70, 108]
SMOOTH_GAP = 1e-4      # neighbouring smoothed bins differ by more than this, relative
# (frame, bins) of the device comparison: every bin count at one frame, every frame at the Ensamble's 70 bins, the largest
# frames at 108 and at the 17-bin window, and the smallest of both; batches of two, seed 100 + bins
POSTERIOR_CASES = ([((5, 7), s) for s in BINS] + [(f, 70) for f in FRAMES if f != (5, 7)]
                   + [((33, 65), 108), ((3, 130), 17), ((1, 1), 1), ((2, 3), 3)])


GT_STEP = 1.125        # every gt value is a whole multiple of it: on the grid of 1/8, and two different values are >= 1 apart


def make_gt(b, h, w, seed):
    """(b, h, w) float32, whole multiples of GT_STEP = 9/8: plateaus, and single pixels (no two of them adjacent, diagonals
    included) that stand one or two steps off their plateau, so neighbourhoods hold several distinct values.  Every value
    lies on the grid of 1/8 and every jump is at least 1.  Differences, Sobel sums and their squares are then exact in float32
    (multiples of 1/64 far below 2^24 / 64), so `sqrt(.) > 0.5` is `sum > 16/64` on exact numbers: no path can round across
    the edge threshold; and the float64 sums of the 2-means are exact too, so both paths divide the same numbers."""
    rng = np.random.RandomState(seed)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    out = np.zeros((b, h, w), np.float32)
    for i in range(b):
        cut_x, cut_y = rng.randint(0, w + 1), rng.randint(0, h + 1)
        plateau = rng.randint(1, 3) * (xs >= cut_x) - rng.randint(1, 3) * ((ys >= cut_y) & (xs % 11 < 6))
        single = ((ys + 2 * xs) % 5 == 0) & (rng.rand(h, w) < 0.6)
        steps = plateau + single * rng.choice([-2, -1, 1, 2], size=(h, w))
        out[i] = steps.astype(np.float32) * np.float32(GT_STEP)
    return out


def smooth_gap(smoothed):
    """smallest relative difference of neighbouring bins of (b, s, h, w) smoothed values, per pixel (inf for s == 1)"""
    if smoothed.shape[1] < 2:
        return np.full(smoothed[:, 0].shape, np.inf)
    a, c = smoothed[:, :-1].astype(np.float64), smoothed[:, 1:].astype(np.float64)
    return (np.abs(a - c) / np.maximum(np.abs(a), np.abs(c))).min(1)


def make_posterior(b, s, h, w, seed, smooth):
    """(b, s, h, w) float32, positive, one to three bumps per pixel under multiplicative noise, normalised over the bins.
    `smooth` is the smoothing under test's CPU form (multimodal.smooth_bins on numpy): pixels where two neighbouring smoothed
    bins come closer than SMOOTH_GAP are drawn again, so an extremum never hangs on the last bit of a sum."""
    rng = np.random.RandomState(seed)

    def draw(n):
        bins = np.arange(s, dtype=np.float64)[None, :]
        p = np.full((n, s), 0.02)
        for _ in range(3):
            centre, width = rng.uniform(0, s, (n, 1)), rng.uniform(1.0, 6.0, (n, 1))
            height = rng.uniform(0.2, 1.0, (n, 1)) * (rng.rand(n, 1) < 0.7)
            p = p + height * np.exp(-0.5 * ((bins - centre) / width) ** 2)
        p = p * rng.uniform(0.5, 1.5, (n, s))
        return (p / p.sum(1, keepdims=True)).astype(np.float32)

    post = draw(b * h * w).reshape(b, h, w, s).transpose(0, 3, 1, 2).copy()
    for _ in range(50):
        bad = smooth_gap(smooth(post)) <= SMOOTH_GAP
        if not bad.any():
            return post
        bi, yi, xi = np.nonzero(bad)
        post[bi, :, yi, xi] = draw(len(bi))
    raise AssertionError('make_posterior: could not separate the smoothed bins')


def zero_gap_posterior():
    """(1, 70, 1, 2): 17 raw zeros around bin 35 between two bumps, so exactly ONE smoothed bin is 0 and it is a strict
    minimum between the two maxima: mode_prop is IEEE inf.  The second pixel has the gap filled (finite)."""
    bins = np.arange(70, dtype=np.float64)
    p = 0.01 + np.exp(-0.5 * ((bins - 15) / 8.0) ** 2) + 0.6 * np.exp(-0.5 * ((bins - 55) / 8.0) ** 2)
    q = p.copy()
    p[27:44] = 0.0
    return np.stack([p, q], -1).reshape(1, 70, 1, 2).astype(np.float32)
