"""Shared inputs and restatements for the scene builder's tests (mmlf_amd/scenes.py): the seeded synthetic
centre view, the golden shapes of tests/golden/g15_texture_mask.npz, a float64 evaluation of the texture window, the
bounds both test files hold the float32 results to, and a numpy restatement of reference hci4d.py:141-241."""
import numpy as np
import torch

# (B, H, W, wsize, threshold) of tests/golden/g15_texture_mask.npz
GOLDEN_SHAPES = [
    (1, 64, 80, 23, .02),
    (2, 37, 53, 23, .02),        # two different images
    (1, 48, 48, 5, .02),
    (1, 40, 56, 3, .01),
    (1, 20, 22, 23, .02),        # a frame smaller than the window: all zero
    (1, 23, 23, 23, .02),        # one interior pixel
]
KINDS = ('float', 'dyadic')


def tag(B, H, W, wsize, kind):
    return f'{kind}.{B}x{H}x{W}.w{wsize}'


def centre(B, H, W, dyadic=False, seed=0):
    """(B,3,H,W) float32 in [0,1]: 0.5 + 0.004 sin(x/17) cos(y/13) on all three channels plus 0.07 x/(W-1) U(-1,1) per
    element -- textureless on the left, textured on the right, so both classes of the mask are present.  dyadic: rounded
    to multiples of 1/256, which makes every float32 partial sum of |x - c| exact."""
    rs = np.random.RandomState(15000 + seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    base = 0.5 + 0.004 * np.sin(x / 17.0) * np.cos(y / 13.0)
    amp = 0.07 * x / max(W - 1, 1)
    c = np.clip(base[None, None] + amp[None, None] * rs.uniform(-1.0, 1.0, size=(B, 3, H, W)), 0.0, 1.0)
    if dyadic:
        c = np.round(c * 256.0) / 256.0
    return c.astype(np.float32)


def window_sum64(center, wsize):
    """float64 (B,H,W) tensor on center's device: the sum over the zero-padded 3 * wsize^2 window of |x - c|, accumulated
    over the window offsets in float64 (exact for a dyadic centre)"""
    c = center.to(torch.float64)
    B, _, H, W = c.shape
    R = wsize // 2
    pad = torch.nn.functional.pad(c, (R, R, R, R))
    acc = torch.zeros((B, H, W), dtype=torch.float64, device=c.device)
    for dy in range(wsize):
        for dx in range(wsize):
            acc += (pad[:, :, dy:dy + H, dx:dx + W] - c).abs_().sum(1)
    return acc


def rel_bound(wsize):
    """relative error of a float32 sum of 3 * wsize^2 non-negative terms in any order (n - 1 additions), plus the rounding
    of a term and of the division: (3 wsize^2 + 2) 2^-24 (first order); 9.5e-5 at wsize 23"""
    return (3 * wsize * wsize + 2) * 2.0 ** -24


def interior(H, W, wsize):
    R = wsize // 2
    m = np.zeros((H, W), dtype=bool)
    if H > 2 * R and W > 2 * R:
        m[R:H - R, R:W - R] = True
    return m


BAND_CAP = 0.005          # share of interior pixels that may sit within the rounding band of the threshold


def check_mae(mae, center, wsize, what):
    """|mae32 - mae64| <= rel_bound * mae64 at every pixel, the zero-padded border included"""
    ref = (window_sum64(center, wsize) / float(3 * wsize * wsize)).cpu().numpy()
    got = mae.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == ref.shape, (what, got.dtype, got.shape)
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err / np.maximum(ref, 1e-300)).max()) if ref.max() > 0 else 0.0
    print(f'{what}: worst relative error {worst:.3e}, bound {rel_bound(wsize):.3e}')
    assert (err <= rel_bound(wsize) * ref).all(), (what, worst)


def check_mask_band(mask, golden, center, wsize, threshold, what):
    """mask == golden wherever |mae64 - float32(threshold)| exceeds rel_bound * threshold; the pixels inside that band may
    differ, and number at most BAND_CAP of the interior"""
    thr = float(np.float32(threshold))
    ref = (window_sum64(center, wsize) / float(3 * wsize * wsize)).cpu().numpy()
    got = mask.cpu().numpy() if isinstance(mask, torch.Tensor) else np.asarray(mask)
    assert got.shape == golden.shape, (what, got.shape, golden.shape)
    inner = interior(got.shape[-2], got.shape[-1], wsize)[None]
    band = (np.abs(ref - thr) <= rel_bound(wsize) * thr) & inner
    n_in = int(inner.sum()) * got.shape[0]
    print(f'{what}: {int(band.sum())} of {n_in} interior pixels in the band, '
          f'{int((got != golden).sum())} differ from the golden, ones {float(golden[:, inner[0]].mean()) if n_in else 0:.3f}')
    assert band.sum() <= BAND_CAP * n_in, (what, int(band.sum()), n_in)
    assert np.array_equal(got[~band], golden[~band]), (what, int((got != golden)[~band].sum()))


# ---------------------------------------------------------------- a numpy restatement of hci4d.py:141-241
def view_indices_ref(nviews):
    w, h = nviews
    us = [int(h / 2) * w + i for i in range(h)]
    vs = [int(w / 2) + w * i for i in range(h)]
    ids = list(reversed([w - i - 1 + w * i for i in range(h)]))
    dds = [i + w * i for i in range(h)]
    return us, vs, ids, dds


def assemble_ref(views, gt, mpi, mask, index, nviews, texture):
    """(h, v, i, d, center, gt, mpi, mask, index) in numpy from decoded `views` (N,H,W,3); `texture` is the (H,W) texture
    mask of the centre (held to the golden on its own)"""
    w, h = nviews
    if views.dtype == np.uint8:
        as_float = (views.astype(np.float64) * (1.0 / 255)).astype(np.float32)
    else:
        as_float = views.astype(np.float32)
    stacks = [np.stack([as_float[i] for i in idx]).transpose((0, 3, 1, 2)) for idx in view_indices_ref(nviews)]
    center = stacks[1][int(h / 2)].copy()
    gt = np.zeros_like(center[0]) if gt is None else np.asarray(gt, dtype=np.float32)
    if mpi is not None:
        m = np.flip(np.asarray(mpi), 0).copy().transpose((2, 3, 0, 1)).astype(np.float32)
        m[np.isnan(m)] = 0.0
        m = m[:12]
    else:
        m = np.zeros((1, 5, gt.shape[0], gt.shape[1]), dtype=np.float32)
        m[0, :3] = center
        m[0, 3] = 1.0
        m[0, 4] = gt
    msk = np.ones(gt.shape, dtype=np.int32) if mask is None else (np.asarray(mask) > 0).astype(np.int32)
    msk = msk * np.asarray(texture, dtype=np.int32)
    return (*stacks, center, gt, m, msk, np.atleast_1d(index))


def scene_inputs(nviews, H, W, seed, dtype=np.uint8, planes=2):
    """decoded views (N,H,W,3), gt (H,W), mpi (H,W,planes,5) with one NaN, mask (H,W) uint8 with zeros: textured towards the
    right like centre()"""
    rs = np.random.RandomState(15500 + seed)
    w, h = nviews
    N = w * h
    x = np.arange(W, dtype=np.float64)[None, None, :, None] / max(W - 1, 1)
    v = np.clip(0.5 + 0.2 * x * rs.uniform(-1.0, 1.0, size=(N, H, W, 3)), 0.0, 1.0)
    views = np.round(v * 255.0).astype(np.uint8) if dtype == np.uint8 else v.astype(np.float32)
    gt = (4.0 * rs.uniform(size=(H, W)) - 2.0).astype(np.float32)
    mpi = rs.uniform(0.0, 1.0, size=(H, W, planes, 5)).astype(np.float32)
    mpi[H // 2, W // 3, 0, 2] = np.nan
    mask = (255 * (rs.uniform(size=(H, W)) > 0.2)).astype(np.uint8)
    return views, gt, mpi, mask


ASSEMBLE_CASES = [
    dict(nviews=(3, 3), dtype=np.uint8, gt=True, mpi=2, mask=True),
    dict(nviews=(3, 3), dtype=np.float32, gt=False, mpi=0, mask=False),
    dict(nviews=(5, 3), dtype=np.uint8, gt=True, mpi=13, mask=False),
    dict(nviews=(3, 3), dtype=np.float32, gt=True, mpi=0, mask=True),
]


def assemble_case(assemble_scene, case, device, H=26, W=31, wsize=5, seed=0):
    views, gt, mpi, mask = scene_inputs(case['nviews'], H, W, seed, case['dtype'], planes=max(case['mpi'], 1))
    gt = gt if case['gt'] else None
    mpi = mpi if case['mpi'] else None
    mask = mask if case['mask'] else None
    out = assemble_scene(views, gt, mpi, mask, index=7, nviews=case['nviews'], wsize=wsize, device=device)
    return (views, gt, mpi, mask), out


def case_id(c):
    return f"{c['nviews'][0]}x{c['nviews'][1]}-{np.dtype(c['dtype']).name}-mpi{c['mpi']}"
