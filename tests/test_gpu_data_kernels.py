"""The kernels that decide what the network is trained on and which numbers `validate` reports -- shift_kernel
(mmlf_shift_views), patch_stacks_kernel / patch_planes_kernel (mmlf_patch_gather), patch_contrast_kernel (mmlf_patch_contrast),
ensamble_reduce_kernel (mmlf_ensamble_reduce) and lmm_to_discrete_kernel (mmlf_lmm_to_discrete) of csrc/elementwise.hip -- each
called directly through its C entry point and held to the numpy references of tests_helpers (pinned to the reference's goldens
by tests/test_data_refs_cpu.py).  Every output lies between guard bands and is pre-filled with NaN (-1 for the mask).

  * the shear, the patch gather and Contrast are float32 restatements of the reference, operation for operation: the kernels must
    give the reference's BITS.  Contrast's mean is a double sum in arbitrary order here and a float32 pairwise sum in numpy: the
    sum is held to math.fsum within n 2^-52, and the Contrast output to the bits that ONE of the three float32 numbers around
    float32(fsum / n) gives;
  * the arg-min outputs of the ensemble reduction are exact (the first minimum); its posterior and the discretised mixture are
    held to float64 within the per-element bounds of ensamble_reduce_ref and lmm_ref, which count the roundings of the
    kernel's path under the ASSUMPTION of a device expf good to 1 ulp.  The bounds are not tuned: a miss is a finding about the
    kernel or about expf.

Headroom of the first run on an MI355X: see EXPERIMENTS.md section 4.16."""
import math
import random

import numpy as np
import pytest
import torch

from conftest import load_golden
from tests_helpers import (RATIOS, _Pool, contrast_ref, ensamble_reduce_ref, lmm_edges, lmm_mass_ref, lmm_ref, patch_ref,
                           shift_ref, shift_table_ref)

pytestmark = pytest.mark.gpu
NAN = float('nan')


def _dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _api():
    from mmlf_amd import _lib
    _lib.load()
    return _lib.call, _lib.ptr, _lib.stream_ptr


@pytest.fixture(scope='module', autouse=True)
def _report_ratios():
    yield
    for k in sorted(RATIOS):
        print(f'\n[data kernels headroom] {k}: max error / bound = {RATIOS[k]:.4f}', end='')
    print()
    RATIOS.clear()


def _bits(got, want, what):
    """the same bits, element for element (so -0.0 is not 0.0 and a NaN left in the output fails)"""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    view = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    bad = np.ascontiguousarray(got).view(view) != want.view(view)
    if bad.any():
        k = int(np.argmax(bad.reshape(-1)))
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.size} elements differ; flat index {k} ({np.unravel_index(k, bad.shape)}) '
                             f'holds {got.reshape(-1)[k]!r}, reference {want.reshape(-1)[k]!r}')


def _within(got, ref, bound, key, what):
    """|got - ref| <= bound element-wise (a NaN fails); the largest ratio is kept for the headroom report"""
    got = got.detach().cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref)
    ratio = err / bound
    worst = float(ratio.max()) if not np.isnan(ratio).any() else float('inf')
    RATIOS[key] = max(RATIOS.get(key, 0.0), worst)
    ok = err <= bound
    if not ok.all():
        k = int(np.argmax(~ok.reshape(-1)))
        raise AssertionError(f'{what} [{key}]: {int((~ok).sum())} of {ok.size} over the bound, worst ratio {worst}; first at '
                             f'{np.unravel_index(k, ok.shape)}: got {got.reshape(-1)[k]!r}, reference {ref.reshape(-1)[k]!r}, '
                             f'bound {bound.reshape(-1)[k]!r}')


# ------------------------------------------------------------------ mmlf_shift_views
# (views, H, W): the smallest frame | an even view count (half = 1: no view pair symmetric about zero shift) | one row (every
# vertical roll is the identity clamp) and W > 256 (a thread of the 256-wide block takes a second column) | one column | W just
# past 256 | a large view count | the golden's frame
SHIFT_FRAMES = [(1, 1, 1), (2, 5, 6), (3, 1, 300), (3, 300, 1), (5, 7, 257), (11, 5, 6), (9, 12, 14)]
SHIFT_BASE_DISPS = [0.0, -0.0, 0.3, -0.3, 1.0, -1.0, 2.5]            # +-1.0: alpha == 0 and s1 = s0 +- 1


def shift_disps(views, H, W):
    """the base list and, where a view is sheared at all (half > 0), three disparities per extent n = W, n = H that give the
    outermost view (k = 0, at -half) an integer shift s0 of n - 1, n, n + 1 (and s1 one further): the last wrap, and the
    identity clamp of s1 alone and of both.  Returns (disps, [(index, n, m)])"""
    disps, edge = list(SHIFT_BASE_DISPS), []
    half = int(views / 2)
    if half:
        for n, sign in ((W, 1.0), (H, -1.0)):
            for m in (n - 1, n, n + 1):
                edge.append((len(disps), n, m))
                disps.append(sign * (m + 0.5) / half)
    return disps, edge


@pytest.mark.parametrize('frame', SHIFT_FRAMES, ids=lambda f: 'x'.join(map(str, f)))
def test_shift_views_gives_the_bits_of_the_reference(frame):
    from mmlf_amd.ensamble import shift_table
    call, ptr, stream = _api()
    dev = _dev()
    views, H, W = frame
    disps, edge = shift_disps(views, H, W)
    S = len(disps)
    tab_s, tab_w = shift_table_ref(disps, views)
    prod = shift_table(disps, views)                                     # what the product passes is the same table
    assert np.array_equal(prod[0], tab_s) and np.array_equal(prod[1], tab_w)
    for idx, n, m in edge:
        assert abs(int(tab_s[idx, 0, 0])) == m and abs(int(tab_s[idx, 0, 1])) == m + 1, (idx, n, m, tab_s[idx, 0])
    n = views * 3 * H * W
    vals = np.random.RandomState(n).permutation(4 * n).astype(np.float32) / np.float32(4 * n)     # distinct, in [0, 1)
    assert 4 * n < 2 ** 24 and len(np.unique(vals)) == 4 * n
    stacks = [vals[i * n:(i + 1) * n].reshape(views, 3, H, W) for i in range(4)]
    want = shift_ref(stacks, disps)
    pool = _Pool(dev)
    src = [torch.from_numpy(s).to(dev) for s in stacks]
    outs = [pool.new(S * n, NAN).view(S, views, 3, H, W) for _ in range(4)]
    ts, tw = torch.from_numpy(tab_s).to(dev), torch.from_numpy(tab_w).to(dev)
    call('mmlf_shift_views', *[ptr(t) for t in src], *[ptr(t) for t in outs], ptr(ts), ptr(tw), S, views, H, W, stream())
    torch.cuda.synchronize()
    pool.check(f'shift {frame}')
    for i, name in enumerate('hvid'):
        for k, d in enumerate(disps):
            _bits(outs[i][k], want[i][k], f'shift {frame} stack {name} disp {d!r}')


# ------------------------------------------------------------------ mmlf_patch_gather / mmlf_patch_contrast
# (V, P, Hf, Wf, ps, factors, disparities): the pipeline's own shape | one view, one plane | no planes: null mpi / o_mpi |
# ps = 129 > the 128-thread block: a thread takes two columns | f = 2 on a 9 x 7 frame, disp = +-1: the outer views' shifts
# reach Wd = 4 and Hd = 5, so the identity clamp and the wrap both occur | a one-pixel patch
PATCH_DISPS = (0.37, -0.81, 1.0, -1.0)
PATCH_CASES = {
    'pipeline': (9, 2, 40, 44, 6, (1, 2, 3), PATCH_DISPS),
    'one-view': (1, 1, 20, 23, 5, (1, 2, 3), PATCH_DISPS),
    'no-planes': (3, 0, 31, 29, 7, (1, 2, 3), PATCH_DISPS),
    'two-columns': (9, 3, 150, 157, 129, (1,), PATCH_DISPS),
    'clamp-and-wrap': (9, 2, 9, 7, 3, (2,), (1.0, -1.0)),
    # at disp = +-1 a shift of exactly Wd is the identity either way and s1 has weight 0: a kernel WITHOUT the clamp passes that
    # case (tried).  disp = +-1.3: the outer views' s0 = 5 lies past Wd = 4 and s1 = 6 past Hd = 5, with weights 0.8 and 0.2
    'clamp-past-the-frame': (9, 2, 9, 7, 3, (2,), (1.3, -1.3)),
    'one-pixel': (5, 1, 12, 12, 1, (1, 2, 3), PATCH_DISPS),
}
PATCH_B = 8


def patch_params(case, picks=range(PATCH_B)):
    """explicit parameters of the samples `picks` of a case: sample b has rot = b % 4, flags = b (every value 0 - 7 once), the
    factors in turn, the disparities in turn over the samples that shear (odd b), brightness 0.1 and 1.9, scene 1 - b % 2 of
    two, a colour matrix of its own, and a crop origin that walks from 0 to the last position the down-sampled frame allows"""
    from oracle import oracle as orc
    V, P, Hf, Wf, ps, factors, disps = PATCH_CASES[case]
    out = []
    for b in picks:
        f = factors[b % len(factors)]
        Hd, Wd = -(-Hf // f), -(-Wf // f)
        assert ps <= Hd and ps <= Wd
        out.append(dict(ps=ps, scene=(b + 1) % 2, f=f, disp=disps[(b // 2) % len(disps)], rot=b % 4, flags=b % 8,
                        y0=(Hd - ps) * ((b + b // 3) % 3) // 2, x0=(Wd - ps) * ((2 * b + 1 + b // 3) % 3) // 2,
                        mat=orc.draw_redist_matrix(random.Random(1000 + b)), bright=(0.1, 1.9)[b % 2]))
    return out


def test_patch_cases_hold_what_they_exist_for():
    """(needs no launch, but belongs to the lists above)"""
    for case, (V, P, Hf, Wf, ps, factors, disps) in PATCH_CASES.items():
        ps_ = patch_params(case)
        assert {p['flags'] for p in ps_} == set(range(8)) and {p['rot'] for p in ps_} == {0, 1, 2, 3}
        assert {p['f'] for p in ps_} == set(factors) and {p['disp'] for p in ps_} == set(disps)
        assert {p['scene'] for p in ps_} == {0, 1} and {p['bright'] for p in ps_} == {0.1, 1.9}
        for p in ps_:
            assert p['y0'] + ps <= -(-Hf // p['f']) and p['x0'] + ps <= -(-Wf // p['f'])
        assert any(p['y0'] + ps == -(-Hf // p['f']) for p in ps_) and any(p['x0'] + ps == -(-Wf // p['f']) for p in ps_)
    assert any(Hf % f or Wf % f for _, _, Hf, Wf, _, fs, _ in PATCH_CASES.values() for f in fs)
    assert PATCH_CASES['two-columns'][4] > 128 and PATCH_CASES['no-planes'][1] == 0
    # clamp-and-wrap: under disp = +-1 the outermost views' shifts are 4 = Wd (identity) and s1 = 5 = Hd, the others wrap
    tab_s, _ = shift_table_ref([1.0], 9)
    assert sorted({abs(int(s)) for s in tab_s[0, :, 0]}) == [0, 1, 2, 3, 4] and int(np.abs(tab_s[0, :, 1]).max()) == 5
    tab_s, tab_w = shift_table_ref([1.3], 9)
    assert abs(int(tab_s[0, 0, 0])) == 5 and abs(int(tab_s[0, 0, 1])) == 6 and 0.1 < tab_w[0, 0, 1] < 0.3
    assert abs(int(tab_s[0, 1, 0])) == 3 and abs(int(tab_s[0, 1, 1])) == 4       # s1 = Wd with a weight: the wrap's last step


_SCENES = {}


def _scenes(case):
    """two scenes of the case's frame (computed once), and their device copies laid out as PatchPipeline keeps them"""
    from mmlf_amd import synth
    if case not in _SCENES:
        V, P, Hf, Wf = PATCH_CASES[case][:4]
        scenes = [synth.synth_scene(40 + s, Hf, Wf, V, P) for s in range(2)]
        dev = _dev()
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)   # noqa: E731
        d = dict(stacks=torch.stack([torch.stack([f32(s[k]) for k in range(4)]) for s in scenes]),
                 center=torch.stack([f32(s[4]) for s in scenes]), gt=torch.stack([f32(s[5]) for s in scenes]),
                 mpi=torch.stack([f32(s[6]) for s in scenes]) if P else None,
                 mask=torch.stack([torch.from_numpy(np.ascontiguousarray(s[7]).astype(np.int32)).to(dev) for s in scenes]))
        _SCENES[case] = (scenes, d)
    return _SCENES[case]


_PATCH_REFS = {}


def _patch_refs(case, picks):
    key = (case, tuple(picks))
    if key not in _PATCH_REFS:
        scenes, _ = _scenes(case)
        params = patch_params(case, picks)
        _PATCH_REFS[key] = (params, [patch_ref(scenes[p['scene']], p) for p in params])
    return _PATCH_REFS[key]


def _gather(case, params, with_sum):
    """one mmlf_patch_gather launch -> (pool, o_stacks (4,B,V,3,ps,ps), o_center, o_gt, o_mpi or None, o_mask, mean_sum or None)"""
    from mmlf_amd import patches
    call, ptr, stream = _api()
    dev = _dev()
    V, P, Hf, Wf, ps = PATCH_CASES[case][:5]
    _, d = _scenes(case)
    B = len(params)
    ip, fp, mat = np.zeros((B, 8), np.int32), np.zeros((B, 4), np.float32), np.zeros((B, 9), np.float64)
    for b, p in enumerate(params):
        ip[b, :6] = (p['scene'], p['f'], p['y0'], p['x0'], p['rot'], p['flags'])
        fp[b, :3] = (float(p['f']), p['disp'], p['bright'])
        mat[b] = np.asarray(p['mat']).reshape(-1)
    tab_s, tab_w = shift_table_ref([p['disp'] for p in params], V)
    up = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
    ins = [up(a) for a in (ip, fp, tab_s, tab_w, mat, patches.rotation_sources(V))]
    pool = _Pool(dev)
    o_st = pool.new(4 * B * V * 3 * ps * ps, NAN).view(4, B, V, 3, ps, ps)
    o_c = pool.new(B * 3 * ps * ps, NAN).view(B, 3, ps, ps)
    o_gt = pool.new(B * ps * ps, NAN).view(B, ps, ps)
    o_mpi = pool.new(B * P * 5 * ps * ps, NAN).view(B, P, 5, ps, ps) if P else None
    o_mask = pool.new(B * ps * ps, -1, torch.int32).view(B, ps, ps)
    msum = pool.new(B, 0.0, torch.float64) if with_sum else None
    call('mmlf_patch_gather', ptr(d['stacks']), ptr(d['center']), ptr(d['gt']), ptr(d['mpi']), ptr(d['mask']), 2, V, P, Hf, Wf,
         *[ptr(t) for t in ins], ptr(o_st), ptr(o_c), ptr(o_gt), ptr(o_mpi), ptr(o_mask), ptr(msum), B, ps, stream())
    torch.cuda.synchronize()
    pool.check(f'patch_gather {case}')
    return pool, o_st, o_c, o_gt, o_mpi, o_mask, msum


def _check_gather(case, params, refs, o_st, o_c, o_gt, o_mpi, o_mask, what):
    P = PATCH_CASES[case][1]
    for b, (p, ref) in enumerate(zip(params, refs)):
        tag = f'{what} {case} sample {b} (f={p["f"]} disp={p["disp"]} rot={p["rot"]} flags={p["flags"]} at {p["y0"]},{p["x0"]})'
        for k, name in enumerate('hvid'):
            _bits(o_st[k, b], ref[k], f'{tag} stack {name}')
        _bits(o_c[b], ref[4], f'{tag} center')
        _bits(o_gt[b], ref[5], f'{tag} gt')
        if P:
            _bits(o_mpi[b], ref[6], f'{tag} mpi')
        else:
            assert ref[6].size == 0
        _bits(o_mask[b], ref[7].astype(np.int32), f'{tag} mask')


def _check_sum(msum, refs, what):
    """mean_sum[b] against math.fsum of the reference's horizontal stack: n double additions in arbitrary order of
    non-negative numbers lose at most n 2^-52 of the sum"""
    got = msum.cpu().numpy()
    for b, ref in enumerate(refs):
        h = ref[0].astype(np.float64).reshape(-1)
        exact = math.fsum(h.tolist())
        assert abs(got[b] - exact) <= h.size * 2.0 ** -52 * abs(exact), (what, b, got[b], exact)


@pytest.mark.parametrize('case', list(PATCH_CASES))
def test_patch_gather_gives_the_bits_of_the_reference(case):
    picks = list(range(PATCH_B))
    params, refs = _patch_refs(case, picks)
    # without mean_sum: every output, and nothing else written
    _, o_st, o_c, o_gt, o_mpi, o_mask, _ = _gather(case, params, False)
    _check_gather(case, params, refs, o_st, o_c, o_gt, o_mpi, o_mask, 'mean_sum NULL')
    # with it zeroed
    _, o_st, o_c, o_gt, o_mpi, o_mask, msum = _gather(case, params, True)
    _check_gather(case, params, refs, o_st, o_c, o_gt, o_mpi, o_mask, 'mean_sum zeroed')
    _check_sum(msum, refs, f'mean_sum {case}')


CONTRAST_ALPHAS = (0.1, 1.0, 1.9)
CONTRAST_PICKS = (7, 2, 5)                                   # flags 7, 2, 5; rot 3, 2, 1; both scenes


@pytest.mark.parametrize('case', ['pipeline', 'two-columns'])
def test_patch_contrast_gives_the_bits_of_the_reference(case):
    call, ptr, stream = _api()
    V, ps = PATCH_CASES[case][0], PATCH_CASES[case][4]
    params, refs = _patch_refs(case, CONTRAST_PICKS)
    B = len(params)
    pool, o_st, o_c, o_gt, o_mpi, o_mask, msum = _gather(case, params, True)
    _check_gather(case, params, refs, o_st, o_c, o_gt, o_mpi, o_mask, 'before Contrast')
    _check_sum(msum, refs, f'mean_sum {case}')
    alpha = np.array([(a, 1.0 - a) for a in CONTRAST_ALPHAS], np.float32)         # float32(alpha), float32(1 - alpha)
    al = torch.from_numpy(alpha).to(o_st.device)
    call('mmlf_patch_contrast', ptr(o_st), ptr(o_c), ptr(msum), ptr(al), B, V, ps, stream())
    torch.cuda.synchronize()
    pool.check(f'patch_contrast {case}')
    _bits(o_gt, np.stack([r[5] for r in refs]), 'Contrast leaves gt alone')
    _bits(o_mask, np.stack([r[7] for r in refs]).astype(np.int32), 'Contrast leaves the mask alone')
    got_st, got_c = o_st.cpu().numpy(), o_c.cpu().numpy()
    n = V * 3 * ps * ps
    for b, (ref, a) in enumerate(zip(refs, CONTRAST_ALPHAS)):
        m = np.float32(math.fsum(ref[0].astype(np.float64).reshape(-1).tolist()) / n)
        fits = []
        for mean32 in (np.nextafter(m, np.float32(-np.inf)), m, np.nextafter(m, np.float32(np.inf))):
            st, c = contrast_ref(ref[:4], ref[4], a, mean32)
            fits.append(all(np.array_equal(got_st[k, b].view(np.uint32), st[k].view(np.uint32)) for k in range(4))
                        and np.array_equal(got_c[b].view(np.uint32), c.view(np.uint32)))
        assert any(fits), (case, b, a, 'no float32 mean next to fsum / n gives the bits of the stacks and the centre', fits)


# ------------------------------------------------------------------ mmlf_ensamble_reduce
# (S, B, H, W): the smallest | two members | B > 1 and H W no multiple of the 64-thread block | the validation's member count |
# 540000 pixels: past 8192 blocks of 64, a thread takes a second pixel
REDUCE_SHAPES = [(1, 1, 1, 1), (2, 1, 1, 3), (7, 3, 5, 13), (70, 1, 9, 31), (2, 1, 600, 900)]


def _reduce(means, logvars, grid):
    """one mmlf_ensamble_reduce launch on numpy inputs -> (mean, logvar, posterior) device tensors, guard bands checked"""
    call, ptr, stream = _api()
    dev = _dev()
    S, B, H, W = means.shape
    pool = _Pool(dev)
    m, lv, g = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (means, logvars, grid)]
    mean, logvar = pool.new(B * H * W, NAN).view(B, H, W), pool.new(B * H * W, NAN).view(B, H, W)
    post = pool.new(B * S * H * W, NAN).view(B, S, H, W)
    call('mmlf_ensamble_reduce', ptr(m), ptr(lv), ptr(g), ptr(mean), ptr(logvar), ptr(post), S, B, H, W, stream())
    torch.cuda.synchronize()
    pool.check(f'ensamble_reduce {means.shape}')
    return mean, logvar, post


def _reduce_inputs(shape, lo, hi, seed):
    """means in [-4, 4]; log-variances: per pixel a random permutation of S distinct values in [lo, hi] (no ties)"""
    S, B, H, W = shape
    rs = np.random.RandomState(seed)
    vals = np.sort(rs.uniform(lo, hi, S).astype(np.float32))
    assert len(np.unique(vals)) == S
    perm = np.argsort(rs.uniform(size=(S, B, H, W)), 0)
    means = rs.uniform(-4, 4, (S, B, H, W)).astype(np.float32)
    return means, vals[perm], np.linspace(-3.5, 3.5, S).astype(np.float32)


def _check_reduce(means, logvars, grid, key, what, expect_idx=None):
    idx, mean_ref, logvar_ref, ref, bound = ensamble_reduce_ref(means, logvars, grid)
    if expect_idx is not None:
        assert (idx == expect_idx).all()
    mean, logvar, post = _reduce(means, logvars, grid)
    _bits(mean, mean_ref, f'{what} mean')
    _bits(logvar, logvar_ref, f'{what} logvar')
    _within(post, ref, bound, key, f'{what} posterior')


@pytest.mark.parametrize('shape', REDUCE_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_ensamble_reduce_against_float64(shape):
    means, logvars, grid = _reduce_inputs(shape, -8.0, 2.0, sum(shape))
    _check_reduce(means, logvars, grid, 'ensemble posterior', f'reduce {shape}')


def test_ensamble_reduce_at_very_small_variances():
    """log-variances in [-12, -6]: |t| runs into the thousands and terms underflow"""
    means, logvars, grid = _reduce_inputs((7, 3, 5, 13), -12.0, -6.0, 11)
    _check_reduce(means, logvars, grid, 'ensemble posterior, small variances', 'reduce small variances')


def test_ensamble_reduce_takes_the_first_of_tied_minima():
    S, B, H, W = 4, 2, 3, 5
    rs = np.random.RandomState(2)
    means = rs.uniform(-4, 4, (S, B, H, W)).astype(np.float32)
    logvars = rs.uniform(-1, 2, (S, B, H, W)).astype(np.float32)
    logvars[1] = logvars[3] = rs.uniform(-8, -2, (B, H, W)).astype(np.float32)
    assert (means[1] != means[3]).all() and (logvars[1] < np.minimum(logvars[0], logvars[2])).all()
    _check_reduce(means, logvars, np.linspace(-3.5, 3.5, S).astype(np.float32), 'ensemble posterior', 'reduce ties', expect_idx=1)


def test_ensamble_reduce_on_the_golden_members():
    from test_data_refs_cpu import TIED_SHARE_MAX, tied_pixels
    g = load_golden('g4_ensamble.npz')
    means, logvars = g['means'], g['logvars']
    grid = np.linspace(-3.5, 3.5, means.shape[0]).astype(np.float32)
    mean, logvar, post = _reduce(means, logvars, grid)
    tied = tied_pixels(logvars)
    assert float(tied.mean()) <= TIED_SHARE_MAX
    _bits(logvar, g['logvar'], 'golden logvar')
    mean = mean.cpu().numpy()
    assert np.array_equal(mean[~tied].view(np.uint32), g['mean'][~tied].view(np.uint32))
    _, _, _, ref, bound = ensamble_reduce_ref(means, logvars, grid)
    _within(post, ref, bound, 'ensemble posterior, golden members', 'golden posterior')


# ------------------------------------------------------------------ mmlf_lmm_to_discrete
# (S, B, n_bins, HW): the smallest | the validation's bins, B > 1 | one pixel per image | many members, few bins | 2.16 M
# outputs: past 8192 blocks of 256, a thread takes a second output
LMM_SHAPES = [(1, 1, 1, 1), (5, 2, 108, 252), (3, 3, 7, 1), (70, 1, 7, 33), (1, 1, 108, 20000)]


def _lmm(means, logvars, edges):
    """one mmlf_lmm_to_discrete launch on numpy inputs (S, B, 1, HW) -> (B, n_bins, 1, HW) float64 device tensor"""
    call, ptr, stream = _api()
    dev = _dev()
    S, B, _, HW = means.shape
    n_bins = len(edges) - 1
    pool = _Pool(dev)
    m, lv, e = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (means, logvars, np.asarray(edges, np.float64))]
    out = pool.new(B * n_bins * HW, NAN, torch.float64).view(B, n_bins, 1, HW)
    call('mmlf_lmm_to_discrete', ptr(m), ptr(lv), ptr(e), ptr(out), S, B, n_bins, HW, stream())
    torch.cuda.synchronize()
    pool.check(f'lmm_to_discrete {means.shape} {n_bins}')
    return out


@pytest.mark.parametrize('shape', LMM_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_lmm_to_discrete_against_float64(shape):
    """every bin within the bound of lmm_ref.  The bin masses of an image add up to cdf(last edge) - cdf(first edge) of the
    mixture within 1e-12: the mixture is the one the kernel evaluates, whose variances are the DEVICE's expf (numpy's float32 exp
    may differ from it in the last place, which moves that difference by some 1e-8), so the right-hand side is the kernel's own
    answer for one bin from the first edge to the last -- itself held to lmm_ref's bound for those two edges."""
    S, B, n_bins, HW = shape
    rs = np.random.RandomState(S * 1000 + n_bins)
    means = rs.uniform(-4, 4, (S, B, 1, HW)).astype(np.float32)               # some lie outside every bin
    logvars = rs.uniform(-8, 2, (S, B, 1, HW)).astype(np.float32)
    edges = lmm_edges(n_bins, -3.5, 3.5)
    ref, bound = lmm_ref(means, logvars, edges)
    got = _lmm(means, logvars, edges)
    _within(got, ref, bound, 'mixture', f'lmm {shape}')
    ends = edges[[0, -1]]
    ref1, bound1 = lmm_ref(means, logvars, ends)
    whole = _lmm(means, logvars, ends)
    _within(whole, ref1, bound1, 'mixture', f'lmm {shape}, one bin over all edges')
    total, whole = got.sum(1).cpu().numpy(), whole[:, 0].cpu().numpy()
    assert (np.abs(total - whole) <= 1e-12).all(), (shape, float(np.abs(total - whole).max()))
    print(f'\n[lmm {shape}] sum of the bins against the one-bin launch: max |diff| = {float(np.abs(total - whole).max()):.3e}; '
          f'against numpy-exp mass: {float(np.abs(total - lmm_mass_ref(means, logvars, edges)).max()):.3e}', end='')


def test_metrics_entry_points_match_their_cpu_branches():
    """metrics.lmm_to_discrete and metrics.laplace_to_discrete on CUDA tensors, B = 2, a non-contiguous logvars view, against
    the CPU branch of the same functions (torch's float32 exp on the host: another exponential good to 1 ulp)"""
    from mmlf_amd import metrics
    dev = _dev()
    S, B, H, W, n_bins = 5, 2, 6, 7, 108
    rs = np.random.RandomState(8)
    means = torch.from_numpy(rs.uniform(-4, 4, (S, B, H, W)).astype(np.float32))
    wide = torch.from_numpy(rs.uniform(-8, 2, (S, B, H, 2 * W)).astype(np.float32))
    logvars = wide[..., ::2]
    assert not logvars.is_contiguous()
    edges = metrics._bin_edges(n_bins, -3.5, 3.5, torch.device('cpu')).numpy()
    _, bound = lmm_ref(means.numpy(), logvars.numpy(), edges)
    cpu = metrics.lmm_to_discrete(n_bins, -3.5, 3.5, means, logvars)
    dv = wide.to(dev)[..., ::2]
    assert not dv.is_contiguous()
    got = metrics.lmm_to_discrete(n_bins, -3.5, 3.5, means.to(dev), dv)
    assert got.dtype == torch.float64 and got.shape == (B, n_bins, H, W)
    _within(got, cpu.numpy(), bound, 'mixture, through metrics', 'metrics.lmm_to_discrete')
    _, bound1 = lmm_ref(means.numpy()[:1], logvars.numpy()[:1], edges)
    cpu1 = metrics.laplace_to_discrete(n_bins, -3.5, 3.5, means[0], logvars[0])
    got1 = metrics.laplace_to_discrete(n_bins, -3.5, 3.5, means[0].to(dev), dv[0])
    assert not dv[0].is_contiguous() and got1.shape == (B, n_bins, H, W)
    _within(got1, cpu1.numpy(), bound1, 'mixture, through metrics', 'metrics.laplace_to_discrete')
