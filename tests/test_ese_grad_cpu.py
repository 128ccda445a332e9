"""The Ensamble's gradients without a GPU: the third library (libmmlf_ese_hip.so: what it exports, its ABI number, its
argument checks, its kernels' resources), the two ABIs beside it untouched, the float64 restatement of tests/ese_grad_refs.py
against the reference's own autograd (tests/golden/g14_ensamble_grad.npz), the formulas of include/mmlf_ese_hip.h against
float64 autograd, and the conditioning of the end-to-end cases tests/test_gpu_ese_grad.py runs.

The reference's Ensamble (mmlf/model/ensamble.py:40-118) is torch code over torch.cat, gather and a sum of Laplace densities:
autograd differentiates its five outputs in the four stacks and in the model's parameters."""
import ctypes
import inspect
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import ese_grad_refs as refs
from conftest import ROOT, load_golden
from mmlf_amd import _lib
from mmlf_amd.csrc import build
from mmlf_amd.ensamble import Ensamble, shift_table

needs_hipcc = pytest.mark.skipif(not os.path.exists(build.HIPCC), reason='no hipcc')


# ------------------------------------------------------------------------------------------------ the third library
def test_the_other_two_abis_are_untouched():
    assert len(_lib.SIGNATURES) == 73
    assert not any(name.startswith('mmlf_ese_') for name in list(_lib.SIGNATURES) + list(_lib.EVAL_SIGNATURES))
    assert set(_lib.EVAL_SIGNATURES) == {'mmlf_eval_last_error', 'mmlf_eval_abi_version', 'mmlf_eval_gt_modes',
                                         'mmlf_eval_posterior_modes', 'mmlf_eval_two_mode_error'}
    assert _lib.EVAL_ABI_VERSION == 1
    assert build.SOURCES == ['conv.hip', 'wgrad.hip', 'elementwise.hip'] and build.EVAL_SOURCES == ['evaluate.hip']
    assert build.ESE_SOURCES == ['ensamble_grad.hip']
    assert not any('ensamble' in d or 'ese' in d for d in build.HASHED + build.SOURCES + build.EVAL_SOURCES)
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert set(_lib.ESE_SIGNATURES) == {'mmlf_ese_last_error', 'mmlf_ese_abi_version', 'mmlf_ese_reduce_bwd',
                                        'mmlf_ese_unshift_sum'}
    assert _lib.ESE_SIGNATURES['mmlf_ese_reduce_bwd'] == (i, [vp] * 8 + [i] * 4 + [vp])
    assert _lib.ESE_SIGNATURES['mmlf_ese_unshift_sum'] == (i, [vp, i, i, vp, vp, i, i, i, i, vp, vp])


@needs_hipcc
def test_ese_library_builds_and_exports_exactly_its_header():
    lib_path = build.build_ese(verbose=False)
    assert lib_path == build.ESE_LIB == _lib.ESE_LIB_PATH and os.path.exists(lib_path)
    header = open(os.path.join(ROOT, 'include', 'mmlf_ese_hip.h')).read()
    declared = set(_lib.ESE_SIGNATURES)
    assert set(re.findall(r'\b(mmlf_ese_[a-z0-9_]+)\s*\(', header)) <= declared
    nm = subprocess.run(['nm', '-D', '--defined-only', lib_path], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.split() and line.split()[-1].startswith('mmlf_')}
    assert exported == declared, exported ^ declared
    lib = ctypes.CDLL(lib_path)
    macro = int(re.search(r'^#define\s+MMLF_ESE_ABI_VERSION\s+(\d+)', header, re.M).group(1))
    assert lib.mmlf_ese_abi_version() == _lib.ESE_ABI_VERSION == macro == 1
    assert int(re.search(r'^#define\s+MMLF_ESE_MAX_TAB\s+(\d+)', header, re.M).group(1)) == _lib.ESE_MAX_TAB


@needs_hipcc
def test_ese_entry_points_refuse_bad_arguments_before_any_launch():
    """no GPU here: a call that got as far as a launch would fail differently (and say so)"""
    _lib.load_ese()
    one = ctypes.c_void_p(8)                                       # never dereferenced: every call below is refused first
    rb = lambda **k: tuple({**dict(means=one, logvars=one, grid=one, g_mean=one, g_logvar=one, g_post=one, g_means=one,   # noqa: E731
                                   g_logvars=one, S=4, B=1, H=4, W=4, stream=None), **k}.values())
    us = lambda **k: tuple({**dict(g=one, cs=32, kind=0, tab_s=one, tab_w=one, n=4, views=9, H=4, W=4, out=one,          # noqa: E731
                                   stream=None), **k}.values())
    bad = [('mmlf_ese_reduce_bwd', rb(means=None), 'null'), ('mmlf_ese_reduce_bwd', rb(g_logvars=None), 'null'),
           ('mmlf_ese_reduce_bwd', rb(S=0), 'S=0'), ('mmlf_ese_reduce_bwd', rb(S=(1 << 20) + 1), 'S='),
           ('mmlf_ese_reduce_bwd', rb(H=0), 'shape'), ('mmlf_ese_reduce_bwd', rb(B=-1), 'shape'),
           ('mmlf_ese_reduce_bwd', rb(B=1 << 20, H=1 << 20, W=1 << 20), 'shape'),
           ('mmlf_ese_unshift_sum', us(g=None), 'null'), ('mmlf_ese_unshift_sum', us(out=None), 'null'),
           ('mmlf_ese_unshift_sum', us(kind=4), 'kind=4'), ('mmlf_ese_unshift_sum', us(kind=-1), 'kind=-1'),
           ('mmlf_ese_unshift_sum', us(cs=30), 'cs=30'), ('mmlf_ese_unshift_sum', us(cs=24), 'cs=24'),
           ('mmlf_ese_unshift_sum', us(views=0), 'views=0'), ('mmlf_ese_unshift_sum', us(n=0), 'n=0'),
           ('mmlf_ese_unshift_sum', us(n=228), 'n=228'), ('mmlf_ese_unshift_sum', us(W=0), 'shape'),
           ('mmlf_ese_unshift_sum', us(H=1 << 25), 'shape')]
    for name, args, word in bad:
        with pytest.raises(RuntimeError) as e:
            _lib.call_ese(name, *args)
        assert name in str(e.value) and word in str(e.value), (name, str(e.value))


def test_load_ese_raises_when_the_library_is_missing(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, '_ese_lib', None)
    monkeypatch.setattr(_lib, 'ESE_LIB_PATH', str(tmp_path / 'libmmlf_ese_hip.so'))
    with pytest.raises(RuntimeError) as e:
        _lib.load_ese()
    assert 'not found' in str(e.value)


@needs_hipcc
def test_ese_kernels_use_no_scratch():
    """the compiler's resource remarks: a thread keeps two (reduce) or three (unshift) sums and no array"""
    flags = [f for f in build.FLAGS if f not in ('-fPIC', '-Wall')]
    usage = {}
    with tempfile.TemporaryDirectory() as tmp:
        for src in build.ESE_SOURCES:
            cmd = [build.HIPCC, *flags, '--cuda-device-only', '-Rpass-analysis=kernel-resource-usage', '-c',
                   os.path.join(build.HERE, src), '-o', os.path.join(tmp, src + '.co')]
            run = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
            assert run.returncode == 0, run.stderr
            for block in re.split(r'remark: [^\n]*Function Name: ', run.stderr)[1:]:
                usage[block.split(' [')[0]] = int(re.search(r'ScratchSize \[bytes/lane\]: (\d+)', block).group(1))
    assert [v for k, v in usage.items() if 'reduce_bwd_kernel' in k] == [0], usage
    assert [v for k, v in usage.items() if 'unshift_sum_kernel' in k] == [0] * 4, usage


def test_engine_hands_back_unpacked_gradients_by_default():
    from mmlf_amd.engine import Trunk
    sig = inspect.signature(Trunk.backward).parameters
    assert sig['packed_grads'].default is False
    assert list(sig)[:7] == ['self', 'p', 'tape', 'grad_output', 'grads', 'on_done', 'input_grads']


# ------------------------------------------------------------------------------------------------ the formulas
def reduce_bwd_formula(means, logvars, grid, g_mean, g_logvar, g_post):
    """include/mmlf_ese_hip.h's statement of mmlf_ese_reduce_bwd in numpy float64"""
    m, lv, grid = (np.asarray(a, dtype=np.float64) for a in (means, logvars, grid))
    S = m.shape[0]
    gm, glv = np.zeros_like(m), np.zeros_like(m)
    if g_post is not None:
        gp = np.asarray(g_post, dtype=np.float64)
        for j in range(S):
            b = np.exp(lv[j])
            for k in range(S):
                d = grid[k] - m[j]
                a = np.abs(d) / b
                gl = gp[:, k] * np.exp(-a) / (2 * b)
                gm[j] += gl * np.sign(d) / b
                glv[j] += gl * (a - 1)
        gm /= S
        glv /= S
    best = np.argmin(lv, axis=0)                                   # the first minimum: strict <
    for j in range(S):
        if g_mean is not None:
            gm[j] += np.where(best == j, g_mean, 0)
        if g_logvar is not None:
            glv[j] += np.where(best == j, g_logvar, 0)
    return gm, glv


@pytest.mark.parametrize('nulls', [(0, 0, 0), (1, 0, 0), (0, 1, 1), (1, 1, 0)])
def test_reduce_backward_formula_is_the_autograd_gradient(nulls):
    rs = np.random.RandomState(3)
    S, B, H, W = 5, 2, 3, 7
    means = rs.uniform(-1, 1, (S, B, H, W)).astype(np.float32)
    logvars = rs.uniform(-2, 1, (S, B, H, W)).astype(np.float32)
    logvars[3, 0] = logvars[1, 0]                                  # ties: the lower index takes the gradient
    grid = np.linspace(-1, 1, S).astype(np.float32)
    means[2, 1, 0] = grid[3]                                       # a mean exactly on a grid value: sign(0) = 0
    gs = [None if off else rs.uniform(-1, 1, shape).astype(np.float32)
          for off, shape in zip(nulls, ((B, H, W), (B, H, W), (B, S, H, W)))]
    want = refs.reduce_bwd_f64(means, logvars, grid, *gs)
    got = reduce_bwd_formula(means, logvars, grid, *gs)
    for g, w in zip(got, want):
        np.testing.assert_allclose(g, w.numpy(), rtol=1e-12, atol=1e-14)


def unroll_src(x, s, n):
    """the source index of the adjoint gather (csrc/ensamble_grad.hip): roll_src with the shift negated"""
    return x if abs(s) >= n else (x + s) % n


def unshift_formula(g, kind, tab_s, tab_w):
    """include/mmlf_ese_hip.h's statement of mmlf_ese_unshift_sum in numpy float64: a gather, members in order"""
    g = np.asarray(g, dtype=np.float64)
    n, views, _, H, W = g.shape
    out = np.zeros(g.shape[1:])
    ys, xs = np.arange(H), np.arange(W)
    for s in range(n):
        for k in range(views):
            (s0, s1), (w0, w1) = (int(t) for t in tab_s[s, k]), (float(t) for t in tab_w[s, k])
            sg = -1 if kind == 2 else 1
            xa, xb = [[unroll_src(x, t, W) for x in xs] for t in (s0, s1)] if kind != 1 else (xs, xs)
            ya, yb = [[unroll_src(y, sg * t, H) for y in ys] for t in (s0, s1)] if kind != 0 else (ys, ys)
            gk = g[s, k]
            at = lambda yy, xx: gk[:, yy][:, :, xx]                                  # noqa: E731
            if kind == 0:
                out[k] += w0 * at(ys, xa) + w1 * at(ys, xb)
            elif kind == 1:
                out[k] += w0 * at(ya, xs) + w1 * at(yb, xs)
            else:
                out[k] += w0 * (w0 * at(ya, xa) + w1 * at(ya, xb)) + w1 * (w0 * at(yb, xa) + w1 * at(yb, xb))
    return out


@pytest.mark.parametrize('members', [np.arange(-1, 1.5, 0.5), np.array([-3.5, -1.75, 0, 1.75])])
@pytest.mark.parametrize('kind', range(4))
def test_negated_gather_is_the_adjoint_of_the_shear(kind, members):
    """... with shifts up to 15 on a (9, 13) frame: the |s| >= n identity rule on both sides"""
    views, H, W = 9, 9, 13
    tab_s, tab_w = shift_table(members, views)
    assert len(members) == 5 or int(np.abs(tab_s).max()) >= max(H, W)
    g = np.random.RandomState(kind).uniform(-1, 1, (len(members), views, 3, H, W)).astype(np.float32)
    want, mag = refs.unshift_f64(g, kind, tab_s, tab_w)
    got = unshift_formula(g, kind, tab_s, tab_w)
    assert np.all(np.abs(got - want.numpy()) <= 1e-13 * (1 + mag.numpy()))
    assert float(mag.min()) > 0


def test_shear_restatement_equals_the_modules():
    from mmlf_amd.ensamble import shift_views_torch
    stacks = refs.case_inputs((2, 9, 13), 0)
    for disp in (-3.5, -0.5, 0.0, 1.75):
        for a, b in zip(refs.shift_f64(stacks, disp), shift_views_torch(stacks, disp)):
            assert torch.equal(a, b)
        tab_s, tab_w = shift_table([disp], 9)
        for kind, (a, x) in enumerate(zip(refs.shift_f64(stacks, disp), stacks)):
            assert torch.equal(a[0], refs.shift_one_f64(x[0], kind, tab_s, tab_w)[0])


# ------------------------------------------------------------------------------------------------ the reference's autograd
def test_restatement_against_the_references_autograd():
    g = load_golden('g14_ensamble_grad.npz')
    frame, seed = tuple(int(v) for v in g['frame']), int(g['seed'])
    assert (frame, seed) == refs.CPU_CASES[0] and tuple(g['disp']) == refs.DISP and str(g['dtype']) == 'float64'
    ref = refs.reference(frame, seed)
    assert sum(np.abs(np.asarray(v, dtype=np.float64)).sum() for v in ref['state'].values()) == float(g['state_checksum'])
    for k, v in ref['out'].items():
        # (posterior: the reference accumulates it in a float32 buffer, ensamble.py:95-99)
        tol = dict(rtol=1e-5, atol=1e-7) if k == 'posterior' else dict(rtol=1e-9, atol=1e-11)
        np.testing.assert_allclose(v.numpy(), g[f'out/{k}'], err_msg=k, **tol)
    for k, dx in zip('hvid', ref['dx']):
        want = torch.from_numpy(g[f'dx/{k}']) * ref['scale']
        assert refs.ratio(dx, want) <= 1e-3, k                  # (the table's float32 weights against Shift's float64 alpha)
    for n in refs.PARAMS:
        assert refs.ratio(ref['dp'][n], torch.from_numpy(g[f'dp/{n}']) * ref['scale']) <= 1e-3, n


# ------------------------------------------------------------------------------------------------ conditioning
@pytest.mark.parametrize('keys', [('mean', 'logvar', 'posterior'), refs.ALL_KEYS])
@pytest.mark.parametrize('frame,seed', refs.CPU_CASES)
def test_cases_are_well_conditioned(frame, seed, keys):
    """the float32 CPU run of the module sits within a tenth of the bar of the float64 restatement, for every stack and
    every parameter: what the GPU test measures is the kernels"""
    ref = refs.reference(frame, seed, keys=keys)
    m = refs.build(ref['state'])
    ens = Ensamble(m, *refs.DISP)
    out, dx = refs.run_module(ens, refs.case_inputs(frame, seed), ref['weights'], ref['scale'], keys)
    assert torch.equal(torch.min(out['logvars'], 0)[1], torch.min(ref['out']['logvars'], 0)[1])
    worst_x = max(refs.ratio(g, r) for g, r in zip(dx, ref['dx']))
    worst_p = max(refs.ratio(p.grad, ref['dp'][n]) for n, p in m.named_parameters())
    print(f'{frame} seed {seed}: loss x {ref["scale"]:g}, float32 at {worst_x:.2e} (stacks) and {worst_p:.2e} (parameters) of '
          f'the bar; smallest gap between the two lowest logvar members {ref["gap"]:.1e}')
    assert worst_x <= 0.1 and worst_p <= 0.1
    assert min(float(r.abs().max()) for r in ref['dx']) >= refs.GRAD_FLOOR


@pytest.mark.parametrize('frame,seed', refs.GPU_CASES)
def test_masked_share_stays_under_the_cap_in_float64(frame, seed):
    ref = refs.reference(frame, seed, masked=True)
    share = float(ref['mask'].double().mean())
    print(f'{frame} seed {seed}: {share:.2%} of the pixels have two logvar members closer than tau = {refs.TAU:g}')
    assert share <= refs.MASK_CAP
    assert refs.TAU == 10 * refs.LOGVAR_ATOL == 5e-5
    # two members that each move by the tolerance the GPU test holds the logvars to cannot swap across a gap of tau
    assert 2 * (refs.LOGVAR_ATOL + refs.LOGVAR_RTOL * float(ref['out']['logvars'].abs().max())) < refs.TAU


def test_cpu_tensors_keep_the_stock_path(monkeypatch):
    """nothing native on CPU tensors: neither node is used, and the five outputs are differentiable as ever"""
    from mmlf_amd import ensamble

    def refuse(*a, **k):
        raise AssertionError('a native node on CPU tensors')
    monkeypatch.setattr(ensamble._ReduceFn, 'apply', refuse)
    monkeypatch.setattr(ensamble._MembersFn, 'apply', refuse)
    frame, seed = refs.CPU_CASES[0]
    ref = refs.reference(frame, seed)
    ens = Ensamble(refs.build(ref['state']), *refs.DISP)
    out, dx = refs.run_module(ens, refs.case_inputs(frame, seed), ref['weights'], ref['scale'], want=(True, False, False, True))
    assert [g is not None for g in dx] == [True, False, False, True]
    assert all(out[k].grad_fn is not None for k in ('mean', 'logvar', 'means', 'logvars', 'posterior'))
