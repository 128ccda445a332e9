"""The numpy references of the data-side and validation-side kernels (tests_helpers: shift_ref, patch_ref, contrast_ref,
ensamble_reduce_ref, lmm_ref) against the goldens the reference itself produced, and their two error bounds against float32
restatements of the kernels' arithmetic: what tests/test_gpu_data_kernels.py compares the kernels with is pinned here, on a
machine without a GPU."""
import os
import random

import numpy as np
import pytest
import torch

from conftest import load_golden
from mmlf_amd import synth
from tests_helpers import (PATCH_NAMES, contrast_ref, ensamble_posterior_f32, ensamble_reduce_ref, lmm_edges, lmm_ref,
                           patch_ref, shift_ref, shift_table_ref)

HERE = os.path.dirname(os.path.abspath(__file__))
DISPS = (-3.5, -0.3, 0.0, 0.3, 2.5, 1.0)              # the six disparities of g4_shift.npz
TIED_SHARE_MAX = 1e-3


def tied_pixels(logvars):
    """(B, H, W) bool: the minimum of logvars over the members is taken more than once"""
    return (logvars == logvars.min(0, keepdims=True)).sum(0) > 1


def test_shift_ref_matches_the_golden_and_the_torch_path():
    from mmlf_amd.ensamble import shift_table, shift_views_torch
    g = load_golden('g4_shift.npz')
    stacks = [g[f'in{i}'][0] for i in range(4)]
    got = shift_ref(stacks, DISPS)
    for k, d in enumerate(DISPS):
        tor = shift_views_torch([torch.from_numpy(s) for s in stacks], float(d))
        for i in range(4):
            assert got[i].dtype == np.float32 and got[i].shape == (len(DISPS), *stacks[i].shape)
            np.testing.assert_allclose(got[i][k], g[f'shift_{d}_{i}'][0], rtol=1e-6, atol=1e-7, err_msg=f'{d} {i}')
            np.testing.assert_array_equal(got[i][k], tor[i].numpy(), err_msg=f'torch {d} {i}')
    # the table of the helper is the product's, for odd, even and single view counts and both zeros
    disps = [0.0, -0.0, 0.3, -0.3, 1.0, -1.0, 2.5, 13.5, -299.5]
    for views in (1, 2, 3, 9, 11):
        a, b = shift_table_ref(disps, views), shift_table(disps, views)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), views


def test_shift_ref_at_an_even_view_count_and_one_row():
    """what the goldens do not hold: 2 views (half = 1: views at -1 and 0) and a one-row frame, against a direct statement of
    the shear of the horizontal and the vertical stack"""
    rs = np.random.RandomState(3)
    stacks = [rs.uniform(size=(2, 3, 1, 7)).astype(np.float32) for _ in range(4)]
    h, v, i, d = [a[0] for a in shift_ref(stacks, [2.25])]
    # view 0: disp * (0 - 1) = -2.25 -> s0 = -2, s1 = -3, alpha = 0.25; view 1: shift 0
    want = np.roll(stacks[0][0], -2, -1) * np.float32(0.75) + np.roll(stacks[0][0], -3, -1) * np.float32(0.25)
    np.testing.assert_array_equal(h[0], want)
    np.testing.assert_array_equal(h[1], stacks[0][1])
    np.testing.assert_array_equal(v, stacks[1])                          # one row: every vertical roll is the identity
    np.testing.assert_array_equal(i, shift_ref([stacks[2]] * 4, [2.25])[0][0])          # I and D: the W pass alone
    np.testing.assert_array_equal(d, shift_ref([stacks[3]] * 4, [2.25])[0][0])


def test_ensamble_reduce_ref_matches_the_golden():
    g = load_golden('g4_ensamble.npz')
    means, logvars = g['means'], g['logvars']
    S = means.shape[0]
    grid = np.linspace(-3.5, 3.5, S).astype(np.float32)
    idx, mean, logvar, ref, bound = ensamble_reduce_ref(means, logvars, grid)
    tied = tied_pixels(logvars)
    share = float(tied.mean())
    print(f'\n[g4_ensamble] tied pixels: {int(tied.sum())} of {tied.size} ({share:.4%})', [tuple(p) for p in np.argwhere(tied)])
    assert share <= TIED_SHARE_MAX
    np.testing.assert_array_equal(logvar, g['logvar'])                    # the minimum itself: every pixel, tied or not
    assert np.array_equal(mean[~tied], g['mean'][~tied])
    err = np.abs(g['posterior'].astype(np.float64) - ref)
    print(f'[g4_ensamble] golden posterior: max |err| / bound = {float((err / bound).max()):.4f}')
    assert (err <= bound).all(), float((err / bound).max())


def test_lmm_ref_matches_the_golden():
    g = load_golden('g6_multimodal.npz')
    edges = lmm_edges(108, -3.5, 3.5)
    # the reference's caller passes exp(logvars) under the name `logvars` (validate/cli.py:302,318), and so was the golden made
    ref, bound = lmm_ref(g['lmm_means'], np.exp(g['lmm_logvars']), edges)
    err = np.abs(g['lmm_to_discrete'] - ref)
    assert ref.shape == g['lmm_to_discrete'].shape and (err <= bound).all(), float((err / bound).max())
    ref1, bound1 = lmm_ref(g['mean'][None, :1], g['logvar'][None, :1], edges)          # S = 1: laplace_to_discrete
    err1 = np.abs(g['laplace_to_discrete'] - ref1)
    assert (err1 <= bound1).all(), float((err1 / bound1).max())
    # and the CPU branch of the product, whose edges come from torch.linspace
    from mmlf_amd import metrics
    cpu = metrics.lmm_to_discrete(108, -3.5, 3.5, torch.from_numpy(g['lmm_means']), torch.exp(torch.from_numpy(g['lmm_logvars'])))
    assert (np.abs(cpu.numpy() - ref) <= bound).all()


@pytest.fixture(scope='module')
def g7():
    return np.load(os.path.join(HERE, 'golden', 'g7_patch_pipeline.npz'))


@pytest.mark.parametrize('tag', 'abcd')
def test_patch_ref_matches_the_golden(g7, tag):
    from oracle import oracle as orc
    from mmlf_amd import patches
    from test_patch_pipeline import TOL
    seed, H, W, ps, max_down, augment = [int(x) for x in g7[f'{tag}.cfg']]
    assert (tag == 'c') == (not augment)
    scene = synth.synth_scene(seed, H, W)
    for k in range(6):
        random.seed(100 * seed + k)
        p = patches.draw_sample((H, W), ps, max_down, bool(augment))
        params = dict(ps=ps, f=p['f'], disp=p['disp'], y0=p['y0'], x0=p['x0'], rot=p['rot'], flags=7 if augment else 0,
                      mat=p['mat'], bright=p['bright'])
        out = patch_ref(scene, params)
        if augment:
            out = orc.tf_contrast(out, p['contrast'])
        for name, arr in zip(PATCH_NAMES, out):
            ref = g7[f'{tag}.{k}.{name}']
            assert arr.shape == ref.shape, (tag, k, name)
            if name == 'mask' or not augment:
                assert np.array_equal(arr, ref), (tag, k, name)
            else:
                assert np.abs(arr.astype(np.float64) - ref).max() <= TOL, (tag, k, name)


def test_patch_ref_single_flags_and_contrast_ref():
    """each flag alone changes what it names and nothing else; contrast_ref with the float32 mean of the horizontal stack is
    tf_contrast"""
    from oracle import oracle as orc
    scene = synth.synth_scene(3, 20, 23, views=3, planes=1)
    base = dict(ps=5, f=2, disp=0.37, y0=2, x0=3, rot=0, flags=0, mat=orc.draw_redist_matrix(random.Random(1)), bright=1.9)
    plain = patch_ref(scene, base)
    np.testing.assert_array_equal(plain[0], scene[0][..., ::2, ::2][..., 2:7, 3:8])
    np.testing.assert_array_equal(plain[5], (scene[5][::2, ::2] / np.float32(2))[2:7, 3:8])
    sh = patch_ref(scene, dict(base, flags=1))
    assert not np.array_equal(sh[0], plain[0]) and np.array_equal(sh[4], plain[4]) and np.array_equal(sh[7], plain[7])
    np.testing.assert_array_equal(sh[5], plain[5] - np.float32(0.37))
    np.testing.assert_array_equal(sh[6][:, 4], plain[6][:, 4] - np.float32(0.37))
    np.testing.assert_array_equal(sh[6][:, :4], plain[6][:, :4])
    col = patch_ref(scene, dict(base, flags=2))
    assert not np.array_equal(col[4], plain[4]) and all(np.array_equal(col[k], plain[k]) for k in (5, 6, 7))
    br = patch_ref(scene, dict(base, flags=4))
    np.testing.assert_array_equal(br[0], plain[0] * np.float32(1.9))
    assert all(np.array_equal(br[k], plain[k]) for k in (5, 6, 7))
    rot = patch_ref(scene, dict(base, rot=1))
    np.testing.assert_array_equal(rot[7], plain[7])                       # the mask is cropped and not rotated
    np.testing.assert_array_equal(rot[5], np.flip(plain[5].T, -2))
    np.testing.assert_array_equal(rot[0], np.flip(np.swapaxes(plain[1], -1, -2), -2))  # the new H stack is the old V stack
    full = patch_ref(scene, dict(base, flags=7, rot=3))
    for alpha in (0.1, 1.0, 1.9):
        want = orc.tf_contrast(full, alpha)
        st, c = contrast_ref(full[:4], full[4], alpha, full[0].mean(dtype=np.float32))
        for k in range(4):
            np.testing.assert_array_equal(st[k], want[k])
        np.testing.assert_array_equal(c, want[4])


def _exp32_correctly_rounded(x):
    return np.exp(x.astype(np.float64)).astype(np.float32)


@pytest.mark.parametrize('S', [1, 2, 7, 70])
def test_posterior_bound_holds_for_the_float32_restatement(S):
    rs = np.random.RandomState(S)
    worst = 0.0
    for lo, hi in ((-8.0, 2.0), (-12.0, -6.0), (-12.0, 3.0)):
        means = rs.uniform(-4, 4, (S, 2, 5, 13)).astype(np.float32)
        logvars = rs.uniform(lo, hi, (S, 2, 5, 13)).astype(np.float32)
        grid = np.linspace(-3.5, 3.5, S).astype(np.float32)
        _, _, _, ref, bound = ensamble_reduce_ref(means, logvars, grid)
        with np.errstate(under='ignore'):
            err = np.abs(ensamble_posterior_f32(means, logvars, grid).astype(np.float64) - ref)
        assert (err <= bound).all(), (S, lo, hi, float((err / bound).max()))
        worst = max(worst, float((err / bound).max()))
    print(f'\n[posterior bound] S = {S}: float32 restatement uses {worst:.4f} of it')


def test_argmin_ref_takes_the_first_minimum():
    means = np.arange(4 * 2 * 3 * 5, dtype=np.float32).reshape(4, 2, 3, 5)
    logvars = np.full((4, 2, 3, 5), 1.0, np.float32)
    logvars[1] = logvars[3] = -2.0
    idx, mean, logvar, _, _ = ensamble_reduce_ref(means, logvars, np.linspace(-3.5, 3.5, 4).astype(np.float32))
    assert (idx == 1).all() and np.array_equal(mean, means[1]) and (logvar == -2.0).all()
    assert tied_pixels(logvars).all()


@pytest.mark.parametrize('shape', [(1, 1, 1, 1, 1), (5, 2, 108, 14, 18), (70, 1, 7, 3, 11)])
def test_mixture_bound_holds_for_another_float32_exponential(shape):
    S, B, n_bins, H, W = shape
    rs = np.random.RandomState(S + n_bins)
    means = rs.uniform(-4, 4, (S, B, H, W)).astype(np.float32)
    logvars = rs.uniform(-8, 2, (S, B, H, W)).astype(np.float32)
    edges = lmm_edges(n_bins, -3.5, 3.5)
    ref, bound = lmm_ref(means, logvars, edges)
    worst = 0.0
    for exp32 in (_exp32_correctly_rounded,
                  lambda x: np.nextafter(np.exp(x), np.float32(np.inf)), lambda x: np.nextafter(np.exp(x), np.float32(0))):
        got, _ = lmm_ref(means, logvars, edges, exp32=exp32)
        err = np.abs(got - ref)
        assert (err <= bound).all(), (shape, float((err / bound).max()))
        worst = max(worst, float((err / bound).max()))
    print(f'\n[mixture bound] {shape}: another float32 exp uses {worst:.4f} of it')
    assert (ref >= -4e-16).all() and (ref.sum(1) <= 1 + 1e-12).all()
