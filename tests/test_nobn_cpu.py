"""--model_no_batchnorm without a GPU: which configurations take the native trunk (2x2 filters only), the state_dict layout, the
stock-torch (CPU) path against the reference's tiny run (tests/golden/g13_nobn_tiny_*.npz, make_golden_nobn.py), the C ABI of
the ReLU-backward slice kernel that the concat boundary needs, and the compiler's resource figures of the kernels such a step
adds to the launch kinds tests/test_kernel_resources.py already holds (reference feed_forward.py:122-137)."""
import ctypes
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, TINY_KW, VARIANTS, load_golden
from mmlf_amd import synth

NOBN_TINY_KW = dict(TINY_KW, model_no_batchnorm=True)
NOBN_SYMBOLS = ['mmlf_relu_bwd_slice', 'mmlf_audit_relu_bwd_slice']


def gained_state(kw, seed, gain=np.sqrt(6.0)):
    """synth.synth_state with every convolution filter multiplied by `gain` (float32).  The default, sqrt(6), turns torch's
    filter bound 1 / sqrt(fan_in) into sqrt(6 / fan_in), which keeps the signal's variance through a ReLU: with the plain
    bound a net without BatchNorm shrinks it at every block and the stream nets' gradients sink below the absolute floors
    of the gradient bars (tests/golden/make_golden_nobn.py)."""
    spec = synth.param_spec(**kw)
    state = synth.synth_state(spec, seed=seed)
    return {n: (state[n] * np.float32(gain) if kind == 'conv_w' else state[n]) for n, _, kind in spec}


def nobn_golden(variant):
    """(golden arrays, model kwargs, state) of g13: the weights are regenerated from their seed and gain, and checked"""
    g = load_golden(f'g13_nobn_tiny_{variant}.npz')
    kw = dict(NOBN_TINY_KW, **VARIANTS[variant])
    state = gained_state(kw, int(g['state_seed']), g['state_gain'])
    chk = sum(np.abs(np.asarray(v, dtype=np.float64)).sum() for v in state.values())
    assert chk == float(g['state_checksum'])
    return g, kw, state


def loss_of(variant, out, gt, mask):
    from mmlf_amd import dl, loss
    if variant == 'upr':
        return loss.ImprovedUncertaintyL1Loss()(out, gt, mask, None)
    if variant == 'dpp':
        return loss.MaskedCrossEntropy()(out, dl.reg_to_class(gt, -3.5, 3.5, 108), mask)
    return loss.MaskedL1Loss()(out, gt, mask)


def test_no_batchnorm_with_2x2_filters_is_native():
    from mmlf_amd.feed_forward import FeedForward
    for extra in VARIANTS.values():
        m = FeedForward(**dict(NOBN_TINY_KW, **extra))
        assert m._native_ok
        assert m._trunk is not None and m._trunk.ksize == 2 and m._trunk.batchnorm is False
        kinds = [b.bn for _, _, blocks in m._trunk.streams for b in blocks] + [b.bn for b in m._trunk.out_blocks]
        assert kinds == [False] * 8 + [False, False, None]          # ReLU-only blocks, then the head
    t = FeedForward(**TINY_KW)._trunk                                # the default: BatchNorm blocks, then the head
    assert t.batchnorm is True and [b.bn for b in t.out_blocks] == [True, True, None]


def test_no_batchnorm_with_other_flags_is_not_native():
    from mmlf_amd.feed_forward import FeedForward
    for extra in (dict(model_ksize=3), dict(model_cross=True), dict(model_unet=True), dict(model_ksize=4)):
        m = FeedForward(**dict(NOBN_TINY_KW, **extra))
        assert not m._native_ok and m._trunk is None, extra
    from mmlf_amd.engine import Trunk
    with pytest.raises(ValueError, match='2x2'):
        Trunk(8, 2, 3, 9, 1, 0.1, ksize=3, batchnorm=False)


@pytest.mark.parametrize('variant', list(VARIANTS))
def test_state_dict_matches_the_reference_layout(variant):
    from mmlf_amd.feed_forward import FeedForward
    g, kw, state = nobn_golden(variant)
    sd = FeedForward(**kw).state_dict()
    spec = synth.param_spec(**kw)
    assert list(sd) == [n for n, _, _ in spec]
    assert all(tuple(sd[n].shape) == tuple(s) for n, s, _ in spec)
    assert list(sd) == [k[len('grad/'):] for k in g if k.startswith('grad/')]      # no buffers: every key is a parameter
    assert not any('.3.' in k for k in sd)
    assert all(kind in ('conv_w', 'conv_b') for _, _, kind in spec)


@pytest.mark.parametrize('variant', list(VARIANTS))
def test_cpu_stock_path_matches_reference(variant):
    from mmlf_amd.feed_forward import FeedForward
    g, kw, state = nobn_golden(variant)
    m = FeedForward(**kw)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    stacks = [torch.from_numpy(g[f'in{i}']) for i in range(4)]
    m.eval()
    with torch.no_grad():
        out = m(*stacks)
    for k, v in out.items():
        assert (v is None) == (f'eval_{k}' not in g), k
        if v is not None:
            np.testing.assert_allclose(v.numpy(), g[f'eval_{k}'], rtol=1e-5, atol=1e-6, err_msg=f'eval {k}')
    m.train()
    out = m(*stacks)
    for k, v in out.items():
        if v is not None:
            np.testing.assert_allclose(v.detach().numpy(), g[f'train_{k}'], rtol=1e-5, atol=1e-6, err_msg=f'train {k}')
    lv = loss_of(variant, out, torch.from_numpy(g['gt']), torch.from_numpy(g['mask']))
    np.testing.assert_allclose(lv.item(), g['loss'], rtol=1e-5, atol=1e-6)
    lv.backward()
    for n, p in m.named_parameters():
        np.testing.assert_allclose(p.grad.numpy(), g[f'grad/{n}'], rtol=1e-5, atol=1e-6, err_msg=n)
    assert float(g['f64_worst']) <= 1.0       # the generator's float32 / float64 check of the fixture's conditioning
    # every gradient tensor stands above the absolute floor of the G1 bar (5e-7 against 5e-4 of its maximum): the GPU test's
    # bar is the relative one everywhere, the stream nets included
    smallest = min(np.abs(v).max() for k, v in g.items() if k.startswith('grad/'))
    assert smallest == float(g['grad_smallest']) and smallest >= 1e-2


def test_slice_symbols_in_header_binding_and_library():
    from mmlf_amd import _lib
    with open(f'{ROOT}/include/mmlf_hip.h') as f:
        header = f.read()
    for name in NOBN_SYMBOLS:
        assert re.search(r'\b' + name + r'\s*\(', header), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.load(), name), name
    macro = int(re.search(r'^#define\s+MMLF_ABI_VERSION\s+(\d+)', header, re.M).group(1))
    assert macro == _lib.ABI_VERSION == _lib.load().mmlf_abi_version()
    assert macro >= 10                          # 9 had no mmlf_relu_bwd_slice


SLICE_CASES = [(70, 280, 0), (70, 280, 70), (70, 280, 210), (8, 32, 24), (70, 72, 0)]


@pytest.mark.parametrize('B,H,W', [(2, 9, 9), (3, 5, 29), (1, 1, 1), (2, 7, 130)])
def test_slice_audit_stays_inside_what_the_size_queries_allocate(B, H, W):
    """mmlf_audit_relu_bwd_slice against the allocations of engine.Geometry.buf (mmlf_grid_alloc_positions,
    mmlf_amax_entries): what MMLF_CHECK_EXTENTS=1 compares before the launch"""
    from mmlf_amd import _lib
    L = _lib.load()
    alloc, amax_n = L.mmlf_grid_alloc_positions(B, H, W), L.mmlf_amax_entries(B, H, W)
    P, R = W + L.mmlf_grid_pad_w(), H + L.mmlf_grid_pad_h()
    for C, cs_src, c_off in SLICE_CASES:
        cs_dst = (C + 7) // 8 * 8
        e = (ctypes.c_int64 * 4)()
        assert L.mmlf_audit_relu_bwd_slice(cs_src, c_off, cs_src, c_off, C, cs_dst, B, H, W, e) == 0, _lib.last_error()
        assert 0 < e[0] <= alloc * cs_src * 4 and e[1] == e[0]
        assert e[0] == ((((B - 1) * R + H) * P + W) * cs_src + c_off + C) * 4        # the last interior position's slice
        assert e[2] == B * R * P * cs_dst * 4 <= alloc * cs_dst * 4
        assert 0 < e[3] <= amax_n * 4
    e = (ctypes.c_int64 * 4)()
    assert L.mmlf_audit_relu_bwd_slice(280, 211, 280, 210, 69, 72, B, H, W, e) != 0       # odd c_off
    assert L.mmlf_audit_relu_bwd_slice(280, 212, 280, 210, 70, 72, B, H, W, e) != 0       # a slice past cs_src
    assert 'mmlf_audit_relu_bwd_slice' in _lib.last_error()


# ------------------------------------------------------------------ compiler resource figures
@pytest.fixture(scope='module')
def usage():
    import os
    from test_kernel_resources import HIPCC, _resource_usage
    if not os.path.exists(HIPCC):
        pytest.skip('no hipcc')
    return _resource_usage()


def test_slice_kernel_fits_beside_a_wide_weight_gradient(usage):
    """relu_slice_rows_kernel is held to what its bn_rows_kernel siblings are: no scratch and at most the 48 registers that
    two waves of a wide weight-gradient workgroup leave per SIMD lane (tests/test_kernel_resources.py)"""
    from test_kernel_resources import _demangled
    vgprs, _, scratch, _ = _demangled(usage, 'relu_slice_rows_kernel', (4,))
    assert scratch == 0 and 0 <= vgprs <= 48, (vgprs, scratch)


# (G, planes, epilogue kind, waves, transposed) of conv4tap_x6s_kernel that a no-BatchNorm step launches at G = 5 / 18 beyond
# test_kernel_resources.CONV_KINDS: ReLU into a 70-channel slice of the concat buffer (kind 1, not transposed: 70 % 4 != 0),
# and the data gradient masked by the activations themselves (kind 8 = EPI_REF_IN, which has no transposed form)
NOBN_CONV_KINDS = [(5, 2, 1, 16, False), (5, 2, 1, 8, False), (5, 2, 8, 16, False), (5, 2, 8, 8, False), (18, 2, 8, 8, False)]


@pytest.mark.parametrize('args', NOBN_CONV_KINDS)
def test_conv_launch_kinds_of_a_no_batchnorm_step_do_not_spill(usage, args):
    from test_kernel_resources import _demangled
    vgprs, agprs, scratch, waves = _demangled(usage, 'conv4tap_x6s_kernel', args)
    assert scratch == 0, (args, vgprs, scratch)
    assert waves >= (2 if args[0] == 18 else 4), (args, waves)
    assert vgprs <= (256 if args[0] == 18 else 128)
