"""--model_ksize 3 without a GPU: which configurations take the native 3x3 trunk, the C ABI of the 3x3 kernels, and the
stock-torch (CPU) path against the reference's tiny k=3 run (tests/golden/g12_k3_tiny_*.npz, make_golden_k3.py)."""
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, TINY_KW, VARIANTS, load_golden
from mmlf_amd import synth

K3_TINY_KW = dict(TINY_KW, model_ksize=3)
K3_SYMBOLS = ['mmlf_grid_alloc_positions_k3', 'mmlf_zero_slack_k3', 'mmlf_zero_slack4_k3', 'mmlf_packed_filter3x3_floats',
              'mmlf_pack_filter3x3', 'mmlf_conv3x3', 'mmlf_wgrad3x3_workspace_floats', 'mmlf_conv3x3_wgrad',
              'mmlf_fold_bn_eval3x3', 'mmlf_audit_conv3x3', 'mmlf_audit_wgrad3x3']


def k3_spec(kw):
    return [(n, (shape[0], shape[1], 3, 3) if kind == 'conv_w' else shape, kind) for n, shape, kind in synth.param_spec(**kw)]


def k3_golden(variant):
    """(golden arrays, model kwargs, state) of g12: the weights are regenerated from their seed and checked"""
    g = load_golden(f'g12_k3_tiny_{variant}.npz')
    kw = dict(K3_TINY_KW, **VARIANTS[variant])
    state = synth.synth_state(k3_spec(kw), seed=int(g['state_seed']))
    chk = sum(np.abs(np.asarray(v, dtype=np.float64)).sum() for v in state.values())
    assert chk == float(g['state_checksum'])
    return g, kw, state


def test_native_ok_for_ksize_2_and_3_only():
    from mmlf_amd.feed_forward import FeedForward
    assert FeedForward(**K3_TINY_KW)._native_ok
    assert FeedForward(**dict(K3_TINY_KW, model_uncert=True))._native_ok
    assert FeedForward(**dict(K3_TINY_KW, model_discrete=True))._native_ok
    assert FeedForward(**K3_TINY_KW)._trunk.ksize == 3
    assert FeedForward(**TINY_KW)._trunk.ksize == 2
    for k in (1, 4, 5):
        assert not FeedForward(**dict(TINY_KW, model_ksize=k))._native_ok, k
    assert not FeedForward(**dict(K3_TINY_KW, model_cross=True))._native_ok
    assert not FeedForward(**dict(K3_TINY_KW, model_unet=True))._native_ok
    assert not FeedForward(**dict(K3_TINY_KW, model_no_batchnorm=True))._native_ok


def test_k3_state_dict_matches_the_reference_layout():
    from mmlf_amd.feed_forward import FeedForward
    sd = FeedForward(**K3_TINY_KW).state_dict()
    spec = k3_spec(K3_TINY_KW)
    assert list(sd) == [n for n, _, _ in spec]
    assert all(tuple(sd[n].shape) == tuple(s) for n, s, _ in spec)


def test_k3_symbols_in_header_and_binding():
    from mmlf_amd import _lib
    with open(f'{ROOT}/include/mmlf_hip.h') as f:
        header = f.read()
    for name in K3_SYMBOLS:
        assert re.search(r'\b' + name + r'\s*\(', header), name
        assert name in _lib.SIGNATURES, name


@pytest.mark.parametrize('variant', list(VARIANTS))
def test_k3_cpu_stock_path_matches_reference(variant):
    from mmlf_amd import dl, loss
    from mmlf_amd.feed_forward import FeedForward
    g, kw, state = k3_golden(variant)
    m = FeedForward(**kw)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    stacks = [torch.from_numpy(g[f'in{i}']) for i in range(4)]
    m.eval()
    with torch.no_grad():
        out = m(*stacks)
    for k, v in out.items():
        if v is not None:
            np.testing.assert_allclose(v.numpy(), g[f'eval_{k}'], rtol=1e-5, atol=1e-6, err_msg=f'eval {k}')
    m.train()
    out = m(*stacks)
    for k, v in out.items():
        if v is not None and f'train_{k}' in g:
            np.testing.assert_allclose(v.detach().numpy(), g[f'train_{k}'], rtol=1e-5, atol=1e-6, err_msg=f'train {k}')
    gt, mask = torch.from_numpy(g['gt']), torch.from_numpy(g['mask'])
    if variant == 'upr':
        lv = loss.ImprovedUncertaintyL1Loss()(out, gt, mask, None)
    elif variant == 'dpp':
        lv = loss.MaskedCrossEntropy()(out, dl.reg_to_class(gt, -3.5, 3.5, 108), mask)
    else:
        lv = loss.MaskedL1Loss()(out, gt, mask)
    np.testing.assert_allclose(lv.item(), g['loss'], rtol=1e-6)
    lv.backward()
    for n, p in m.named_parameters():
        ref = g[f'grad/{n}']
        assert np.abs(p.grad.numpy() - ref).max() <= 1e-5 * max(np.abs(ref).max(), 1e-6) + 1e-8, n
    for k, v in m.state_dict().items():
        if 'running' in k or 'num_batches' in k:
            np.testing.assert_allclose(v.numpy(), g[f'post/{k}'], rtol=1e-6, atol=1e-7, err_msg=k)
