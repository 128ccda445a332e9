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


# ------------------------------------------------------------------ the float64 references of tests/test_gpu_ksize3.py
@pytest.mark.parametrize('variant', [0, 1, 2])
def test_grid_float64_references_match_torch_conv2d(variant):
    """tests_helpers.conv9_ref / dgrad9_ref / wgrad9_ref (per-tap matmuls on the grid layout, what the GPU tests hold the 3x3
    kernels against at every size) are nn.Conv2d(k=3, padding=1) on the stream's transformed image, and its two gradients"""
    import torch.nn.functional as F
    from tests_helpers import conv9_ref, dgrad9_ref, filter9, unfilter9, wgrad9_ref

    def stock(x, w, b):          # feed_forward.py _torch_trunk: the H / I streams run on the transposed (and flipped) image
        if variant == 0:
            return F.conv2d(x, w, b, padding=1)
        if variant == 1:
            return F.conv2d(x.transpose(2, 3), w, b, padding=1).transpose(2, 3)
        return F.conv2d(x.transpose(2, 3).flip(-1), w, b, padding=1).flip(-1).transpose(2, 3)

    gen = torch.Generator().manual_seed(5 + variant)
    B, K, N, H, W = 2, 5, 6, 4, 7
    x = torch.randn((B, K, H, W), generator=gen, dtype=torch.float64, requires_grad=True)
    w = torch.randn((N, K, 3, 3), generator=gen, dtype=torch.float64, requires_grad=True)
    b = torch.randn((N,), generator=gen, dtype=torch.float64, requires_grad=True)
    g = torch.randn((B, N, H, W), generator=gen, dtype=torch.float64)
    z = stock(x, w, b)
    z.backward(g)
    pad = lambda t: F.pad(t.detach().permute(0, 2, 3, 1), (0, 0, 1, 1, 1, 1))         # NCHW -> zero-framed grid view
    wv = filter9(w.detach(), variant)
    torch.testing.assert_close(conv9_ref(pad(x), wv, b.detach()), z.detach().permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(dgrad9_ref(pad(g), wv), x.grad.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    gw, gb = wgrad9_ref(pad(x), pad(g))
    torch.testing.assert_close(unfilter9(gw, variant), w.grad, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(gb, b.grad, rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------ G: the GPU shapes hit what they exist for
def test_k3_gpu_shapes_cover_the_kernel_edges():
    """tests/test_gpu_ksize3.py's kernel shapes, read through the ABI's size queries only, must reach every path of the 3x3
    kernels the sweep exists for -- so that an edit of a shape list cannot quietly drop one:
      * a pitch longer than conv9tap_kernel's 258-position window row; frames of one row and of one column; a batch whose
        tile padding NQpad - NQ holds a whole 256-position tile without a valid position;
      * in every weight-gradient class (nsplit from mmlf_wgrad3x3_workspace_floats) splits of >= 3 chunks -- the prefetch
        and the two-barrier chunk loop of wgrad9tap_kernel -- with a ragged last split where the class allows one;
      * the three column blocks of N > 128: a third block wholly past N_store, one partly live, one full."""
    import test_gpu_ksize3 as k3
    from mmlf_amd import _lib
    L = _lib.load()
    pw, ph, tile = L.mmlf_grid_pad_w(), L.mmlf_grid_pad_h(), 256          # include/mmlf_hip.h MMLF_TILE_POSITIONS

    def grid(B, H, W):
        P, R = W + pw, H + ph
        NQpad = L.mmlf_relu_mask_words(B, H, W) // 4096 * tile             # [tile][8 waves][8 rows][64 lanes] words
        return P, B * R * P, NQpad

    geoms = list(k3.GEOMS) + list(k3.FULL_GEOMS) + [k3.HEAD_GEOM, k3.GUARD_GEOM]
    assert max(grid(*g)[0] for g in geoms) > 258
    assert any(H == 1 for _, H, _ in k3.GEOMS) and any(W == 1 for _, _, W in k3.GEOMS)
    assert any(grid(*g)[2] - grid(*g)[1] >= tile for g in k3.GEOMS)

    def nsplit(cin, cout):
        np_cols = L.mmlf_packed_filter3x3_floats(8, cout) // (9 * 2 * 4)       # packed columns: NT * 32
        rows = (cin + 1 + 31) // 32 * 32                                        # ci slices of 32 (+ the ones row)
        ws = L.mmlf_wgrad3x3_workspace_floats(cin, cout, 1, 1, 1)
        assert ws % (9 * rows * np_cols) == 0
        return ws // (9 * rows * np_cols)

    classes = {}
    for cin, cout in k3.SWEEP_PAIRS:
        classes.setdefault(nsplit(cin, cout), []).append((cin, cout))
    assert sorted(classes) == [16, 40, 56, 168], classes        # Cin+1 <= 32 / 96 / 128 / 288: every class of the network
    for ns, pairs in classes.items():
        deep = []
        for B, H, W in k3.GEOMS:
            nchunks = grid(B, H, W)[2] // 32
            per = -(-nchunks // ns)
            if per >= 3:
                deep.append((B, H, W, nchunks % per))
        assert deep, (ns, pairs)
        # NQpad is a multiple of 512 positions = 16 chunks: 16 splits always divide the chunks evenly
        if ns != 16:
            assert any(tail for *_, tail in deep), (ns, deep)

    ncols = [L.mmlf_packed_filter3x3_floats(8, n) // (9 * 2 * 4) for n in k3.HEAD_NS]
    assert all(c == 288 for c in ncols)                         # conv9_shape: three column blocks of 96
    third = set()
    for n in k3.HEAD_NS:
        for n_store in (n, (n + 7) // 8 * 8):
            third.add('dead' if n_store <= 192 else 'full' if n_store == 288 else 'partly live')
    assert third == {'dead', 'partly live', 'full'}
