"""Gradients with respect to the four view stacks on the native trunk, and its backward without weight gradients
(reference mmlf/model/feed_forward.py:226-269: nn.Conv2d modules, which autograd differentiates in h_views ... d_views).

  * the input gradients of the three native trunk kinds (2x2 with BatchNorm, 2x2 model_no_batchnorm, 3x3), three heads and
    three non-square frames against the same module in float64 on the CPU (tests/test_input_grad_cpu.py: seeds, the exact
    power-of-two loss scaling, and the conditioning that is asserted first), at the project's gradient bar; the parameter
    gradients of the same backward bit for bit those of a backward that forms no input gradient;
  * eval mode under autograd, a partial request (one stack) with its launch counts, frozen nets in train mode (no weight
    gradient launch, the BatchNorm buffers still move) and in eval mode (2x2 with BatchNorm: the inference launches, the
    bits of the no_grad forward and a backward without any BatchNorm launch), the other two arithmetic modes in child
    processes, the extent audit, nn.DataParallel replicas;
  * kernel level: the data gradient K -> N of a stream net's first convolution without a ReLU reference at out_shift = P + 1,
    three filter variants, three modes and the 3x3 kernel, against float64 conv2d autograd on the transformed image."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, VARIANTS
from test_gpu_kernels import grid_from_nchw, nchw_from_grid
from test_input_grad_cpu import (DGRAD_FRAMES, DGRAD_SHAPES, EVAL_FRAMES, FRAMES, K3_DGRAD_SHAPES, KINDS, bar, build, inputs,
                                 ratio, reference, run)

pytestmark = pytest.mark.gpu

MODES = ['f32', 'bf16x6', 'f16x3']


def _dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


class _Spy:
    """records the entry points that go through _lib.call from the engine and the module"""

    def __init__(self, monkeypatch):
        from mmlf_amd import _lib, engine, feed_forward
        self.names = []
        real = _lib.call

        def call(name, *args):
            self.names.append(name)
            return real(name, *args)
        for mod in (_lib, engine, feed_forward):
            monkeypatch.setattr(mod, 'call', call)

    def count(self, *prefixes):
        return sum(1 for n in self.names if n.startswith(prefixes))


def _conv_entries():
    """the convolution (= data gradient) and weight-gradient entry points of the current mode's 2x2 kernels, and the 3x3 ones"""
    from mmlf_amd import engine
    conv = {'f16x3': 'mmlf_conv2x2_h2', 'bf16x6': 'mmlf_conv2x2_split'}.get(engine.CONV_MODE, 'mmlf_conv2x2')
    return (conv, 'mmlf_conv3x3'), ('mmlf_conv2x2_wgrad', 'mmlf_conv3x3_wgrad')


def _gpu_run(kind, variant, frame, eval_mode=False, want=(True,) * 4, frozen=False):
    """(module, output dict, input gradients, reference tuple) of one scaled forward + backward on the GPU"""
    ref = reference(kind, variant, frame, eval_mode)
    kw, state, seed, scale, _, cond = ref
    assert cond <= 0.1, cond                              # conditioning first: the float32 stock run sits at the float64 one
    m = build(kw, state, _dev())
    assert m._native_ok
    m.train(not eval_mode)
    if frozen:
        for p in m.parameters():
            p.requires_grad_(False)
    out, dx = run(m, variant, *inputs(frame, seed, _dev()), scale=scale, want=want)
    return m, out, dx, ref


def _check_dx(tag, dx, ref, want=(True,) * 4):
    for k, (g, r, w) in enumerate(zip(dx, ref[4], want)):
        if not w:
            assert g is None, (tag, 'hvid'[k])
            continue
        assert g is not None and g.shape == r.shape and g.dtype == torch.float32, (tag, 'hvid'[k])
        q = ratio(g, r)
        print(f'{tag} d loss / d {"hvid"[k]}_views: max |gradient| {float(r.abs().max()):.3e}, error at {q:.3e} of the bar '
              f'{bar(r):.3e}')
        assert q <= 1.0, (tag, 'hvid'[k], q)


def check_parity(kind, variant, frame, eval_mode=False):
    """the four input gradients against float64; every parameter gradient of the same backward bit for bit that of a second
    run from the same state in which no stack requires a gradient"""
    tag = f'{"eval " if eval_mode else ""}{kind} {variant} {frame}'
    m, out, dx, ref = _gpu_run(kind, variant, frame, eval_mode)
    _check_dx(tag, dx, ref)
    m2, out2, dx2, _ = _gpu_run(kind, variant, frame, eval_mode, want=(False,) * 4)
    assert dx2 == [None] * 4
    for k, v in out.items():
        assert (v is None and out2[k] is None) or torch.equal(v, out2[k]), (tag, k)
    for (n, p), (_, q) in zip(m.named_parameters(), m2.named_parameters()):
        assert p.grad is not None and q.grad is not None, (tag, n)
        assert torch.equal(p.grad, q.grad), (tag, n)
    for (n, a), (_, b) in zip(m.named_buffers(), m2.named_buffers()):
        assert torch.equal(a, b), (tag, n)


# ------------------------------------------------------------------------------------------------ 1, 2: parity
@pytest.mark.parametrize('frame', FRAMES)
@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('kind', KINDS)
def test_input_gradients_against_float64_in_train_mode(kind, variant, frame):
    check_parity(kind, variant, frame)


@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('kind', KINDS)
def test_input_gradients_against_float64_in_eval_mode(kind, variant):
    """m.eval() with parameters that require gradients: BatchNorm's running statistics are constants of the graph"""
    check_parity(kind, variant, EVAL_FRAMES[kind], eval_mode=True)


# ------------------------------------------------------------------------------------------------ 3: a partial request
@pytest.mark.parametrize('kind', KINDS)
def test_only_the_v_stack_asks(kind, monkeypatch):
    variant, frame = 'upr', (2, 9, 13)
    convs, wgrads = _conv_entries()
    counts = {}
    for want in ((False,) * 4, (False, True, False, False)):
        spy = _Spy(monkeypatch)
        m, _, dx, ref = _gpu_run(kind, variant, frame, want=want)
        _check_dx(f'partial {kind}', dx, ref, want)
        counts[want] = (sum(spy.names.count(n) for n in convs), spy.names.count('mmlf_unpack_nchw'), spy.count(*wgrads))
        assert all(p.grad is not None for p in m.parameters())
    (c0, u0, w0), (c1, u1, w1) = counts.values()
    assert (c1 - c0, u1 - u0, w1 - w0) == (1, 1, 0), counts
    assert u0 == 1                                        # (the forward's own unpack of the network output)


# ------------------------------------------------------------------------------------------------ 4: frozen, train mode
@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('kind', KINDS)
def test_frozen_net_in_train_mode(kind, variant, monkeypatch):
    frame = (3, 5, 29)
    spy = _Spy(monkeypatch)
    m, out, dx, ref = _gpu_run(kind, variant, frame, frozen=True)
    _check_dx(f'frozen train {kind} {variant}', dx, ref)
    assert not [n for n in spy.names if 'wgrad' in n], spy.names
    assert all(p.grad is None for p in m.parameters())
    if kind != 'nobn2':
        assert spy.names.count('mmlf_bn_bwd_reduce') == spy.names.count('mmlf_bn_bwd_apply') == 10      # 4 x 2 + 2 blocks
    # the BatchNorm buffers moved exactly as in an unfrozen forward, and the output is the same function
    m2, out2, _, _ = _gpu_run(kind, variant, frame, want=(False,) * 4)
    moved = 0
    for (n, a), (_, b) in zip(m.named_buffers(), m2.named_buffers()):
        assert torch.equal(a, b), n
        moved += int(n.endswith('num_batches_tracked') and int(a) > 0)
    assert moved == (0 if kind == 'nobn2' else 6)
    for k, v in out.items():
        assert (v is None and out2[k] is None) or torch.equal(v, out2[k]), k


# ------------------------------------------------------------------------------------------------ 5: frozen, eval mode
@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('kind', KINDS)
def test_frozen_net_in_eval_mode(kind, variant, monkeypatch):
    """2x2 with BatchNorm: the folded inference launches under a tape, and a ReLU-only backward through the folded filters.
    3x3: the unfolded eval path, whose backward takes BatchNorm's coefficients from the saved scale (no reduce pass)."""
    frame = EVAL_FRAMES[kind]
    spy = _Spy(monkeypatch)
    m, out, dx, ref = _gpu_run(kind, variant, frame, eval_mode=True, frozen=True)
    names = list(spy.names)
    _check_dx(f'frozen eval {kind} {variant}', dx, ref)
    assert all(p.grad is None for p in m.parameters())
    assert not [n for n in names if 'wgrad' in n], names
    assert 'mmlf_bn_bwd_reduce' not in names
    assert not [n for n in names if n.startswith('mmlf_bn_stats_')], names
    if kind == 'bn2':
        assert not [n for n in names if n.startswith('mmlf_bn_apply_relu') or n.startswith('mmlf_bn_bwd')], names
        assert names.count('mmlf_fold_bn_eval') == 10 and names.count('mmlf_relu_bwd_slice') == 4
        # (mmlf_bn_coeffs_eval is the fold's own: the forward's; the backward makes no mmlf_bn_* launch at all)
        after_fwd = names[names.index('mmlf_unpack_nchw'):]
        assert 'mmlf_relu_bwd_slice' in after_fwd and not [n for n in after_fwd if n.startswith('mmlf_bn_')], after_fwd
    if kind != 'k3':
        with torch.no_grad():
            plain = m(*inputs(frame, ref[2], _dev())[0])
        for k, v in out.items():
            assert (v is None and plain[k] is None) or torch.equal(v.detach(), plain[k]), k
    for n, b in m.named_buffers():                         # eval mode: nothing moves
        assert torch.equal(b.cpu(), torch.from_numpy(np.asarray(ref[1][n]))), n


@pytest.mark.parametrize('eval_mode', [False, True])
@pytest.mark.parametrize('mode', ['f32', 'bf16x6'])
def test_frozen_net_in_the_other_modes(mode, eval_mode, monkeypatch):
    """no ReLU bits in these modes: the ReLU-only backward of the folded blocks goes by the saved activations"""
    from mmlf_amd import engine
    monkeypatch.setattr(engine, 'CONV_MODE', mode)
    frame = EVAL_FRAMES['bn2']
    spy = _Spy(monkeypatch)
    m, out, dx, ref = _gpu_run('bn2', 'upr', frame, eval_mode=eval_mode, frozen=True)
    _check_dx(f'frozen {mode} eval={eval_mode}', dx, ref)
    assert not [n for n in spy.names if 'wgrad' in n or n == 'mmlf_conv2x2_h2'], spy.names
    assert ('mmlf_bn_bwd_apply' in spy.names) == (not eval_mode)
    assert all(p.grad is None for p in m.parameters())


# ------------------------------------------------------------------------------------------------ 6: the other modes
CHILD = """
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {root!r} + '/tests')
from mmlf_amd import engine
assert engine.CONV_MODE == {mode!r}, engine.CONV_MODE
import test_gpu_input_grad as t
t.check_parity('bn2', 'upr', (2, 9, 13))
print('child ok')
"""


@pytest.mark.parametrize('mode', ['bf16x6', 'f32'])
def test_input_gradients_in_the_other_modes(mode):
    """MMLF_CONV_MODE is read once per process: a fresh child each (tests/test_gpu_kernels.py does the same)"""
    env = dict(os.environ, MMLF_CONV_MODE=mode)
    p = subprocess.run([sys.executable, '-c', CHILD.format(root=ROOT, mode=mode)], env=env, capture_output=True, text=True,
                       timeout=300)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and 'child ok' in p.stdout, p.stderr[-3000:]


# ------------------------------------------------------------------------------------------------ audit, replicas
@pytest.mark.parametrize('kind', KINDS)
def test_extent_audit_covers_the_input_gradient_launches(kind, monkeypatch):
    from mmlf_amd import engine
    monkeypatch.setattr(engine, 'CONV_MODE', 'f16x3')
    monkeypatch.setattr(engine, 'CHECK_EXTENTS', True)
    spy = _Spy(monkeypatch)
    before = engine.EXTENT_CHECKS
    _, _, dx, ref = _gpu_run(kind, 'upr', (2, 9, 13))
    _check_dx(f'audited {kind}', dx, ref)
    audited = ('mmlf_conv2x2_h2', 'mmlf_conv2x2_wgrad_h2', 'mmlf_relu_bwd_slice', 'mmlf_conv3x3', 'mmlf_conv3x3_wgrad')
    launches = [n for n in spy.names if n in audited]
    assert launches and engine.EXTENT_CHECKS - before == len(launches)
    assert spy.count('mmlf_audit_') == len(launches)


def test_dataparallel_replicas_return_input_gradients():
    """two replicas on the one GPU (tests/test_gpu_nobn.py): without BatchNorm the net is a function of each patch alone, so
    the scattered stacks' gradients are those of the whole batch"""
    kind, variant, frame = 'nobn2', 'upr', (4, 9, 13)
    from test_input_grad_cpu import loss_of
    kw, state, seed, scale, ref, cond = reference(kind, variant, frame)
    assert cond <= 0.1
    dev = _dev()
    m = build(kw, state, dev)
    dp = torch.nn.DataParallel(m, device_ids=[0, 0])
    dp.train()
    stacks, gt, mask, cls = inputs(frame, seed, dev)
    xs = [s.clone().requires_grad_(True) for s in stacks]
    out = dp(*xs)
    (loss_of(variant, out, gt, mask, cls) * scale).backward()
    _check_dx('DataParallel', [x.grad for x in xs], reference(kind, variant, frame))
    assert all(p.grad is not None for p in m.parameters())


# ------------------------------------------------------------------------------------------------ 7: kernel level
def _transform(x, variant):
    """the image transform of a stream's filter variant (tests/test_gpu_kernels.py::test_filter_variants_equal_image_transforms)"""
    if variant == 0:
        return x
    x = x.transpose(2, 3)
    return x.flip(-1) if variant == 2 else x


def _untransform(y, variant):
    if variant == 0:
        return y
    return (y.flip(-1) if variant == 2 else y).transpose(2, 3)


def _dgrad_reference(w, g, variant, B, N, H, W, ksize):
    """float64 autograd of the forward layer N -> K (pad 1) on the variant-transformed image, in the gradient g of its output"""
    x = torch.zeros((B, N, H, W), dtype=torch.float64, requires_grad=True)
    y = _untransform(torch.nn.functional.conv2d(_transform(x, variant), torch.from_numpy(w).double(), padding=1), variant)
    assert y.shape == g.shape, (y.shape, g.shape)
    (y * torch.from_numpy(g).double()).sum().backward()
    assert ksize in (2, 3)
    return x.grad.numpy()


def _check_stored(tag, out, cs, N, geo, H, W, ref):
    full = out.cpu().numpy()
    assert np.isfinite(full).all(), tag
    got, g = nchw_from_grid(full, cs, N, geo, H, W, 1)
    np.testing.assert_allclose(got, ref, rtol=2e-5, atol=2e-5 * max(1.0, np.abs(ref).max()), err_msg=tag)
    assert np.abs(ref).max() > 1e-3, tag
    # everything outside the stored extent is exactly zero: border, pad channels and slack
    g2 = g.copy()
    g2[:, 1:H + 1, 1:W + 1, :N] = 0
    assert not g2.any(), tag
    assert not full.reshape(geo.alloc, cs)[geo.NQ:].any(), tag


@pytest.mark.parametrize('B,H,W', DGRAD_FRAMES)
@pytest.mark.parametrize('mode', MODES)
def test_first_layer_data_gradient_2x2(mode, B, H, W, monkeypatch):
    from mmlf_amd import engine
    monkeypatch.setattr(engine, 'CONV_MODE', mode)
    dev = _dev()
    geo = engine.Geometry(B, H, W)
    for K, N in DGRAD_SHAPES:
        cs_g, cs_dx = engine.cs_of(K), engine.cs_of(N)
        for variant in (0, 1, 2):
            tag = f'{mode} {K}->{N} variant {variant} B={B} {H}x{W}'
            rs = np.random.RandomState(K * 1000 + N * 10 + variant + W)
            w = rs.uniform(-0.5, 0.5, (K, N, 2, 2)).astype(np.float32)
            g = rs.uniform(-1, 1, (B, K, H + 1, W + 1)).astype(np.float32)
            ref = _dgrad_reference(w, g, variant, B, N, H, W, 2)
            pk = engine.pack_filter(torch.from_numpy(w).to(dev), variant, True)
            gg = torch.from_numpy(grid_from_nchw(g, cs_g, geo, offset=0)).to(dev)
            out = torch.full((geo.alloc * cs_dx,), float('nan'), device=dev)
            out[:(geo.P + 1) * cs_dx] = 0
            out[geo.NQ * cs_dx:] = 0
            engine.conv(geo, gg, cs_g, K, pk, None, N, out, cs_dx, geo.P + 1, H, W, False)
            _check_stored(tag, out, cs_dx, N, geo, H, W, ref)


@pytest.mark.parametrize('B,H,W', DGRAD_FRAMES)
def test_first_layer_data_gradient_3x3(B, H, W):
    from mmlf_amd import engine
    dev = _dev()
    geo = engine.Geometry(B, H, W, 3)
    for K, N in K3_DGRAD_SHAPES:
        cs_g, cs_dx = engine.cs_of(K), engine.cs_of(N)
        for variant in (0, 1, 2):
            tag = f'3x3 {K}->{N} variant {variant} B={B} {H}x{W}'
            rs = np.random.RandomState(K * 1000 + N * 10 + variant + W + 5)
            w = rs.uniform(-0.5, 0.5, (K, N, 3, 3)).astype(np.float32)
            g = rs.uniform(-1, 1, (B, K, H, W)).astype(np.float32)
            ref = _dgrad_reference(w, g, variant, B, N, H, W, 3)
            pk = engine.pack_filter3(torch.from_numpy(w).to(dev), variant, True)
            gg = torch.from_numpy(grid_from_nchw(g, cs_g, geo, offset=1)).to(dev)
            out = torch.full((geo.alloc * cs_dx,), float('nan'), device=dev)
            out[:(geo.P + 1) * cs_dx] = 0
            out[geo.NQ * cs_dx:] = 0
            engine.conv3(geo, gg, cs_g, K, pk, None, N, out, cs_dx, False)
            _check_stored(tag, out, cs_dx, N, geo, H, W, ref)
