"""--model_ksize 3 on the GPU: the exact-f32 3x3 kernels (mmlf_conv3x3 forward / data gradient, mmlf_conv3x3_wgrad) against
float64 torch on the CPU, and the native k=3 trunk against the reference's tiny run (g12) and against the stock-torch path of
the same module (`_native_ok = False`) at larger shapes, in TrainStep and in the Ensamble."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import BASE_KW, TINY_KW, VARIANTS, load_golden
from mmlf_amd import synth

pytestmark = pytest.mark.gpu
K3_TINY_KW = dict(TINY_KW, model_ksize=3)
K3_BASE_KW = dict(BASE_KW, model_ksize=3)
PAIRS = [(27, 8), (8, 8), (27, 70), (70, 70), (280, 280), (280, 2), (2, 2), (280, 108), (108, 108)]


def _dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def k3_spec(kw):
    return [(n, (shape[0], shape[1], 3, 3) if kind == 'conv_w' else shape, kind) for n, shape, kind in synth.param_spec(**kw)]


def _model(kw, state, dev):
    from mmlf_amd.feed_forward import FeedForward
    m = FeedForward(**kw)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    return m.to(dev)


# ------------------------------------------------------------------------------------------------ kernel level
def _fwd_ref(x, w, b, variant):
    """what the stock path computes for a stream net on the transformed image (feed_forward.py _torch_trunk)"""
    if variant == 0:
        return F.conv2d(x, w, b, padding=1)
    if variant == 1:
        return F.conv2d(x.transpose(2, 3), w, b, padding=1).transpose(2, 3)
    return F.conv2d(x.transpose(2, 3).flip(-1), w, b, padding=1).flip(-1).transpose(2, 3)


def _to_grid(geo, t, cs):
    from mmlf_amd import _lib
    from mmlf_amd._lib import call, ptr
    g = geo.buf(cs, t.device)
    call('mmlf_pack_nchw', ptr(t.contiguous()), t.shape[1], ptr(g), cs, geo.B, geo.H, geo.W, ptr(g.absmax), _lib.stream_ptr())
    return g


def _grid_view(geo, g, cs):
    return g[:geo.NQ * cs].view(geo.B, geo.R, geo.P, cs)


def _check(got, ref, bound, what, tol=2e-5):
    err = (got - ref).abs()
    lim = tol * bound + 1e-6 * float(bound.max()) + 1e-30
    assert bool((err <= lim).all()), (what, float((err / lim).max()))


@pytest.mark.parametrize('variant', [0, 1, 2])
@pytest.mark.parametrize('cin,cout', PAIRS)
def test_conv3x3_kernels_against_float64(cin, cout, variant):
    from mmlf_amd import engine
    dev = _dev()
    B, H, W = 2, 9, 13
    gen = torch.Generator().manual_seed(cin * 1000 + cout * 10 + variant)
    x = torch.randn((B, cin, H, W), generator=gen, dtype=torch.float64)
    w = torch.randn((cout, cin, 3, 3), generator=gen, dtype=torch.float64) / np.sqrt(9 * cin)
    b = torch.randn((cout,), generator=gen, dtype=torch.float64)
    ref = torch.randn((B, cout, H, W), generator=gen, dtype=torch.float64)
    gout = torch.randn((B, cout, H, W), generator=gen, dtype=torch.float64)
    geo = engine.Geometry(B, H, W, 3)
    cs_in, cs_out = engine.cs_of(cin), engine.cs_of(cout)
    xf, wf, bf = x.float().to(dev), w.float().to(dev), b.float().to(dev)
    xg = _to_grid(geo, xf, cs_in)
    z = _fwd_ref(x, w, b, variant)
    bound = _fwd_ref(x.abs(), w.abs(), b.abs(), variant)
    pk = engine.pack_filter3(wf, variant, False)

    # plain forward: the whole grid (zero frame, zero pad channels) is what it should be
    out = geo.buf(cs_out, dev)
    engine.conv3(geo, xg, cs_in, cin, pk, bf, cout, out, cs_out, False)
    full = _grid_view(geo, out, cs_out).double().cpu()
    want = torch.zeros_like(full)
    want[:, 1:H + 1, 1:W + 1, :cout] = z.permute(0, 2, 3, 1)
    bfull = torch.zeros_like(full)
    bfull[:, 1:H + 1, 1:W + 1, :cout] = bound.permute(0, 2, 3, 1)
    _check(full, want, bfull, 'forward')

    # fused ReLU, ReLU by reference, channel-slice store (the other channels keep what they held)
    refg = _to_grid(geo, ref.float().to(dev), cs_out)
    off, cs_wide = 8, cs_out + 16
    wide = geo.buf(cs_wide, dev)
    wv = _grid_view(geo, wide, cs_wide)
    wv[:, :, :, :] = 7.0
    wv[:, 0] = 0.0
    wv[:, :, 0] = 0.0
    engine.conv3(geo, xg, cs_in, cin, pk, bf, cout, wide, cs_wide, True, ref=refg, cs_ref=cs_out, n_store=cout, out_off=off)
    wv = _grid_view(geo, wide, cs_wide).double().cpu()
    got = wv[:, 1:H + 1, 1:W + 1, off:off + cout].permute(0, 3, 1, 2)
    _check(got, torch.relu(z) * (ref > 0), bound, 'forward relu/ref/slice')
    assert bool((wv[:, 1:, 1:, :off] == 7.0).all()) and bool((wv[:, 1:, 1:, off + cout:] == 7.0).all())
    frame = wv[..., off:off + cout].clone()
    frame[:, 1:H + 1, 1:W + 1] = 0
    assert bool((frame == 0).all())

    # data gradient: the same kernel on the dgrad-packed filter
    xr = x.clone().requires_grad_(True)
    _fwd_ref(xr, w, b, variant).backward(gout)
    xa = x.abs().requires_grad_(True)
    _fwd_ref(xa, w.abs(), None, variant).backward(gout.abs())
    gg = _to_grid(geo, gout.float().to(dev), cs_out)
    dx = geo.buf(cs_in, dev)
    engine.conv3(geo, gg, cs_out, cout, engine.pack_filter3(wf, variant, True), None, cin, dx, cs_in, False)
    got = _grid_view(geo, dx, cs_in).double().cpu()[:, 1:H + 1, 1:W + 1, :cin].permute(0, 3, 1, 2)
    _check(got, xr.grad, xa.grad, 'data gradient')

    # weight + bias gradient, accumulated into what gw / gb hold
    wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    _fwd_ref(x, wr, br, variant).backward(gout)
    wa, ba = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    _fwd_ref(x.abs(), wa, ba, variant).backward(gout.abs())
    gw0 = torch.randn((cout, cin, 3, 3), generator=gen, dtype=torch.float64)
    gb0 = torch.randn((cout,), generator=gen, dtype=torch.float64)
    gw, gb = gw0.float().to(dev), gb0.float().to(dev)
    wsp = torch.empty(int(engine._lib.load().mmlf_wgrad3x3_workspace_floats(cin, cout, B, H, W)), device=dev)
    engine.wgrad3(geo, xg, cs_in, cin, gg, cs_out, cout, gw, gb, variant, wsp)
    _check(gw.double().cpu(), gw0.float().double() + wr.grad, wa.grad + gw0.abs(), 'weight gradient')
    _check(gb.double().cpu(), gb0.float().double() + br.grad, ba.grad + gb0.abs(), 'bias gradient')


def test_k3_training_step_passes_the_extent_audit(monkeypatch):
    from mmlf_amd import engine
    from mmlf_amd.train import TrainStep
    dev = _dev()
    kw = dict(K3_TINY_KW, model_uncert=True)
    m = _model(kw, synth.synth_state(k3_spec(kw), seed=3), dev)
    monkeypatch.setattr(engine, 'CHECK_EXTENTS', True)
    before = engine.EXTENT_CHECKS
    stacks, gt, mask = synth.synth_inputs(2, 20, seed=4)
    step = TrainStep(m, lr=1e-3, loss_margin=3)
    loss = step(*[torch.from_numpy(s).to(dev) for s in stacks], torch.from_numpy(gt).to(dev), torch.from_numpy(mask).to(dev), 1)
    m.eval()
    with torch.no_grad():
        m(*[torch.from_numpy(s).to(dev) for s in stacks])
    torch.cuda.synchronize()
    assert np.isfinite(float(loss))
    assert engine.EXTENT_CHECKS > before + 40


# ------------------------------------------------------------------------------------------------ module level
@pytest.mark.parametrize('variant', list(VARIANTS))
def test_g12_k3_tiny_forward_backward_vs_reference(variant):
    from mmlf_amd import dl, loss
    g = load_golden(f'g12_k3_tiny_{variant}.npz')
    kw = dict(K3_TINY_KW, **VARIANTS[variant])
    state = synth.synth_state(k3_spec(kw), seed=int(g['state_seed']))
    dev = _dev()
    m = _model(kw, state, dev)
    assert m._native_ok
    stacks = [torch.from_numpy(g[f'in{i}']).to(dev) for i in range(4)]
    m.eval()
    with torch.no_grad():
        out = m(*stacks)
    for k, v in out.items():
        if v is not None:
            np.testing.assert_allclose(v.cpu().numpy(), g[f'eval_{k}'], rtol=5e-5, atol=5e-6, err_msg=f'eval {k}')
    m.train()
    out = m(*stacks)
    for k, v in out.items():
        if v is not None and k != 'one_hot' and f'train_{k}' in g:
            np.testing.assert_allclose(v.detach().cpu().numpy(), g[f'train_{k}'], rtol=1e-4, atol=1e-5, err_msg=f'train {k}')
    gt, mask = torch.from_numpy(g['gt']).to(dev), torch.from_numpy(g['mask']).to(dev)
    if variant == 'upr':
        lv = loss.ImprovedUncertaintyL1Loss()(out, gt, mask, None)
    elif variant == 'dpp':
        lv = loss.MaskedCrossEntropy()(out, dl.reg_to_class(gt, -3.5, 3.5, 108), mask)
    else:
        lv = loss.MaskedL1Loss()(out, gt, mask)
    np.testing.assert_allclose(lv.item(), g['loss'], rtol=2e-5)
    lv.backward()
    for n, p in m.named_parameters():
        ref = g[f'grad/{n}']
        scale = max(np.abs(ref).max(), 1e-6)
        err = np.abs(p.grad.cpu().numpy() - ref).max()
        assert err <= 5e-4 * scale + 5e-7, (n, err, scale)
    for k, v in m.state_dict().items():
        if 'running' in k:
            np.testing.assert_allclose(v.cpu().numpy(), g[f'post/{k}'], rtol=1e-5, atol=1e-6, err_msg=k)
        if 'num_batches' in k:
            assert int(v) == int(g[f'post/{k}']), k


def _rel(a, b):
    return float((a - b).double().norm() / max(float(b.double().norm()), 1e-30))


@pytest.mark.parametrize('variant', list(VARIANTS))
def test_k3_base_size_native_vs_stock_on_cuda(variant):
    """BASE_KW with 3x3 filters, B=4, 64 x 64: the native trunk against the module's own stock-torch path on the same device"""
    from mmlf_amd import dl, loss
    dev = _dev()
    kw = dict(K3_BASE_KW, **VARIANTS[variant])
    state = synth.synth_state(k3_spec(kw), seed=21)
    stacks, gt, mask = synth.synth_inputs(4, 64, seed=8)
    m_mask = torch.from_numpy(mask).int() * loss.create_mask_margin(mask.shape, 11)
    res = {}
    for native in (True, False):
        m = _model(kw, state, dev)
        m._native_ok = native
        m.train()
        out = m(*[torch.from_numpy(s).to(dev) for s in stacks])
        gtd, md = torch.from_numpy(gt).to(dev), m_mask.to(dev)
        if variant == 'upr':
            lv = loss.ImprovedUncertaintyL1Loss()(out, gtd, md, None)
        elif variant == 'dpp':
            lv = loss.MaskedCrossEntropy()(out, dl.reg_to_class(gtd, -3.5, 3.5, 108), md)
        else:
            lv = loss.MaskedL1Loss()(out, gtd, md)
        lv.backward()
        res[native] = ({k: v.detach().cpu() for k, v in out.items() if v is not None and k != 'one_hot'}, lv.item(),
                       {n: p.grad.cpu() for n, p in m.named_parameters()},
                       {k: v.cpu() for k, v in m.state_dict().items() if 'running' in k})
    (o1, l1, g1, s1), (o0, l0, g0, s0) = res[True], res[False]
    for k in o0:
        if variant == 'dpp' and k in ('mean', 'logvar'):
            continue          # arg-max depth and the variance around it: a flipped bin moves a pixel by 7/107 (below)
        assert _rel(o1[k], o0[k]) <= 2e-4, (k, _rel(o1[k], o0[k]))
    if variant == 'dpp':
        flips = float((o1['mean'] != o0['mean']).double().mean())
        assert flips <= 2e-3, flips
    assert abs(l1 - l0) <= 1e-4 * abs(l0)
    # Gradients of an 11-block net are ill-conditioned (tests/test_gpu_model.py G2_GRAD_BAR: 1.2-2.6 % per tensor between the
    # reference's float32 run and the native one at k=2); here two float32 implementations of the k=3 net are compared.  Measured
    # (UPR, the widest): 0.1-0.2 % on the out_net tensors, 2-3.4 % on every stream tensor below them (median 2.5 %) -- the pattern
    # of a ReLU flipping near the head; the tiny nets' gradients agree with the reference's to 5e-4 (g12 above).  The bias of a convolution in front of BatchNorm has a gradient of
    # exactly zero in exact arithmetic: both paths give rounding noise of ~1e-8 there, hence the absolute floor.
    rels = {}
    for n in g0:
        err = float((g1[n] - g0[n]).double().norm())
        rels[n] = err / (float(g0[n].double().norm()) + 1e-6 * g0[n].numel() ** 0.5 / 3e-2)
    worst = max(rels, key=rels.get)
    assert rels[worst] <= 6e-2 and float(np.median(list(rels.values()))) <= 4e-2, (worst, sorted(rels.values())[-5:],
                                                                                     float(np.median(list(rels.values()))))
    for k in s0:
        assert _rel(s1[k], s0[k]) <= 1e-4, k


def test_k3_train_step_native_vs_stock():
    from mmlf_amd.train import TrainStep
    dev = _dev()
    kw = dict(K3_TINY_KW, model_uncert=True)
    state = synth.synth_state(k3_spec(kw), seed=17)
    w0 = {k: torch.from_numpy(np.asarray(v)) for k, v in state.items()}
    res = {}
    for native in (True, False):
        m = _model(kw, state, dev)
        m._native_ok = native
        step = TrainStep(m, lr=1e-3, loss_margin=3)
        for it in range(3):
            stacks, gt, mask = synth.synth_inputs(2, 24, seed=40 + it)
            step(*[torch.from_numpy(s).to(dev) for s in stacks], torch.from_numpy(gt).to(dev),
                 torch.from_numpy(mask).to(dev), it + 1)
        res[native] = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    for k, v in res[False].items():
        if v.dtype != torch.float32:
            assert torch.equal(res[True][k], v), k
            continue
        if k.endswith('.2.bias') and k[:-len('2.bias')] + '3.weight' in res[False]:
            continue      # in front of BatchNorm: a zero gradient up to rounding noise, which Adam turns into +-lr steps
        moved = float((v - w0[k]).double().norm())
        assert float((res[True][k] - v).double().norm()) <= 0.05 * moved + 1e-6, k


def test_k3_ensamble_native_vs_stock():
    from mmlf_amd.ensamble import Ensamble
    dev = _dev()
    kw = dict(K3_TINY_KW, model_uncert=True)
    state = synth.synth_state(k3_spec(kw), seed=31)
    stacks, _, _ = synth.synth_inputs(1, 32, seed=9)
    res = {}
    for native in (True, False):
        m = _model(kw, state, dev).eval()
        m._native_ok = native
        ens = Ensamble(m, -3.5, 3.5, 0.1).eval()
        with torch.no_grad():
            res[native] = {k: v.cpu() for k, v in ens(*[torch.from_numpy(s).to(dev) for s in stacks]).items()}
    for k in res[False]:
        np.testing.assert_allclose(res[True][k].numpy(), res[False][k].numpy(), rtol=1e-4, atol=2e-5, err_msg=k)
