"""The head outputs under autograd on the native path (round 5).

The reference builds `posterior` (UPR: a Laplace density over 108 depth bins; DPP: the softmax of the scores) and the DPP
`logvar` as differentiable functions of the network output (reference mmlf/model/feed_forward.py:276-302).  None of its
losses uses them (mmlf/model/loss.py:70,146,264), but the graph is there; the native path used to compute them from a
detached tensor.  They are autograd Functions over mmlf_head_upr / mmlf_head_dpp with backward kernels now: checked here
against torch's own autograd of the reference's expressions in float64, and end to end against the stock-torch branch of
the same module on the CPU."""
import numpy as np
import pytest
import torch

from conftest import TINY_KW
from mmlf_amd import synth

pytestmark = pytest.mark.gpu


def _laplacian(x, mu, b):                      # reference feed_forward.py:9-12
    return 1.0 / (2.0 * b.unsqueeze(1)) * torch.exp(-torch.abs(x - mu.unsqueeze(1)) / b.unsqueeze(1))


def test_upr_posterior_gradient_equals_autograd_of_the_reference_expression():
    from mmlf_amd.feed_forward import _HeadUprFn
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(4)
    B, S, H, W = 3, 108, 5, 7
    out = torch.stack([torch.randn((B, H, W), generator=g) * 1.5, torch.rand((B, H, W), generator=g) * 3 - 2], 1)
    go = torch.randn((B, S, H, W), generator=g)
    grid64 = torch.from_numpy(np.linspace(-3.5, 3.5, S))
    grid = grid64.float()
    # float64 autograd of the reference graph (the float32 grid values, as the module uses them)
    o64 = out.double().requires_grad_(True)
    post64 = _laplacian(grid.double().view(1, S, 1, 1).expand(B, S, H, W), o64[:, 0], torch.exp(o64[:, 1]))
    post64.backward(go.double())
    od = out.to(dev).requires_grad_(True)
    post = _HeadUprFn.apply(od, grid.to(dev), S)
    post.backward(go.to(dev))
    torch.testing.assert_close(post.detach().cpu().double(), post64.detach(), rtol=2e-5, atol=1e-7)
    ref = o64.grad
    err = (od.grad.cpu().double() - ref).abs().max() / ref.abs().max()
    assert float(err) <= 2e-5, float(err)


@pytest.mark.parametrize('which', ['posterior', 'logvar', 'both', 'posterior_alone', 'logvar_alone'])
def test_dpp_head_gradients_equal_autograd_of_the_reference_expressions(which):
    """*_alone (round 6): the other output is not part of the graph at all, so its gradient arrives as None
    (ctx.set_materialize_grads(False)) and mmlf_head_dpp_bwd runs with a NULL pointer for it"""
    from mmlf_amd.feed_forward import _HeadDppFn
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(5)
    B, S, H, W = 2, 108, 4, 6
    scores = torch.randn((B, S, H, W), generator=g) * 2
    go_post, go_lv = torch.randn((B, S, H, W), generator=g), torch.randn((B, H, W), generator=g)
    grid_t = torch.linspace(-3.5, 3.5, S)                                     # dl.py:177
    grid_np = torch.from_numpy(np.linspace(-3.5, 3.5, S)).float()             # feed_forward.py:287-288
    s64 = scores.double().requires_grad_(True)
    one_hot = (torch.max(s64, 1, keepdim=True)[0] == s64).double()
    e = torch.exp(s64)
    post64 = e / torch.sum(e, 1, keepdim=True)
    mean64 = torch.sum(grid_t.double().view(1, -1, 1, 1) * one_hot, 1)
    lv64 = torch.log(torch.sum((grid_np.double().view(1, -1, 1, 1) - mean64.unsqueeze(1)) ** 2.0 * post64, 1))
    alone = which.endswith('_alone')
    which = which.replace('_alone', '')
    loss64 = (post64 * go_post.double()).sum() * (which != 'logvar') + (lv64 * go_lv.double()).sum() * (which != 'posterior')
    loss64.backward()
    sd = scores.to(dev).requires_grad_(True)
    oh, post, mean, lv = _HeadDppFn.apply(sd, grid_t.to(dev), grid_np.to(dev), S)
    assert not oh.requires_grad and not mean.requires_grad and post.requires_grad and lv.requires_grad
    if alone:
        loss = (post * go_post.to(dev)).sum() if which == 'posterior' else (lv * go_lv.to(dev)).sum()
    else:
        loss = (post * go_post.to(dev)).sum() * (which != 'logvar') + (lv * go_lv.to(dev)).sum() * (which != 'posterior')
    loss.backward()
    torch.testing.assert_close(mean.cpu().double(), mean64.detach(), rtol=0, atol=1e-6)
    torch.testing.assert_close(lv.detach().cpu().double(), lv64.detach(), rtol=1e-5, atol=1e-5)
    ref = s64.grad
    err = (sd.grad.cpu().double() - ref).abs().max() / ref.abs().max()
    assert float(err) <= 2e-5, float(err)


@pytest.mark.parametrize('variant', ['upr', 'dpp'])
def test_a_loss_on_the_posterior_trains_the_network_on_the_native_path(variant):
    """end to end: d (sum w * posterior [+ logvar]) / d parameters, native cuda path against the stock-torch branch of the
    same module on the CPU (what the reference's graph gives)"""
    from mmlf_amd.feed_forward import FeedForward
    kw = dict(TINY_KW, model_uncert=variant == 'upr', model_discrete=variant == 'dpp')
    state = synth.synth_state(synth.param_spec(**kw), seed=9)
    stacks, _, _ = synth.synth_inputs(2, 16, seed=9)
    g = torch.Generator().manual_seed(9)
    wts = torch.rand((2, 108, 16, 16), generator=g)
    grads = {}
    for dev in ('cpu', 'cuda:0'):
        m = FeedForward(**kw)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
        m.to(dev).train()
        out = m(*[torch.from_numpy(s).to(dev) for s in stacks])
        assert out['posterior'].requires_grad
        loss = (out['posterior'] * wts.to(dev)).sum() + (out['logvar'].sum() if variant == 'dpp' else 0.0)
        loss.backward()
        grads[dev] = {n: p.grad.detach().cpu().double() for n, p in m.named_parameters()}
    # the biases of the convolutions in front of a train-mode BatchNorm have an analytically ZERO gradient (rounding noise
    # of 1e-14 on both devices): compared in absolute terms; every other tensor relative to its own norm
    big = max(float(v.norm()) for v in grads['cpu'].values())
    assert big > 1.0
    worst = 0.0
    for n, ref in grads['cpu'].items():
        got = grads['cuda:0'][n]
        if float(ref.norm()) > 1e-4 * big:
            worst = max(worst, float((got - ref).norm() / ref.norm()))
        else:
            assert n.endswith('.2.bias') and float(got.norm()) <= 1e-6 * big, (n, float(got.norm()))
    assert worst <= 1e-3, worst          # (float32 trunks on two devices: 1e-5 measured; the head kernels are pinned above at 2e-5)


# ------------------------------------------------------------------------------------- the four kernels, called directly
# mmlf_head_upr / _upr_bwd / _dpp / _dpp_bwd through their C entry points, with the conventions of tests/test_gpu_elementwise.py
# (guard bands, NaN pre-fill, every element compared) against tests_helpers.upr_ref / dpp_ref / dpp_bwd_ref, which
# tests/test_loss_head_cpu.py pins to autograd of the expressions above.  Element-wise bars, U = 2^-24, c = 2 EXPLOG_ULPS:
# EXPLOG_ULPS = 2 float32 ulps is the accuracy this module ASSUMES of the device expf and logf -- an assumption, not a
# measurement (tests/test_gpu_losses.py says the same of the losses).  A result below the normal range may carry 2^-126
# absolute (a flushed or denormal expf): FLOOR.
#
# Headroom of the first run on an MI355X (largest error / bar per bar): upr posterior 0.4987, upr backward 0.4371; dpp
# posterior 0.3538, mean 0.6794, logvar 0.4023, backward 0.2215 (both) / 0.3428 (posterior) / 0.1348 (logvar).  Every bar but
# the mean's holds EXPLOG_ULPS: the worst ratio seen with it is 0.4987.
from tests_helpers import (LOSS_FRAMES, LOSS_STRIDE_FRAME, RATIOS, _Pool, _bar, _close, _same, dpp_bwd_ref,  # noqa: E402
                           dpp_ref, upr_ref)

HEAD_FRAMES, HEAD_STRIDE_FRAME, HEAD_STEPS, HEAD_STRIDE_STEPS = LOSS_FRAMES, LOSS_STRIDE_FRAME, [1, 2, 108], 2
EXPLOG_ULPS = 2.0
U, FLOOR, NAN = 2.0 ** -24, 2.0 ** -126, float('nan')
TOP = 7.0                                    # the tied maxima: above every drawn score (they are clamped to +-6)


@pytest.fixture(scope='module', autouse=True)
def _report_ratios():
    yield
    for k in sorted(RATIOS):
        print(f'\n[head headroom] {k}: max error / bar = {RATIOS[k]:.4f}', end='')
    print()
    RATIOS.clear()


def _head_cases():
    return [(f, s) for f in HEAD_FRAMES for s in HEAD_STEPS] + [(HEAD_STRIDE_FRAME, HEAD_STRIDE_STEPS)]


def head_grids(steps, dev):
    """(torch.linspace, np.linspace as float32): dl.py:177 and feed_forward.py:287-288"""
    return torch.linspace(-3.5, 3.5, steps).to(dev), torch.from_numpy(np.linspace(-3.5, 3.5, steps)).float().to(dev)


def upr_inputs(frame, steps, dev, seed):
    """out (B, 2, H, W) with mu exactly on a float32 grid value at pixel 0 (and at pixel 37 mod n, on the last one)"""
    B, H, W = frame
    n = B * H * W
    gen = torch.Generator(device=dev).manual_seed(seed)
    grid = head_grids(steps, dev)[1]
    out = torch.stack([1.5 * torch.randn((B, H * W), device=dev, generator=gen),
                       5 * torch.rand((B, H * W), device=dev, generator=gen) - 3], 1)
    for j, k in ((37 % n, steps - 1), (0, steps // 2)):
        out[j // (H * W), 0, j % (H * W)] = grid[k]
    go = torch.randn((B, steps, H, W), device=dev, generator=gen)
    return out.view(B, 2, H, W).contiguous(), grid, go


def _upr_rel(r):
    """posterior_k = a expf(t'), a = 1 / (2 b), b = expf(lv) within c U: a within (c + 1) U (the doubling is exact, the quotient
    U); t' = -|g_k - mu| / b: the difference U, b c U, the quotient U: (c + 2) U t, which expf turns into (c + 2) U t relative,
    plus its own c U; the product U: (2 c + 2 + (c + 2) t) U relative"""
    c = 2 * EXPLOG_ULPS
    return 2 * c + 2 + (c + 2) * r.t


@pytest.mark.parametrize('frame,steps', _head_cases(), ids=lambda v: str(v).replace(' ', ''))
def test_head_upr_and_its_backward_element_by_element(frame, steps):
    from mmlf_amd import _lib
    from mmlf_amd._lib import call, ptr
    dev = torch.device('cuda:0')
    B, H, W = frame
    c = 2 * EXPLOG_ULPS
    out, grid, go = upr_inputs(frame, steps, dev, 11 * steps + B * H * W % 1000)
    what = f'mmlf_head_upr B={B} {H}x{W} steps={steps}'
    r = upr_ref(out, grid, go)
    pool = _Pool(dev)
    post = pool.new(B * steps * H * W, NAN)
    call('mmlf_head_upr', ptr(out), ptr(grid), ptr(post), steps, B, H, W, _lib.stream_ptr())
    floor = FLOOR * (1 + 1 / (2 * r.b))
    rel = _upr_rel(r)
    _bar((post.view(B, steps, H, W).double() - r.post).abs(), U * rel * r.post + floor,
         'upr posterior: (2c + 2 + (c + 2) t) U relative', what)
    # mu on a grid value: t = 0 there, the posterior is its peak 1 / (2 b)
    on = r.t[0, steps // 2, 0, 0]
    assert float(on) == 0.0 and float(r.post[0, steps // 2, 0, 0]) == float(1 / (2 * r.b[0, 0, 0, 0]))
    assert float(post.view(B, steps, H, W)[0, :, 0, 0].max()) == float(post.view(B, steps, H, W)[0, steps // 2, 0, 0])
    # backward.  gm = sum_k fmaf(go p_k, sgn / b, gm): go p_k: U; sgn / b: (c + 1) U; every fmaf rounds the running sum:
    # steps U sum |term|.  gl = sum_k fmaf(go p_k, |d| / b - 1, gl): |d| / b within (c + 2) U t, the difference U |t - 1|.
    gout = pool.new(B * 2 * H * W, NAN)
    call('mmlf_head_upr_bwd', ptr(out), ptr(grid), ptr(go), ptr(gout), steps, B, H, W, _lib.stream_ptr())
    gop = (go.double() * r.post).abs()
    bm = U * (r.tm.abs() * (rel + c + 2)).sum(1) + steps * U * r.tm.abs().sum(1) + ((go.double() / r.b).abs() * floor).sum(1)
    bl = U * (gop * ((c + 2) * r.t + (r.t - 1).abs()) + r.tl.abs() * (rel + 1)).sum(1) + steps * U * r.tl.abs().sum(1) \
        + ((go.double() * (r.t - 1)).abs() * floor).sum(1)
    _bar((gout.view(B, 2, H, W).double() - r.gout).abs(), torch.stack([bm, bl], 1), 'upr backward: counted roundings', what)
    if steps == 1:                           # the one bin IS the grid value at pixel 0: its mu-gradient term is exactly 0
        assert float(r.gout[0, 0, 0, 0]) == 0.0 and float(gout.view(B, 2, H, W)[0, 0, 0, 0]) == 0.0, what
    pool.check(what)


def dpp_inputs(frame, steps, dev, seed):
    """scores within +-6 with, where the frame has the pixels, two equal maxima at pixel 0, three at pixel 37 (mod n) and at
    the last pixel all the mass on bin 0 (every other score -inf: the variance is 0, logvar -inf)"""
    B, H, W = frame
    n, HW = B * H * W, H * W
    gen = torch.Generator(device=dev).manual_seed(seed)
    sc = (2 * torch.randn((B, steps, HW), device=dev, generator=gen)).clamp(-6, 6)
    ties = {}
    if n > 1:
        for j, cnt in ((0, 2), (37 % n, 3)):
            ks = sorted({0, steps - 1} if cnt == 2 else {0, steps // 2, steps - 1})
            sc[j // HW, ks, j % HW] = TOP
            ties[j] = ks
    sc[(n - 1) // HW, 1:, (n - 1) % HW] = float('-inf')
    go_post = torch.randn((B, steps, H, W), device=dev, generator=gen)
    go_lv = torch.randn((B, H, W), device=dev, generator=gen)
    return sc.view(B, steps, H, W).contiguous(), go_post, go_lv, ties


@pytest.mark.parametrize('frame,steps', _head_cases(), ids=lambda v: str(v).replace(' ', ''))
def test_head_dpp_and_its_backward_element_by_element(frame, steps):
    from mmlf_amd import _lib
    from mmlf_amd._lib import call, ptr
    dev = torch.device('cuda:0')
    B, H, W = frame
    n, c = B * H * W, 2 * EXPLOG_ULPS
    sc, go_post, go_lv, ties = dpp_inputs(frame, steps, dev, 13 * steps + n % 1000)
    grid_t, grid_np = head_grids(steps, dev)
    assert float(grid_t[0]) == float(grid_np[0])            # precondition of the -inf pixel: d = 0 on its bin
    what = f'mmlf_head_dpp B={B} {H}x{W} steps={steps}'
    r = dpp_ref(sc, grid_t, grid_np)
    pool = _Pool(dev)
    oh, post = pool.new(sc.numel(), NAN), pool.new(sc.numel(), NAN)
    mean, lv = pool.new(n, NAN), pool.new(n, NAN)
    call('mmlf_head_dpp', ptr(sc), ptr(grid_t), ptr(grid_np), ptr(oh), ptr(post), ptr(mean), ptr(lv), steps, B, H, W,
         _lib.stream_ptr())
    _same(oh.view(B, steps, H, W), r.one_hot, what + ' one_hot')
    for j, ks in ties.items():               # every maximum is marked
        got = oh.view(B, steps, -1)[j // (H * W), :, j % (H * W)]
        assert got.nonzero().view(-1).tolist() == ks, (what, 'maxima marked at pixel', j, got.nonzero().view(-1).tolist(), ks)
        assert float(r.one_hot.view(B, steps, -1)[j // (H * W), :, j % (H * W)].sum()) == len(ks)
    # p_k = expf(s_k) / z: expf c U, z sums `steps` of them: (c + steps - 1) U, the quotient U
    rp = 2 * c + steps
    _bar((post.view(B, steps, H, W).double() - r.post).abs(), U * rp * r.post + FLOOR, 'dpp posterior: (2c + steps) U relative',
         what)
    # mean = sum grid_k one_hot_k in float32: exact for one maximum, one rounding per further one
    nties = r.one_hot.sum(1)
    dm = U * (nties - 1) * (grid_t.double().view(1, -1, 1, 1).abs() * r.one_hot).sum(1)
    _bar((mean.view(B, H, W).double() - r.mean).abs(), dm, 'dpp mean: (maxima - 1) U sum |grid one_hot|', what)
    # logvar = logf(V), V = sum (g_k - m)^2 p_k: d: U, d d: 3 U, p_k: rp U, the product U, the sum (steps - 1) U:
    # (2c + 2 steps + 3) U relative, and 2 sum |d| p dm / V for the mean; logf turns it absolute and adds c U |logvar|
    blv = U * (2 * c + 2 * steps + 3) + 2 * (r.d.abs() * r.post).sum(1) * dm / r.V + c * U * r.logvar.abs()
    _close(lv.view(B, H, W), r.logvar, blv, 'dpp logvar: (2c + 2 steps + 3) U + c U |logvar|', what)
    last = r.logvar.view(-1)[n - 1]
    assert float(last) == float('-inf') and float(lv[n - 1]) == float('-inf'), (what, 'all mass on the arg-max bin')
    pool.check(what)
    # backward, the three forms; the mean is the float32 one the forward hands over
    m32 = r.mean.float()
    for form in ('both', 'posterior', 'logvar'):
        gp, gl = go_post if form != 'logvar' else None, go_lv if form != 'posterior' else None
        b = dpp_bwd_ref(sc, grid_np, m32, gp, gl)
        gsc = pool.new(sc.numel(), NAN)
        call('mmlf_head_dpp_bwd', ptr(sc), ptr(grid_np), ptr(m32), ptr(gp), ptr(gl), ptr(gsc), steps, B, H, W,
             _lib.stream_ptr())
        # z, p_k as above (rp U); V by fmaf: (2c + 2 steps + 3) U =: rv; gl = glv / V: (rv + 1) U; q_k = gl d d: d twice and
        # two products: (rv + 5) U |q_k|; dp_k = gpost_k + q_k: U |dp_k|; dot = sum fmaf(dp_k, p_k): the operands, and steps U
        # sum |dp p| for the running sum; gs_k = p_k (dp_k - dot): the difference U, p_k and the product (rp + 1) U
        rv = 2 * c + 2 * steps + 3
        q = b.gl * b.d * b.d if gl is not None else torch.zeros_like(b.dp)
        edp = U * ((rv + 5) * q.abs() + (b.dp.abs() if gl is not None else 0.0))
        dpp = (b.dp * b.post).abs()
        edot = (edp * b.post + U * rp * dpp).sum(1, keepdim=True) + steps * U * dpp.sum(1, keepdim=True)
        bar = b.post * (edp + edot + U * (b.dp - b.dot).abs()) + U * (rp + 1) * b.gs.abs() + FLOOR * ((b.dp - b.dot).abs() + 1)
        _close(gsc.view(B, steps, H, W), b.gs, bar, f'dpp backward ({form}): counted roundings', f'{what} backward {form}')
        pool.check(what + ' backward ' + form)
