"""The float64 references of tests_helpers for the losses, the heads and Adam (loss_ref, upr_ref, dpp_ref, dpp_bwd_ref,
adam_ref), pinned on the CPU: against torch autograd in float64 of the CPU branches of mmlf_amd/loss.py, against autograd of
the reference's head expressions as tests/test_gpu_heads.py states them, and against torch.optim.Adam in float64 -- on the
very inputs, constructed edges included, that tests/test_gpu_losses.py and tests/test_gpu_heads.py give the kernels.  The
shape lists of those modules are held to the classes they exist for.  Nothing here needs a GPU.

Where a CPU module itself computes a factor in float32 the pin allows that rounding and nothing else (U = 2^-24 per float32
operation): the n / count factors of ImprovedUncertaintyL1Loss (mask_padding.float()) and ImprovedMultiUncertaintyL1Loss
(oor.float()), and the float32 sum of alphas of dl.mpi_to_weights."""
import numpy as np
import pytest
import torch

import test_gpu_heads as th
import test_gpu_losses as tl
from mmlf_amd import dl, loss as L
from tests_helpers import (ADAM_N, LOSS_FRAMES, LOSS_NBLOCKS, LOSS_NBLOCKS_FRAMES, LOSS_STRIDE_FRAME, adam_ref, dpp_bwd_ref,
                           dpp_ref, loss_ref, upr_ref)

CPU = torch.device('cpu')
U = 2.0 ** -24
PIN_FRAMES = [(1, 1, 1), (1, 1, 257), (3, 5, 7), (2, 1, 300)]


def _module_loss(inp, o, f32=False):
    """the CPU branch of mmlf_amd/loss.py for inp.kind on the raw output o (B, oc, H, W), which is float64 unless f32"""
    k = inp.kind
    tgt = inp.target if f32 else inp.target.double()
    if k == 0:
        return L.MaskedL1Loss()({'mean': o[:, 0]}, tgt, inp.mask)
    if k == 1:
        return L.ImprovedUncertaintyL1Loss()({'mean': o[:, 0], 'logvar': o[:, 1]}, tgt, inp.mask)
    if k == 2:                               # the decisions in float32, as dl.reg_to_class takes them
        return L.MaskedCrossEntropy()({'scores': o}, dl.reg_to_class(inp.target, *tl.DISP, inp.oc).double(), inp.mask)
    if k == 3:
        return L.MultiMaskedL1Loss()({'mean': o[:, 0]}, tgt, inp.mask)
    if k == 4:
        return L.ImprovedMultiUncertaintyL1Loss()({'mean': o[:, 0], 'logvar': o[:, 1]}, tgt, inp.mask)
    if k == 5:
        return L.MaskedCrossEntropy()({'scores': o}, dl.mpi_to_weights(inp.target, *tl.DISP, inp.oc).double(), inp.mask)
    return L.ImprovedUncertaintyL1Loss()({'mean': o[:, 0], 'logvar': o[:, 1]}, tgt, inp.mask, inp.mp)


def _pin_bars(inp, r):
    """what the CPU module's own float32 factors may differ by (see the module docstring): (per-pixel loss, gradient)"""
    p, mkd = r.parts, (inp.mask.double() / r.den_used).unsqueeze(1)
    zl, zg = torch.zeros_like(r.l), torch.zeros_like(r.grad)
    if inp.kind == 4:                        # f1 = n / sum(oor.float())
        of1 = p['oor'] * p['f1']
        return 2 * U * p['l_oor'].abs(), torch.stack([zl, 2 * U * of1 / 2], 1) * mkd
    if inp.kind == 6:                        # f0 = n / mp.sum(), f1 = n / oor.sum()
        g1 = (((1 - p['ed']) * p['mp'] * p['f0']).abs() + p['oor'] * p['f1']) / 2
        return 2 * U * (p['l_in'].abs() + p['l_oor'].abs()), torch.stack([2 * U * r.g[:, 0].abs(), 2 * U * g1], 1) * mkd
    if inp.kind == 5:                        # t_k: a float32 sum of P alphas
        e = 2 * U * max(inp.P - 1, 0)
        return e * p['dot'].abs(), e * p['t'] * mkd
    return zl, zg


def _pin(inp):
    used = 1 if inp.kind in (0, 3) else inp.oc if inp.kind in (2, 5) else 2
    o = inp.out.double().requires_grad_(True)
    loss = _module_loss(inp, o)
    loss.backward()
    r = loss_ref(inp.kind, inp.out, inp.target, inp.mask, inp.mp, inp.grid, inp.half)
    if bool(torch.isnan(r.loss)):
        assert bool(torch.isnan(loss)), inp.tag
        return r
    bl, bg = _pin_bars(inp, r)
    lim = (inp.mask.double() * bl).sum() / r.den_used + 1e-12 * (inp.mask.double() * r.l.abs()).sum() / r.den_used + 1e-300
    assert float((loss.detach() - r.loss).abs()) <= float(lim), (inp.tag, float(loss), float(r.loss))
    err = (o.grad[:, :used] - r.grad).abs()
    assert bool((err <= bg + 1e-12 * r.grad.abs() + 1e-15).all()), (inp.tag, float(err.max()))
    assert not bool(o.grad[:, used:].any()), inp.tag
    return r


@pytest.mark.parametrize('integer', [True, False], ids=['exact', 'real'])
@pytest.mark.parametrize('kind', tl.KINDS)
def test_loss_ref_equals_autograd_of_the_cpu_modules(kind, integer):
    for i, frame in enumerate(PIN_FRAMES):
        for j, (oc, P) in enumerate(tl._oc_p(kind)):
            for mask_mode in ('some', 'zero'):
                inp = tl.make_inputs(kind, frame, oc, P, integer, 100 * kind + 10 * i + j, CPU, mask_mode=mask_mode,
                                     alpha_edge=False)
                r = _pin(inp)
                if mask_mode == 'zero' and bool(torch.isfinite(r.loss)):
                    assert float(r.loss) == 0.0 and not bool(r.grad.any())
            if kind == 6:
                for mp_mode in ('ones', 'zeros'):
                    _pin(tl.make_inputs(kind, frame, oc, P, integer, 7 + i, CPU, mp_mode=mp_mode))


def test_constructed_edges_are_what_they_claim():
    """on the reference alone: out == gt gives a gradient of exactly 0; a gt outside every bin and a gt exactly half a step from
    a centre give an all-zero target; the score exactly 0 has gradient 0; the alpha of float32 0.01 is NOT surface-less"""
    for kind in tl.KINDS:
        for oc, P in tl._oc_p(kind):
            inp = tl.make_inputs(kind, (3, 5, 7), oc, P, False, 5, CPU)
            r = loss_ref(inp.kind, inp.out, inp.target, inp.mask, inp.mp, inp.grid, inp.half)
            e = tl._edge_pixels(inp.n, 3)
            flat = lambda t: t.reshape(t.shape[0], -1, 35).permute(0, 2, 1).reshape(105, -1)       # (pixel, channel)
            if kind in (0, 1) or (kind == 3 and P == 1):
                assert float(flat(r.grad)[e[0], 0]) == 0.0 and int(inp.mask.view(-1)[e[0]]) == 1
            if kind in (2, 5):
                t = flat(r.parts['t'])
                assert not bool(t[e[1]].any()) and not bool(t[e[2]].any()) and bool(t.any())
                disp = inp.target.view(-1)[e[2]] if kind == 2 else inp.target.view(3, P, 5, 35)[e[2] // 35, 0, 4, e[2] % 35]
                half32 = torch.tensor(inp.half, dtype=torch.float64).float()
                assert bool((torch.abs(inp.grid - disp) == half32).any())
                sc = flat(inp.out)[e[0]]
                assert float(sc[0]) < 0 and (oc < 2 or float(sc[1]) == 0.0) and (oc < 3 or float(sc[2]) > 0)
                assert oc < 2 or float(flat(r.grad)[e[0], 1]) == 0.0
            if kind == 4:
                assert float(flat(r.parts['oor'])[e[1], 0]) == 0.0 and float(r.aux[1]) > 0


@pytest.mark.parametrize('P', [1, 3])
def test_multi_upr_edges_against_the_float32_cpu_module(P):
    """the float32 alpha 0.01 belongs to a surface (tot < 0.01 is strict): the CPU module evaluated in float32, where it takes
    the same decision, against loss_ref; without a surface-less pixel both are NaN"""
    for frame in PIN_FRAMES[1:]:
        inp = tl.make_inputs(4, frame, 2, P, False, 21, CPU)
        r = loss_ref(4, inp.out, inp.target, inp.mask)
        got = _module_loss(inp, inp.out, f32=True)
        scale = float((inp.mask.double() * r.l.abs()).sum() / r.den_used)
        assert abs(float(got) - float(r.loss)) <= 2e-5 * scale, inp.tag
        # were that pixel counted as surface-less the loss would move by ten times that allowance and more
        t2 = inp.target.clone()
        e = tl._edge_pixels(inp.n, 2)[1]
        t2.view(frame[0], P, 5, -1)[e // (frame[1] * frame[2]), 0, 3, e % (frame[1] * frame[2])] = 0.0
        other = loss_ref(4, inp.out, t2, inp.mask)
        assert abs(float(other.loss) - float(r.loss)) > 2e-4 * scale
        nan = tl.make_inputs(4, frame, 2, P, False, 22, CPU, surfaceless='none')
        assert bool(torch.isnan(loss_ref(4, nan.out, nan.target, nan.mask).loss))
        assert bool(torch.isnan(_module_loss(nan, nan.out, f32=True)))


@pytest.mark.parametrize('kind', tl.KINDS)
def test_overrides_of_loss_ref(kind):
    inp = tl.make_inputs(kind, (3, 5, 7), tl.MIN_OC[kind] + 1, tl.PLANES[kind][-1], False, 31, CPU)
    args = (inp.kind, inp.out, inp.target, inp.mask, inp.mp, inp.grid, inp.half)
    r = loss_ref(*args)
    same = loss_ref(*args, den_override=r.count.reshape(1))
    twice = loss_ref(*args, den_override=2 * r.count.reshape(1))
    assert torch.equal(same.loss, r.loss) and torch.equal(same.grad, r.grad)
    assert torch.equal(twice.loss, r.loss / 2) and torch.equal(twice.grad, r.grad / 2)
    zero = loss_ref(*args, den_override=torch.zeros(1, dtype=torch.float64))           # count 0 -> denominator 1
    assert torch.equal(zero.loss, r.sum) and float(zero.den) == 0.0 and float(zero.den_used) == 1.0
    if kind in (4, 6):
        own = torch.stack([r.aux[0], r.aux[1] if kind == 4 else torch.zeros(())]).double()
        again = loss_ref(*args, aux_override=own)
        assert torch.equal(again.loss, r.loss) and torch.equal(again.grad, r.grad)
        # the sums of a batch twice as large with the same statistics: the same factors, the same loss
        if kind == 6:
            other = loss_ref(*args, aux_override=torch.tensor([inp.n / 2.0, 0.0], dtype=torch.float64))
            assert float(other.parts['f0']) == 2.0 and float(other.parts['f1']) == 2.0
        else:
            other = loss_ref(*args, aux_override=torch.tensor([2.0 * inp.n, inp.n / 4.0], dtype=torch.float64))
            assert float(other.parts['f0']) == 2.0 and float(other.parts['f1']) == 4.0
        assert not torch.equal(other.loss, r.loss)


# ------------------------------------------------------------------------------------------------ heads
@pytest.mark.parametrize('steps', th.HEAD_STEPS)
def test_upr_ref_equals_autograd_of_the_reference_expression(steps):
    for frame in PIN_FRAMES:
        out, grid, go = th.upr_inputs(frame, steps, CPU, 3)
        B, H, W = frame
        o64 = out.double().requires_grad_(True)
        post64 = th._laplacian(grid.double().view(1, steps, 1, 1).expand(B, steps, H, W), o64[:, 0], torch.exp(o64[:, 1]))
        post64.backward(go.double())
        r = upr_ref(out, grid, go)
        torch.testing.assert_close(r.post, post64.detach(), rtol=1e-13, atol=0)
        scale = torch.stack([r.tm.abs().sum(1), r.tl.abs().sum(1)], 1)
        assert bool(((r.gout - o64.grad).abs() <= 1e-12 * scale).all())
        assert float(r.t[0, steps // 2, 0, 0]) == 0.0 and float(r.tm[0, steps // 2, 0, 0]) == 0.0      # mu on a grid value


@pytest.mark.parametrize('form', ['both', 'posterior', 'logvar'])
@pytest.mark.parametrize('steps', th.HEAD_STEPS)
def test_dpp_refs_equal_autograd_of_the_reference_expressions(steps, form):
    for frame in PIN_FRAMES:
        sc, go_post, go_lv, ties = th.dpp_inputs(frame, steps, CPU, 4)
        grid_t, grid_np = th.head_grids(steps, CPU)
        n, hw = sc.numel() // steps, frame[1] * frame[2]
        s64 = sc.double().requires_grad_(True)
        one_hot = (torch.max(s64, 1, keepdim=True)[0] == s64).double()
        e = torch.exp(s64)
        post64 = e / torch.sum(e, 1, keepdim=True)
        mean64 = torch.sum(grid_t.double().view(1, -1, 1, 1) * one_hot, 1)
        lv64 = torch.log(torch.sum((grid_np.double().view(1, -1, 1, 1) - mean64.unsqueeze(1)) ** 2.0 * post64, 1))
        r = dpp_ref(sc, grid_t, grid_np)
        assert torch.equal(r.one_hot, one_hot.detach()) and torch.equal(r.mean, mean64.detach())
        for j, ks in ties.items():
            assert r.one_hot.view(sc.shape[0], steps, -1)[j // hw, :, j % hw].nonzero().view(-1).tolist() == ks
        torch.testing.assert_close(r.post, post64.detach(), rtol=1e-13, atol=0)
        fin = torch.isfinite(lv64.detach())
        assert torch.equal(torch.isfinite(r.logvar), fin) and float(r.logvar.view(-1)[n - 1]) == float('-inf')
        assert torch.equal(r.logvar[~fin], lv64.detach()[~fin])
        torch.testing.assert_close(r.logvar[fin], lv64.detach()[fin], rtol=1e-12, atol=1e-12)
        gp, gl = go_post if form != 'logvar' else None, go_lv if form != 'posterior' else None
        loss = 0.0
        if gp is not None:
            loss = loss + (post64 * gp.double()).sum()
        if gl is not None:
            loss = loss + (lv64 * gl.double()).sum()
        loss.backward()
        # the analytic gradient takes the mean as a constant: the float64 one here (the kernel gets its float32 value)
        b = dpp_bwd_ref(sc, grid_np, r.mean, gp, gl)
        auto = s64.grad
        # wherever the analytic form is not finite (log at 0) autograd's is not either; everywhere else they agree
        bad = ~torch.isfinite(b.gs)
        assert not bool(torch.isfinite(auto[bad]).any())
        scale = b.post * (b.dp.abs() + (b.dp * b.post).abs().sum(1, keepdim=True))
        ok = (b.gs - auto).abs() <= 1e-10 * scale + 1e-300
        assert bool(ok[~bad].all()), (frame, steps, form, float(((b.gs - auto).abs() / scale.clamp_min(1e-300))[~bad].max()))
        if gl is not None:
            assert bool(bad.view(sc.shape[0], steps, -1)[(n - 1) // hw, :, (n - 1) % hw].all())


# ------------------------------------------------------------------------------------------------ Adam
@pytest.mark.parametrize('gs', [1.0, 0.125])
@pytest.mark.parametrize('betas', [(0.9, 0.999), (0.5, 0.75)])
def test_adam_ref_equals_torch_optim_adam(betas, gs):
    gen = torch.Generator().manual_seed(1)
    n, lr, eps = 257, 1e-3, 1e-8
    for first in (1, 2, 1000):
        p = torch.randn(n, generator=gen, dtype=torch.float64)
        m, v = 0.3 * torch.randn(n, generator=gen, dtype=torch.float64), torch.rand(n, generator=gen, dtype=torch.float64) ** 2
        if first == 1:
            m, v = torch.zeros_like(m), torch.zeros_like(v)
        q = torch.nn.Parameter(p.clone())
        opt = torch.optim.Adam([q], lr=lr, betas=betas, eps=eps)
        if first > 1:
            opt.state[q] = {'step': torch.tensor(float(first - 1)), 'exp_avg': m.clone(), 'exp_avg_sq': v.clone()}
        for step in (first, first + 1):
            g = torch.randn(n, generator=gen, dtype=torch.float64) / gs
            q.grad = g * gs
            opt.step()
            p, m, v = adam_ref(p, g, m, v, lr, betas[0], betas[1], eps, step, gs)
            torch.testing.assert_close(p, q.detach(), rtol=1e-13, atol=1e-15)
            torch.testing.assert_close(m, opt.state[q]['exp_avg'], rtol=1e-13, atol=1e-300)
            torch.testing.assert_close(v, opt.state[q]['exp_avg_sq'], rtol=1e-13, atol=1e-300)


# ------------------------------------------------------------------------------------------------ the shape lists
def _ew_blocks(total):
    return max(1, min(8192, (total + 255) // 256))           # csrc/elementwise.hip ew_blocks


def test_gpu_shape_lists_reach_every_class():
    frames = tl.FRAMES + [tl.STRIDE_FRAME]
    assert set(tl.FRAMES) >= {(1, 1, 1), (1, 1, 255), (1, 1, 256), (1, 1, 257), (3, 5, 7), (2, 1, 300)} == set(LOSS_FRAMES)
    assert th.HEAD_FRAMES == tl.FRAMES and th.HEAD_STRIDE_FRAME == tl.STRIDE_FRAME == LOSS_STRIDE_FRAME
    totals = [b * h * w for b, h, w in frames]
    assert 1 in totals and any(t < 256 for t in totals) and 256 in totals and any(256 < t <= 8192 * 256 for t in totals)
    assert 255 in totals and 257 in totals                                   # one thread short of a block, one over
    # one total above 8192 * 256: some thread of the capped launch takes a second turn -- and only just above, to stay small
    stride = totals[-1]
    assert 8192 * 256 < stride < 8192 * 256 + 4096 and _ew_blocks(stride) == 8192 and stride < 2 ** 31
    assert all(_ew_blocks(t) * 256 >= t for t in totals[:-1])                # every other frame: one turn
    assert any(b > 1 and (h * w) % 2 == 1 for b, h, w in frames)             # the b / p split with an odd HW
    # nblocks below, at and above the 64 lanes of the one-wave finalize; engine's own; the wrapper's limit; more blocks than
    # there are 256-pixel groups (blocks with nothing to sum must still write their partial)
    from mmlf_amd import engine
    nb = tl.NBLOCKS
    assert nb == LOSS_NBLOCKS and {63, 64, 65} <= set(nb) and min(nb) == 1 and max(nb) == 4096 and 3 in nb
    assert engine.LOSS_BLOCKS in nb and tl.LOSS_BLOCKS == engine.LOSS_BLOCKS
    assert tl.NBLOCKS_FRAMES == LOSS_NBLOCKS_FRAMES == [(3, 5, 7), (2, 1, 300)]
    for b, h, w in tl.NBLOCKS_FRAMES:
        groups = (b * h * w + 255) // 256
        assert any(k > groups for k in nb) and any(k <= groups for k in nb)
    assert any((b * h * w + 255) // 256 > 1 for b, h, w in tl.NBLOCKS_FRAMES)   # a frame with more than one group
    # oc: the minimum of every kind, one more where the loss ignores channels, {1, 3, 108} for the cross-entropy kinds
    for kind in tl.KINDS:
        assert min(tl.OC[kind]) == tl.MIN_OC[kind] == (2 if kind in (1, 4, 6) else 1)
        assert (set(tl.OC[kind]) == {1, 3, 108}) if kind in (2, 5) else (tl.MIN_OC[kind] + 1 in tl.OC[kind])
        assert tl.PLANES[kind] == ([1, 3] if kind in (3, 4, 5) else [0])
        assert tl.THIN_OC[kind] == (2 if kind in (2, 5) else tl.MIN_OC[kind])
    assert th.HEAD_STEPS == [1, 2, 108] and th.HEAD_STRIDE_STEPS == 2
    # Adam: n = 1, a block short / exact / over, and one element above 8192 * 256
    assert ADAM_N == [1, 255, 256, 257, 8192 * 256 + 1]
    assert float(np.float32(tl.EXPLOG_ULPS)) == 2.0 and th.EXPLOG_ULPS == tl.EXPLOG_ULPS
