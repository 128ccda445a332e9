"""Nets wider than 288 channels on the native trunk (model_chs 74, 96, 128 with 2x2 filters: the convolutions and weight
gradients of their merge blocks run as column blocks), module level: training-mode forward, loss and backward
against the same module in float64 on the CPU in the three arithmetic modes, with and without BatchNorm; the DPP and BASE
heads; eval mode (folded inference, the frozen forward, input gradients); TrainStep; the extent check; the Ensamble's fused
members.  The float64 references, their seeds and the conditioning that pins them are tests/test_wide_cpu.py's; the bars are
the ones the 70-channel tests hold the native path to (named at each test).  On a library without the column blocks every one
of these modules takes the stock-torch tree (`_native_ok` is False): each test asserts the predicate first.

Replaces the nn.Conv2d / nn.BatchNorm2d tree of reference mmlf/model/feed_forward.py:86-204 at --model_chs above 72."""
import numpy as np
import pytest
import torch

from mmlf_amd import synth
from test_wide_cpu import (GRAD_MEDIAN, GRAD_WORST, LOSS_BAR, OUT_BAR, WIDE_CHS, WIDE_FRAMES, compare_runs, wide_kw, wide_model,
                           wide_reference, wide_run, wide_state)

pytestmark = pytest.mark.gpu

MODES = ['f32', 'bf16x6', 'f16x3']


def _dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


class _Spy:
    """records the names that go through _lib.call from the engine, the module and the Ensamble"""

    def __init__(self, monkeypatch):
        from mmlf_amd import _lib, engine, ensamble, feed_forward
        self.names = []
        real = _lib.call

        def call(name, *args):
            self.names.append(name)
            return real(name, *args)
        for mod in (_lib, engine, ensamble, feed_forward):
            monkeypatch.setattr(mod, 'call', call)


def _native_run(chs, bn, H, W, monkeypatch, mode, **head):
    from mmlf_amd import engine
    monkeypatch.setattr(engine, 'CONV_MODE', mode)
    kw, state, ref = wide_reference(chs, bn, H, W, **head)
    m = wide_model(kw, state, _dev())
    assert m._native_ok and m._trunk is not None
    spy = _Spy(monkeypatch)
    got = wide_run(m, kw, H, W, _dev(), torch.float32)
    conv = {'f16x3': 'mmlf_conv2x2_h2', 'bf16x6': 'mmlf_conv2x2_split', 'f32': 'mmlf_conv2x2'}[mode]
    wg = {'f16x3': 'mmlf_conv2x2_wgrad_h2', 'bf16x6': 'mmlf_conv2x2_wgrad_split', 'f32': 'mmlf_conv2x2_wgrad'}[mode]
    assert conv in spy.names and wg in spy.names, set(spy.names)           # the kernels ran, not the stock tree
    return got, ref


# ------------------------------------------------------------------------------------------------ nets
@pytest.mark.parametrize('H,W', WIDE_FRAMES)
@pytest.mark.parametrize('bn', [True, False], ids=['bn', 'nobn'])
@pytest.mark.parametrize('chs', WIDE_CHS)
@pytest.mark.parametrize('mode', MODES)
def test_wide_net_against_float64(mode, chs, bn, H, W, monkeypatch):
    """two stream blocks, three merge blocks, UPR head, bs = 3, train mode: outputs 1e-4, loss 1e-4 relative, gradients per
    tensor relative L2 (with the floor) worst 6e-2, median 4e-2 -- tests/test_gpu_nobn.py::test_70_channel_net_against_float64"""
    got, ref = _native_run(chs, bn, H, W, monkeypatch, mode)
    compare_runs(f'wide {mode} model_chs={chs} bn={bn} {H}x{W}', got, ref, OUT_BAR, LOSS_BAR, GRAD_WORST, GRAD_MEDIAN)


@pytest.mark.parametrize('head,H,W', [('dpp', 9, 7), ('base', 5, 130)])
@pytest.mark.parametrize('bn', [True, False], ids=['bn', 'nobn'])
def test_wide_net_dpp_and_base_heads(head, bn, H, W, monkeypatch):
    """model_chs = 96 under the 108-class head (384 -> 108: a wide input under the 128-column kernels) and under the one-channel
    head (the thin kernels at cs_in = 384), at the same bars"""
    kw = {'dpp': {'model_discrete': True}, 'base': {'model_uncert': False}}[head]
    got, ref = _native_run(96, bn, H, W, monkeypatch, 'f16x3', **kw)
    compare_runs(f'wide {head} model_chs=96 bn={bn} {H}x{W}', got, ref, OUT_BAR, LOSS_BAR, GRAD_WORST, GRAD_MEDIAN)


# ------------------------------------------------------------------------------------------------ eval mode
def _eval_inputs(H, W, dev, dtype, B=3):
    stacks, gt, mask = synth.synth_inputs(B, H, seed=11, ps_w=W)
    return [torch.from_numpy(s).to(dev, dtype) for s in stacks], torch.from_numpy(gt).to(dev, dtype), torch.from_numpy(mask).to(dev)


@pytest.mark.parametrize('bn', [True, False], ids=['bn', 'nobn'])
def test_wide_net_eval_mode(bn, monkeypatch):
    """model_chs = 96, eval mode: the no_grad forward (BatchNorm folded into conv2: mmlf_fold_bn_eval at Cout = 384) against
    float64 at 1e-4; the frozen forward (inputs require gradients, parameters do not) gives the bits of the no_grad output; its
    input gradients against float64 at tests/test_gpu_input_grad.py's bar (5e-4 max |gradient| + 5e-7 per stack, the loss
    scaled by the power of two that lifts every stack's largest gradient to 1e-2, the float32 stock run within a tenth of it)"""
    import math
    from mmlf_amd import loss
    from test_input_grad_cpu import GRAD_FLOOR, bar, ratio
    H, W = 9, 7
    kw = wide_kw(96, bn)
    state = wide_state(kw)
    res = {}
    for dt in (torch.float64, torch.float32):
        m = wide_model(kw, state, dtype=dt).eval()
        stacks, gt, mask = _eval_inputs(H, W, torch.device('cpu'), dt)
        xs = [s.clone().requires_grad_(True) for s in stacks]
        out = m(*xs)
        loss.ImprovedUncertaintyL1Loss()(out, gt, mask, None).backward()
        res[dt] = ({k: out[k].detach().double() for k in ('mean', 'logvar')}, [x.grad.double() for x in xs])
    o0, g0 = res[torch.float64]
    smallest = min(float(g.abs().max()) for g in g0)
    assert smallest > 0
    scale = 2.0 ** max(0, math.ceil(math.log2(GRAD_FLOOR / smallest)))
    ref = [g * scale for g in g0]
    cond = max(ratio(g * scale, r) for g, r in zip(res[torch.float32][1], ref))
    assert cond <= 0.1, cond                                # conditioning first
    dev = _dev()
    m = wide_model(kw, state, dev).eval()
    assert m._native_ok
    stacks, gt, mask = _eval_inputs(H, W, dev, torch.float32)
    spy = _Spy(monkeypatch)
    with torch.no_grad():
        plain = m(*stacks)
    assert spy.names.count('mmlf_fold_bn_eval') == (10 if bn else 0), spy.names      # 4 x 2 stream blocks + 2 merge blocks
    for k in ('mean', 'logvar'):
        err = float((plain[k].double().cpu() - o0[k]).abs().max())
        print(f'wide eval bn={bn} {k}: max |error| {err:.3e}')
        assert err <= 1e-4, (k, err)
    for p in m.parameters():
        p.requires_grad_(False)
    xs = [s.clone().requires_grad_(True) for s in stacks]
    out = m(*xs)
    for k, v in plain.items():
        assert (v is None and out[k] is None) or torch.equal(out[k].detach(), v), k
    (loss.ImprovedUncertaintyL1Loss()(out, gt, mask, None) * scale).backward()
    assert not [n for n in spy.names if 'wgrad' in n], spy.names
    for k, (x, r) in enumerate(zip(xs, ref)):
        q = ratio(x.grad, r)
        print(f'wide eval bn={bn} d loss / d {"hvid"[k]}_views: error at {q:.3e} of the bar {bar(r):.3e}')
        assert q <= 1.0, ('hvid'[k], q)


# ------------------------------------------------------------------------------------------------ TrainStep
def _steps(m, dev, n=2):
    from mmlf_amd.train import TrainStep
    step = TrainStep(m, lr=1e-3, loss_margin=3)
    for it in range(n):
        stacks, gt, mask = synth.synth_inputs(2, 16, seed=60 + it)
        step(*[torch.from_numpy(s).to(dev) for s in stacks], torch.from_numpy(gt).to(dev), torch.from_numpy(mask).to(dev), it + 1)
    return step


@pytest.mark.parametrize('mode', MODES)
def test_wide_train_step_two_steps_against_the_float64_reference_loop(mode, monkeypatch):
    """TrainStep at model_chs = 96 (no BatchNorm, variance-preserving filters) against autograd and torch.optim.Adam on the
    stock path in float64 -- the case and bar of
    tests/test_gpu_nobn.py::test_train_step_two_steps_against_the_float64_reference_loop: per tensor within 5 % of how far the
    two steps moved it.  (The BatchNorm net of this width is no case for this bar: the stock path's own float32 run misses it
    against float64, at 1.05 of the bar on the CPU -- two Adam steps amplify the rounding of BatchNorm's small gradients.  Its
    step is held to float64 through its gradients, test_wide_net_against_float64, and runs under the extent check below.)"""
    from mmlf_amd import engine, loss
    monkeypatch.setattr(engine, 'CONV_MODE', mode)
    dev = _dev()
    kw = wide_kw(96, False)
    state = wide_state(kw, 17)
    w0 = {k: torch.from_numpy(np.asarray(v)).double() for k, v in state.items()}
    m = wide_model(kw, state, dev)
    assert m._native_ok
    _steps(m, dev)
    got = {k: v.detach().double().cpu() for k, v in m.state_dict().items()}
    ref = wide_model(kw, state, dtype=torch.float64)
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3)
    ref.train()
    for it in range(2):
        stacks, gt, mask = synth.synth_inputs(2, 16, seed=60 + it)
        mk = torch.from_numpy(mask).int() * loss.create_mask_margin(mask.shape, 3)
        opt.zero_grad()
        out = ref(*[torch.from_numpy(s).double() for s in stacks])
        loss.ImprovedUncertaintyL1Loss()(out, torch.from_numpy(gt).double(), mk, None).backward()
        opt.step()
    for k, v in ref.state_dict().items():
        moved = float((v - w0[k]).norm())
        dist = float((got[k] - v).norm())
        print(f'wide TrainStep {mode} {k}: {dist:.3e} from float64, moved {moved:.3e}')
        assert moved >= 2e-4 * v.numel() ** 0.5, (k, moved)          # (two Adam steps of 1e-3: an rms of a tenth of that at least)
        assert dist <= 0.05 * moved + 1e-6, (k, dist, moved)


@pytest.mark.parametrize('bn', [True, False], ids=['bn', 'nobn'])
def test_wide_training_step_passes_the_extent_check(bn, monkeypatch):
    """one step under MMLF_CHECK_EXTENTS: every convolution and weight-gradient launch of a model_chs = 96 net is audited
    (mmlf_audit_conv_h2 / mmlf_audit_wgrad_h2 follow the column blocks) and none is refused"""
    from mmlf_amd import engine
    dev = _dev()
    monkeypatch.setattr(engine, 'CONV_MODE', 'f16x3')
    monkeypatch.setattr(engine, 'CHECK_EXTENTS', True)
    kw = wide_kw(96, bn)
    m = wide_model(kw, wide_state(kw, 3), dev)
    assert m._native_ok
    spy = _Spy(monkeypatch)
    before = engine.EXTENT_CHECKS
    step = _steps(m, dev, n=1)
    torch.cuda.synchronize()
    assert torch.isfinite(step.grad).all() and float(step.grad.abs().max()) > 0
    launches = [n for n in spy.names if n in ('mmlf_conv2x2_h2', 'mmlf_conv2x2_wgrad_h2', 'mmlf_relu_bwd_slice')]
    assert engine.EXTENT_CHECKS - before == len(launches) > 0
    assert spy.names.count('mmlf_audit_conv_h2') == spy.names.count('mmlf_conv2x2_h2')
    assert spy.names.count('mmlf_audit_wgrad_h2') == spy.names.count('mmlf_conv2x2_wgrad_h2')


# ------------------------------------------------------------------------------------------------ the Ensamble
@pytest.mark.parametrize('bn', [True, False], ids=['bn', 'nobn'])
def test_wide_ensamble_fused_members_give_the_bits_of_the_module_path(bn, monkeypatch):
    """a model_chs = 96 UPR net in eval mode: the fused member path (mmlf_shift_pack + the trunk on packed inputs) against
    MMLF_ESE_FUSED=0 (mmlf_shift_views + the module's own forward) -- equal bits, the bar of tests/test_ensamble.py"""
    from mmlf_amd import ensamble
    dev = _dev()
    kw = wide_kw(96, bn)
    m = wide_model(kw, wide_state(kw, 31), dev).eval()
    assert m._native_ok
    stacks, _, _ = synth.synth_inputs(1, 9, seed=9, ps_w=13)
    res = {}
    for fused in (True, False):
        monkeypatch.setattr(ensamble, 'FUSED_MEMBERS', fused)
        ens = ensamble.Ensamble(m, -0.1, 0.15, 0.1).eval()
        assert len(ens.members()) == 3
        spy = _Spy(monkeypatch)
        with torch.no_grad():
            res[fused] = ens(*[torch.from_numpy(s).to(dev) for s in stacks])
        assert ('mmlf_shift_pack' in spy.names) == fused and ('mmlf_shift_views' in spy.names) != fused, spy.names
    for k, v in res[False].items():
        assert torch.equal(res[True][k], v), k
    assert torch.isfinite(res[True]['mean']).all()
