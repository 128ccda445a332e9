"""Partial training without a GPU: the plan both passes of the native trunk follow (engine.Trunk.plan) against hand-written
launch tables, the CPU TrainStep on a partly frozen model against a torch.optim.Adam loop, the refusal of a changed
requires_grad flag, the compiler's figures for the bias-only kernel and the widened contract of the five weight-gradient
entry points in the header.

The reference trains through nn.Module parameters (mmlf/train/cli.py:243-258: optim.Adam(model.parameters()) after
loss.backward()): autograd forms no gradient for a parameter with requires_grad False and Adam skips it."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, TINY_KW
from mmlf_amd import synth
from test_input_grad_cpu import KINDS, build, kind_kw, kind_state
from test_kernel_resources import usage  # noqa: F401  (the module-scoped fixture: one compiler run)

NO_X = (False,) * 4
V_ONLY = (False, True, False, False)


def _conv_weight(name):
    return name.endswith(('.0.weight', '.2.weight'))


# freeze patterns: name -> (which parameter names stay trainable, input gradients asked for)
PATTERNS = {
    'all': (lambda n: True, NO_X),
    'head': (lambda n: n.startswith('out_net.2.'), NO_X),
    'out_net': (lambda n: n.startswith('out_net.'), NO_X),
    'id_frozen': (lambda n: not n.startswith('in_net_id.'), NO_X),
    'mid_frozen': (lambda n: not n.startswith('out_net.1.'), NO_X),
    'hv00': (lambda n: n in ('in_net_hv.0.0.weight', 'in_net_hv.0.0.bias'), NO_X),
    'v_only': (lambda n: False, V_ONLY),
    'streams_frozen_v': (lambda n: n.startswith('out_net.'), V_ONLY),
    'bias_bn': (lambda n: not _conv_weight(n), NO_X),
}

# TINY_KW (2 stream blocks, 3 out_net blocks), train mode, BatchNorm: weight-gradient launches / mmlf_bn_bwd_reduce /
# mmlf_bn_bwd_apply / data gradients / bias-only launches among the weight gradients -- counted by hand from the rule of
# DESIGN.md 4.15 (a live block runs a launch iff something wanted depends on its result):
#   all        every block: 2 weight gradients, 2 data gradients (1 in a stream's block 0), reduce + apply below the head
#   head       conv2's and conv1's weight gradient, and the data gradient of conv2 that feeds conv1's
#   out_net    3 blocks; out_net.0 needs no dx
#   id_frozen  out_net and the H, V streams
#   mid_frozen out_net.1 passes the gradient on: reduce + apply (batch statistics) and both data gradients, no weight gradient
#   hv00       conv1 of H's and V's block 0: everything above passes the gradient on; block 0 runs reduce, apply, dgrad2, wgrad1
#   v_only     out_net's 3 blocks and V's 2 pass the gradient down to the stack: 4 reduce = apply, 3 x 2 + 2 x 2 data gradients
#   streams_frozen_v  v_only with out_net trainable: its 6 weight gradients on top
#   bias_bn    every weight-gradient launch is a bias-only one
# (the issue's own count for v_only read 0 / 5 / 9; by its rule, which it says decides, out_net has two BatchNorm blocks and V
# two, and the data gradients are 3 x 2 in out_net and 2 x 2 in V: 0 / 4 / 10)
BN_TABLE = {
    'all': (22, 10, 10, 18, 0),
    'head': (2, 0, 0, 1, 0),
    'out_net': (6, 2, 2, 5, 0),
    'id_frozen': (14, 6, 6, 12, 0),
    'mid_frozen': (20, 10, 10, 18, 0),
    'hv00': (2, 6, 6, 12, 0),
    'v_only': (0, 4, 4, 10, 0),
    'streams_frozen_v': (6, 4, 4, 10, 0),
    'bias_bn': (22, 10, 10, 18, 22),
}
# mmlf_relu_bwd_slice launches of the model_no_batchnorm trunk: one per live stream
SLICES = {'all': 4, 'head': 0, 'out_net': 0, 'id_frozen': 2, 'mid_frozen': 4, 'hv00': 2, 'v_only': 1, 'streams_frozen_v': 1,
          'bias_bn': 4}


def trunk_of(kind):
    from mmlf_amd.feed_forward import FeedForward
    m = FeedForward(**kind_kw(kind, 'base'))
    assert m._native_ok
    return m._trunk


def wanted(trunk, pattern):
    keep, want_x = PATTERNS[pattern]
    return {n for n in trunk._grad_names if keep(n)}, want_x


def expected_counts(kind, pattern):
    """{'wgrad', 'reduce', 'apply', 'dgrad', 'slice', 'bias_only'} of a train-mode backward"""
    w, r, a, d, b = BN_TABLE[pattern]
    if kind == 'nobn2':
        r = a = 0
    return {'wgrad': w, 'reduce': r, 'apply': a, 'dgrad': d, 'slice': SLICES[pattern] if kind == 'nobn2' else 0, 'bias_only': b}


@pytest.mark.parametrize('pattern', list(PATTERNS))
@pytest.mark.parametrize('kind', KINDS)
def test_plan_against_the_hand_written_tables(kind, pattern):
    trunk = trunk_of(kind)
    names, want_x = wanted(trunk, pattern)
    plan = trunk.plan(names, want_x)
    assert plan.counts() == expected_counts(kind, pattern), (kind, pattern, plan.blocks())
    assert plan.stream_live == {'all': [True] * 4, 'head': [False] * 4, 'out_net': [False] * 4,
                                'id_frozen': [True, True, False, False], 'mid_frozen': [True] * 4,
                                'hv00': [True, True, False, False], 'v_only': [False, True, False, False],
                                'streams_frozen_v': [False, True, False, False], 'bias_bn': [True] * 4}[pattern]
    # a block that is not live has no entry; live blocks sit on top of their chain
    for chain in plan.streams + [plan.out]:
        live = [b is not None for b in chain]
        assert live == sorted(live), (kind, pattern, live)


@pytest.mark.parametrize('kind', KINDS)
def test_plan_defaults_and_edges(kind):
    trunk = trunk_of(kind)
    full = trunk.plan(set(trunk._grad_names), NO_X)
    assert trunk.plan(None, None) == full and trunk.plan(None, NO_X) == full
    # today's full backward, block by block: every launch of a block, dx everywhere but at a stream's input
    bn = ['reduce', 'apply'] if kind != 'nobn2' else []
    for chain in full.streams:
        assert [b.launches() for b in chain] == [bn + ['wgrad2', 'dgrad2', 'wgrad1'], bn + ['wgrad2', 'dgrad2', 'wgrad1', 'dgrad1']]
    assert [b.launches() for b in full.out] == [bn + ['wgrad2', 'dgrad2', 'wgrad1', 'dgrad1']] * 2 + [['wgrad2', 'dgrad2', 'wgrad1', 'dgrad1']]
    # the empty set: today's grads=None backward -- no weight gradient; BatchNorm's sums only for batch statistics
    for train in (True, False):
        none = trunk.plan((), (True,) * 4, train=train, fold=False)
        c = none.counts()
        assert c['wgrad'] == 0 and c['dgrad'] == 22 and c['apply'] == (0 if kind == 'nobn2' else 10)
        assert c['reduce'] == (10 if train and kind != 'nobn2' else 0)
    # nothing wanted at all: nothing runs
    assert trunk.plan((), NO_X).blocks() == []
    # eval mode with nothing trainable folds BatchNorm on the 2x2 trunk only, and a fold has no parameter gradients
    assert trunk.plan((), V_ONLY, train=False).fold == (kind == 'bn2')
    assert not trunk.plan(None, V_ONLY, train=False).fold
    if kind == 'bn2':
        folded = trunk.plan((), (True,) * 4, train=False)
        assert folded.counts() == {'wgrad': 0, 'reduce': 0, 'apply': 0, 'dgrad': 22, 'slice': 4, 'bias_only': 0}
        with pytest.raises(ValueError, match='folded'):
            trunk.plan(None, NO_X, train=False, fold=True)
    with pytest.raises(ValueError, match='no parameter'):
        trunk.plan({'out_net.9.0.weight'}, NO_X)
    # a BatchNorm parameter alone in the top BatchNorm block: its sums, and nothing else in that block
    if kind != 'nobn2':
        only = trunk.plan({'out_net.1.3.weight'}, NO_X)
        assert [b.launches() for b in only.blocks()] == [['dgrad2', 'dgrad1'], ['reduce']]
    # in eval mode a frozen block between trainable ones needs no sums
    if kind != 'nobn2':
        keep, _ = PATTERNS['mid_frozen']
        ev = trunk.plan({n for n in trunk._grad_names if keep(n)}, NO_X, train=False)
        assert ev.out[1].launches() == ['apply', 'dgrad2', 'dgrad1']


# ------------------------------------------------------------------------------------------------ TrainStep on the CPU
def _cpu_batches(n):
    out = []
    for it in range(n):
        stacks, gt, mask = synth.synth_inputs(2, 16, seed=40 + it)
        out.append(([torch.from_numpy(s) for s in stacks], torch.from_numpy(gt), torch.from_numpy(mask)))
    return out


def _frozen_model(frozen_prefixes):
    kw = kind_kw('bn2', 'base')
    m = build(kw, kind_state('bn2', kw, 3))
    for n, p in m.named_parameters():
        if n.startswith(frozen_prefixes):
            p.requires_grad_(False)
    return m


def test_cpu_train_step_skips_frozen_parameters_like_adam():
    from mmlf_amd import loss
    from mmlf_amd.train import TrainStep
    frozen = ('in_net_hv.', 'in_net_id.')
    m = _frozen_model(frozen)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    step = TrainStep(m, lr=1e-3, loss_margin=3)
    assert step.trainable == {n for n in before if not n.startswith(frozen)}
    batches = _cpu_batches(2)
    for it, (stacks, gt, mask) in enumerate(batches):
        step(*stacks, gt, mask, it + 1)              # (raised at p.grad = None before frozen parameters were skipped)
    ref = _frozen_model(frozen)
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3, foreach=False)
    ref.train()
    for stacks, gt, mask in batches:
        mk = mask.int() * loss.create_mask_margin(mask.shape, 3).int()
        opt.zero_grad()
        loss.MaskedL1Loss()(ref(*stacks), gt, mk).backward()
        opt.step()
    moved = 0
    sd = step.optimizer_state_dict()
    assert len(sd['state']) == len(step.layout) == len(before)          # the optimizer state keeps its shape
    for (n, o, sz), (_, q) in zip(step.layout, ref.named_parameters()):
        p = dict(m.named_parameters())[n]
        if n.startswith(frozen):
            assert torch.equal(p, before[n]), n
            for buf in (step.grad, step.exp_avg, step.exp_avg_sq):
                assert not bool(buf[o:o + sz].any()), n
            assert q.grad is None and torch.equal(q, before[n])
        else:
            assert torch.equal(p, q), n
            moved += int(not torch.equal(p, before[n]))
    assert moved == len(step.trainable)
    for (n, a), (_, b) in zip(m.named_buffers(), ref.named_buffers()):   # the frozen stream nets' BatchNorm buffers move
        assert torch.equal(a, b), n


def test_a_changed_flag_is_refused():
    from mmlf_amd.train import TrainStep
    m = _frozen_model(('in_net_id.',))
    step = TrainStep(m, lr=1e-3, loss_margin=3)
    (stacks, gt, mask), = _cpu_batches(1)
    step(*stacks, gt, mask, 1)
    m.in_net_id[0][0].weight.requires_grad_(True)
    with pytest.raises(ValueError, match=r"in_net_id\.0\.0\.weight"):
        step(*stacks, gt, mask, 2)
    m.in_net_id[0][0].weight.requires_grad_(False)
    m.out_net[2][2].bias.requires_grad_(False)
    with pytest.raises(ValueError, match=r"out_net\.2\.2\.bias"):
        step(*stacks, gt, mask, 2)


# ------------------------------------------------------------------------------------------------ kernel, header
def test_bias_only_kernel_resources(usage):  # noqa: F811
    """what the slice kernel is held to: no scratch and at most 48 registers, so that the pass fits beside a resident wide
    weight gradient (2 x 232 + 48 <= 512 per SIMD lane)"""
    rows = [v for k, v in usage.items() if 'bias_grad_rows_kernel' in k]
    assert len(rows) == 1, list(usage)
    vgprs, agprs, scratch, waves = rows[0]
    print(f'bias_grad_rows_kernel: {vgprs} VGPRs, {agprs} AGPRs, {scratch} bytes of scratch, {waves} waves per SIMD')
    assert scratch == 0 and vgprs <= 48 and agprs <= 0, rows
    fin = [v for k, v in usage.items() if 'bias_grad_finish_kernel' in k]
    assert len(fin) == 1 and fin[0][2] == 0, fin


def test_header_states_the_widened_contract():
    from mmlf_amd import _lib
    assert len(_lib.SIGNATURES) == 73
    text = open(os.path.join(ROOT, 'include', 'mmlf_hip.h')).read()
    for entry in ('mmlf_conv2x2_wgrad', 'mmlf_conv2x2_wgrad_split', 'mmlf_conv2x2_wgrad_h2', 'mmlf_conv2x2_wgrad_thin',
                  'mmlf_conv3x3_wgrad'):
        proto = re.search(r'\nint ' + entry + r'\(', text)
        assert proto, entry
        comment = text[text.rindex('/*', 0, proto.start()):proto.start()]
        assert re.search(r'gw_oihw == NULL', comment) and 'bias' in comment and 'gradient alone' in comment, (entry, comment)
    assert 'Both NULL is\n * an error' in text or 'both NULL is an error' in text
