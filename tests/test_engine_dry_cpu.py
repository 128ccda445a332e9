"""The host code of the native trunk (mmlf_amd/engine.py) run dry, without a GPU: engine.call records instead of launching
(tests_helpers.dry_engine, what `tools/launch_trace.py --dry` does), so the calls of a pass can be held against the plan
that is to decide them (Trunk.plan), against the block listing both passes walk (Trunk.sites) and against the extent audit.
Frames are (2, 7, 5) on the tiny nets and the hand-written tables of tests/test_finetune_cpu.py."""
import pytest
import torch

from test_finetune_cpu import PATTERNS, expected_counts, wanted
from test_input_grad_cpu import KINDS, kind_kw
from tests_helpers import dry_engine

B, H, W = 2, 7, 5
WGRAD = {'mmlf_conv2x2_wgrad_h2': 7, 'mmlf_conv2x2_wgrad_thin': 7, 'mmlf_conv3x3_wgrad': 6}     # entry -> index of gw_oihw
CONV = ('mmlf_conv2x2_h2', 'mmlf_conv2x2_thin', 'mmlf_conv3x3')
AUDITED = ('mmlf_conv2x2_h2', 'mmlf_conv2x2_wgrad_h2', 'mmlf_conv3x3', 'mmlf_conv3x3_wgrad', 'mmlf_relu_bwd_slice')
KEYS = ['out_net.2', 'out_net.1', 'out_net.0', 'in_net_id', 'in_net_hv']                     # on_done's documented order


def model_of(kind):
    from mmlf_amd.feed_forward import FeedForward
    torch.manual_seed(0)
    m = FeedForward(**kind_kw(kind, 'base'))
    assert m._native_ok
    return m


def dry_pass(kind, pattern, extents=False):
    """one train-mode forward and backward of `pattern`: (model, tape, forward calls, backward calls, grads, on_done keys)"""
    m = model_of(kind)
    trunk = m._trunk
    names, want_x = wanted(trunk, pattern)
    p = {n: t.detach() for n, t in m._tensor_dict().items()}
    stacks = [torch.zeros(B, 9, 3, H, W) for _ in range(4)]
    grads = {n: torch.zeros_like(p[n]) for n in trunk._grad_names if n in names}
    done = []
    with dry_engine(extents=extents) as calls, torch.no_grad():
        out, tape = trunk.forward(p, stacks, True, True, input_grads=want_x, trainable=names)
        n_fwd = len(calls)
        kept = (tape.concat is not None, [r is not None for r in tape.recs])
        dx = trunk.backward(p, tape, torch.zeros_like(out), grads or None, on_done=done.append, input_grads=want_x)
    assert [g is not None for g in dx] == list(want_x)
    return m, tape, kept, calls[:n_fwd], calls[n_fwd:], grads, done


def counts_of(calls):
    n = dict.fromkeys(('wgrad', 'reduce', 'apply', 'dgrad', 'slice', 'bias_only'), 0)
    for name, args in calls:
        if name in WGRAD:
            n['wgrad'] += 1
            n['bias_only'] += args[WGRAD[name]] is None
        n['reduce'] += name == 'mmlf_bn_bwd_reduce'
        n['apply'] += name == 'mmlf_bn_bwd_apply'
        n['dgrad'] += name in CONV
        n['slice'] += name == 'mmlf_relu_bwd_slice'
    return n


@pytest.mark.parametrize('pattern', list(PATTERNS))
@pytest.mark.parametrize('kind', KINDS)
def test_nothing_but_the_plan_decides_a_backward_launch(kind, pattern):
    m, tape, kept, _, bwd, _, done = dry_pass(kind, pattern)
    trunk = m._trunk
    names, want_x = wanted(trunk, pattern)
    plan = trunk.plan(names, want_x)
    got = counts_of(bwd)
    print(kind, pattern, got)
    assert got == plan.counts() == expected_counts(kind, pattern)
    # on_done: exactly once per key, in the documented order, also for the keys whose blocks launch nothing
    assert done == KEYS
    # forward kept a record for the live blocks and no other, the concat buffer for mmlf_relu_bwd_slice alone ...
    assert kept == (any(plan.slices), [plan.of(site) is not None for site in trunk.sites])
    # ... and backward has released all of it
    assert tape.concat is None and tape.recs == [None] * len(trunk.sites)


@pytest.mark.parametrize('kind', KINDS)
def test_sites_list_the_blocks_in_the_order_of_both_passes(kind):
    m, _, _, fwd, bwd, grads, _ = dry_pass(kind, 'all')
    sites = m._trunk.sites
    assert [s.index for s in sites] == list(range(len(sites)))
    # the module's blocks in state_dict order; H and V run in_net_hv, I and D in_net_id
    blocks = list(dict.fromkeys(k.rsplit('.', 2)[0] for k in m.state_dict()))
    by_net = {net: [b for b in blocks if b.startswith(net + '.')] for net in ('in_net_hv', 'in_net_id', 'out_net')}
    assert sum(by_net.values(), []) == blocks
    assert [s.spec.prefix for s in sites] == by_net['in_net_hv'] * 2 + by_net['in_net_id'] * 2 + by_net['out_net']
    chains = [[s for s in sites if s.chain == c] for c in range(5)]
    for c, chain in enumerate(chains):
        assert [s.k for s in chain] == list(range(len(chain))) and [s.last for s in chain] == [False] * (len(chain) - 1) + [True]
        assert all(s.chain == c and s.var == chain[0].var for s in chain)
    # forward: every block's first convolution reads its filter (or, the thin head, the master filter's) bias, in this order
    bias = {p.data_ptr(): n.rsplit('.', 2)[0] for n, p in m.named_parameters() if n.endswith('.0.bias')}
    first = [bias[args[4]] for name, args in fwd if name in CONV and args[4] in bias]
    assert first == [s.spec.prefix for s in sites]
    # backward: a block's two weight-gradient launches (conv2's, then conv1's) name it by the bias gradient they write
    gb = {g.data_ptr(): n.rsplit('.', 2)[0] for n, g in grads.items() if n.endswith(('.0.bias', '.2.bias'))}
    order = [gb[args[WGRAD[name] + 1]] for name, args in bwd if name in WGRAD]
    assert order[0::2] == order[1::2] == [s.spec.prefix for s in reversed(sites)]


@pytest.mark.parametrize('kind', KINDS)
def test_a_dry_pass_is_audited_launch_by_launch(kind):
    from mmlf_amd import engine
    _, _, _, fwd, bwd, _, _ = dry_pass(kind, 'all', extents=True)
    audited = sum(name in AUDITED for name, _ in fwd + bwd)
    assert audited > 0 and engine.EXTENT_CHECKS == audited == sum(name.startswith('mmlf_audit_') for name, _ in fwd + bwd)
