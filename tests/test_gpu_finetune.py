"""Partial training on the native trunk: backward only where something trains.

  * module level: a partly frozen model against the same model, all trainable, on the same inputs -- outputs, BatchNorm
    buffers and every wanted gradient bit for bit, frozen parameters without a gradient, and the launches of the pass those
    of engine.Trunk.plan (tests/test_finetune_cpu.py holds the plan to hand-written tables); three trunk kinds, three heads,
    two frames, train and eval mode, the other two arithmetic modes in child processes;
  * TrainStep: frozen parameters and their moments do not move a bit, the trained ones move exactly as in a run that forms
    every gradient and zeroes the frozen slices before Adam; the extent audit; the order of the gradient-bucket hook;
  * kernel level: the bias gradient without a weight gradient (gw = NULL) through each of the five weight-gradient entry
    points against the float64 sum.

The reference trains through nn.Module parameters (mmlf/train/cli.py:243-258): autograd forms no gradient for a parameter
with requires_grad False and optim.Adam skips it."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, VARIANTS
from mmlf_amd import synth
from test_finetune_cpu import PATTERNS, wanted
from test_gpu_kernels import grid_from_nchw
from test_input_grad_cpu import KINDS, bar, build, inputs, kind_kw, kind_state, run, seed_of

pytestmark = pytest.mark.gpu

FRAMES = [(2, 9, 13), (3, 5, 29)]
EVAL_FRAME = (3, 5, 29)
GPU_PATTERNS = ['head', 'out_net', 'id_frozen', 'mid_frozen', 'streams_frozen_v', 'bias_bn']
# ... and the full run that also wants V's gradient, for the pattern that does
RUNS = dict(PATTERNS, all_v=(PATTERNS['all'][0], PATTERNS['streams_frozen_v'][1]))
WGRAD_ENTRIES = ('mmlf_conv2x2_wgrad', 'mmlf_conv3x3_wgrad')


def _dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


class _Spy:
    """records the entry points (and their arguments) that go through _lib.call from the engine and the module"""

    def __init__(self, monkeypatch):
        from mmlf_amd import _lib, engine, feed_forward
        self.calls = []
        real = _lib.call

        def call(name, *args):
            self.calls.append((name, args))
            return real(name, *args)
        for mod in (_lib, engine, feed_forward):
            monkeypatch.setattr(mod, 'call', call)

    def counts(self):
        """the backward launches by the kinds of Plan.counts()"""
        from mmlf_amd import engine
        names = [n for n, _ in self.calls]
        conv = {'f16x3': 'mmlf_conv2x2_h2', 'bf16x6': 'mmlf_conv2x2_split'}.get(engine.CONV_MODE, 'mmlf_conv2x2')
        bwd = names[names.index('mmlf_unpack_nchw') + 1:]              # (the forward ends with the output's unpack)
        wg = [(n, a) for n, a in self.calls if n.startswith(WGRAD_ENTRIES)]
        # gw is the 8th argument of the 2x2 entry points, the 7th of the 3x3 one
        null_gw = sum(1 for n, a in wg if a[6 if n.startswith('mmlf_conv3x3') else 7] is None)
        return {'wgrad': len(wg), 'reduce': names.count('mmlf_bn_bwd_reduce'), 'apply': names.count('mmlf_bn_bwd_apply'),
                'dgrad': sum(1 for n in bwd if n in (conv, 'mmlf_conv3x3')), 'slice': names.count('mmlf_relu_bwd_slice'),
                'bias_only': null_gw}


def _model_run(kind, variant, frame, eval_mode, pattern, spy=None):
    """one forward + backward of a model frozen by `pattern`: (module, output dict, input gradients)"""
    seed = seed_of(kind, variant, frame, eval_mode)
    kw = kind_kw(kind, variant)
    m = build(kw, kind_state(kind, kw, seed), _dev())
    assert m._native_ok
    m.train(not eval_mode)
    keep, want_x = RUNS[pattern]
    for n, p in m.named_parameters():
        p.requires_grad_(bool(keep(n)))
    if spy is not None:
        del spy.calls[:]
    out, dx = run(m, variant, *inputs(frame, seed, _dev()), want=want_x)
    return m, out, dx


def check_pattern(kind, variant, frame, eval_mode, pattern, spy):
    tag = f'{"eval " if eval_mode else ""}{kind} {variant} {frame} {pattern}'
    keep, want_x = PATTERNS[pattern]
    full, out0, dx0 = _model_run(kind, variant, frame, eval_mode, 'all' if want_x == PATTERNS['all'][1] else 'all_v')
    m, out, dx = _model_run(kind, variant, frame, eval_mode, pattern, spy)
    got = spy.counts()
    names, _ = wanted(m._trunk, pattern)
    plan = m._trunk.plan(names, want_x, train=not eval_mode)
    print(f'{tag}: launches {got}')
    assert got == plan.counts(), (tag, got, plan.counts())
    for k, v in out.items():
        assert (v is None and out0[k] is None) or torch.equal(v, out0[k]), (tag, k)
    for (n, a), (_, b) in zip(m.named_buffers(), full.named_buffers()):
        assert torch.equal(a, b), (tag, n)
    for a, b, w in zip(dx, dx0, want_x):
        assert (a is None) == (not w) and (not w or torch.equal(a, b)), tag
    for (n, p), (_, q) in zip(m.named_parameters(), full.named_parameters()):
        if not keep(n):
            assert p.grad is None, (tag, n)
        elif pattern == 'bias_bn' and n.endswith(('.0.bias', '.2.bias')):
            # another kernel than the weight gradient's ones row: the project's gradient bar, not bit equality
            err = float((p.grad.double() - q.grad.double()).abs().max())
            print(f'{tag} {n}: bias-only gradient {err:.3e} from the weight-gradient launch\'s, bar {bar(q.grad):.3e}')
            assert err <= bar(q.grad), (tag, n, err)
        else:
            assert p.grad is not None and torch.equal(p.grad, q.grad), (tag, n)


@pytest.mark.parametrize('frame', FRAMES)
@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('kind', KINDS)
def test_partly_frozen_models_in_train_mode(kind, variant, frame, monkeypatch):
    spy = _Spy(monkeypatch)
    for pattern in GPU_PATTERNS:
        check_pattern(kind, variant, frame, False, pattern, spy)


@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('kind', KINDS)
def test_partly_frozen_models_in_eval_mode(kind, variant, monkeypatch):
    spy = _Spy(monkeypatch)
    for pattern in GPU_PATTERNS:
        check_pattern(kind, variant, EVAL_FRAME, True, pattern, spy)


CHILD = """
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {root!r} + '/tests')
from mmlf_amd import engine
assert engine.CONV_MODE == {mode!r}, engine.CONV_MODE
import pytest
import test_gpu_finetune as t
mp = pytest.MonkeyPatch()
spy = t._Spy(mp)
for pattern in t.GPU_PATTERNS:
    t.check_pattern('bn2', 'upr', (2, 9, 13), False, pattern, spy)
mp.undo()
print('child ok')
"""


@pytest.mark.parametrize('mode', ['bf16x6', 'f32'])
def test_partly_frozen_models_in_the_other_modes(mode):
    """MMLF_CONV_MODE is read once per process: a fresh child each (tests/test_gpu_input_grad.py does the same)"""
    env = dict(os.environ, MMLF_CONV_MODE=mode)
    p = subprocess.run([sys.executable, '-c', CHILD.format(root=ROOT, mode=mode)], env=env, capture_output=True, text=True,
                       timeout=300)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and 'child ok' in p.stdout, p.stderr[-3000:]


# ------------------------------------------------------------------------------------------------ TrainStep
STEP_PATTERNS = {'head': lambda n: n.startswith('out_net.2.'), 'in_net_frozen': lambda n: n.startswith('out_net.')}


def _batches(n, dev):
    out = []
    for it in range(n):
        stacks, gt, mask = synth.synth_inputs(2, 16, seed=70 + it)
        out.append(([torch.from_numpy(s).to(dev) for s in stacks], torch.from_numpy(gt).to(dev), torch.from_numpy(mask).to(dev)))
    return out


def _step_model(keep, kind='bn2'):
    kw = kind_kw(kind, 'upr')
    m = build(kw, kind_state(kind, kw, 5), _dev())
    for n, p in m.named_parameters():
        p.requires_grad_(bool(keep(n)))
    return m


@pytest.mark.parametrize('pattern', list(STEP_PATTERNS))
def test_train_step_leaves_frozen_parameters_and_moves_the_rest_as_a_full_backward_does(pattern):
    from mmlf_amd.train import TrainStep
    keep = STEP_PATTERNS[pattern]
    dev = _dev()
    batches = _batches(2, dev)
    m = _step_model(keep)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    step = TrainStep(m, lr=1e-3, loss_margin=3)
    assert step.trainable == {n for n in before if keep(n)}
    for it, (stacks, gt, mask) in enumerate(batches):
        step(*stacks, gt, mask, it + 1)
    # the same parameters trained by a step that forms every gradient and zeroes the frozen ones' slices before Adam
    full = _step_model(lambda n: True)
    ref = TrainStep(full, lr=1e-3, loss_margin=3)
    adam = ref._adam

    def masked_adam(lr, grad_scale):
        for n, o, sz in ref.layout:
            if not keep(n):
                ref.grad[o:o + sz].zero_()
        adam(lr, grad_scale)
    ref._adam = masked_adam
    for it, (stacks, gt, mask) in enumerate(batches):
        ref(*stacks, gt, mask, it + 1)
    torch.cuda.synchronize()
    moved = 0
    for n, o, sz in step.layout:
        p = dict(m.named_parameters())[n]
        if keep(n):
            assert torch.equal(p, dict(full.named_parameters())[n]), (pattern, n)
            assert torch.equal(step.exp_avg[o:o + sz], ref.exp_avg[o:o + sz]), (pattern, n)
            assert torch.equal(step.exp_avg_sq[o:o + sz], ref.exp_avg_sq[o:o + sz]), (pattern, n)
            moved += int(not torch.equal(p, before[n]))
        else:
            # bit for bit, the sign of a zero included
            assert torch.equal(p.view(torch.int32), before[n].view(torch.int32)), (pattern, n)
            for buf in (step.grad, step.exp_avg, step.exp_avg_sq):
                assert not bool(buf[o:o + sz].view(torch.int32).any()), (pattern, n)
    assert moved == len(step.trainable)
    for (n, a), (_, b) in zip(m.named_buffers(), full.named_buffers()):
        assert torch.equal(a, b), (pattern, n)
    assert len(step.optimizer_state_dict()['state']) == len(step.layout)


@pytest.mark.parametrize('kind', KINDS)
def test_extent_audit_passes_a_pruned_step(kind, monkeypatch):
    from mmlf_amd import engine
    from mmlf_amd.train import TrainStep
    monkeypatch.setattr(engine, 'CONV_MODE', 'f16x3')
    monkeypatch.setattr(engine, 'CHECK_EXTENTS', True)
    (stacks, gt, mask), = _batches(1, _dev())
    for pattern in list(STEP_PATTERNS) + ['bias_bn']:
        keep = STEP_PATTERNS.get(pattern) or PATTERNS[pattern][0]
        step = TrainStep(_step_model(keep, kind), lr=1e-3, loss_margin=3)
        before = engine.EXTENT_CHECKS
        loss = step(*stacks, gt, mask, 1)
        assert np.isfinite(float(loss)) and engine.EXTENT_CHECKS > before, (kind, pattern)


@pytest.mark.parametrize('kind', KINDS)
def test_on_done_reports_every_key_once_in_order(kind):
    dev = _dev()
    (stacks, gt, mask), = _batches(1, dev)
    for pattern in ['all'] + GPU_PATTERNS + ['v_only', 'hv00']:
        keep, want_x = PATTERNS[pattern]
        m = _step_model(keep, kind)
        m.train()
        p = m._tensor_dict()
        names = [n for n in m._param_names if keep(n)]
        with torch.no_grad():
            out, tape = m._trunk.forward(p, stacks, True, True, input_grads=want_x, trainable=names)
            grads = {n: torch.zeros_like(p[n]) for n in names} or None
            done = []
            dx = m._trunk.backward(p, tape, torch.ones_like(out), grads, on_done=done.append, input_grads=want_x)
        torch.cuda.synchronize()
        assert done == ['out_net.2', 'out_net.1', 'out_net.0', 'in_net_id', 'in_net_hv'], (kind, pattern, done)
        assert [g is not None for g in dx] == list(want_x), (kind, pattern)


# ------------------------------------------------------------------------------------------------ kernel level
BIAS_WIDTHS = [1, 2, 8, 70, 72, 108, 280, 288, 512]
BIAS_FRAMES = [(1, 1, 1), (3, 5, 29), (1, 7, 130), (1, 2, 382)]
ENTRIES = {                                # entry point -> (widths it takes, 3x3 geometry)
    'mmlf_conv2x2_wgrad': (BIAS_WIDTHS, False),
    'mmlf_conv2x2_wgrad_split': (BIAS_WIDTHS, False),
    'mmlf_conv2x2_wgrad_h2': (BIAS_WIDTHS, False),
    'mmlf_conv2x2_wgrad_thin': ([1, 2], False),
    'mmlf_conv3x3_wgrad': ([c for c in BIAS_WIDTHS if c <= 288], True),
}
CIN, GUARD = 8, 64
SENTINEL = 12345.0


def _workspace_floats(entry, C, B, H, W):
    from mmlf_amd import _lib
    L = _lib.load()
    if entry == 'mmlf_conv2x2_wgrad_thin':
        return int(L.mmlf_conv2x2_wgrad_thin_workspace_floats(CIN))
    if entry == 'mmlf_conv3x3_wgrad':
        return int(L.mmlf_wgrad3x3_workspace_floats(CIN, C, B, H, W))
    return int(L.mmlf_wgrad_workspace_floats(CIN, C, B, H, W))


def _bias_only(entry, geo, x, g, cs_g, C, g_shift, gw, gb, accumulate, ws):
    """one launch of `entry` (returns its status instead of raising)"""
    from mmlf_amd import _lib
    from mmlf_amd._lib import ptr
    L = _lib.load()
    st = _lib.stream_ptr()
    head = (ptr(x), CIN, CIN, ptr(g), cs_g, C)
    tail = (ptr(gw), ptr(gb), 0, accumulate, ptr(ws), geo.B, geo.H, geo.W)
    if entry == 'mmlf_conv3x3_wgrad':
        return L.mmlf_conv3x3_wgrad(*head, *tail, st)
    if entry == 'mmlf_conv2x2_wgrad_h2':
        return L.mmlf_conv2x2_wgrad_h2(*head, g_shift, *tail, ptr(x.amax), ptr(g.amax), st)
    return getattr(L, entry)(*head, g_shift, *tail, st)


@pytest.mark.parametrize('B,H,W', BIAS_FRAMES)
@pytest.mark.parametrize('entry', list(ENTRIES))
def test_bias_gradient_without_a_weight_gradient(entry, B, H, W):
    """gb[c] (+)= sum_q g[q + g_shift][c] against the float64 sum, per channel within
        2^-23 |ref| + 2^-40 sum_q |g[q][c]|
    -- one or two float32 roundings of a float64 accumulation plus that accumulation's own error over at most 2^31 terms;
    small integers bit for bit; two launches the same bits; nothing outside gb[0:C] and the workspace is written."""
    from mmlf_amd import _lib, engine
    dev = _dev()
    widths, k3 = ENTRIES[entry]
    geo = engine.Geometry(B, H, W, 3 if k3 else 2)
    x = torch.zeros(geo.alloc * CIN, device=dev)
    x.amax = geo.amax_of(x, CIN)
    for C in widths:
        cs_g = engine.cs_of(C)
        nws = _workspace_floats(entry, C, B, H, W)
        assert nws > 0
        for g_shift in ([geo.P + 1] if k3 else [0, geo.P + 1]):
            for integers in (False, True):
                rs = np.random.RandomState(C * 7 + W + g_shift + integers)
                h, w, off = (H + 1, W + 1, 0) if g_shift == 0 else (H, W, 1)
                a = (rs.randint(-3, 4, (B, C, h, w)) if integers else rs.uniform(-1, 1, (B, C, h, w))).astype(np.float32)
                g = torch.from_numpy(grid_from_nchw(a, cs_g, geo, offset=off)).to(dev)
                g.amax = geo.amax_of(g, cs_g)
                g0 = g.clone()
                total = a.astype(np.float64).sum((0, 2, 3))
                slack = 2.0 ** -40 * np.abs(a.astype(np.float64)).sum((0, 2, 3))
                for accumulate in (0, 1):
                    tag = f'{entry} C={C} B={B} {H}x{W} g_shift={g_shift} accumulate={accumulate} integers={integers}'
                    old = (rs.randint(-5, 6, C) if integers else rs.uniform(-2, 2, C)).astype(np.float32)
                    ref = total + old.astype(np.float64) if accumulate else total
                    results = []
                    for _ in range(2):
                        gb = torch.full((C + 2 * GUARD,), SENTINEL, device=dev)
                        gb[GUARD:GUARD + C] = torch.from_numpy(old).to(dev)
                        ws = torch.full((nws + 2 * GUARD,), SENTINEL, device=dev)
                        rc = _bias_only(entry, geo, x, g, cs_g, C, g_shift, None, gb[GUARD:], accumulate, ws[GUARD:])
                        assert rc == 0, (tag, _lib.last_error())
                        got = gb.cpu().numpy()
                        assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + C:] == SENTINEL).all(), tag
                        assert bool((ws[:GUARD] == SENTINEL).all() & (ws[GUARD + nws:] == SENTINEL).all()), tag
                        results.append(got[GUARD:GUARD + C].copy())
                    assert torch.equal(g, g0) and not bool(x.any()), tag
                    assert results[0].tobytes() == results[1].tobytes(), tag
                    err = np.abs(results[0].astype(np.float64) - ref)
                    bound = 2.0 ** -23 * np.abs(ref) + slack
                    assert (err <= bound).all(), (tag, float((err - bound).max()))
                    if integers:
                        assert results[0].tobytes() == ref.astype(np.float32).tobytes(), tag
    # both pointers NULL: an error, and nothing is launched or written
    C = widths[-1]
    ws = torch.full((_workspace_floats(entry, C, B, H, W),), SENTINEL, device=dev)
    g = torch.zeros(geo.alloc * engine.cs_of(C), device=dev)
    g.amax = geo.amax_of(g, engine.cs_of(C))
    assert _bias_only(entry, geo, x, g, engine.cs_of(C), C, geo.P + 1, None, None, 0, ws) != 0
    assert 'null pointer' in _lib.last_error()
    torch.cuda.synchronize()
    assert bool((ws == SENTINEL).all())


def test_engine_passes_a_missing_weight_gradient_through(monkeypatch):
    """engine.wgrad / wgrad3 with gw=None under MMLF_CHECK_EXTENTS: the audit is handed no extent for gw, the launch is the
    bias-only one, and a weight gradient with gb=None still leaves the bias gradient alone"""
    from mmlf_amd import engine
    monkeypatch.setattr(engine, 'CHECK_EXTENTS', True)
    dev = _dev()
    B, H, W, cin, cout = 2, 5, 9, 16, 24
    for ksize in (2, 3):
        geo = engine.Geometry(B, H, W, ksize)
        rs = np.random.RandomState(ksize)
        a = rs.uniform(-1, 1, (B, cout, H, W)).astype(np.float32)
        xa = rs.uniform(-1, 1, (B, cin, H, W)).astype(np.float32)
        g = torch.from_numpy(grid_from_nchw(a, engine.cs_of(cout), geo, offset=1)).to(dev)
        x = torch.from_numpy(grid_from_nchw(xa, engine.cs_of(cin), geo, offset=1)).to(dev)
        ws = engine._Workspace.get(dev).wgrad_ws(geo, cin, cout)
        gw = torch.zeros(cout, cin, ksize, ksize, device=dev)
        gb, gb_only = torch.zeros(cout, device=dev), torch.zeros(cout, device=dev)
        before = engine.EXTENT_CHECKS
        if ksize == 3:
            engine.wgrad3(geo, x, engine.cs_of(cin), cin, g, engine.cs_of(cout), cout, gw, gb, 0, ws)
            engine.wgrad3(geo, x, engine.cs_of(cin), cin, g, engine.cs_of(cout), cout, None, gb_only, 0, ws)
        else:
            engine.wgrad(geo, x, engine.cs_of(cin), cin, g, engine.cs_of(cout), cout, geo.P + 1, gw, gb, 0, ws)
            engine.wgrad(geo, x, engine.cs_of(cin), cin, g, engine.cs_of(cout), cout, geo.P + 1, None, gb_only, 0, ws)
        assert engine.EXTENT_CHECKS == before + 2
        ref = torch.from_numpy(a.astype(np.float64).sum((0, 2, 3)))
        assert float((gb_only.double().cpu() - ref).abs().max()) <= 2.0 ** -23 * float(ref.abs().max()) + 2.0 ** -40 * float(np.abs(a).sum())
        assert float((gb.double().cpu() - ref).abs().max()) <= bar(ref)
        assert bool(gw.any())
