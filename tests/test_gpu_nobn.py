"""--model_no_batchnorm on the native 2x2 path (reference feed_forward.py:122-137: conv -> ReLU -> conv -> ReLU blocks).

  * mmlf_relu_bwd_slice, the one new kernel (the ReLU backward of a stream's channel slice of the concat buffer), bit for bit
    against the float32 torch expression;
  * the data gradient with the ReLU of its OUTPUT at out_shift = P + 1 (the gradient behind a block's trailing ReLU comes out
    of the next block's first data gradient), in the three arithmetic modes against float64, on the operands, references and
    bars of tests/test_gpu_backward2x2.py, and the f16 split's bit form against the activation form;
  * the tiny nets against the reference's run (tests/golden/g13_nobn_tiny_*.npz), a 70-channel net against the module's own
    float64 CPU path, TrainStep, nn.DataParallel replicas, the Ensamble's fused members and a checkpoint round trip."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, VARIANTS
from mmlf_amd import synth
from test_nobn_cpu import NOBN_TINY_KW, SLICE_CASES, gained_state, loss_of, nobn_golden

pytestmark = pytest.mark.gpu

MODES = ['f32', 'bf16x6', 'f16x3']
SENTINEL = 1234.5
# (1, 6, 10): B R P = 96, no multiple of 512 (nor are the others: 242, 651, 846 -- the tile padding behind the last patch)
SLICE_GEOMS = [(2, 9, 9), (3, 5, 29), (2, 7, 45), (1, 6, 10)]
# forward layers (Cin, Cout) whose data gradient Cout -> Cin is masked: 70 -> 70, 70 -> 27, 280 -> 280, 8 -> 8
DGRAD_PAIRS = [(70, 70), (27, 70), (280, 280), (8, 8)]
# pitch 132: the eight-wave and register-streamed kernels; pitch 384: the two-segment activation window
DGRAD_GEOMS = SLICE_GEOMS + [(1, 3, 130), (1, 2, 382)]


def _dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _model(kw, state, dev=None):
    from mmlf_amd.feed_forward import FeedForward
    m = FeedForward(**kw)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    return m.to(dev or _dev())


@pytest.fixture(autouse=True)
def _mode():
    from mmlf_amd import engine
    keep = engine.CONV_MODE
    yield
    engine.CONV_MODE = keep


# ------------------------------------------------------------------------------------------------ the slice kernel
@pytest.mark.parametrize('B,H,W', SLICE_GEOMS)
@pytest.mark.parametrize('C,cs_src,c_off', SLICE_CASES)
def test_relu_bwd_slice_is_the_float32_select(C, cs_src, c_off, B, H, W):
    from mmlf_amd import _lib, engine
    from mmlf_amd._lib import call, ptr
    dev = _dev()
    geo = engine.Geometry(B, H, W)
    cs_dst = engine.cs_of(C)
    gen = torch.Generator(device=dev).manual_seed(B * 1009 + H * 101 + W * 7 + C + c_off)
    view = lambda t, cs: t[:geo.NQ * cs].view(B, geo.R, geo.P, cs)
    inner = (slice(None), slice(1, H + 1), slice(1, W + 1))
    # source and reference: values everywhere, border and neighbouring slices included (a read of the wrong place shows)
    src = torch.rand(geo.alloc * cs_src, device=dev, generator=gen) * 2 - 1
    # the activations of a ReLU: zeros where the unit is off (about half of them), a few negative zeros and a NaN-free tensor
    ref = (torch.rand(geo.alloc * cs_src, device=dev, generator=gen) * 2 - 1).clamp_min(0)
    ref[::7] *= -1                                                   # -0.0 and some negative values: not > 0
    # ... and a reference of a channel stride of its own (the ABI's cs_ref: the second address computation)
    cs_own = cs_dst + 6
    ref_own = (torch.rand(geo.alloc * cs_own, device=dev, generator=gen) * 2 - 1).clamp_min(0)
    src0, ref0, ref_own0 = src.clone(), ref.clone(), ref_own.clone()
    for ref_t, ref_t0, cs_ref, ref_off, what in (
            (ref, ref0, cs_src, c_off, 'ReLU of the same slice'),
            (ref, ref0, cs_src, (c_off + 2) % (cs_src - C + 1) // 2 * 2, 'ReLU of another slice'),
            (ref_own, ref_own0, cs_own, 4, 'ReLU of a tensor of another channel stride')):
        what = f'{what} C={C} cs_src={cs_src} c_off={c_off} B={B} {H}x{W}'
        dst = torch.full((geo.alloc * cs_dst,), SENTINEL, device=dev)
        amax = torch.zeros(geo.amax_n, device=dev)
        call('mmlf_relu_bwd_slice', ptr(src), cs_src, c_off, ptr(ref_t), cs_ref, ref_off, C, ptr(dst), cs_dst, B, H, W, ptr(amax),
             _lib.stream_ptr())
        want = torch.full_like(dst, SENTINEL)
        wv = view(want, cs_dst)
        wv[:] = 0                                                    # border, pad channels
        s = view(src0, cs_src)[inner][..., c_off:c_off + C]
        r = view(ref_t0, cs_ref)[inner][..., ref_off:ref_off + C]
        wv[inner][..., :C] = torch.where(r > 0, s, torch.zeros_like(s))
        assert torch.equal(dst, want), what                          # (behind the B R P positions: the sentinel)
        assert torch.equal(src, src0) and torch.equal(ref, ref0) and torch.equal(ref_own, ref_own0), what
        assert torch.equal(geo.amax_canonical(amax), geo.amax_of(dst, cs_dst)), what


def test_relu_bwd_slice_refuses_bad_layouts():
    from mmlf_amd import _lib
    from mmlf_amd._lib import call, ptr
    dev = _dev()
    p = ptr(torch.zeros(64, device=dev))
    st = _lib.stream_ptr()

    def refused(*args):
        with pytest.raises(RuntimeError, match='mmlf_relu_bwd_slice'):
            call('mmlf_relu_bwd_slice', *args, None, st)

    #        src cs_src c_off ref cs_ref ref_off C dst cs_dst B H W
    refused(p, 280, 71, p, 280, 70, 70, p, 72, 1, 1, 1)              # odd c_off
    refused(p, 280, 70, p, 280, 71, 70, p, 72, 1, 1, 1)              # odd ref_off
    refused(p, 280, 212, p, 280, 0, 70, p, 72, 1, 1, 1)              # a slice past cs_src
    refused(p, 280, 0, p, 72, 4, 70, p, 72, 1, 1, 1)                 # a slice past cs_ref
    refused(p, 280, 0, p, 280, 0, 0, p, 72, 1, 1, 1)                 # C = 0
    refused(p, 280, 0, p, 280, 0, 76, p, 72, 1, 1, 1)                # C > cs_dst
    refused(p, 1040, 0, p, 1040, 0, 516, p, 520, 1, 1, 1)            # C > 512
    refused(p, 280, 0, p, 280, 0, 70, p, 70, 1, 1, 1)                # cs_dst % 4
    refused(p, 281, 0, p, 280, 0, 70, p, 72, 1, 1, 1)                # odd cs_src
    refused(p, 280, 0, p, 280, 0, 70, p, 72, 0, 1, 1)                # B = 0
    refused(p, 280, 0, p, 280, 0, 70, p, 72, 1, 1, 0)                # W = 0
    refused(None, 280, 0, p, 280, 0, 70, p, 72, 1, 1, 1)             # no source
    refused(p, 280, 0, None, 280, 0, 70, p, 72, 1, 1, 1)             # no reference
    refused(p, 280, 0, p, 280, 0, 70, None, 72, 1, 1, 1)             # no destination


# ------------------------------------------------------------------------------------------------ masked data gradient
def _case(cin, cout, B, H, W, integer):
    import test_gpu_backward2x2 as b2
    # pad 1: the forward layer is the block's first convolution, its data gradient writes extent (H, W) at out_shift = P + 1
    return b2._Case(B, H, W, cin, cout, 1, 2 if (cin, cout) in b2.STREAM_PAIRS and W % 2 else 0, integer,
                    b2._seed(B, H, W, cin, cout, 1, integer) + 17)


@pytest.mark.parametrize('B,H,W', DGRAD_GEOMS)
@pytest.mark.parametrize('cin,cout', DGRAD_PAIRS)
@pytest.mark.parametrize('mode', MODES)
def test_dgrad_with_the_relu_of_its_output_at_shift_p_plus_1(mode, cin, cout, B, H, W):
    """plain, relu_ref and (f16 split) relu_mask_in, every position of the buffer: the real-valued leg at the shared float64
    bar, the exact-integer leg bit for bit (tests/test_gpu_backward2x2.py: _Case.check_dgrad, unchanged).  That file's pad-1
    sweep holds the same three forms at this shift on its own frames; what this one adds are the frames of the no-BatchNorm
    tests and pitch 132."""
    for integer in (False, True):
        c = _case(cin, cout, B, H, W, integer)
        assert c.geo.P + 1 - c.fwd_shift == c.geo.P + 1 and (c.ih, c.iw, c.ioff) == (H, W, 1)
        c.check_dgrad(mode)


@pytest.mark.parametrize('B,H,W', DGRAD_GEOMS)
@pytest.mark.parametrize('cin,cout', DGRAD_PAIRS)
def test_f16_split_mask_bits_give_the_bits_of_the_activation_form(cin, cout, B, H, W):
    """the bits a real conv2 forward launch of the same geometry and width left (ReLU, out_shift = P + 1, mask_out) against
    relu_ref = that launch's output"""
    c = _case(cin, cout, B, H, W, False)
    geo, cs = c.geo, c.cs_in
    y, mask = c.relu_mask('f16x3')
    outs = []
    for kw in (dict(ref=y), dict(mask_in=mask)):
        out = torch.full((geo.alloc * cs,), SENTINEL, device=c.dev)
        out.absmax = torch.zeros(geo.amax_n, device=c.dev)
        c.launch_dgrad('f16x3', out, cs, 0, cs, **kw)
        outs.append(out)
    assert torch.equal(outs[0], outs[1]), c.tag
    assert torch.equal(outs[0].absmax, outs[1].absmax), c.tag
    live = (outs[0][:geo.NQ * cs].view(B, geo.R, geo.P, cs)[:, 1:H + 1, 1:W + 1, :cin] != 0).float().mean()
    assert 0.05 < float(live) < 0.95, (c.tag, float(live))           # the mask kept some elements and removed some


# ------------------------------------------------------------------------------------------------ tiny nets against g13
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


@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('mode', MODES)
def test_g13_tiny_forward_backward_vs_reference(mode, variant, monkeypatch):
    """eval outputs, train outputs, loss and every gradient at the bars tests/test_gpu_model.py applies to G1"""
    from mmlf_amd import engine
    monkeypatch.setattr(engine, 'CONV_MODE', mode)
    g, kw, state = nobn_golden(variant)
    dev = _dev()
    m = _model(kw, state)
    assert m._native_ok
    stacks = [torch.from_numpy(g[f'in{i}']).to(dev) for i in range(4)]
    spy = _Spy(monkeypatch)
    m.eval()
    with torch.no_grad():
        ev = m(*stacks)
    for k, v in ev.items():
        if v is None:
            assert f'eval_{k}' not in g
        else:
            np.testing.assert_allclose(v.cpu().numpy(), g[f'eval_{k}'], rtol=5e-5, atol=5e-6, err_msg=f'eval {k}')
    m.train()
    out = m(*stacks)
    for k, v in out.items():
        if v is not None and k != 'one_hot':
            np.testing.assert_allclose(v.detach().cpu().numpy(), g[f'train_{k}'], rtol=1e-4, atol=1e-5, err_msg=f'train {k}')
    # one function in both modes, from the same launches: identical bits (the saving pass only adds the mask words)
    for k, v in out.items():
        if v is not None:
            assert torch.equal(v.detach(), ev[k]), k
    lv = loss_of(variant, out, torch.from_numpy(g['gt']).to(dev), torch.from_numpy(g['mask']).to(dev))
    np.testing.assert_allclose(lv.item(), g['loss'], rtol=2e-5)
    lv.backward()
    for n, p in m.named_parameters():
        ref = g[f'grad/{n}']
        scale = max(np.abs(ref).max(), 1e-6)
        err = np.abs(p.grad.cpu().numpy() - ref).max()
        print(f'g13 {variant} {mode} {n}: max |gradient error| {err:.3e} of bar {5e-4 * scale + 5e-7:.3e}')
        assert err <= 5e-4 * scale + 5e-7, (n, err, scale)
    names = set(spy.names)
    conv = {'f16x3': 'mmlf_conv2x2_h2', 'bf16x6': 'mmlf_conv2x2_split', 'f32': 'mmlf_conv2x2'}[mode]
    wg = {'f16x3': 'mmlf_conv2x2_wgrad_h2', 'bf16x6': 'mmlf_conv2x2_wgrad_split', 'f32': 'mmlf_conv2x2_wgrad'}[mode]
    assert conv in names and wg in names, names
    assert spy.names.count('mmlf_relu_bwd_slice') == 4, spy.names      # one per stream
    assert not [n for n in names if n.startswith('mmlf_bn_') or n.startswith('mmlf_fold_bn')], names


# ------------------------------------------------------------------------------------------------ a 70-channel net
@pytest.mark.parametrize('H,W', [(17, 21), (5, 130)])
@pytest.mark.parametrize('mode', MODES)
def test_70_channel_net_against_float64(mode, H, W, monkeypatch):
    """model_chs = 70 (the 80- and 288-column kernels, the 70-wide slices of the 280-wide concat buffer), two stream blocks,
    three merge blocks, UPR head, bs = 3, against the same module in float64 on the CPU.  Outputs to 1e-4; gradients per
    tensor at the bar tests/test_gpu_ksize3.py::test_k3_base_size_native_vs_stock_on_cuda holds two implementations of a net of
    this width to (relative L2: worst tensor 6e-2, median 4e-2, with its absolute floor) -- the bar of the ill-conditioned
    end-to-end gradient, not of the kernels, which the tests above hold to float64 element by element."""
    from mmlf_amd import engine, loss
    monkeypatch.setattr(engine, 'CONV_MODE', mode)
    kw = dict(NOBN_TINY_KW, model_chs=70, model_in_blocks=2, model_out_blocks=3, model_uncert=True)
    # variance-preserving filters, and the first seed from 23 at which the head's two units are not both off over the whole
    # frame (23: every gradient below the head is exactly zero): asserted on the float64 run below
    state = gained_state(kw, 24)
    stacks, gt, mask = synth.synth_inputs(3, H, seed=11, ps_w=W)
    m_mask = torch.from_numpy(mask).int() * loss.create_mask_margin(mask.shape, 2)
    runs = {}
    for dev, dt in ((_dev(), torch.float32), (torch.device('cpu'), torch.float64)):
        m = _model(kw, state, dev).to(dt)
        assert m._native_ok
        m.train()
        out = m(*[torch.from_numpy(s).to(dev, dt) for s in stacks])
        lv = loss.ImprovedUncertaintyL1Loss()(out, torch.from_numpy(gt).to(dev, dt), m_mask.to(dev), None)
        lv.backward()
        runs[dev.type] = ({k: out[k].detach().double().cpu() for k in ('mean', 'logvar')}, float(lv),
                          {n: p.grad.double().cpu() for n, p in m.named_parameters()})
    (o1, l1, g1), (o0, l0, g0) = runs['cuda'], runs['cpu']
    assert min(float(v.norm()) for v in g0.values()) >= 1e-1       # above the measure's floor, 1e-6 sqrt(numel) / 3e-2 <= 0.019
    for k in o0:
        err = float((o1[k] - o0[k]).abs().max())
        print(f'nobn70 {mode} {H}x{W} {k}: max |error| {err:.3e}')
        assert err <= 1e-4, (k, err)
    assert abs(l1 - l0) <= 1e-4 * abs(l0)
    rels = {}
    for n in g0:
        rels[n] = float((g1[n] - g0[n]).norm()) / (float(g0[n].norm()) + 1e-6 * g0[n].numel() ** 0.5 / 3e-2)
    worst = max(rels, key=rels.get)
    med = float(np.median(list(rels.values())))
    print(f'nobn70 {mode} {H}x{W}: gradient relative L2 per tensor: median {med:.3e}, worst {worst} {rels[worst]:.3e}')
    assert rels[worst] <= 6e-2 and med <= 4e-2, (worst, rels[worst], med)


# ------------------------------------------------------------------------------------------------ TrainStep
def _steps(m, dev, n=2, eval_mode=False):
    from mmlf_amd.train import TrainStep
    step = TrainStep(m, lr=1e-3, loss_margin=3, train_eval_mode=eval_mode)
    for it in range(n):
        stacks, gt, mask = synth.synth_inputs(2, 16, seed=60 + it)
        step(*[torch.from_numpy(s).to(dev) for s in stacks], torch.from_numpy(gt).to(dev), torch.from_numpy(mask).to(dev), it + 1)
    return step


@pytest.mark.parametrize('mode', MODES)
def test_train_step_two_steps_against_the_float64_reference_loop(mode, monkeypatch):
    """TrainStep (flat parameters, native loss, mmlf_adam_step) on the tiny UPR net against the reference's loop shape --
    autograd and torch.optim.Adam on the stock path -- in float64 on the CPU.  The bar is the one
    tests/test_gpu_ksize3.py::test_k3_train_step_native_vs_stock holds a native and a stock run to: per tensor within 5 % of
    how far the two steps moved it (Adam normalises each element's step to about lr whatever the size of its gradient, so an
    element whose gradient is rounding noise moves by lr in a direction that is noise too).  --train_eval_mode changes nothing
    in a net without BatchNorm: the same bits."""
    from mmlf_amd import engine, loss
    monkeypatch.setattr(engine, 'CONV_MODE', mode)
    dev = _dev()
    kw = dict(NOBN_TINY_KW, model_uncert=True)
    state = gained_state(kw, 17)
    w0 = {k: torch.from_numpy(np.asarray(v)).double() for k, v in state.items()}
    m = _model(kw, state)
    step = _steps(m, dev)
    assert [n for n, _ in m.named_buffers()] == [] and step.sync_buffers() is None      # nothing to broadcast
    got = {k: v.detach().double().cpu() for k, v in m.state_dict().items()}
    ref = _model(kw, state, torch.device('cpu')).double()
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
        print(f'nobn TrainStep {mode} {k}: {dist:.3e} from float64, moved {moved:.3e}')
        assert moved >= 2e-4 * v.numel() ** 0.5, (k, moved)          # (two Adam steps of 1e-3: an rms of a tenth of that at least)
        assert dist <= 0.05 * moved + 1e-6, (k, dist, moved)
    m2 = _model(kw, state)
    _steps(m2, dev, eval_mode=True)
    for (k, a), (_, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k


CHILD = """
import sys
import numpy as np, torch
sys.path.insert(0, {root!r})
from mmlf_amd import engine, synth
from mmlf_amd.feed_forward import FeedForward
from mmlf_amd.train import TrainStep
kw = {kw!r}
m = FeedForward(**kw)
sys.path.insert(0, {root!r} + '/tests')
from test_nobn_cpu import gained_state
m.load_state_dict({{k: torch.from_numpy(np.asarray(v)) for k, v in gained_state(kw, 20).items()}})
m = m.to('cuda:0')
step = TrainStep(m, lr=1e-3, loss_margin=3)
for it in range(2):
    stacks, gt, mask = synth.synth_inputs(2, 16, seed=70 + it)
    step(*[torch.from_numpy(s).to('cuda:0') for s in stacks], torch.from_numpy(gt).to('cuda:0'), torch.from_numpy(mask).to('cuda:0'), it + 1)
torch.cuda.synchronize()
torch.save({{'overlap': engine.OVERLAP_WGRAD, 'grad': step.grad.cpu(), 'flat': step.flat.cpu(), 'layout': list(step.layout)}}, {out!r})
"""


def test_side_stream_weight_gradient_gives_the_same_bits(tmp_path):
    """MMLF_OVERLAP_WGRAD is read once per process: one child each.  model_chs = 32 makes the merge blocks 128 wide, the
    width from which the side stream takes the first weight gradient (the tiny net's 32-wide blocks never do)."""
    kw = dict(NOBN_TINY_KW, model_chs=32, model_uncert=True)
    res = {}
    for overlap in ('0', '1'):
        out = str(tmp_path / f'overlap{overlap}.pt')
        env = dict(os.environ, MMLF_OVERLAP_WGRAD=overlap)
        p = subprocess.run([sys.executable, '-c', CHILD.format(root=ROOT, kw=kw, out=out)], env=env, capture_output=True,
                           text=True, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        res[overlap] = torch.load(out)
        assert res[overlap]['overlap'] is (overlap == '1')
    for name, o, n in res['0']['layout']:                            # (a seed at which no tensor's gradient is all zero)
        assert float(res['0']['grad'][o:o + n].abs().max()) > 0, name
    assert torch.equal(res['0']['grad'], res['1']['grad']) and torch.equal(res['0']['flat'], res['1']['flat'])


def test_training_step_passes_the_extent_audit_and_a_short_dst_is_refused(monkeypatch):
    from mmlf_amd import engine
    dev = _dev()
    monkeypatch.setattr(engine, 'CONV_MODE', 'f16x3')
    monkeypatch.setattr(engine, 'CHECK_EXTENTS', True)
    kw = dict(NOBN_TINY_KW, model_uncert=True)
    m = _model(kw, gained_state(kw, 3))
    spy = _Spy(monkeypatch)
    before = engine.EXTENT_CHECKS
    step = _steps(m, dev, n=1)
    torch.cuda.synchronize()
    assert torch.isfinite(step.grad).all() and float(step.grad.abs().max()) > 0
    # every convolution, weight-gradient and slice launch of the step was checked: no gap
    launches = [n for n in spy.names if n in ('mmlf_conv2x2_h2', 'mmlf_conv2x2_wgrad_h2', 'mmlf_relu_bwd_slice')]
    assert spy.names.count('mmlf_relu_bwd_slice') == 4
    assert engine.EXTENT_CHECKS - before == len(launches)
    assert spy.names.count('mmlf_audit_relu_bwd_slice') == 4
    geo = engine.Geometry(2, 16, 16)
    src = geo.buf(32, dev)
    short = torch.zeros(geo.NQ * 8 - 1, device=dev)
    with pytest.raises(RuntimeError, match='MMLF_CHECK_EXTENTS.*dst'):
        engine.relu_bwd_slice(geo, src, 32, 8, src, 32, 8, 8, short, 8)
    assert spy.names.count('mmlf_relu_bwd_slice') == 4                # (refused before the launch)


# ------------------------------------------------------------------------------------------------ above the trunk
def test_dataparallel_replicas_on_the_native_path():
    """two replicas on the one GPU (tests/test_round2.py): without BatchNorm the network is a function of each patch alone,
    so the gathered output and the reduced gradients are those of the un-wrapped module on the whole batch"""
    from mmlf_amd import loss
    dev = _dev()
    kw = dict(NOBN_TINY_KW, model_uncert=True)
    state = gained_state(kw, 5)
    stacks, gt, mask = synth.synth_inputs(4, 16, seed=3)
    data = [torch.from_numpy(s).to(dev) for s in stacks]
    tgt, tmask = torch.from_numpy(gt).to(dev), torch.from_numpy(mask).to(dev)
    m = _model(kw, state)
    # (torch accepts duplicate device ids and runs two replicas on the one device: nothing of the code under test stands
    # inside a try, a failure of the replicated forward is a failure of this test)
    dp = torch.nn.DataParallel(m, device_ids=[0, 0])
    dp.train()
    out = dp(*data)
    loss.ImprovedUncertaintyL1Loss()(out, tgt, tmask, None).backward()
    ref = _model(kw, state)
    ref.train()
    out2 = ref(*data)
    loss.ImprovedUncertaintyL1Loss()(out2, tgt, tmask, None).backward()
    for k in ('mean', 'logvar'):
        np.testing.assert_allclose(out[k].detach().cpu().numpy(), out2[k].detach().cpu().numpy(), rtol=1e-5, atol=1e-6)
    for (n, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
        scale = max(float(q.grad.abs().max()), 1e-6)
        assert float((p.grad - q.grad).abs().max()) <= 2e-4 * scale + 1e-7, n


def test_ensamble_fused_members_give_the_bits_of_the_module_path(monkeypatch):
    from mmlf_amd import ensamble
    dev = _dev()
    kw = dict(NOBN_TINY_KW, model_uncert=True)
    m = _model(kw, gained_state(kw, 31)).eval()
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
        assert not [n for n in spy.names if n.startswith('mmlf_bn_') or n.startswith('mmlf_fold_bn')], spy.names
    for k, v in res[False].items():
        assert torch.equal(res[True][k], v), k


def test_checkpoint_round_trip(tmp_path):
    from mmlf_amd import dl
    dev = _dev()
    kw = dict(NOBN_TINY_KW, model_uncert=True)
    m = _model(kw, gained_state(kw, 41))
    step = _steps(m, dev, n=1)
    path = str(tmp_path / 'nobn.pt')
    dl.ModelSaver()(path, m, step, kw, 0, 1, 0.5)
    saved = torch.load(path)
    assert list(saved['model_state_dict']) == [n for n, _, _ in synth.param_spec(**kw)]
    m2 = _model(kw, gained_state(kw, 42))
    from mmlf_amd.train import TrainStep
    step2 = TrainStep(m2, lr=1e-3, loss_margin=3)
    it, _ = dl.load_checkpoint(path, m2, step2, map_location=dev)
    assert it == 1
    for (k, a), (_, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
    stacks, _, _ = synth.synth_inputs(1, 12, seed=2)
    m.eval(), m2.eval()
    with torch.no_grad():
        a, b = (mm(*[torch.from_numpy(s).to(dev) for s in stacks]) for mm in (m, m2))
    assert torch.equal(a['mean'], b['mean']) and torch.equal(a['logvar'], b['logvar'])
