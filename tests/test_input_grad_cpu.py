"""Gradients with respect to the four view stacks, and a backward without weight gradients, without a GPU: the float64
reference of tests/test_gpu_input_grad.py (the module's own stock path) with its seeds, loss scaling and conditioning, the
audited extents of the launch that forms the input gradient (the data gradient model_chs -> 3 model_views of a stream
net's first convolution), the defaults of the engine's new arguments, and the stock path on CPU tensors.

The reference's FeedForward (mmlf/model/feed_forward.py:226-269) is a tree of nn.Conv2d modules: autograd differentiates it
in h_views ... d_views like any other module."""
import ctypes
import functools
import inspect
import math

import numpy as np
import pytest
import torch

from conftest import TINY_KW, VARIANTS
from mmlf_amd import synth
from test_ksize3_cpu import K3_TINY_KW, k3_spec
from test_nobn_cpu import NOBN_TINY_KW, gained_state

# the three native trunk kinds on the tiny net (model_chs = 8, model_views = 9)
KINDS = ['bn2', 'nobn2', 'k3']
KIND_KW = {'bn2': TINY_KW, 'nobn2': NOBN_TINY_KW, 'k3': K3_TINY_KW}
# (B, H, W): non-square, so that a wrong transpose in the H / I variants cannot pass; pitches 15, 31 and 132
FRAMES = [(2, 9, 13), (3, 5, 29), (1, 7, 130)]
# one frame per trunk kind under m.eval()
EVAL_FRAMES = {'bn2': (3, 5, 29), 'nobn2': (2, 9, 13), 'k3': (1, 7, 130)}
GRAD_FLOOR = 1e-2           # every stack's max |gradient| is lifted to it (tests/golden/make_golden_nobn.py: the floor rule)


def kind_kw(kind, variant):
    return dict(KIND_KW[kind], **VARIANTS[variant])


def kind_state(kind, kw, seed):
    if kind == 'nobn2':
        return gained_state(kw, seed)                    # sqrt(6) filter gain: the signal survives the ReLU-only blocks
    return synth.synth_state(k3_spec(kw) if kind == 'k3' else synth.param_spec(**kw), seed=seed)


def seed_of(kind, variant, frame, eval_mode):
    """0, except where the float32 stock run of seed 0 is not within a tenth of the bar of the float64 one (a ReLU or an
    arg-max that flips between the two precisions: 35 bars for BatchNorm / dpp / (1, 7, 130) in train mode, 1.5 bars for
    (3, 5, 29) in eval mode)"""
    if eval_mode:
        return 1 if frame == (3, 5, 29) else 0
    return 1 if (kind, variant, frame) == ('bn2', 'dpp', (1, 7, 130)) else 0


def build(kw, state, device='cpu', dtype=torch.float32):
    from mmlf_amd.feed_forward import FeedForward
    m = FeedForward(**kw)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    return m.to(device).to(dtype) if dtype != torch.float32 else m.to(device)


def loss_of(variant, out, gt, mask, cls):
    """the variant's own loss; cls: reg_to_class(gt, -3.5, 3.5, 108), taken once from the float32 targets"""
    from mmlf_amd import loss
    if variant == 'upr':
        return loss.ImprovedUncertaintyL1Loss()(out, gt, mask, None)
    if variant == 'dpp':
        return loss.MaskedCrossEntropy()(out, cls, mask)
    return loss.MaskedL1Loss()(out, gt, mask)


def inputs(frame, seed, device='cpu', dtype=torch.float32):
    from mmlf_amd import dl
    B, H, W = frame
    stacks, gt, mask = synth.synth_inputs(B, H, seed=seed, ps_w=W)
    gt = torch.from_numpy(gt)
    cls = dl.reg_to_class(gt, -3.5, 3.5, 108)
    return ([torch.from_numpy(s).to(device, dtype) for s in stacks], gt.to(device, dtype), torch.from_numpy(mask).to(device),
            cls.to(device, dtype))


def run(m, variant, stacks, gt, mask, cls, scale=1.0, want=(True,) * 4):
    """one forward and one backward of loss * scale; returns (output dict, the four input gradients or None)"""
    xs = [s.clone().requires_grad_(w) for s, w in zip(stacks, want)]
    out = m(*xs)
    (loss_of(variant, out, gt, mask, cls) * scale).backward()
    return out, [x.grad for x in xs]


def bar(ref):
    """the project's gradient bar per tensor (tests/test_gpu_model.py, test_gpu_nobn.py, test_gpu_ksize3.py)"""
    return 5e-4 * float(ref.abs().max()) + 5e-7


def ratio(got, ref):
    return float((got.double().cpu() - ref).abs().max()) / bar(ref)


@functools.lru_cache(maxsize=None)
def reference(kind, variant, frame, eval_mode=False):
    """(kw, state, seed, scale, [four float64 input gradients of loss * scale], worst ratio to the bar of the float32 stock
    run): computed once per case and shared.  scale: the power of two that lifts every stack's max |gradient| to
    GRAD_FLOOR -- exact in every precision, so the float64 gradients are taken at scale 1 and multiplied."""
    seed = seed_of(kind, variant, frame, eval_mode)
    kw = kind_kw(kind, variant)
    state = kind_state(kind, kw, seed)
    res = {}
    for dt in (torch.float64, torch.float32):
        m = build(kw, state, dtype=dt)
        m.train(not eval_mode)
        res[dt] = run(m, variant, *inputs(frame, seed, dtype=dt))[1]
    smallest = min(float(g.abs().max()) for g in res[torch.float64])
    assert smallest > 0
    scale = 2.0 ** max(0, math.ceil(math.log2(GRAD_FLOOR / smallest)))
    ref = [g * scale for g in res[torch.float64]]
    assert min(float(g.abs().max()) for g in ref) >= GRAD_FLOOR
    cond = max(ratio(g * scale, r) for g, r in zip(res[torch.float32], ref))
    return kw, state, seed, scale, ref, cond


# ------------------------------------------------------------------------------------------------ conditioning
@pytest.mark.parametrize('frame', FRAMES)
@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('kind', KINDS)
def test_train_mode_cases_are_well_conditioned(kind, variant, frame):
    """the float32 stock run stays within a tenth of the bar of the float64 one: what the GPU test measures is the kernels"""
    _, _, seed, scale, ref, cond = reference(kind, variant, frame)
    print(f'{kind} {variant} {frame} seed {seed}: loss x {scale:g}, float32 stock run at {cond:.2e} of the bar')
    assert cond <= 0.1, cond
    assert all(tuple(g.shape) == (frame[0], 9, 3, frame[1], frame[2]) for g in ref)


@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('kind', KINDS)
def test_eval_mode_cases_are_well_conditioned(kind, variant):
    frame = EVAL_FRAMES[kind]
    _, _, seed, scale, ref, cond = reference(kind, variant, frame, True)
    print(f'eval {kind} {variant} {frame} seed {seed}: loss x {scale:g}, float32 stock run at {cond:.2e} of the bar')
    assert cond <= 0.1, cond
    if kind != 'nobn2':
        assert scale >= 2 ** 8           # eval-mode input gradients of the BatchNorm nets sit far below the floor unscaled


# ------------------------------------------------------------------------------------------------ the dx launch's extents
# the data gradient K -> N of tests/test_gpu_input_grad.py's kernel test, on the frames of that test
DGRAD_SHAPES = [(70, 27), (8, 27), (72, 27), (70, 9), (2, 3)]
DGRAD_FRAMES = [(1, 1, 1), (3, 5, 29), (1, 7, 130), (1, 2, 382)]
K3_DGRAD_SHAPES = [(70, 27), (8, 27)]


def cs_of(c):
    return (c + 7) // 8 * 8


@pytest.mark.parametrize('B,H,W', DGRAD_FRAMES)
def test_input_gradient_launch_stays_inside_what_the_size_queries_allocate(B, H, W):
    """mmlf_audit_conv_h2 for the launch Trunk.backward makes for a wanted stream: the gradient of conv1's output (cs_of(K))
    into a grid tensor of stride cs_of(N), whole rows stored, out_shift = P + 1, no ReLU reference"""
    from mmlf_amd import _lib
    L = _lib.load()
    P = W + L.mmlf_grid_pad_w()
    alloc, amax = L.mmlf_grid_alloc_positions(B, H, W), L.mmlf_amax_entries(B, H, W) * 4
    for K, N in DGRAD_SHAPES:
        cs_in, cs_out = cs_of(K), cs_of(N)
        e = (ctypes.c_int64 * 9)()
        assert L.mmlf_audit_conv_h2(cs_in, K, N, cs_out, cs_out, P + 1, 0, B, H, W, e) == 0, _lib.last_error()
        tag = f'{K}->{N} B={B} {H}x{W}'
        assert 0 < e[0] <= alloc * cs_in * 4, tag                                   # in
        assert 0 < e[1] <= L.mmlf_packed_filter_h2_bytes(cs_in, N), tag             # packed
        assert 0 < e[3] <= alloc * cs_out * 4, tag                                  # out
        assert e[3] >= (((B - 1) * (H + 2) + H) * P + W) * cs_out * 4 + N * 4, tag  # ... reaches the last interior position
        assert 0 < e[5] <= amax and 0 < e[6] <= amax, tag                           # in_amax, out_amax


@pytest.mark.parametrize('B,H,W', DGRAD_FRAMES)
def test_input_gradient_launch_of_the_3x3_trunk_stays_inside_its_allocations(B, H, W):
    from mmlf_amd import _lib
    L = _lib.load()
    P = W + L.mmlf_grid_pad_w()
    alloc = L.mmlf_grid_alloc_positions_k3(B, H, W)
    for K, N in K3_DGRAD_SHAPES:
        cs_in, cs_out = cs_of(K), cs_of(N)
        e = (ctypes.c_int64 * 5)()
        assert L.mmlf_audit_conv3x3(cs_in, K, N, cs_out, cs_out, 0, B, H, W, e) == 0, _lib.last_error()
        tag = f'3x3 {K}->{N} B={B} {H}x{W}'
        assert 0 < e[0] <= alloc * cs_in * 4, tag
        assert 0 < e[1] <= L.mmlf_packed_filter3x3_floats(cs_in, N) * 4, tag
        assert 0 < e[3] <= alloc * cs_out * 4, tag
        assert e[3] >= (((B - 1) * (H + 2) + H) * P + W) * cs_out * 4 + N * 4, tag


# ------------------------------------------------------------------------------------------------ defaults, CPU path
def test_engine_defaults_ask_for_no_input_gradient():
    from mmlf_amd.engine import Trunk
    sig = inspect.signature(Trunk.backward).parameters
    assert sig['input_grads'].default is None and list(sig)[:6] == ['self', 'p', 'tape', 'grad_output', 'grads', 'on_done']
    sig = inspect.signature(Trunk.forward).parameters
    assert sig['input_grads'].default is None and sig['frozen'].default is False
    assert list(sig)[:6] == ['self', 'p', 'stacks', 'train', 'save', 'packed']
    # a trunk without BatchNorm on 3x3 filters still has no native form: frozen evaluation does not make one
    with pytest.raises(ValueError, match='2x2'):
        Trunk(8, 2, 3, 9, 1, 0.1, ksize=3, batchnorm=False)


@pytest.mark.parametrize('kind', KINDS)
def test_cpu_tensors_take_the_stock_path_unchanged(kind, monkeypatch):
    """on CPU tensors nothing native runs, with or without input gradients, frozen or not; asking for input gradients does
    not change a bit of the outputs or of the parameter gradients"""
    from mmlf_amd import feed_forward

    def refuse(*a, **k):
        raise AssertionError('the native node on CPU tensors')
    monkeypatch.setattr(feed_forward._TrunkFn, 'apply', refuse)
    variant, frame = 'upr', (2, 9, 13)
    kw = kind_kw(kind, variant)
    state = kind_state(kind, kw, 0)
    data = inputs(frame, 0)
    runs = []
    for want in ((False,) * 4, (True,) * 4, (False, True, False, False)):
        m = build(kw, state)
        out, dx = run(m, variant, *data, want=want)
        assert [g is not None for g in dx] == list(want)
        runs.append((out, {n: p.grad for n, p in m.named_parameters()}, m.state_dict()))
    for out, grads, sd in runs[1:]:
        for k, v in runs[0][0].items():
            assert (v is None and out[k] is None) or torch.equal(v, out[k]), k
        for n, g in runs[0][1].items():
            assert torch.equal(g, grads[n]), n
        for k, v in runs[0][2].items():
            assert torch.equal(v, sd[k]), k
    # frozen: only the inputs are differentiated
    m = build(kw, state)
    for p in m.parameters():
        p.requires_grad_(False)
    _, dx = run(m, variant, *data)
    assert all(p.grad is None for p in m.parameters())
    ref = reference(kind, variant, frame)
    for g, r in zip(dx, ref[4]):
        assert ratio(g * ref[3], r) <= 0.1
