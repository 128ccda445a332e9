"""The pointer checks (mmlf_amd/_lib.py check) on real device tensors.  The negative cases run with `_lib.load` replaced by a
stub that raises: a missing or late guard fails with its AssertionError and launches nothing, so no known-bad tensor can
reach a kernel.  The positive cases hold what was accepted before the checks to the same bits."""
import numpy as np
import pytest
import torch

from conftest import TINY_KW

pytestmark = pytest.mark.gpu

B, H, W = 2, 7, 5


def _dev():
    return torch.device('cuda:0')


def _model(dev, **kw):
    from mmlf_amd import synth
    from mmlf_amd.feed_forward import FeedForward
    kw = dict(TINY_KW, **kw)
    model = FeedForward(**kw)
    state = synth.synth_state(synth.param_spec(**kw), seed=5)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    return model.to(dev)


def _stacks(dev, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand((B, 9, 3, H, W), generator=g).to(dev) for _ in range(4)]


def _same_values_other_strides(t):
    """a permuted-and-back view: the shape and values of t, not contiguous"""
    nc = t.transpose(-1, -2).contiguous().transpose(-1, -2)
    assert not nc.is_contiguous() and torch.equal(nc, t)
    return nc


@pytest.fixture
def no_library(monkeypatch):
    from mmlf_amd import _lib

    def stub():
        raise AssertionError('reached the library')
    monkeypatch.setattr(_lib, 'load', stub)


# ------------------------------------------------------------------ negative: nothing reaches the library
def test_cpu_model_with_device_stacks_through_the_module(no_library):
    model = _model('cpu').eval()
    with torch.no_grad(), pytest.raises(ValueError, match=r'in_net_hv\.0\.0\.weight'):
        model(*_stacks(_dev()))


def test_channels_last_model_through_the_module(no_library):
    model = _model(_dev()).to(memory_format=torch.channels_last).eval()
    with torch.no_grad(), pytest.raises(ValueError, match=r'\.weight.*contiguous'):
        model(*_stacks(_dev()))


def _step_args(dev):
    return _stacks(dev) + [torch.zeros((B, H, W), device=dev), torch.ones((B, H, W), dtype=torch.int32, device=dev), 1]


def test_cpu_model_with_device_stacks_through_the_train_step(no_library):
    from mmlf_amd.train import TrainStep
    step = TrainStep(_model('cpu'), lr=1e-3, loss_margin=1)
    with pytest.raises(ValueError, match=r'in_net_hv\.0\.0\.weight'):
        step(*_step_args(_dev()))


def test_transposed_stack_through_the_train_step(no_library):
    from mmlf_amd.train import TrainStep
    dev = _dev()
    step = TrainStep(_model(dev), lr=1e-3, loss_margin=1)
    args = _step_args(dev)
    args[1] = _same_values_other_strides(args[1])
    with pytest.raises(ValueError, match='v_views'):
        step(*args)


def test_cpu_model_with_device_stacks_through_the_fused_ensemble(no_library):
    from mmlf_amd.ensamble import Ensamble, _fused_members
    model = _model('cpu', model_uncert=True).eval()
    ens = Ensamble(model, -3.5, 3.5, 1.0).eval()
    assert len(ens.members()) == 7
    with torch.no_grad():
        assert _fused_members(model, model, 9, 3)
        with pytest.raises(ValueError, match=r'in_net_hv\.0\.0\.weight'):
            ens(*_stacks(_dev()))


def test_dpp_head_on_two_channel_scores(no_library):
    """model_uncert with model_discrete: two output channels, and the head kernel would write 108 into buffers of two"""
    from mmlf_amd.feed_forward import _HeadDppFn
    dev = _dev()
    model = _model('cpu', model_uncert=True, model_discrete=True)
    assert model.out_chs == 2 and model.steps == 108
    with pytest.raises(RuntimeError, match='108'):
        _HeadDppFn.apply(torch.zeros((B, 2, H, W), device=dev), model._grid('torch', dev), model._grid('np', dev), model.steps)


# ------------------------------------------------------------------ positive: accepted as before, the same bits
def test_ensemble_takes_non_contiguous_stacks():
    from mmlf_amd.ensamble import Ensamble
    dev = _dev()
    ens = Ensamble(_model(dev, model_uncert=True).eval(), -3.5, 3.5, 1.0).eval()
    assert len(ens.members()) == 7
    stacks = _stacks(dev)
    with torch.no_grad():
        ref = {k: v.clone() for k, v in ens(*stacks).items()}
        got = ens(_same_values_other_strides(stacks[0]), *stacks[1:])
    for k in ref:
        assert torch.equal(got[k], ref[k]), k
    assert torch.isfinite(ref['mean']).all()


def test_native_loss_converts_mask_and_target():
    from mmlf_amd import loss
    dev = _dev()
    g = torch.Generator().manual_seed(11)
    out = torch.randn((B, 2, H, W), generator=g).to(dev)
    gt = torch.randn((B, H, W), generator=g).to(dev)
    mask = (torch.rand((B, H, W), generator=g) > 0.3).to(dev)
    ref_loss, ref_grad = loss.native_loss(loss.KIND_UPR, out, gt, mask.to(torch.int32))
    got_loss, got_grad = loss.native_loss(loss.KIND_UPR, out, gt.double(), mask)
    assert torch.equal(got_loss, ref_loss) and torch.equal(got_grad, ref_grad)
    assert torch.isfinite(ref_loss) and bool(ref_grad.abs().sum() > 0)


def test_trunk_backward_takes_a_non_contiguous_grad_output():
    dev = _dev()
    model = _model(dev).train()
    p = {n: t.detach() for n, t in model._tensor_dict().items()}
    stacks = _stacks(dev)
    gout = torch.randn((B, 1, H, W), generator=torch.Generator().manual_seed(17)).to(dev)
    res = []
    with torch.no_grad():
        for go in (gout, _same_values_other_strides(gout)):
            _, tape = model._trunk.forward(p, stacks, True, True)
            grads = {n: torch.zeros_like(p[n]) for n in model._param_names}
            model._trunk.backward(p, tape, go, grads)
            res.append(grads)
    for n in res[0]:
        assert torch.equal(res[0][n], res[1][n]), n
    assert bool(res[0]['out_net.2.2.weight'].abs().sum() > 0) and bool(res[0]['in_net_hv.0.0.weight'].abs().sum() > 0)
