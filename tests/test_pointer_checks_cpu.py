"""A tensor is validated where its pointer is taken (mmlf_amd/_lib.py check): bad input never reaches the library.  No GPU
and no library here: `_lib.load` is replaced by a stub that raises, so a missing or late guard fails with its AssertionError
and launches nothing; `meta` tensors stand for "another device"."""
import pytest
import torch

from conftest import TINY_KW

B, H, W = 2, 7, 5
CPU = torch.device('cpu')


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    from mmlf_amd import _lib

    def stub():
        raise AssertionError('reached the library')
    monkeypatch.setattr(_lib, 'load', stub)
    monkeypatch.setattr(_lib, 'stream_ptr', lambda: 0)          # (an argument of every launch; there is no GPU to ask)


def _model(**kw):
    from mmlf_amd.feed_forward import FeedForward
    torch.manual_seed(0)
    return FeedForward(**dict(TINY_KW, **kw)).eval()


def _params(model):
    return {n: t.detach() for n, t in model._tensor_dict().items()}


def _stacks(**kw):
    return [torch.zeros(B, 9, 3, H, W, **kw) for _ in range(4)]


# ------------------------------------------------------------------ the check itself
@pytest.mark.parametrize('tensor, kw', [
    (torch.zeros(4, device='meta'), {}),                                        # another device
    (torch.zeros(4, dtype=torch.float64), {}),                                  # another dtype
    (torch.zeros(4), {'shape': (2, 2)}),                                        # another shape
    (torch.zeros(4), {'numel': 5}),
    (torch.zeros(4), {'min_numel': 5}),                                         # too few elements
    (torch.zeros(2, 3).t(), {}),                                                # not contiguous
    (None, {}),
])
def test_check_rejects(tensor, kw):
    from mmlf_amd._lib import check
    with pytest.raises(ValueError, match='the_argument'):
        check(tensor, 'the_argument', CPU, **kw)


def test_check_accepts():
    from mmlf_amd._lib import check
    check(torch.zeros(2, 3), 'x', CPU, shape=(2, 3), numel=6, min_numel=6)
    check(torch.zeros(2, 3).t(), 'x', CPU, contiguous=False)
    check(torch.zeros(3, dtype=torch.bool), 'x', CPU, None, numel=3)
    check(torch.zeros(3, dtype=torch.int64, device='meta'), 'x', torch.device('meta'), torch.int64, min_numel=1)


# ------------------------------------------------------------------ Trunk.forward
def _bad_stack(how):
    stacks = _stacks()
    if how == 'transposed':
        stacks[1] = torch.zeros(B, 9, 3, W, H).transpose(3, 4)
    elif how == 'float64':
        stacks[2] = stacks[2].double()
    elif how == 'shape':
        stacks[3] = torch.zeros(B, 9, 3, H, W + 1)
    elif how == 'meta':
        stacks[1] = stacks[1].to('meta')
    elif how == 'views':
        stacks = [torch.zeros(B, 7, 3, H, W) for _ in range(4)]
    elif how == 'none':
        stacks[2] = None
    return stacks


@pytest.mark.parametrize('how', ['transposed', 'float64', 'shape', 'meta', 'views', 'none'])
def test_trunk_forward_rejects_stacks(how):
    model = _model()
    with pytest.raises(ValueError, match='views|stacks'):
        model._trunk.forward(_params(model), _bad_stack(how), False, False)


def test_trunk_forward_rejects_parameters_of_another_device():
    model = _model().to('meta')
    with pytest.raises(ValueError, match=r'in_net_hv\.0\.0\.weight'):
        model._trunk.forward(_params(model), _stacks(), False, False)


def test_trunk_forward_rejects_channels_last_model():
    model = _model().to(memory_format=torch.channels_last)
    assert not model.in_net_hv[0][0].weight.is_contiguous()
    with pytest.raises(ValueError, match=r'\.weight.*contiguous'):
        model._trunk.forward(_params(model), _stacks(), False, False)


@pytest.mark.parametrize('name', ['out_net.2.2.bias', 'in_net_id.1.3.running_var', 'out_net.0.3.num_batches_tracked'])
def test_trunk_forward_rejects_missing_parameter(name):
    model = _model()
    p = _params(model)
    del p[name]
    with pytest.raises(ValueError, match=name.replace('.', r'\.')):
        model._trunk.forward(p, _stacks(), False, False)


def test_trunk_forward_rejects_parameter_of_another_size_or_dtype():
    model = _model()
    p = _params(model)
    with pytest.raises(ValueError, match=r'in_net_id\.0\.0\.weight'):
        model._trunk.forward(dict(p, **{'in_net_id.0.0.weight': torch.zeros(8, 26, 2, 2)}), _stacks(), False, False)
    with pytest.raises(ValueError, match=r'out_net\.1\.3\.weight'):
        model._trunk.forward(dict(p, **{'out_net.1.3.weight': p['out_net.1.3.weight'].double()}), _stacks(), False, False)
    with pytest.raises(ValueError, match='num_batches_tracked'):
        model._trunk.forward(dict(p, **{'in_net_hv.0.3.num_batches_tracked': torch.zeros((), dtype=torch.int32)}), _stacks(),
                             False, False)


def _geo(ksize=2, alloc=200):
    """a Geometry made without the library: the fields validation reads, and what buf() needs to reach its first launch"""
    from mmlf_amd.engine import Geometry
    geo = object.__new__(Geometry)
    geo.__dict__.update(B=B, H=H, W=W, ksize=ksize, alloc=alloc, amax_n=8)
    return geo


def test_trunk_forward_rejects_packed_input():
    from mmlf_amd.engine import cs_of
    model = _model()
    p, geo = _params(model), _geo()
    need = geo.alloc * cs_of(27)
    good = [torch.zeros(need) for _ in range(4)]
    with pytest.raises(ValueError, match=r'packed\[2\]'):
        model._trunk.forward(p, None, False, False, packed=(geo, good[:2] + [torch.zeros(need - 1)] + good[3:]))
    with pytest.raises(ValueError, match=r'packed\[3\]'):
        model._trunk.forward(p, None, False, False, packed=(geo, good[:3] + [torch.zeros(need, device='meta')]))
    with pytest.raises(ValueError, match='ksize'):
        model._trunk.forward(p, None, False, False, packed=(_geo(ksize=3), good))


def test_trunk_forward_accepts_good_input():
    """well-formed input passes validation: the next thing either path does is to reach for the library"""
    model = _model()
    p = _params(model)
    with pytest.raises(AssertionError, match='reached the library'):
        model._trunk.forward(p, _stacks(), False, False)
    need = 200 * 32
    with pytest.raises(AssertionError, match='reached the library'):
        model._trunk.forward(p, None, False, False, packed=(_geo(), [torch.zeros(need + k) for k in range(4)]))


def test_a_validated_model_is_checked_again_when_a_tensor_changes():
    """the dictionary checks run once per (data_ptr, device) signature: a tensor of other storage is looked at again"""
    model = _model()
    p = _params(model)
    for _ in range(2):
        with pytest.raises(AssertionError, match='reached the library'):
            model._trunk.forward(p, _stacks(), False, False)
    name = 'out_net.0.2.weight'
    for bad in (p[name].double(), p[name].to(memory_format=torch.channels_last), p[name].to('meta'), None):
        with pytest.raises(ValueError, match=name.replace('.', r'\.')):
            model._trunk.forward(dict(p, **{name: bad}), _stacks(), False, False)
    with pytest.raises(ValueError, match='parameters'):               # the same tensors, asked for on another device
        model._trunk.forward(p, _stacks(device='meta'), False, False)
    grads = {n: torch.zeros_like(p[n]) for n in model._param_names}
    for _ in range(2):
        with pytest.raises(AssertionError, match='reached the library'):
            model._trunk.backward(p, _tape(), torch.zeros(B, 1, H, W), grads)
    with pytest.raises(ValueError, match=r'grads'):
        model._trunk.backward(p, _tape(), torch.zeros(B, 1, H, W), dict(grads, **{name: grads[name].double()}))


# ------------------------------------------------------------------ Trunk.backward
def _tape():
    from mmlf_amd.engine import _Tape
    return _Tape(_geo(), CPU)


@pytest.mark.parametrize('gout', [torch.zeros(B, 1, H, W + 1), torch.zeros(B, 2, H, W), torch.zeros(B, 1, H, W).double(),
                                  torch.zeros(B, 1, H, W, device='meta')])
def test_trunk_backward_rejects_grad_output(gout):
    model = _model()
    with pytest.raises(ValueError, match='grad_output'):
        model._trunk.backward(_params(model), _tape(), gout, None)


@pytest.mark.parametrize('how', ['size', 'missing', 'float64', 'meta', 'strided'])
def test_trunk_backward_rejects_grads(how):
    model = _model()
    p = _params(model)
    grads = {n: torch.zeros_like(p[n]) for n in model._param_names}
    name = 'out_net.1.2.weight'
    if how == 'missing':
        del grads[name]
    else:
        grads[name] = {'size': torch.zeros(32, 32, 2, 1), 'float64': grads[name].double(), 'meta': grads[name].to('meta'),
                       'strided': torch.zeros(32, 32, 2, 4)[..., ::2]}[how]
    with pytest.raises(ValueError, match=r"grads\['out_net\.1\.2\.weight'\]"):
        model._trunk.backward(p, _tape(), torch.zeros(B, 1, H, W), grads)


def test_trunk_backward_accepts_good_input():
    """a non-contiguous grad_output stays accepted (backward makes it contiguous), as do gradients of the parameters' sizes"""
    model = _model()
    p = _params(model)
    grads = {n: torch.zeros_like(p[n]) for n in model._param_names}
    with pytest.raises(AssertionError, match='reached the library'):
        model._trunk.backward(p, _tape(), torch.zeros(B, 1, W, H).transpose(2, 3), grads)
    with pytest.raises(AssertionError, match='reached the library'):
        model._trunk.backward(p, _tape(), torch.zeros(B, 1, H, W), None)


# ------------------------------------------------------------------ losses, metrics
def _loss_args():
    return torch.zeros(B, 2, H, W), torch.zeros(B, H, W), torch.ones(B, H, W, dtype=torch.bool)


def test_native_loss_rejects():
    from mmlf_amd import loss
    out, gt, mask = _loss_args()
    n = B * H * W
    with pytest.raises(ValueError, match='target'):
        loss.native_loss(loss.KIND_UPR, out, torch.zeros(n - 1), mask)
    for bad in (torch.ones(n - 1), torch.ones(B, H, W + 1), mask.to('meta')):
        with pytest.raises(ValueError, match='mask'):
            loss.native_loss(loss.KIND_UPR, out, gt, bad)
    with pytest.raises(ValueError, match='target'):
        loss.native_loss(loss.KIND_UPR, out, gt.to('meta'), mask)
    for bad in (torch.zeros(0, dtype=torch.float64), torch.zeros(1), torch.zeros(1, dtype=torch.float64, device='meta')):
        with pytest.raises(ValueError, match='den_override'):
            loss.native_loss(loss.KIND_UPR, out, gt, mask, den_override=bad)
    scores = torch.zeros(B, 108, H, W)
    for bad in (torch.zeros(107), torch.zeros(108).double(), torch.zeros(108, device='meta')):
        with pytest.raises(ValueError, match='grid'):
            loss.native_loss(loss.KIND_CE, scores, gt, mask, grid_torch=bad, half_step=0.03)


def test_native_multi_loss_rejects():
    from mmlf_amd import loss
    out, gt, mask = _loss_args()
    mpi = torch.zeros(B, 3, 5, H, W)
    n = B * H * W
    with pytest.raises(ValueError, match='mask'):
        loss.native_multi_loss(loss.KIND_MULTI_UPR, out, mpi, torch.ones(n + 1))
    with pytest.raises(ValueError, match='mask'):
        loss.native_multi_loss(loss.KIND_MULTI_UPR, out, mpi, mask.to('meta'))
    with pytest.raises(ValueError, match='target'):
        loss.native_multi_loss(loss.KIND_MULTI_UPR, out, mpi.to('meta'), mask)
    with pytest.raises(ValueError, match='target'):
        loss.native_multi_loss(loss.KIND_MULTI_UPR, out, torch.zeros(B, 3, 5, H, W - 1), mask)
    with pytest.raises(ValueError, match='mask_padding'):
        loss.native_multi_loss(loss.KIND_UPR_PADDED, out, gt, mask, torch.ones(n - 1))
    with pytest.raises(ValueError, match='den_override'):
        loss.native_multi_loss(loss.KIND_MULTI_UPR, out, mpi, mask, den_override=torch.zeros(0, dtype=torch.float64))
    for bad in (torch.zeros(1, dtype=torch.float64), torch.zeros(2)):
        with pytest.raises(ValueError, match='aux_override'):
            loss.native_multi_loss(loss.KIND_MULTI_UPR, out, mpi, mask, aux_override=bad)


def test_losses_accept_good_input():
    """what callers pass today gets past validation: a bool mask, a float64 target, (B, H, W) or flat"""
    from mmlf_amd import loss
    out, gt, mask = _loss_args()
    den = torch.ones(1, dtype=torch.float64)
    with pytest.raises(AssertionError, match='reached the library'):
        loss.native_loss(loss.KIND_UPR, out, gt.double().reshape(-1), mask, den_override=den)
    with pytest.raises(AssertionError, match='reached the library'):
        loss.native_multi_loss(loss.KIND_UPR_PADDED, out, gt, mask.int(), mask, den_override=den,
                               aux_override=torch.ones(2, dtype=torch.float64))


def test_lmm_rejects_logvars():
    from mmlf_amd import metrics
    means = torch.zeros(3, B, H, W)
    for bad in (torch.zeros(3, B, H, W - 1), torch.zeros(2, B, H, W), torch.zeros(3, B, H, W, device='meta')):
        with pytest.raises(ValueError, match='logvars'):
            metrics._lmm_hip(8, -1.0, 1.0, means, bad)
    with pytest.raises(AssertionError, match='reached the library'):
        metrics._lmm_hip(8, -1.0, 1.0, means, torch.zeros(3, B, W, H).transpose(2, 3).double())


# ------------------------------------------------------------------ heads, ensemble
def test_dpp_head_rejects_two_channel_scores():
    """model_uncert with model_discrete: the trunk has two output channels and the head kernel would write 108"""
    from mmlf_amd.feed_forward import _HeadDppFn
    model = _model(model_uncert=True, model_discrete=True)
    assert model.out_chs == 2 and model.steps == 108
    grid = torch.zeros(108)
    with pytest.raises(RuntimeError, match='108'):
        _HeadDppFn.apply(torch.zeros(B, 2, H, W), grid, grid, 108)
    with pytest.raises(AssertionError, match='reached the library'):
        _HeadDppFn.apply(torch.zeros(B, 108, H, W), grid, grid, 108)


def test_upr_head_rejects_one_channel_output():
    from mmlf_amd.feed_forward import _HeadUprFn
    with pytest.raises(ValueError, match='UPR head'):
        _HeadUprFn.apply(torch.zeros(B, 1, H, W), torch.zeros(108), 108)


def test_fused_member_path_is_not_for_the_dpp_head():
    from mmlf_amd.ensamble import _fused_members
    with torch.no_grad():
        upr = _model(model_uncert=True)
        assert _fused_members(upr, upr, 9, 3) is True
        both = _model(model_uncert=True, model_discrete=True)
        assert _fused_members(both, both, 9, 3) is False
        assert _fused_members(upr, upr, 7, 3) is False
        assert _fused_members(torch.nn.DataParallel(upr), upr, 9, 3) is False
    assert _fused_members(upr, upr, 9, 3) is False                     # under autograd
