"""Ensamble / Shift: CPU plumbing path and (gpu-marked) HIP path against the reference goldens."""
import numpy as np
import pytest
import torch

from conftest import TINY_KW, load_golden
from mmlf_amd.ensamble import Ensamble, shift_table, shift_views_torch
from mmlf_amd.feed_forward import FeedForward

DISPS = (-3.5, -0.3, 0.0, 0.3, 2.5, 1.0)


def _model(g, dev='cpu'):
    m = FeedForward(**dict(TINY_KW, model_uncert=True))
    m.load_state_dict({k[len('state/'):]: torch.from_numpy(v) for k, v in g.items() if k.startswith('state/')})
    return m.to(dev)


def _check(out, g):
    np.testing.assert_allclose(out['means'].cpu().numpy(), g['means'], rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(out['logvars'].cpu().numpy(), g['logvars'], rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(out['posterior'].cpu().numpy(), g['posterior'], rtol=3e-3, atol=1e-6)
    assert (np.abs(out['logvar'].cpu().numpy() - g['logvar']) < 1e-4).mean() > 0.999
    assert (np.abs(out['mean'].cpu().numpy() - g['mean']) < 1e-4).mean() > 0.99
    assert set(out) == {'mean', 'logvar', 'means', 'logvars', 'posterior'}


def test_shift_torch_matches_reference():
    g = load_golden('g4_shift.npz')
    stacks = [torch.from_numpy(g[f'in{i}']) for i in range(4)]
    for d in DISPS:
        got = shift_views_torch(stacks, float(d))
        for i in range(4):
            np.testing.assert_allclose(got[i].numpy(), g[f'shift_{d}_{i}'], rtol=1e-6, atol=1e-7, err_msg=f'{d} {i}')


def test_shift_table_signed_zero():
    s, w = shift_table([-0.3, 0.3], 9)
    assert tuple(s[0, 5]) == (0, -1) and tuple(s[0, 3]) == (0, 1)      # -0.3*(+1) -> (-0.0, -1)
    assert tuple(s[1, 5]) == (0, 1) and tuple(s[1, 3]) == (0, -1)
    np.testing.assert_allclose(w[0, 5], (0.7, 0.3), rtol=1e-6)


def test_ensamble_cpu_matches_reference():
    g = load_golden('g4_ensamble.npz')
    ens = Ensamble(_model(g), -3.5, 3.5, 0.1)
    ens.eval()
    assert len(ens.members()) == 70
    with torch.no_grad():
        out = ens(*[torch.from_numpy(g[f'in{i}']) for i in range(4)])
    _check(out, g)


def test_two_stack_ensemble_raises_like_the_reference():
    """reference ensamble.py:40 declares i_views=None, d_views=None, but its loop hands Shift a 2-tuple (:63-64) and Shift
    reads data[2] / data[3] unconditionally (hci4d.py:927-928): measured in the build container, the reference raises
    `IndexError: list index out of range` before the first member.  Same exception type here, before any launch."""
    from mmlf_amd.ensamble import Ensamble

    class _Stub(torch.nn.Module):
        def forward(self, *a):
            raise AssertionError('the model must not be reached')

    ens = Ensamble(_Stub(), -3.5, 3.5, 0.1)
    with pytest.raises(IndexError):
        ens(torch.rand(1, 9, 3, 8, 8), torch.rand(1, 9, 3, 8, 8))


@pytest.mark.gpu
def test_shift_hip_matches_reference():
    from mmlf_amd import _lib
    from mmlf_amd._lib import call, ptr
    g = load_golden('g4_shift.npz')
    dev = torch.device('cuda:0')
    src = [torch.from_numpy(g[f'in{i}'][0]).to(dev) for i in range(4)]
    views, c, H, W = src[0].shape
    tab_s, tab_w = shift_table(DISPS, views)
    ts, tw = torch.from_numpy(tab_s).to(dev), torch.from_numpy(tab_w).to(dev)
    outs = [torch.empty((len(DISPS), views, c, H, W), device=dev) for _ in range(4)]
    call('mmlf_shift_views', *[ptr(t) for t in src], *[ptr(t) for t in outs], ptr(ts), ptr(tw), len(DISPS), views,
         H, W, _lib.stream_ptr())
    for k, d in enumerate(DISPS):
        for i in range(4):
            np.testing.assert_array_equal(outs[i][k].cpu().numpy(), g[f'shift_{d}_{i}'][0], err_msg=f'{d} {i}')


# The write-out of shift_pack_kernel walks (position, group of four channels) pairs of a piece of the row with a carry
# (csrc/row_walk.h).  9 views: cs = 32, 8 groups, 256 % 8 = 0 -- never a carry.  7 views: cs = 24, 6 groups, the walk moves on
# by (42, 4): at a pitch of 4 (frame (3, 2)) a thread is out of the row on its first step; at a pitch of 45 (frame (2, 43))
# threads carry in mid-row (x = 0 -> 43) and leave through the carry (x = 2 -> 44 -> 45).  tests/test_elementwise_cpu.py holds
# these lists to that.  One row (every vertical roll is the identity clamp) at a pitch of 302: three pieces of the 128-position
# tile; one column; one view (half = 0: nothing is sheared) and two (an even count: views at -1 and 0).  mmlf_shift_views, the
# other side of the comparison, is held to the oracle's bits at the same kinds of frame by tests/test_gpu_data_kernels.py.
SHIFT_PACK_VIEWS = (9, 7, 1, 2)
SHIFT_PACK_FRAMES = [(24, 24), (9, 40), (33, 17), (3, 2), (2, 43), (1, 300), (300, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize('views', SHIFT_PACK_VIEWS)
@pytest.mark.parametrize('shape', SHIFT_PACK_FRAMES)
def test_shift_pack_writes_the_same_bits_as_shift_then_pack(shape, views):
    """mmlf_shift_pack (round 6: the Ensamble's members sheared straight into the trunk's grid layout) against
    mmlf_shift_views followed by mmlf_pack_nchw, per stream kind: the same grid bytes (borders, pad channels and slack
    included) and the same amax array; the shifts are the golden's (hci4d.py:907-990 is pinned by test_shift_hip_matches_reference)."""
    from mmlf_amd import _lib, engine
    from mmlf_amd._lib import call, ptr
    dev = torch.device('cuda:0')
    H, W = shape
    gen = torch.Generator().manual_seed(H * 100 + W)
    src = [torch.rand((views, 3, H, W), generator=gen).to(dev) for _ in range(4)]
    disps = list(DISPS) + [float(W) + 0.5, -float(H) - 1.25]                 # incl. |shift| >= size: the roll's identity clamp
    S = len(disps)
    tab_s, tab_w = shift_table(disps, views)
    ts, tw = torch.from_numpy(tab_s).to(dev), torch.from_numpy(tab_w).to(dev)
    outs = [torch.empty((S, views, 3, H, W), device=dev) for _ in range(4)]
    call('mmlf_shift_views', *[ptr(t) for t in src], *[ptr(t) for t in outs], ptr(ts), ptr(tw), S, views, H, W, _lib.stream_ptr())
    geo = engine.Geometry(S, H, W)
    cs = engine.cs_of(views * 3)
    for kind in range(4):
        a, b = geo.buf(cs, dev), geo.buf(cs, dev)
        a.fill_(7.0); b.fill_(-3.0)                                        # whatever was there: every grid element must be written
        call('mmlf_zero_slack', ptr(a), cs, S, H, W, ptr(a.absmax), _lib.stream_ptr())
        call('mmlf_zero_slack', ptr(b), cs, S, H, W, ptr(b.absmax), _lib.stream_ptr())
        call('mmlf_pack_nchw', ptr(outs[kind]), views * 3, ptr(a), cs, S, H, W, ptr(a.absmax), _lib.stream_ptr())
        call('mmlf_shift_pack', ptr(src[kind]), kind, ptr(b), cs, ptr(ts), ptr(tw), S, views, H, W, ptr(b.absmax), _lib.stream_ptr())
        torch.cuda.synchronize()
        assert torch.equal(a, b), kind
        assert torch.equal(geo.amax_canonical(a.absmax), geo.amax_canonical(b.absmax)), kind


@pytest.mark.gpu
def test_ensamble_hip_matches_reference(monkeypatch):
    from mmlf_amd import ensamble
    g = load_golden('g4_ensamble.npz')
    dev = torch.device('cuda:0')
    ens = Ensamble(_model(g, dev), -3.5, 3.5, 0.1)
    ens.eval()
    assert ensamble.FUSED_MEMBERS
    with torch.no_grad():
        out = ens(*[torch.from_numpy(g[f'in{i}']).to(dev) for i in range(4)])
    _check(out, g)
    # the fused member path (shift straight into the grid layout, no member posterior) gives the bits of the module's own forward
    monkeypatch.setattr(ensamble, 'FUSED_MEMBERS', False)
    with torch.no_grad():
        plain = ens(*[torch.from_numpy(g[f'in{i}']).to(dev) for i in range(4)])
    for k in ('means', 'logvars', 'mean', 'logvar', 'posterior'):
        assert torch.equal(out[k], plain[k]), k
    monkeypatch.setattr(ensamble, 'FUSED_MEMBERS', True)
    # chunked members give the same result as one batch
    ens.member_budget_bytes = 1
    with torch.no_grad():
        out2 = ens(*[torch.from_numpy(g[f'in{i}']).to(dev) for i in range(4)])
    np.testing.assert_allclose(out2['means'].cpu().numpy(), out['means'].cpu().numpy(), rtol=1e-5, atol=1e-6)


@pytest.mark.gpu
def test_validate_scene_hip():
    from mmlf_amd.validate import validate_scene
    g = load_golden('g4_ensamble.npz')
    dev = torch.device('cuda:0')
    m = _model(g, dev)
    gt = torch.zeros((1, 24, 24), device=dev)
    out, mse, bad = validate_scene(m, *[torch.from_numpy(g[f'in{i}']).to(dev) for i in range(4)], gt, margin=3)
    ref = float(((out['mean'][0, 3:-3, 3:-3]) ** 2).mean())
    np.testing.assert_allclose(float(mse), ref, rtol=1e-5)
    assert 0.0 <= float(bad) <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize('views,b,H,W', [(7, 2, 20, 28), (11, 1, 31, 17), (3, 3, 16, 16)])
def test_fused_members_equal_the_modules_own_forward_on_other_shapes(views, b, H, W, monkeypatch):
    """the fused member path (mmlf_shift_pack + trunk on packed inputs) against mmlf_shift_views + the module's own forward for
    other view counts, batches above one and non-square frames: the same bits in every output of the Ensamble"""
    from mmlf_amd import ensamble, synth
    kw = dict(TINY_KW, model_views=views, model_uncert=True)
    m = FeedForward(**kw)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_state(synth.param_spec(**kw), 5).items()})
    dev = torch.device('cuda:0')
    ens = Ensamble(m.to(dev).eval(), -3.5, 3.5, 0.5).eval()
    g = torch.Generator().manual_seed(views)
    stacks = [torch.rand((b, views, 3, H, W), generator=g).to(dev) for _ in range(4)]
    res = {}
    for fused in (True, False):
        monkeypatch.setattr(ensamble, 'FUSED_MEMBERS', fused)
        with torch.no_grad():
            res[fused] = {k: v.clone() for k, v in ens(*stacks).items()}
    for k in res[True]:
        assert torch.equal(res[True][k], res[False][k]), k
    assert torch.isfinite(res[True]['mean']).all()
