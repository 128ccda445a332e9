"""Multimodal evaluation on the device: the kernels of libmmlf_eval_hip.so (include/mmlf_eval_hip.h) against the CPU path of
mmlf_amd/multimodal.py, which tests/test_multimodal_cpu.py holds to pixel-loop restatements of the reference's scripts
(validate/cluster.py, utils/modecnt.py, validate/multimodal.py).

Both paths run the same IEEE operations in the same order, so integer outputs must be equal, float64 outputs agree to
1e-12 relative (the error sums differ in their order of addition only) and the float32 mode proportion to 1 ulp.  The
inputs (tests/multimodal_refs.py) keep every decision off a rounding: gt on a grid of 1/8, smoothed bins at least 1e-4
apart; test_multimodal_cpu.py checks that on the CPU.  No pixel is excluded from any comparison."""
import numpy as np
import pytest
import torch

import multimodal_refs as refs
from conftest import TINY_KW
from mmlf_amd import multimodal, synth
from mmlf_amd.feed_forward import FeedForward

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _smooth_np(post):
    return multimodal.smooth_bins(torch.from_numpy(post)).numpy()


def close64(got, want):
    np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=1e-12, atol=0)


def within_one_ulp(got, want):
    got, want = got.cpu().numpy(), want.numpy()
    assert got.dtype == want.dtype == np.float32
    finite = np.isfinite(want)
    np.testing.assert_array_equal(got[~finite], want[~finite])
    assert (got[finite] >= 0).all() and (want[finite] >= 0).all()       # (non-negative floats order like their bit patterns)
    ulps = np.abs(got[finite].view(np.int32).astype(np.int64) - want[finite].view(np.int32).astype(np.int64))
    assert ulps.max(initial=0) <= 1, ulps.max()


@pytest.mark.parametrize('radius', [2.0, 4.0])
@pytest.mark.parametrize('frame', refs.FRAMES)
def test_gt_modes_device_vs_cpu(frame, radius):
    gt = torch.from_numpy(refs.make_gt(2, *frame, seed=3))            # two different images: nothing leaks across the batch
    want_m, want_e = multimodal.gt_modes(gt, radius=radius, return_edges=True)
    got_m, got_e = multimodal.gt_modes(gt.to(DEV), radius=radius, return_edges=True)
    assert got_e.dtype == torch.int32 and got_m.dtype == torch.float64 and got_m.shape == (2, *frame, 2)
    assert torch.equal(got_e.cpu(), want_e)
    close64(got_m, want_m)
    if frame[0] * frame[1] >= 35:
        assert 0 < int(want_e.sum()) < want_e.numel()                  # edge and non-edge pixels both


def test_gt_modes_device_ties_and_equal_neighbourhoods():
    modes = multimodal.gt_modes(torch.tensor([[[0.0, 1.0, 2.0]]], device=DEV), radius=1.0)
    assert modes[0, 0, 1].tolist() == [0.0, 1.25]                      # two splits cost 0.75: the lowest index wins
    flat = torch.full((1, 4, 5), 0.1, device=DEV)
    modes, edges = multimodal.gt_modes(flat, edge_threshold=-1.0, return_edges=True)
    assert int(edges.sum()) == 20 and torch.equal(modes, flat.double().unsqueeze(-1).expand(1, 4, 5, 2))
    with pytest.raises(RuntimeError):
        from mmlf_amd import _lib
        out = torch.empty(1, 4, 5, 2, dtype=torch.float64, device=DEV)
        _lib.call_eval('mmlf_eval_gt_modes', flat.data_ptr(), out.data_ptr(), edges.data_ptr(), 1, 4, 5, 4.5, 0.5, None)


@pytest.mark.parametrize('frame,s', refs.POSTERIOR_CASES)
def test_posterior_modes_device_vs_cpu(frame, s):
    post = torch.from_numpy(refs.make_posterior(2, s, *frame, seed=100 + s, smooth=_smooth_np))
    want = multimodal.posterior_analysis(post, -3.5, 3.5)
    got = multimodal.posterior_analysis(post.to(DEV), -3.5, 3.5)
    assert [t.dtype for t in got] == [torch.int32, torch.float64, torch.int32, torch.float32]
    assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[2].cpu(), want[2])
    close64(got[1], want[1])
    within_one_ulp(got[3], want[3])
    # the two public functions are the two halves of the same launch
    a = multimodal.posterior_modes(post.to(DEV), -3.5, 3.5)
    b = multimodal.mode_proportion(post.to(DEV))
    assert torch.equal(a[0], got[0]) and torch.equal(a[1], got[1]) and torch.equal(b[0], got[2]) and torch.equal(b[1], got[3])


def test_posterior_modes_device_fills_and_inf():
    ramp = np.linspace(0.1, 1.0, 9, dtype=np.float32)
    one = np.array([.1, .2, .9, .2, .1, .1, .1, .1, .1], np.float32)
    flat = np.full(9, 0.5, np.float32)
    two = np.array([.1, .5, .1, .1, .5, .1, .7, .1, .1], np.float32)
    post = torch.from_numpy(np.stack([ramp, one, flat, two], -1).reshape(1, 9, 1, 4)).to(DEV)
    n_modes, disp = multimodal.posterior_modes(post, -4.0, 4.0)
    assert n_modes[0, 0].tolist() == [0, 1, 0, 2]
    assert disp[0, 0].tolist() == [[4.0, 4.0], [-2.0, -2.0], [-4.0, -4.0], [-3.0, 2.0]]
    gap = torch.from_numpy(refs.zero_gap_posterior())
    want = multimodal.mode_proportion(gap)
    got = multimodal.mode_proportion(gap.to(DEV))
    assert got[0][0, 0].tolist() == [1, 1] and got[1][0, 0, 0].item() == float('inf')      # a zero minimum between two maxima
    within_one_ulp(got[1], want[1])


def _scene(frame, s, seed):
    gt = torch.from_numpy(refs.make_gt(2, *frame, seed=seed))
    post = torch.from_numpy(refs.make_posterior(2, s, *frame, seed=seed + 1, smooth=_smooth_np))
    n_modes, disp = multimodal.posterior_modes(post, -3.5, 3.5)
    pred = gt + torch.from_numpy(np.random.RandomState(seed).uniform(-0.2, 0.2, gt.shape).astype(np.float32))
    return [disp, n_modes, multimodal.gt_modes(gt), gt, pred]


def _synthetic(frame, seed):
    """the same five tensors without a posterior behind them, for a frame too large to draw one for"""
    g = torch.Generator().manual_seed(seed)
    shape = (2, *frame)
    gt = torch.randint(-28, 29, shape, generator=g).float() / 8
    modes = torch.stack([gt.double(), gt.double() + (torch.rand(shape, generator=g) < 0.3).double()], -1)
    disp = torch.sort(torch.randint(0, 70, (*shape, 2), generator=g).double() / 69 * 7 - 3.5, -1)[0]
    n_modes = torch.randint(0, 3, shape, generator=g, dtype=torch.int32)
    pred = gt + (torch.rand(shape, generator=g) - 0.5) * 0.4
    return [disp, n_modes, modes, gt, pred]


TWO_MODE_SCENES = {}


def two_mode_scene(frame):
    if frame not in TWO_MODE_SCENES:                                  # built once, shared by the cases, never modified
        TWO_MODE_SCENES[frame] = _synthetic(frame, 9) if frame == (512, 512) else _scene(frame, 18, seed=21)
    return TWO_MODE_SCENES[frame]


@pytest.mark.parametrize('lb', [False, True])
@pytest.mark.parametrize('margin', [0, 2, 300])
@pytest.mark.parametrize('frame', [(1, 1), (5, 7), (33, 65), (3, 130), (512, 512)])
def test_two_mode_error_device_vs_cpu(frame, margin, lb):
    """(512, 512) x 2 is twice the 1024 workgroups the first stage launches at most: the grid-stride loop runs"""
    tensors = two_mode_scene(frame)
    want = multimodal.two_mode_error(*tensors, margin=margin, lb=lb)
    on_dev = [t.to(DEV) for t in tensors]
    got = multimodal.two_mode_error(*on_dev, margin=margin, lb=lb)
    again = multimodal.two_mode_error(*on_dev, margin=margin, lb=lb)
    assert torch.equal(got, again)                                     # fixed-order sums: the same bits
    assert got[0].item() == want[0].item() and got[5].item() == want[5].item()      # the counts are equal
    close64(got, want)
    if 2 * margin >= min(frame):
        assert got.tolist() == [0.0] * 6                               # a count of 0 is a result
    elif frame[0] * frame[1] >= 35:
        assert got[0].item() > 0


def test_validate_scenes_multimodal_on_the_device(tmp_path):
    from mmlf_amd import validate
    kw = dict(TINY_KW, model_uncert=True)
    model = FeedForward(**kw)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_state(synth.param_spec(**kw), 4).items()})
    model.cuda().eval()
    scenes = [tuple(torch.from_numpy(np.asarray(a)).unsqueeze(0).cuda() for a in synth.synth_scene(k, 24, 24)[:8])
              + (torch.tensor([[k]]),) for k in range(2)]
    rows, avg = validate.validate_scenes(model, scenes, margin=4, out_dir=str(tmp_path), scene_names=['s0', 's1'], multimodal=True)
    assert 'libmmlf_eval_hip.so' in open('/proc/self/maps').read()
    cnt = sum(r['mm_cnt'] for r in rows)
    assert cnt > 0 and avg['mm_mse'] == sum(r['mm_mse_sum'] for r in rows) / cnt and np.isfinite(avg['um_mse'])
    # the row of scene 1 is what the CPU path makes of the same device outputs
    with torch.no_grad():
        out = model(*scenes[1][:4])
    gt = scenes[1][5].float().cpu()
    n_modes, disp, mode_cnt, prop = multimodal.posterior_analysis(out['posterior'].cpu(), model.disp_min, model.disp_max)
    want = multimodal.two_mode_error(disp, n_modes, multimodal.gt_modes(gt), gt, out['mean'].cpu(), margin=4)
    np.testing.assert_allclose([rows[1][k] for k in multimodal.TWO_MODE_FIELDS], want.numpy(), rtol=1e-12)
    assert rows[1]['mode_cnt_share'] == float(mode_cnt.double().mean())
    assert np.load(str(tmp_path / 'scenes' / 's1' / 'gt_modes.npy')).shape == (24, 24, 2)
