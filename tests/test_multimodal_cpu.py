"""Multimodal evaluation (mmlf_amd/multimodal.py, include/mmlf_eval_hip.h), the part that needs no GPU: the package's CPU
path against pixel-loop restatements of the reference's scripts (tests/multimodal_refs.py: validate/cluster.py,
utils/modecnt.py, validate/multimodal.py, validate/sparsify.py, validate/mm_prediction.py) and against scipy where it is
installed; the definitions chosen where the scripts are arbitrary; `validate_scenes(multimodal=...)`; and the second
library: that it builds, exports exactly its header's entry points, leaves the training ABI alone and spills nothing."""
import ctypes
import itertools
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import multimodal_refs as refs
from conftest import TINY_KW
from mmlf_amd import _lib, multimodal, synth
from mmlf_amd.csrc import build
from mmlf_amd.feed_forward import FeedForward

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOOP_FRAMES = [f for f in refs.FRAMES if f[0] * f[1] <= 400]       # (the pixel loops take the small frames)


def _smooth_np(post):
    return multimodal.smooth_bins(torch.from_numpy(post)).numpy()


# ---------------------------------------------------------------- ground-truth modes

@pytest.mark.parametrize('frame', LOOP_FRAMES)
def test_gt_modes_vs_pixel_loop(frame):
    gt = refs.make_gt(2, *frame, seed=3)
    modes, edges = multimodal.gt_modes(torch.from_numpy(gt), return_edges=True)
    assert modes.dtype == torch.float64 and edges.dtype == torch.int32
    for b in range(2):                                            # (per image: nothing leaks across the batch)
        m_ref, e_ref = refs.gt_modes_ref(gt[b])
        np.testing.assert_array_equal(edges[b].numpy(), e_ref.astype(np.int32))
        np.testing.assert_allclose(modes[b].numpy(), m_ref, rtol=1e-14, atol=0)
    if frame[0] * frame[1] >= 35:
        assert 0 < int(edges.sum()) < edges.numel()                # both branches ran


@pytest.mark.parametrize('radius', [1.0, 2.5, 4.0])
def test_gt_modes_other_radii_vs_pixel_loop(radius):
    gt = refs.make_gt(1, 6, 9, seed=5)
    modes = multimodal.gt_modes(torch.from_numpy(gt), radius=radius, edge_threshold=0.25)
    np.testing.assert_allclose(modes[0].numpy(), refs.gt_modes_ref(gt[0], radius, 0.25)[0], rtol=1e-14, atol=0)
    assert len(multimodal.disc_offsets(4.0)) == 49
    with pytest.raises(ValueError):
        multimodal.gt_modes(torch.from_numpy(gt), radius=4.5)


def test_sobel_vs_scipy():
    ndimage = pytest.importorskip('scipy.ndimage')
    for frame in refs.FRAMES:
        gt = refs.make_gt(1, *frame, seed=7)
        want = np.sqrt(ndimage.sobel(gt[0], 0) ** 2.0 + ndimage.sobel(gt[0], 1) ** 2.0)
        got = multimodal.sobel_magnitude(torch.from_numpy(gt))[0].numpy()
        np.testing.assert_array_equal(got, want)                  # (on the 1/8 grid every sum is exact)
        np.testing.assert_array_equal(refs.sobel_ref(gt[0], 0), ndimage.sobel(gt[0], 0))
        np.testing.assert_array_equal(refs.sobel_ref(gt[0], 1), ndimage.sobel(gt[0], 1))
    rough = np.random.RandomState(0).randn(1, 9, 11).astype(np.float32)
    want = np.sqrt(ndimage.sobel(rough[0], 0) ** 2.0 + ndimage.sobel(rough[0], 1) ** 2.0)
    np.testing.assert_allclose(multimodal.sobel_magnitude(torch.from_numpy(rough))[0].numpy(), want, rtol=1e-6)


def test_two_means_is_the_brute_force_optimum_over_all_splits():
    """every split of 11 values into two non-empty groups, contiguous in sorted order or not: none has a smaller summed
    squared deviation than the one `two_means` returns"""
    rng = np.random.RandomState(11)
    for trial in range(6):
        vals = np.sort(np.round(rng.randn(11) * (1 + trial), 3))
        m0, m1 = (float(t[0]) for t in multimodal.two_means(torch.from_numpy(vals).unsqueeze(0)))
        cost = lambda g: float(((g - g.mean()) ** 2).sum())       # noqa: E731
        best = min(cost(vals[list(c)]) + cost(vals[[i for i in range(11) if i not in c]])
                   for r in range(1, 11) for c in itertools.combinations(range(11), r))
        assign = np.abs(vals - m0) <= np.abs(vals - m1)
        assert assign.any() and not assign.all()
        got = cost(vals[assign]) + cost(vals[~assign])
        assert got <= best * (1 + 1e-12) + 1e-12, (trial, got, best)
        np.testing.assert_allclose([m0, m1], [vals[assign].mean(), vals[~assign].mean()], rtol=1e-12)


def test_two_means_tie_goes_to_the_lowest_split_and_equal_values_stay():
    m0, m1 = multimodal.two_means(torch.tensor([[0.0, 1.0, 2.0], [0.1, 0.1, 0.1]], dtype=torch.float64))
    assert m0.tolist() == [0.0, 0.1] and m1.tolist() == [1.5, 0.1]
    assert refs.two_means_ref([0, 1, 2])[:2] == (0.0, 1.5)
    # through the public function: 1 x 3 image [0, 1, 2], radius 1 -> the centre's neighbourhood is [1, 0, 1, 2, 1]: the splits
    # {0} | {1, 1, 1, 2} and {0, 1, 1, 1} | {2} both cost 0.75
    modes = multimodal.gt_modes(torch.tensor([[[0.0, 1.0, 2.0]]]), radius=1.0)
    assert modes[0, 0, 1].tolist() == [0.0, 1.25]


def test_gt_modes_all_equal_neighbourhood():
    gt = torch.full((1, 4, 5), 0.1)
    modes, edges = multimodal.gt_modes(gt, edge_threshold=-1.0, return_edges=True)      # every pixel takes the edge branch
    assert int(edges.sum()) == 20
    assert torch.equal(modes, gt.double().unsqueeze(-1).expand(1, 4, 5, 2))


# ---------------------------------------------------------------- posterior modes, mode proportion

@pytest.mark.parametrize('s', refs.BINS)
def test_posterior_modes_and_mode_proportion_vs_pixel_loop(s):
    post = refs.make_posterior(2, s, 5, 7, seed=100 + s, smooth=_smooth_np)
    n_modes, disp, cnt, prop = multimodal.posterior_analysis(torch.from_numpy(post), -3.5, 3.5)
    assert (n_modes.dtype, disp.dtype, cnt.dtype, prop.dtype) == (torch.int32, torch.float64, torch.int32, torch.float32)
    for b in range(2):
        n_ref, d_ref = refs.posterior_modes_ref(post[b], -3.5, 3.5)
        np.testing.assert_array_equal(n_modes[b].numpy(), n_ref)
        np.testing.assert_allclose(disp[b].numpy(), d_ref, rtol=1e-15, atol=0)
        c_ref, p_ref = refs.mode_proportion_ref(post[b])
        np.testing.assert_array_equal(cnt[b].numpy(), c_ref)
        np.testing.assert_array_equal(prop[b].numpy(), p_ref)
    if s >= 70:
        assert 2 in n_modes.unique().tolist() and 0 < int(cnt.sum()) and float(prop.max()) > 1      # some pixel keeps two maxima
    a, b_ = multimodal.posterior_modes(torch.from_numpy(post), -3.5, 3.5)
    c, d = multimodal.mode_proportion(torch.from_numpy(post))
    assert torch.equal(a, n_modes) and torch.equal(b_, disp) and torch.equal(c, cnt) and torch.equal(d, prop)


def test_chosen_inputs_keep_every_decision_off_a_rounding():
    """the conditions tests/test_gpu_multimodal.py relies on, held on the CPU path for the seeds it uses"""
    for frame, s in refs.POSTERIOR_CASES:
        post = refs.make_posterior(2, s, *frame, seed=100 + s, smooth=_smooth_np)
        assert post.shape == (2, s, *frame) and (post > 0).all()
        assert (refs.smooth_gap(_smooth_np(post)) > refs.SMOOTH_GAP).all()
    post = refs.make_posterior(2, 18, 33, 65, seed=22, smooth=_smooth_np)             # (the two-mode error's scenes)
    assert (refs.smooth_gap(_smooth_np(post)) > refs.SMOOTH_GAP).all()
    for frame in refs.FRAMES:
        for seed in (3, 21):                                       # the ground-truth comparison's and the error sums' scenes
            gt = refs.make_gt(2, *frame, seed=seed)
            assert np.array_equal(gt * 8, np.round(gt * 8)) and np.abs(gt).max() <= 8          # on the grid of 1/8
            for axis in (1, 2):                                    # neighbours are equal or at least 1 apart
                jumps = np.abs(np.diff(gt.astype(np.float64), axis=axis))
                assert ((jumps == 0) | (jumps >= 1)).all()


def test_smoothing_vs_scipy():
    ndimage = pytest.importorskip('scipy.ndimage')
    for s in refs.BINS:
        post = refs.make_posterior(1, s, 2, 3, seed=s, smooth=_smooth_np)
        want = ndimage.gaussian_filter1d(post[0], sigma=2, axis=0)
        got = _smooth_np(post)[0]
        assert got.dtype == np.float32
        # scipy sums its weights pairwise and its taps from the middle outwards: the last bit of float32 may differ
        np.testing.assert_allclose(got, want, rtol=2.0 ** -22, atol=0)
        np.testing.assert_array_equal(got, refs.gaussian_filter1d_ref(post[0]))
    with pytest.raises(ValueError):
        multimodal.smooth_bins(torch.from_numpy(post), sigma=3.0)


def test_few_modes_are_filled_with_the_mode_there_is():
    ramp = np.linspace(0.1, 1.0, 9, dtype=np.float32)                # no interior maximum: the arg-max bin (8) twice
    one = np.array([.1, .2, .9, .2, .1, .1, .1, .1, .1], np.float32)   # one maximum at bin 2
    flat = np.full(9, 0.5, np.float32)                                # all equal: the FIRST arg-max bin
    two = np.array([.1, .5, .1, .1, .5, .1, .7, .1, .1], np.float32)   # bins 6 and, of the equal 1 and 4, the lower
    post = torch.from_numpy(np.stack([ramp, one, flat, two], -1).reshape(1, 9, 1, 4))
    n_modes, disp = multimodal.posterior_modes(post, -4.0, 4.0)
    assert n_modes[0, 0].tolist() == [0, 1, 0, 2]
    assert disp[0, 0].tolist() == [[4.0, 4.0], [-2.0, -2.0], [-4.0, -4.0], [-3.0, 2.0]]
    single = multimodal.posterior_modes(torch.ones(1, 1, 1, 1), -1.0, 1.0)
    assert single[0].item() == 0 and single[1][0, 0, 0].tolist() == [-1.0, -1.0]


def test_zero_minimum_between_two_maxima_gives_inf():
    post = refs.zero_gap_posterior()
    cnt, prop = multimodal.mode_proportion(torch.from_numpy(post))
    assert cnt[0, 0].tolist() == [1, 1]
    assert prop[0, 0, 0].item() == float('inf') and np.isfinite(prop[0, 0, 1].item()) and prop[0, 0, 1].item() > 1
    c_ref, p_ref = refs.mode_proportion_ref(post[0])
    np.testing.assert_array_equal(prop[0].numpy(), p_ref)
    assert (refs.smooth_gap(_smooth_np(post)) > refs.SMOOTH_GAP).all()


# ---------------------------------------------------------------- two-mode error

def scene_tensors(frame, s, seed):
    """(mode_disp, n_modes, gt_modes, gt, pred) of the CPU path for one batch of two frames"""
    gt = torch.from_numpy(refs.make_gt(2, *frame, seed=seed))
    post = torch.from_numpy(refs.make_posterior(2, s, *frame, seed=seed + 1, smooth=_smooth_np))
    n_modes, disp = multimodal.posterior_modes(post, -3.5, 3.5)
    pred = gt + torch.from_numpy(np.random.RandomState(seed).uniform(-0.2, 0.2, gt.shape).astype(np.float32))
    return disp, n_modes, multimodal.gt_modes(gt), gt, pred


@pytest.mark.parametrize('lb', [False, True])
@pytest.mark.parametrize('margin', [0, 2, 9])
def test_two_mode_error_vs_pixel_loop(margin, lb):
    disp, n_modes, modes, gt, pred = scene_tensors((5, 7), 18, seed=21)
    got = multimodal.two_mode_error(disp, n_modes, modes, gt, pred, margin=margin, lb=lb)
    assert got.dtype == torch.float64 and got.shape == (6,)
    want = np.sum([refs.two_mode_error_ref(disp[b].numpy(), n_modes[b].numpy(), modes[b].numpy(), gt[b].numpy(),
                                           pred[b].numpy(), margin, lb) for b in range(2)], 0)
    np.testing.assert_allclose(got.numpy(), want, rtol=1e-13, atol=0)
    assert (got[0] > 0) == (margin < 3)                            # a margin past half the frame counts nothing: zeros, no division
    if margin == 9:
        assert got.tolist() == [0.0] * 6


# ---------------------------------------------------------------- the two curves

@pytest.mark.parametrize('metric', ['mse', 'badpix'])
def test_sparsification_vs_script_restatement(metric):
    rng = np.random.RandomState(5)
    gt = rng.randn(6, 7).astype(np.float32)
    result = (gt + 0.1 * rng.randn(6, 7)).astype(np.float32)
    error = np.abs(result - gt)
    uncert = np.round(error + 0.05 * rng.rand(6, 7), 1).astype(np.float32)        # coarse: equal keys at the cuts
    got = multimodal.sparsification(*(torch.from_numpy(a) for a in (error, uncert, gt, result)), step=0.05, metric=metric)
    want = refs.sparsification_ref(error.flatten(), uncert.flatten(), gt.flatten(), result.flatten(), 0.05, metric == 'badpix')
    for g, w in zip(got[:4], want[:4]):
        assert len(g) == 20
        np.testing.assert_allclose(g, w, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(got[4], want[4], rtol=1e-12)
    assert got[1][0] == 1.0 and got[0][0] == 0.0                   # normalised by the all-pixels entry, fractions ascending


def test_mode_prediction_curve_vs_script_restatement():
    rng = np.random.RandomState(6)
    modes = np.zeros((6, 7, 2))
    modes[..., 1] = (rng.rand(6, 7) < 0.3)
    prop = np.round(rng.rand(6, 7) * 3, 0).astype(np.float32)      # equal keys everywhere
    prop[0, 0] = np.inf
    got = multimodal.mode_prediction_curve(torch.from_numpy(prop), torch.from_numpy(modes), step=0.05)
    want = refs.mode_prediction_ref(prop, modes, 0.05)
    for g, w in zip(got[:4], want[:4]):
        np.testing.assert_allclose(g, w, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(got[4], want[4], rtol=1e-12)
    assert got[1][0] == 1.0 and got[1][-1] == 0.0                  # the oracle has found every bimodal pixel well before 95 %


# ---------------------------------------------------------------- validate_scenes

def _tiny_upr():
    kw = dict(TINY_KW, model_uncert=True)
    model = FeedForward(**kw)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_state(synth.param_spec(**kw), 4).items()})
    return model.eval()


def _scenes(n, size=16):
    return [tuple(torch.from_numpy(np.asarray(a)).unsqueeze(0) for a in synth.synth_scene(k, size, size)[:8])
            + (torch.tensor([[k]]),) for k in range(n)]


BASE_KEYS = {'mse', 'badpix', 'kld', 'kld_mm', 'kld_um', 'nll', 'runtime'}
MM_KEYS = {'mm_cnt', 'mm_mse_sum', 'mm_badpix_sum', 'um_mse_sum', 'um_badpix_sum', 'mm_few_modes', 'mode_cnt_share'}


def test_validate_scenes_multimodal(tmp_path):
    from mmlf_amd import pfm, validate
    model = _tiny_upr()
    rows0, avg0 = validate.validate_scenes(model, _scenes(2), margin=2, out_dir=str(tmp_path / 'off'), scene_names=['s0', 's1'])
    assert all(set(r) == BASE_KEYS for r in rows0) and set(avg0) == BASE_KEYS - {'runtime'}
    assert not (tmp_path / 'off' / 'scenes' / 's0' / 'gt_modes.npy').exists()
    rows, avg = validate.validate_scenes(model, _scenes(2), margin=2, out_dir=str(tmp_path / 'on'), scene_names=['s0', 's1'],
                                         multimodal=True)
    assert all(set(r) == BASE_KEYS | MM_KEYS for r in rows)
    assert set(avg) == (BASE_KEYS - {'runtime'}) | {'mm_mse', 'mm_badpix', 'um_mse', 'um_badpix'}
    for r0, r in zip(rows0, rows):                                 # what was there is what it was
        assert all(r0[k] == r[k] for k in BASE_KEYS - {'runtime'})
    cnt = sum(r['mm_cnt'] for r in rows)
    assert cnt > 0
    for k in ('mm_mse', 'mm_badpix', 'um_mse', 'um_badpix'):       # total sums over the total count, not a mean of means
        assert avg[k] == sum(r[k + '_sum'] for r in rows) / cnt
    # one scene against the functions themselves, and the files
    scene = _scenes(2)[1]
    with torch.no_grad():
        out = model(*scene[:4])
    gt = scene[5].float()
    modes = multimodal.gt_modes(gt)
    n_modes, disp, mode_cnt, prop = multimodal.posterior_analysis(out['posterior'], model.disp_min, model.disp_max)
    assert out['posterior'].shape[1] == 108
    want = multimodal.two_mode_error(disp, n_modes, modes, gt, out['mean'], margin=2)
    assert [rows[1][k] for k in multimodal.TWO_MODE_FIELDS] == want.tolist()
    assert rows[1]['mode_cnt_share'] == float(mode_cnt.double().mean())
    np.testing.assert_array_equal(np.load(str(tmp_path / 'on' / 'scenes' / 's1' / 'gt_modes.npy')), modes[0].numpy())
    np.testing.assert_array_equal(pfm.load(str(tmp_path / 'on' / 'scenes' / 's1' / 'mode_prop.pfm')), prop[0].numpy()[::-1])


def test_validate_scenes_multimodal_without_a_posterior_adds_no_key():
    from mmlf_amd import validate
    model = FeedForward(**TINY_KW)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_state(synth.param_spec(**TINY_KW), 4).items()})
    rows, avg = validate.validate_scenes(model.eval(), _scenes(1), margin=2, multimodal=True)
    assert set(rows[0]) == BASE_KEYS and set(avg) == BASE_KEYS - {'runtime'}


# ---------------------------------------------------------------- the second library

needs_hipcc = pytest.mark.skipif(not os.path.exists(build.HIPCC), reason='no hipcc')


def test_training_abi_is_untouched():
    assert len(_lib.SIGNATURES) == 73
    assert not any(name.startswith('mmlf_eval_') for name in _lib.SIGNATURES)
    assert build.SOURCES == ['conv.hip', 'wgrad.hip', 'elementwise.hip']
    assert not any('eval' in d for d in build.HASHED)
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    assert set(_lib.EVAL_SIGNATURES) == {'mmlf_eval_last_error', 'mmlf_eval_abi_version', 'mmlf_eval_gt_modes',
                                         'mmlf_eval_posterior_modes', 'mmlf_eval_two_mode_error'}
    assert _lib.EVAL_SIGNATURES['mmlf_eval_gt_modes'] == (i, [vp, vp, vp, i, i, i, d, d, vp])
    assert _lib.EVAL_SIGNATURES['mmlf_eval_posterior_modes'] == (i, [vp] * 5 + [i] * 4 + [d] * 4 + [vp])
    assert _lib.EVAL_SIGNATURES['mmlf_eval_two_mode_error'] == (i, [vp] * 5 + [i] * 5 + [vp, vp, vp])


@needs_hipcc
def test_eval_library_builds_and_exports_exactly_its_header():
    lib_path = build.build_eval(verbose=False)
    assert lib_path == build.EVAL_LIB == _lib.EVAL_LIB_PATH and os.path.exists(lib_path)
    header = open(os.path.join(ROOT, 'include', 'mmlf_eval_hip.h')).read()
    declared = set(_lib.EVAL_SIGNATURES)
    assert set(re.findall(r'\b(mmlf_eval_[a-z0-9_]+)\s*\(', header)) <= declared
    nm = subprocess.run(['nm', '-D', '--defined-only', lib_path], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.split() and line.split()[-1].startswith('mmlf_')}
    assert exported == declared, exported ^ declared
    lib = ctypes.CDLL(lib_path)
    macro = int(re.search(r'^#define\s+MMLF_EVAL_ABI_VERSION\s+(\d+)', header, re.M).group(1))
    assert lib.mmlf_eval_abi_version() == _lib.EVAL_ABI_VERSION == macro == 1
    assert int(re.search(r'^#define\s+MMLF_EVAL_MAX_RADIUS\s+(\d+)', header, re.M).group(1)) == multimodal.MAX_RADIUS
    assert int(re.search(r'^#define\s+MMLF_EVAL_PARTIALS\s+(\d+)', header, re.M).group(1)) == multimodal._PARTIALS


@needs_hipcc
def test_eval_entry_points_refuse_bad_arguments_before_any_launch():
    """no GPU here: a call that got as far as a launch would fail differently (and say so)"""
    lib = _lib.load_eval()
    one = ctypes.c_void_p(8)                                       # never dereferenced: every call below is refused first
    bad = [('mmlf_eval_gt_modes', (one, one, one, 1, 4, 4, 4.5, 0.5, None), 'radius'),
           ('mmlf_eval_gt_modes', (one, one, one, 1, 0, 4, 2.0, 0.5, None), 'shape'),
           ('mmlf_eval_gt_modes', (None, one, one, 1, 4, 4, 2.0, 0.5, None), 'null'),
           ('mmlf_eval_posterior_modes', (one, one, one, one, one, 1, 0, 4, 4, -1.0, 1.0, 2.0, 0.1, None), 'shape'),
           ('mmlf_eval_posterior_modes', (one, one, one, one, one, 1, 9, 4, 4, -1.0, 1.0, 3.0, 0.1, None), 'sigma'),
           ('mmlf_eval_two_mode_error', (one, one, one, one, one, 1, 4, 4, -1, 0, one, one, None), 'margin'),
           ('mmlf_eval_two_mode_error', (one, one, one, one, one, 1, 4, 4, 0, 2, one, one, None), 'lb')]
    for name, args, word in bad:
        with pytest.raises(RuntimeError) as e:
            _lib.call_eval(name, *args)
        assert word in str(e.value), (name, str(e.value))


def test_load_eval_raises_when_the_library_is_missing(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, '_eval_lib', None)
    monkeypatch.setattr(_lib, 'EVAL_LIB_PATH', str(tmp_path / 'libmmlf_eval_hip.so'))
    with pytest.raises(RuntimeError) as e:
        _lib.load_eval()
    assert 'not found' in str(e.value)


def _eval_resource_usage():
    """kernel name -> scratch bytes per lane of every kernel of the evaluation library, read from the compiler"""
    flags = [f for f in build.FLAGS if f not in ('-fPIC', '-Wall')]
    usage = {}
    with tempfile.TemporaryDirectory() as tmp:
        for src in build.EVAL_SOURCES:
            cmd = [build.HIPCC, *flags, '--cuda-device-only', '-Rpass-analysis=kernel-resource-usage', '-c',
                   os.path.join(build.HERE, src), '-o', os.path.join(tmp, src + '.co')]
            run = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
            assert run.returncode == 0, run.stderr
            for block in re.split(r'remark: [^\n]*Function Name: ', run.stderr)[1:]:
                usage[block.split(' [')[0]] = int(re.search(r'ScratchSize \[bytes/lane\]: (\d+)', block).group(1))
    return usage


@needs_hipcc
def test_eval_kernels_use_no_scratch():
    """one thread per pixel with a 17-bin window and a 49-value sort: a per-thread array indexed at run time would sit in
    scratch memory, so the window moves by unrolled copies and the sort lives in an LDS tile"""
    usage = _eval_resource_usage()
    for stem in ('gt_modes_kernel', 'posterior_modes_kernel', 'two_mode_partial_kernel', 'two_mode_final_kernel'):
        hits = [v for k, v in usage.items() if stem in k]
        assert hits == [0], (stem, usage)
