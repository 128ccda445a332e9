"""PatchPipeline(chain=[...]): the composable transform chain of mmlf_amd/transforms.py on
libmmlf_data_hip.so.  CPU: the numpy restatement (tests/transform_refs.py) and the host draws against the reference's
recorded outputs (tests/golden/g12_patch_chain.npz), the index tables against scipy, the slot order, the binding.
GPU: every golden chain on the device, the CLI chain against chain=None bit for bit, batches, and the noise generator."""
import inspect
import math
import os
import random
import re
import sys

import numpy as np
import pytest
import torch

from mmlf_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import transform_refs as refs  # noqa: E402

NAMES = refs.NAMES
# the bar of tests/test_patch_pipeline.py and its reason: every op is a float32 blend / 3x3 colour mix of values in [0,2);
# implementations differ only in the summation order of the contrast mean (pairwise float32 vs double)
TOL = 2e-6


@pytest.fixture(scope='module')
def g12():
    return np.load(os.path.join(HERE, 'golden', 'g12_patch_chain.npz'))


@pytest.fixture(scope='module')
def scenes():
    return {tag: synth.synth_scene(seed, H, W, views=refs.VIEWS, planes=refs.PLANES)
            for tag, (seed, (H, W), _) in refs.CASES.items()}


def _compare(out, expect, tag):
    for name, arr, ref in zip(NAMES, out, expect):
        arr = arr.cpu().numpy() if isinstance(arr, torch.Tensor) else arr
        assert arr.shape == ref.shape, (tag, name, arr.shape, ref.shape)
        if name == 'mask':
            assert np.array_equal(arr, ref), (tag, name)
        else:
            assert arr.dtype == np.float32, (tag, name, arr.dtype)
            assert np.abs(arr.astype(np.float64) - ref).max() <= TOL, (tag, name)


def _golden(g12, tag, k):
    return [g12[f'{tag}.{k}.{n}'] for n in NAMES]


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize('tag', list(refs.CASES))
def test_restatement_matches_the_reference(g12, scenes, tag):
    _, _, chain = refs.CASES[tag]
    for k in range(refs.SAMPLES):
        random.seed(refs.case_seed(tag, k))
        out = refs.apply_chain(scenes[tag], chain)
        _compare(out[:8], _golden(g12, tag, k), (tag, k))
        assert np.array_equal(out[8], scenes[tag][8])                       # index: untouched
        assert random.random() == float(g12[f'{tag}.{k}.after']), (tag, k)


@pytest.mark.parametrize('tag', list(refs.CASES))
def test_host_draws_leave_random_where_the_reference_does(g12, tag):
    from mmlf_amd import patches, transforms as T
    _, frame, chain = refs.CASES[tag]
    plan = patches.validate_chain(refs.build(T, chain), refs.PS)
    for k in range(refs.SAMPLES):
        random.seed(refs.case_seed(tag, k))
        p = patches.draw_chain_sample(plan, frame, refs.VIEWS)
        assert random.random() == float(g12[f'{tag}.{k}.after']), (tag, k)
        assert 0 <= p['y0'] and p['y0'] + refs.PS <= p['hs'] and 0 <= p['x0'] and p['x0'] + refs.PS <= p['ws']


def test_cli_chain_draws_what_draw_sample_draws():
    from mmlf_amd import patches
    for augment in (True, False):
        plan = patches.validate_chain(patches.cli_chain(8, 2, augment), 8)
        for seed in range(20):
            random.seed(seed)
            old = patches.draw_sample((64, 72), 8, 2, augment)
            after = random.random()
            random.seed(seed)
            new = patches.draw_chain_sample(plan, (64, 72), 5)
            assert random.random() == after
            assert (new['y0'], new['x0'], new['rot']) == (old['y0'], old['x0'], old['rot'])
            if augment:
                assert (new['down'], new['disp'], new['bright'], new['contrast']) == (old['f'], old['disp'], old['bright'],
                                                                                     old['contrast'])
                assert np.array_equal(new['mat'], old['mat'])


def test_index_tables_match_scipy_zoom():
    """zoom of a ramp 1..n IS the table + 1; scipy's constant 0 is the table's -1 (transforms.zoom_map)"""
    ndimage = pytest.importorskip('scipy').ndimage
    from mmlf_amd import transforms as T
    factors = [0.3 + 0.05 * k for k in range(29)] + [0.5, 1.0, 1.3, 1.0 / 3.0, 0.999, 1.001]
    filled = 0
    for n in range(9, 71):
        ramp = np.arange(1, n + 1, dtype=np.int64)
        for f in factors:
            n_out = T.zoom_size(n, f)
            ref = ndimage.zoom(ramp, f, order=0)
            assert len(ref) == n_out, (n, f)
            table = T.zoom_map(n, n_out)
            assert table.dtype == np.int32 and np.array_equal(table + 1, ref), (n, f)
            assert table[:-1].min() >= 0 and table.max() < n
            filled += int(table[-1] < 0)
    assert filled > 0                                   # 15 -> 26 is one: 25 * (14 / 25) > 14 in double
    assert T.zoom_map(15, 26)[-1] == -1 and T.zoom_map(40, 52)[-1] == 39
    # both axes at once, through the last two axes of a stack, as Zoom.__call__ does it; the restatement likewise
    for shape, f in (((3, 23, 31), 0.7), ((2, 15, 15), 1.7)):
        img = (1.0 + np.arange(np.prod(shape), dtype=np.float32)).reshape(shape)
        ref = ndimage.zoom(img, [1.0, f, f], order=0)
        ym, xm = T.zoom_map(shape[1], T.zoom_size(shape[1], f)), T.zoom_map(shape[2], T.zoom_size(shape[2], f))
        got = np.where((ym[:, None] | xm[None, :]) < 0, np.float32(0), img[:, ym[:, None], xm[None, :]])
        assert np.array_equal(got, ref), (shape, f)
        gt, mpi = img[0].copy(), np.stack([img[:1]] * 5, 1)
        out = refs.tf_zoom((img, img, img, img, img, gt, mpi, img[0].astype(np.int64), np.zeros(1)), f)
        assert np.array_equal(out[0], ref) and np.array_equal(out[7], ref[0].astype(np.int64))
        assert np.array_equal(out[5], ref[0] * np.float32(f)) and np.array_equal(out[6][0, 4], ref[0] * np.float32(f))
        assert np.array_equal(out[6][0, 3], ref[0])
    assert np.array_equal(T.down_map(41, 3), np.arange(41)[::3])


def test_constructor_type_rules():
    from mmlf_amd import transforms as T
    for make in (lambda: T.Zoom(1), lambda: T.Shift(1), lambda: T.RandomShift(1), lambda: T.IntegerShift(1.0),
                 lambda: T.Brightness(1), lambda: T.Contrast(1), lambda: T.Noise(1), lambda: T.RandomCrop(8.0),
                 lambda: T.RandomCrop(8, pad=1.0), lambda: T.CenterCrop('8'), lambda: T.DownSampling(2.0),
                 lambda: T.RandomDownSampling(4.0)):
        with pytest.raises(TypeError):
            make()
    for make in (lambda: T.RandomShift(-1.0), lambda: T.RandomShift((1.0, 2.0, 3.0)), lambda: T.DownSampling(0),
                 lambda: T.Zoom(0.0), lambda: T.RandomCrop((8, 8, 8)), lambda: T.RandomCrop(8, pad=-1),
                 lambda: T.Noise(-0.1)):
        with pytest.raises(ValueError):
            make()
    assert T.RandomShift(2.0).disp_range == (-2.0, 2.0) and T.RandomShift((0.5, 1.5)).disp_range == (0.5, 1.5)
    assert T.RandomCrop(8).size == (8, 8) and T.RandomCrop(8).pad == 0 and T.CenterCrop((6, 8)).size == (6, 8)
    assert (T.RandomDownSampling().max_factor, T.RandomZoom().interval, T.Brightness().level, T.Contrast().level,
            T.Noise().stdev) == (4, (0.5, 1.0), 0.9, 0.9, 0.01)
    assert not callable(T.Zoom(0.5)) and not callable(T.Noise())          # carriers, not transforms of data


def test_slot_order_and_size_violations_raise():
    from mmlf_amd import patches, transforms as T
    ps = 8
    crop = T.RandomCrop(ps)
    bad = {
        'no crop': [T.Zoom(0.5)],
        'two scales': [T.Zoom(0.5), T.DownSampling(2), crop],
        'two shears': [T.Shift(0.5), T.IntegerShift(1), crop],
        'shear before scale': [T.RandomShift(1.0), T.RandomDownSampling(2), crop],
        'scale after crop': [crop, T.Zoom(0.5)],
        'shear after crop': [crop, T.IntegerShift(1)],
        'centre before crop': [T.CenterCrop(ps), T.RandomCrop(ps + 8)],
        'two crops': [T.RandomCrop(ps + 8), T.RandomCrop(ps)],
        'two rotations': [crop, T.Rotate90(), T.RandomRotate()],
        'rotation before crop': [T.Rotate90(), crop],
        'colour before rotation': [crop, T.RedistColor(), T.RandomRotate()],
        'contrast before brightness': [crop, T.Contrast(), T.Brightness()],
        'noise before contrast': [crop, T.Noise(), T.Contrast()],
        'two noises': [crop, T.Noise(), T.Noise(0.02)],
        'crop is not ps': [T.RandomCrop(ps + 1)],
        'centre is not ps': [T.RandomCrop(ps + 8), T.CenterCrop(ps + 2)],
        'centre larger than crop': [T.RandomCrop(ps - 2), T.CenterCrop(ps)],
        'tuple crop': [T.RandomCrop((ps, ps + 2))],
        'tuple centre': [T.RandomCrop(ps + 8), T.CenterCrop((ps, ps + 2))],
        'not a transform': [crop, 'Noise'],
        'a callable': [crop, lambda data: data],
    }
    for why, chain in bad.items():
        with pytest.raises(ValueError):
            patches.validate_chain(chain, ps)
            pytest.fail(why)
    # the message names the offending element
    with pytest.raises(ValueError, match=r'chain\[1\] = DownSampling\(factor=2\)'):
        patches.validate_chain([T.Zoom(0.5), T.DownSampling(2), crop], ps)
    with pytest.raises(ValueError, match=r'chain\[1\] = Zoom\(factor=0.5\)'):
        patches.validate_chain([crop, T.Zoom(0.5)], ps)
    # the full order passes, with either member of every slot
    full = [T.RandomZoom(), T.IntegerShift(1), T.RandomCrop(ps + 4, 1), T.CenterCrop(ps), T.Rotate90(), T.RedistColor(),
            T.Brightness(0.1), T.Contrast(0.2), T.Noise(0.03)]
    assert list(patches.validate_chain(full, ps)) == list(T.SLOTS)
    assert list(patches.validate_chain(patches.cli_chain(ps), ps)) == [s for s in T.SLOTS if s != 'noise']


def test_frames_the_chain_cannot_crop_raise():
    from mmlf_amd import patches, transforms as T
    def draw(chain, frame, views=3):
        return patches.draw_chain_sample(patches.validate_chain(chain, 8), frame, views)
    with pytest.raises(ValueError):
        draw([T.RandomCrop(8)], (8, 40))                                  # h > size (hci4d.py:656)
    with pytest.raises(ValueError):
        draw([T.Zoom(0.2), T.RandomCrop(8)], (40, 52))                    # 8 x 10 after the zoom
    with pytest.raises(ValueError):
        draw([T.DownSampling(5), T.RandomCrop(8)], (40, 52))              # 8 x 11
    with pytest.raises(ValueError):
        draw([T.RandomCrop(8, 17)], (40, 52))                             # randint(17, 15)
    with pytest.raises(ValueError):
        draw([T.DownSampling(4), T.IntegerShift(10), T.RandomCrop(8)], (40, 52))      # rolls by 10 in a 10-row frame
    with pytest.raises(ValueError):
        draw([T.IntegerShift(-5), T.RandomCrop(8)], (40, 52), views=17)   # |-5| * 8 = 40 rows
    draw([T.DownSampling(4), T.IntegerShift(9), T.RandomCrop(8)], (40, 52))
    assert draw([T.Zoom(0.5), T.RandomCrop(8)], (41, 53))['hs'] == 20     # Python's round: 20.5 -> 20


def test_header_matches_the_binding():
    import ctypes
    from mmlf_amd import _lib
    text = open(os.path.join(os.path.dirname(HERE), 'include', 'mmlf_data_hip.h')).read()
    sigs = _lib.signatures_from_header(text)
    assert sigs == _lib.DATA_SIGNATURES
    assert set(sigs) == {'mmlf_data_last_error', 'mmlf_data_abi_version', 'mmlf_data_gather', 'mmlf_data_finish'}
    assert f'#define MMLF_DATA_ABI_VERSION {_lib.DATA_ABI_VERSION}\n' in text
    res, args = sigs['mmlf_data_gather']
    assert res is ctypes.c_int and len(args) == 29
    assert [k for k, a in enumerate(args) if a is ctypes.c_int] == [5, 6, 7, 8, 9, 13, 15, 26, 27]
    assert all(a is ctypes.c_void_p for k, a in enumerate(args) if k not in (5, 6, 7, 8, 9, 13, 15, 26, 27))
    res, args = sigs['mmlf_data_finish']
    assert args == [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_float, ctypes.c_int64, ctypes.c_int64] + \
        [ctypes.c_int] * 3 + [ctypes.c_void_p]
    assert _lib.DATA_FLAGS == dict(SHEAR=1, COLOR=2, BRIGHT=4, ROLL=8, GT_MUL=16, GT_DIV=32)
    if os.path.exists(_lib.DATA_LIB_PATH):
        lib = ctypes.CDLL(_lib.DATA_LIB_PATH)
        assert lib.mmlf_data_abi_version() == _lib.DATA_ABI_VERSION
        for name in sigs:
            assert hasattr(lib, name), name


def test_a_missing_library_raises(monkeypatch, tmp_path):
    from mmlf_amd import _lib
    monkeypatch.setattr(_lib, '_data_lib', None)
    monkeypatch.setattr(_lib, 'DATA_LIB_PATH', str(tmp_path / 'libmmlf_data_hip.so'))
    with pytest.raises(RuntimeError, match='libmmlf_data_hip.so not found'):
        _lib.load_data()
    with pytest.raises(RuntimeError, match='no fallback'):
        _lib.call_data('mmlf_data_finish')


def test_the_old_constructor_signature_stands():
    from mmlf_amd import patches
    params = list(inspect.signature(patches.PatchPipeline.__init__).parameters.values())
    assert [p.name for p in params[:7]] == ['self', 'scenes', 'ps', 'max_downscale', 'augment', 'train_shift', 'device']
    assert [p.default for p in params[3:7]] == [4, True, 0.0, 'cuda']
    assert {p.name: p.default for p in params[7:]} == {'chain': None, 'noise_seed': 0}
    names = [type(t).__name__ for t in patches.cli_chain(32, 3)]
    assert names == ['RandomDownSampling', 'RandomShift', 'RandomCrop', 'CenterCrop', 'RandomRotate', 'RedistColor',
                     'Brightness', 'Contrast']
    assert [type(t).__name__ for t in patches.cli_chain(32, augment=False)] == ['RandomCrop', 'CenterCrop']
    chain = patches.cli_chain(32, 3)
    assert chain[0].max_factor == 3 and chain[1].disp_range == (-1.0, 1.0) and chain[2].size == (48, 48)
    assert chain[3].size == (32, 32) and chain[6].level == 0.9 and chain[7].level == 0.9


def test_product_code_does_not_import_scipy():
    root = os.path.join(os.path.dirname(HERE), 'mmlf_amd')
    for name in ('transforms.py', 'patches.py'):
        assert re.search(r'^\s*(import|from)\s+scipy', open(os.path.join(root, name)).read(), re.M) is None, name


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize('tag', list(refs.CASES))
def test_device_chain_matches_the_reference(g12, scenes, tag):
    from mmlf_amd import patches, transforms as T
    _, _, chain = refs.CASES[tag]
    pipe = patches.PatchPipeline([scenes[tag]], refs.PS, chain=refs.build(T, chain))
    for k in range(refs.SAMPLES):
        random.seed(refs.case_seed(tag, k))
        out = pipe.sample([0])
        assert random.random() == float(g12[f'{tag}.{k}.after']), (tag, k)
        _compare([t[0] for t in out[:8]], _golden(g12, tag, k), (tag, k))
        assert out[7].dtype == torch.int32 and int(out[8][0, 0]) == refs.CASES[tag][0]


@pytest.mark.gpu
@pytest.mark.parametrize('augment', [True, False])
def test_cli_chain_gives_the_bits_of_the_fixed_pipeline(augment):
    from mmlf_amd import patches
    scene_list = [synth.synth_scene(30 + s, 64, 72, views=5) for s in range(3)]
    idx = [0, 2, 1, 1, 0, 2, 2]
    old = patches.PatchPipeline(scene_list, 8, 2, augment)
    new = patches.PatchPipeline(scene_list, 8, chain=patches.cli_chain(8, 2, augment))
    for seed in (5, 6):
        random.seed(seed)
        a = old.sample(idx)
        after = random.random()
        random.seed(seed)
        b = new.sample(idx)
        assert random.random() == after
        for name, x, y in zip(NAMES + ('index',), a, b):
            assert x.dtype == y.dtype and x.shape == y.shape, name
            assert torch.equal(x, y), (augment, seed, name)


@pytest.mark.gpu
def test_a_batch_is_its_samples_one_after_the_other():
    from mmlf_amd import patches, transforms as T
    scene_list = [synth.synth_scene(40 + s, 41, 53, views=3) for s in range(2)]
    chain = [T.RandomZoom(0.6, 1.4), T.RandomShift(1.5), T.RandomCrop(12, 1), T.CenterCrop(8), T.RandomRotate(),
             T.RedistColor(), T.Brightness(0.4), T.Contrast(0.6)]
    pipe = patches.PatchPipeline(scene_list, 8, chain=chain)
    idx = [1, 0, 0, 1, 1, 0]
    random.seed(11)
    batch = pipe.sample(idx)
    after = random.random()
    random.seed(11)
    singles = [pipe.sample([sc]) for sc in idx]
    assert random.random() == after
    for k, name in enumerate(NAMES + ('index',)):
        assert torch.equal(batch[k], torch.cat([s[k] for s in singles])), name
    # and each of them is the restatement's sample
    random.seed(11)
    spec = [('RandomZoom', (0.6, 1.4)), ('RandomShift', (1.5,)), ('RandomCrop', (12, 1)), ('CenterCrop', (8,)),
            ('RandomRotate', ()), ('RedistColor', ()), ('Brightness', (0.4,)), ('Contrast', (0.6,))]
    for b, sc in enumerate(idx):
        _compare([t[b] for t in batch[:8]], refs.apply_chain(scene_list[sc], spec)[:8], ('batch', b))


@pytest.mark.gpu
def test_zoom_keeps_the_row_scipy_fills_with_zero():
    """15 -> 26 (Zoom(1.7)): the last row and column of the zoomed frame are scipy's constant, in every plane, and the
    shear's taps that wrap onto them read it (transforms.zoom_map; the restatement is held to scipy on the CPU)."""
    from mmlf_amd import patches, transforms as T
    scene = synth.synth_scene(60, 15, 15, views=3)
    pipe = patches.PatchPipeline([scene], 24, chain=[T.Zoom(1.7), T.RandomShift(1.5), T.RandomCrop(24), T.RandomRotate(),
                                                     T.Contrast(0.5)])
    spec = [('Zoom', (1.7,)), ('RandomShift', (1.5,)), ('RandomCrop', (24,)), ('RandomRotate', ()), ('Contrast', (0.5,))]
    random.seed(31)
    out = pipe.sample([0] * 6)
    random.seed(31)
    edge = 0
    for b in range(6):
        ref = refs.apply_chain(scene, spec)
        _compare([t[b] for t in out[:8]], ref[:8], ('fill', b))
        edge += int((ref[7][-1] == 0).all() or (ref[7][:, -1] == 0).all())
    assert edge > 0                                     # (the seed's crops reach the filled row or column)


def _noise_pair(sigma, noise_seed, calls=1):
    from mmlf_amd import patches, transforms as T
    scene = synth.synth_scene(50, 48, 56, views=3)
    base = [T.RandomDownSampling(2), T.RandomShift(1.0), T.RandomCrop(16), T.RandomRotate(), T.RedistColor(),
            T.Brightness(0.5), T.Contrast(0.5)]
    clean = patches.PatchPipeline([scene], 16, chain=base)
    noisy = patches.PatchPipeline([scene], 16, chain=base + [T.Noise(sigma)], noise_seed=noise_seed)
    outs = []
    for call in range(calls):
        random.seed(21)
        a = clean.sample([0] * 4)
        random.seed(21)
        outs.append((a, noisy.sample([0] * 4)))
    return outs


@pytest.mark.gpu
def test_noise_statistics():
    sigma = 0.05
    (clean, noisy), = _noise_pair(sigma, noise_seed=1234)
    for k in (5, 6, 7):                                                   # gt, mpi and mask: untouched
        assert torch.equal(clean[k], noisy[k]), NAMES[k]
    diff = torch.cat([(noisy[k].double() - clean[k].double()).reshape(-1) for k in range(5)]).cpu().numpy()
    N = diff.size
    assert N == 4 * 4 * 3 * 3 * 256 + 4 * 3 * 256
    mean, std = diff.mean(), diff.std()
    frac = float((np.abs(diff) > 2.0 * sigma).mean())
    p2 = math.erfc(2.0 / math.sqrt(2.0))                                  # 0.0455
    print(f'noise: N {N} mean/sigma {mean / sigma:.3e} (bar {5 / math.sqrt(N):.3e}) std/sigma - 1 {std / sigma - 1:.3e} '
          f'(bar {5 / math.sqrt(2 * N):.3e}) beyond 2 sigma {frac:.5f} (0.0455 +- {5 * math.sqrt(p2 * (1 - p2) / N):.5f})')
    assert abs(mean) <= 5.0 * sigma / math.sqrt(N)
    assert abs(std / sigma - 1.0) <= 5.0 / math.sqrt(2.0 * N)
    assert abs(p2 - 0.0455) < 1e-4 and abs(frac - 0.0455) <= 5.0 * math.sqrt(0.0455 * (1.0 - 0.0455) / N)
    # two views of one stack, neighbouring stacks, the centre view against a stack view: independent
    d = [(noisy[k].double() - clean[k].double()).cpu().numpy() for k in range(5)]
    pairs = [(d[0][:, 0], d[0][:, 1]), (d[0][:, 1], d[0][:, 2]), (d[1][:, 0], d[2][:, 0]), (d[3][:, 2], d[0][:, 2]),
             (d[4], d[1][:, 1]), (d[0][0], d[0][1]), (d[0][..., :-1], d[0][..., 1:])]
    for k, (x, y) in enumerate(pairs):
        x, y = x.reshape(-1), y.reshape(-1)
        corr = float(np.corrcoef(x, y)[0, 1])
        print(f'noise: pair {k} n {x.size} corr {corr:.4f} (bar {5 / math.sqrt(x.size):.4f})')
        assert abs(corr) <= 5.0 / math.sqrt(x.size), k


@pytest.mark.gpu
def test_noise_is_a_function_of_seed_and_call():
    sigma = 0.02
    run_a = _noise_pair(sigma, noise_seed=7, calls=2)
    run_b = _noise_pair(sigma, noise_seed=7, calls=2)
    run_c = _noise_pair(sigma, noise_seed=8, calls=1)
    for call in range(2):
        for k in range(9):
            assert torch.equal(run_a[call][1][k], run_b[call][1][k]), (call, k)       # same seed, same call: same bits
    for k in range(5):
        assert not torch.equal(run_a[0][1][k], run_a[1][1][k]), k                     # the next call: other noise
        assert not torch.equal(run_a[0][1][k], run_c[0][1][k]), k                     # another seed: other noise
        assert torch.equal(run_a[0][0][k], run_c[0][0][k]), k                         # (the clean chain is the same)


@pytest.mark.gpu
def test_noise_alone_and_the_bad_launches():
    """Noise without Contrast takes the finish pass without sums; bad extents are refused before any launch."""
    from mmlf_amd import _lib, patches, transforms as T
    scene = synth.synth_scene(51, 40, 52, views=3)
    pipe = patches.PatchPipeline([scene], 7, chain=[T.RandomCrop(7), T.Noise(0.1)], noise_seed=3)   # 7: groups straddle samples
    random.seed(1)
    out = pipe.sample([0, 0, 0])
    random.seed(1)
    y, x = [random.randint(0, 40 - 7 - 0), random.randint(0, 52 - 7 - 0)]
    d = out[4][0].cpu().numpy() - scene[4][:, y:y + 7, x:x + 7]
    assert 0.05 < d.std() < 0.2 and np.array_equal(out[5][0].cpu().numpy(), scene[5][y:y + 7, x:x + 7])
    t = out[0].contiguous()
    for args in ((None, t.data_ptr(), None, None, 1, 0.1, 0, 0, 1, 1, 4, None),
                 (t.data_ptr(), t.data_ptr(), None, None, 1, 0.1, 0, 0, 0, 1, 4, None),
                 (t.data_ptr(), t.data_ptr(), None, None, 1, 0.1, 0, 0, 1, 0, 4, None),
                 (t.data_ptr(), t.data_ptr(), None, None, 1, 0.1, 0, 0, 1, 1, 0, None),
                 (t.data_ptr(), t.data_ptr(), None, None, 0, 0.1, 0, 0, 1, 1, 4, None),
                 (t.data_ptr(), t.data_ptr(), None, t.data_ptr(), 0, 0.1, 0, 0, 1, 1, 4, None)):
        with pytest.raises(RuntimeError, match='mmlf_data_finish'):
            _lib.call_data('mmlf_data_finish', *args)
    p = t.data_ptr()
    good = [p, p, p, p, p, 1, 3, 2, 40, 52, p, p, p, 40, p, 52, p, p, p, p, p, p, p, p, p, None, 1, 7, None]
    for at, value in ((0, None), (10, None), (12, None), (20, None), (5, 0), (6, 0), (8, 0), (9, 0), (26, 0), (27, 0),
                      (13, 6), (15, 6), (7, -1)):
        args = list(good)
        args[at] = value
        with pytest.raises(RuntimeError, match='mmlf_data_gather'):
            _lib.call_data('mmlf_data_gather', *args)


@pytest.mark.gpu
def test_the_data_library_is_what_runs():
    from mmlf_amd import patches, transforms as T
    scene = synth.synth_scene(52, 40, 52, views=3)
    random.seed(2)
    patches.PatchPipeline([scene], 8, chain=[T.Zoom(0.7), T.RandomCrop(8), T.Noise()]).sample([0])
    torch.cuda.synchronize()
    assert 'libmmlf_data_hip.so' in open('/proc/self/maps').read()
