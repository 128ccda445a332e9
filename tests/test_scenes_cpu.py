"""mmlf_amd/scenes.py on the CPU: the view indices, the texture mask against the reference's recorded
masks (tests/golden/g15_texture_mask.npz), assemble_scene against the numpy restatement of tests/scene_refs.py,
load_scene_dir on a directory written here, the binding of libmmlf_scene_hip.so and the texture kernel's resources."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import scene_refs as refs  # noqa: E402

from mmlf_amd import _lib, scenes  # noqa: E402
from mmlf_amd.csrc import build  # noqa: E402


@pytest.fixture(scope='module')
def g15():
    return np.load(os.path.join(HERE, 'golden', 'g15_texture_mask.npz'))


def test_view_indices_of_the_9x9_grid_and_a_non_square_one():
    us, vs, ids, dds = scenes.view_indices((9, 9))
    assert us == [36, 37, 38, 39, 40, 41, 42, 43, 44]
    assert vs == [4, 13, 22, 31, 40, 49, 58, 67, 76]
    assert ids == [72, 64, 56, 48, 40, 32, 24, 16, 8]
    assert dds == [0, 10, 20, 30, 40, 50, 60, 70, 80]
    assert scenes.view_indices() == (us, vs, ids, dds)
    # w = 5 columns, h = 3 rows, every range over h: row 1 from its left, column 2, the 3-step diagonals of a 5-wide grid
    assert scenes.view_indices((5, 3)) == ([5, 6, 7], [2, 7, 12], [12, 8, 4], [0, 6, 12])


@pytest.mark.parametrize('shape', refs.GOLDEN_SHAPES, ids=lambda s: 'x'.join(map(str, s[:4])))
def test_cpu_texture_mask_matches_the_reference(g15, shape):
    B, H, W, wsize, thr = shape
    for kind in refs.KINDS:
        c = torch.from_numpy(refs.centre(B, H, W, dyadic=kind == 'dyadic'))
        golden = g15[refs.tag(B, H, W, wsize, kind)].astype(np.int32)
        mask = scenes.texture_mask(c, wsize, thr)
        mae = scenes.texture_mae(c, wsize)
        assert mask.dtype == torch.int32 and mae.dtype == torch.float32
        refs.check_mae(mae, c, wsize, refs.tag(B, H, W, wsize, kind))
        if kind == 'dyadic':
            s = refs.window_sum64(c, wsize).numpy()
            assert np.array_equal(s.astype(np.float32).astype(np.float64), s)          # the exact sum is a float32
            assert np.array_equal(mae.numpy(), s.astype(np.float32) / np.float32(3 * wsize * wsize))
            assert np.array_equal(mask.numpy(), golden)
        else:
            refs.check_mask_band(mask, golden, c, wsize, thr, refs.tag(B, H, W, wsize, kind))
    if H <= 2 * (wsize // 2):
        assert not golden.any()


def test_cpu_texture_mask_semantics():
    c = torch.from_numpy(refs.centre(1, 30, 34, seed=3))
    inner = refs.interior(30, 34, 5)
    assert np.array_equal(scenes.texture_mask(c, 5, 0.0).numpy()[0], inner.astype(np.int32))
    assert not scenes.texture_mask(c, 5, 1e30).any()
    m_in = torch.from_numpy(np.random.RandomState(1).randint(0, 3, size=(1, 30, 34)).astype(np.int32))
    assert torch.equal(scenes.texture_mask(c, 5, 0.02, m_in), scenes.texture_mask(c, 5, 0.02) * m_in)
    c[0, 1, 12, 20] = float('nan')
    hit = np.zeros((30, 34), dtype=bool)
    hit[10:15, 18:23] = True
    mask = scenes.texture_mask(c, 5, 0.0).numpy()[0]
    assert np.array_equal(mask, (inner & ~hit).astype(np.int32))
    for bad in (0, 4, 22, 65):
        with pytest.raises(ValueError):
            scenes.texture_mask(c, bad)


@pytest.mark.parametrize('case', refs.ASSEMBLE_CASES, ids=refs.case_id)
def test_assemble_scene_on_the_cpu_matches_the_restatement(case):
    (views, gt, mpi, mask), out = refs.assemble_case(scenes.assemble_scene, case, 'cpu')
    texture = scenes.texture_mask(out[4].unsqueeze(0), 5, 0.02)[0].numpy()
    assert 0 < texture.sum() < texture.size
    ref = refs.assemble_ref(views, gt, mpi, mask, 7, case['nviews'], texture)
    assert len(out) == len(ref) == 9
    for k, (a, r) in enumerate(zip(out, ref)):
        assert isinstance(a, torch.Tensor) and a.device.type == 'cpu'
        assert tuple(a.shape) == r.shape, (k, a.shape, r.shape)
        assert np.array_equal(a.numpy(), r), k
    assert [t.dtype for t in out] == [torch.float32] * 7 + [torch.int32, torch.int64]
    assert out[6].shape[0] == (min(case['mpi'], 12) if case['mpi'] else 1)
    assert not torch.isnan(out[6]).any()
    batch = scenes.as_batch(out)
    assert all(b.shape == (1, *t.shape) for b, t in zip(batch, out))


def test_assemble_scene_refuses_what_does_not_fit():
    views, gt, mpi, mask = refs.scene_inputs((3, 3), 12, 14, 0)
    with pytest.raises(ValueError):
        scenes.assemble_scene(views[:8], nviews=(3, 3), wsize=3, device='cpu')          # the grid names image 8
    with pytest.raises(ValueError):
        scenes.assemble_scene(views, gt[:-1], nviews=(3, 3), wsize=3, device='cpu')
    with pytest.raises(ValueError):
        scenes.assemble_scene(views.astype(np.float64), nviews=(3, 3), wsize=3, device='cpu')
    with pytest.raises(ValueError):
        scenes.pack_views(views, [[0, 1, 2], [0, 1, 9], [0, 1, 2], [0, 1, 2]], 0, 'cpu')
    with pytest.raises(ValueError):
        scenes.pack_views(views, [[0, 1, 2], [0, -1, 2], [0, 1, 2], [0, 1, 2]], 0, 'cpu')


def test_load_scene_dir_reads_what_the_reference_reads(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    from mmlf_amd import pfm
    H, W, nviews = 27, 31, (3, 3)
    views, gt, mpi, mask = refs.scene_inputs(nviews, H, W, 4)
    for k, v in enumerate(views):
        Image.fromarray(v).save(tmp_path / f'input_Cam{k:03d}.png')
    Image.fromarray(views[0]).save(tmp_path / 'normals_Cam000.png')                  # filtered out by name
    Image.fromarray(views[1]).save(tmp_path / 'objectids_highres.png')
    Image.fromarray(np.stack([mask] * 3, -1)).save(tmp_path / 'mask.png')
    pfm.save(str(tmp_path / 'gt_disp_lowres.pfm'), np.flip(gt, 0).copy())
    pfm.save(str(tmp_path / 'gt_disp_highres.pfm'), np.zeros((2 * H, 2 * W), np.float32))
    pfm.save(str(tmp_path / 'gt_depth_lowres.pfm'), np.ones((H, W), np.float32))
    np.savez(tmp_path / 'gt_mpi_lowres.npz', mpi=mpi)
    out = scenes.load_scene_dir(str(tmp_path), index=3, nviews=nviews, device='cpu')
    # the module's wsize is the reference's 23: on a 27 x 31 frame the interior is 5 x 9
    expect = scenes.assemble_scene(views, gt, mpi, mask, 3, nviews, device='cpu')
    for k, (a, r) in enumerate(zip(out, expect)):
        assert torch.equal(a, r), k
    texture = scenes.texture_mask(expect[4].unsqueeze(0))[0].numpy()
    ref = refs.assemble_ref(views, gt, mpi, mask, 3, nviews, texture)
    for k, (a, r) in enumerate(zip(out, ref)):
        assert np.array_equal(a.numpy(), r), k
    # without the optional files: zeros, the one-plane target, the texture mask alone
    for name in ('gt_disp_lowres.pfm', 'gt_disp_highres.pfm', 'gt_depth_lowres.pfm', 'gt_mpi_lowres.npz', 'mask.png'):
        os.remove(tmp_path / name)
    bare = scenes.load_scene_dir(str(tmp_path), nviews=nviews, device='cpu')
    assert not bare[5].any() and bare[6].shape == (1, 5, H, W) and torch.equal(bare[6][0, :3], bare[4])
    assert np.array_equal(bare[7].numpy(), texture)


def test_header_matches_the_binding():
    text = open(os.path.join(os.path.dirname(HERE), 'include', 'mmlf_scene_hip.h')).read()
    sigs = _lib.signatures_from_header(text)
    assert sigs == _lib.SCENE_SIGNATURES
    assert set(sigs) == {'mmlf_scene_last_error', 'mmlf_scene_abi_version', 'mmlf_scene_texture', 'mmlf_scene_pack_views'}
    assert f'#define MMLF_SCENE_ABI_VERSION {_lib.SCENE_ABI_VERSION}\n' in text
    assert _lib.SCENE_MAX_WSIZE == 63
    res, args = sigs['mmlf_scene_texture']
    assert res is ctypes.c_int
    assert args == [ctypes.c_void_p, ctypes.c_int, ctypes.c_double] + [ctypes.c_void_p] * 3 + [ctypes.c_int] * 3 + \
        [ctypes.c_void_p]
    res, args = sigs['mmlf_scene_pack_views']
    assert res is ctypes.c_int
    assert args == [ctypes.c_void_p] * 4 + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 3
    assert sigs['mmlf_scene_last_error'] == (ctypes.c_char_p, [])
    if os.path.exists(_lib.SCENE_LIB_PATH):
        lib = ctypes.CDLL(_lib.SCENE_LIB_PATH)
        assert lib.mmlf_scene_abi_version() == _lib.SCENE_ABI_VERSION
        for name in sigs:
            assert hasattr(lib, name), name


def test_the_scene_library_stands_apart_from_the_other_four():
    others = build.SOURCES + build.HASHED + build.EVAL_SOURCES + build.ESE_SOURCES + build.DATA_SOURCES
    assert build.SCENE_SOURCES == ['scene.hip']
    assert not any('scene' in s for s in others)
    assert os.path.basename(build.SCENE_LIB) == 'libmmlf_scene_hip.so' == os.path.basename(_lib.SCENE_LIB_PATH)
    text = open(os.path.join(build.HERE, 'scene.hip')).read()
    assert re.findall(r'#include "([^"]+)"', text) == ['../../include/mmlf_scene_hip.h']


def test_a_missing_library_raises(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, '_scene_lib', None)
    monkeypatch.setattr(_lib, 'SCENE_LIB_PATH', str(tmp_path / 'libmmlf_scene_hip.so'))
    with pytest.raises(RuntimeError, match='libmmlf_scene_hip.so not found'):
        _lib.load_scene_lib()
    with pytest.raises(RuntimeError, match='no fallback'):
        _lib.call_scene('mmlf_scene_texture')


def test_scene_kernels_use_no_scratch():
    """the compiler's resource remarks for scene.hip (the method of tests/test_kernel_resources.py): the texture kernel keeps
    its four accumulators and centre values in registers"""
    if not os.path.exists(build.HIPCC):
        pytest.skip('no hipcc')
    flags = [f for f in build.FLAGS if f not in ('-fPIC', '-Wall')]
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [build.HIPCC, *flags, '--cuda-device-only', '-Rpass-analysis=kernel-resource-usage', '-c',
               os.path.join(build.HERE, 'scene.hip'), '-o', os.path.join(tmp, 'scene.co')]
        job = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    assert job.returncode == 0, job.stderr
    usage = {}
    for block in re.split(r'remark: [^\n]*Function Name: ', job.stderr)[1:]:
        m = re.search(r'ScratchSize \[bytes/lane\]: (\d+)', block)
        usage[block.split(' [')[0]] = int(m.group(1)) if m else -1
    kernels = {k: v for k, v in usage.items() if 'scene_texture_kernel' in k or 'scene_pack_kernel' in k}
    assert len(kernels) == 2, usage
    assert all(v == 0 for v in kernels.values()), kernels
