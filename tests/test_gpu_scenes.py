"""libmmlf_scene_hip.so on the device: the texture kernel against a float64 evaluation, against exact sums
on dyadic centres and against the reference's recorded masks (tests/golden/g15_texture_mask.npz); its semantics; the view
pass against numpy; assemble_scene against its CPU path; PatchPipeline on device-tensor scenes.

The mean absolute error is held to the RELATIVE bound (3 wsize^2 + 2) 2^-24 (scene_refs.rel_bound; 9.5e-5 at 23): a float32
sum of that many non-negative terms in any order, plus the rounding of a term and of the division.  A float centre's mask
is held to the golden wherever the float64 value lies further than that bound from the threshold; the pixels inside the
band are counted and capped (scene_refs.BAND_CAP).  A dyadic centre's results are held bit for bit, at every pixel."""
import os
import random
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import scene_refs as refs  # noqa: E402

from mmlf_amd import scenes  # noqa: E402

pytestmark = pytest.mark.gpu

# beside the golden shapes: a one-tile-row frame with a ragged last tile, several tiles both ways, the window sizes at which
# the row walk changes (1 and 3: no row shared by all four pixels of a lane; 5: the first that has one), the last window
# that fits 64 KB of LDS (41) and the first that does not (43), the largest window, and one full frame
MAE_SHAPES = [s[:4] for s in refs.GOLDEN_SHAPES] + [
    (1, 24, 47, 23), (1, 70, 150, 23), (1, 9, 11, 1), (2, 33, 35, 1), (1, 33, 45, 41), (1, 33, 45, 43), (1, 40, 70, 63),
    (1, 512, 512, 23)]


@pytest.fixture(scope='module')
def g15():
    return np.load(os.path.join(HERE, 'golden', 'g15_texture_mask.npz'))


def dev_centre(B, H, W, **kw):
    return torch.from_numpy(refs.centre(B, H, W, **kw)).cuda()


@pytest.mark.parametrize('shape', MAE_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_texture_mae_against_float64(shape):
    B, H, W, wsize = shape
    c = dev_centre(B, H, W)
    mae = scenes.texture_mae(c, wsize)
    assert mae.is_cuda and mae.dtype == torch.float32
    refs.check_mae(mae, c, wsize, 'x'.join(map(str, shape)))
    if wsize == 1:
        assert not mae.any()                                   # |c - c| of the pixel itself


@pytest.mark.parametrize('shape', refs.GOLDEN_SHAPES, ids=lambda s: 'x'.join(map(str, s[:4])))
def test_dyadic_centres_are_exact(g15, shape):
    B, H, W, wsize, thr = shape
    c = dev_centre(B, H, W, dyadic=True)
    s = refs.window_sum64(c, wsize).cpu().numpy()
    assert np.array_equal(s.astype(np.float32).astype(np.float64), s)
    mae = scenes.texture_mae(c, wsize).cpu().numpy()
    assert np.array_equal(mae, s.astype(np.float32) / np.float32(3 * wsize * wsize))
    mask = scenes.texture_mask(c, wsize, thr)
    assert mask.dtype == torch.int32
    assert np.array_equal(mask.cpu().numpy(), g15[refs.tag(B, H, W, wsize, 'dyadic')].astype(np.int32))


@pytest.mark.parametrize('shape', refs.GOLDEN_SHAPES, ids=lambda s: 'x'.join(map(str, s[:4])))
def test_float_centres_match_the_reference_outside_the_rounding_band(g15, shape):
    B, H, W, wsize, thr = shape
    c = dev_centre(B, H, W)
    golden = g15[refs.tag(B, H, W, wsize, 'float')].astype(np.int32)
    refs.check_mask_band(scenes.texture_mask(c, wsize, thr), golden, c, wsize, thr, refs.tag(B, H, W, wsize, 'float'))
    if H <= 2 * (wsize // 2) or W <= 2 * (wsize // 2):
        assert not scenes.texture_mask(c, wsize, thr).any()
        refs.check_mae(scenes.texture_mae(c, wsize), c, wsize, 'all margin')


def test_texture_semantics():
    from mmlf_amd import _lib
    from mmlf_amd._lib import ptr
    H, W, wsize = 45, 70, 5                                    # 2 x 3 tiles, ragged both ways
    c = dev_centre(2, H, W, seed=3)
    inner = torch.from_numpy(refs.interior(H, W, wsize)).cuda()
    ones = inner.to(torch.int32).expand(2, H, W)
    assert torch.equal(scenes.texture_mask(c, wsize, 0.0), ones)
    assert not scenes.texture_mask(c, wsize, 1e30).any()
    plain = scenes.texture_mask(c, wsize, 0.02)
    assert 0 < int(plain.sum()) < int(ones.sum())
    m_in = torch.from_numpy(np.random.RandomState(1).randint(0, 3, size=(2, H, W)).astype(np.int32)).cuda()
    both = scenes.texture_mask(c, wsize, 0.02, m_in)
    assert torch.equal(both, plain * m_in) and int(both.max()) == 2
    # both outputs of one launch are those of the two single-output launches
    mae = scenes.texture_mae(c, wsize)
    mae2, mask2 = torch.empty_like(mae), torch.empty_like(plain)
    _lib.call_scene('mmlf_scene_texture', ptr(c), wsize, 0.02, None, ptr(mask2), ptr(mae2), 2, H, W, _lib.stream_ptr())
    assert torch.equal(mae2, mae) and torch.equal(mask2, plain)
    # a NaN zeroes exactly the pixels whose window holds it (one across a tile edge, one at the frame's corner)
    cn = c.clone()
    cn[0, 1, 31, 33] = float('nan')
    cn[1, 2, 0, 0] = float('nan')
    hit = torch.zeros((2, H, W), dtype=torch.bool, device='cuda')
    hit[0, 29:34, 31:36] = True
    hit[1, 0:3, 0:3] = True
    assert torch.equal(scenes.texture_mask(cn, wsize, 0.0), (inner & ~hit).to(torch.int32))
    assert torch.equal(torch.isnan(scenes.texture_mae(cn, wsize)), hit)
    # refused before any launch: the Python check, and the library's own
    for bad in (0, 4, 22, 64, 65):
        with pytest.raises(ValueError):
            scenes.texture_mask(c, bad)
    with pytest.raises(RuntimeError, match='even wsize'):
        _lib.call_scene('mmlf_scene_texture', ptr(c), 4, 0.02, None, ptr(mask2), None, 2, H, W, _lib.stream_ptr())
    with pytest.raises(RuntimeError, match='neither'):
        _lib.call_scene('mmlf_scene_texture', ptr(c), 5, 0.02, None, None, None, 2, H, W, _lib.stream_ptr())
    with pytest.raises(ValueError):
        scenes.texture_mask(c, wsize, 0.02, m_in.cpu())
    with pytest.raises(ValueError):
        scenes.texture_mask(c, wsize, 0.02, m_in[:1])
    with pytest.raises(ValueError):
        scenes.texture_mask(c.permute(0, 1, 3, 2), wsize, 0.02, m_in)
    torch.cuda.synchronize()
    assert torch.equal(mask2, plain)                           # (nothing was launched on the refused calls)


@pytest.mark.parametrize('nviews,H,W', [((3, 3), 5, 7), ((9, 9), 16, 24), ((3, 3), 3, 300)])
def test_pack_views_is_a_gather_and_a_table(nviews, H, W):
    sel = np.array(scenes.view_indices(nviews))
    V = sel.shape[1]
    lut = scenes.uint8_table()
    assert np.array_equal(lut, (np.arange(256).astype(np.float64) * (1 / 255)).astype(np.float32))
    for dtype in (np.uint8, np.float32):
        views = refs.scene_inputs(nviews, H, W, 2, dtype)[0]
        slot = V + V // 2
        stacks, center = scenes.pack_views(views, sel, slot, 'cuda')
        as_float = lut[views] if dtype == np.uint8 else views
        expect = as_float[sel.reshape(-1)].transpose(0, 3, 1, 2).reshape(4, V, 3, H, W)
        assert stacks.is_cuda and stacks.dtype == torch.float32
        assert np.array_equal(stacks.cpu().numpy(), expect)
        assert np.array_equal(center.cpu().numpy(), expect[1, V // 2])
        cpu_stacks, cpu_center = scenes.pack_views(views, sel, slot, 'cpu')
        assert np.array_equal(cpu_stacks.numpy(), expect) and np.array_equal(cpu_center.numpy(), expect[1, V // 2])
        # a device tensor goes in as it is
        again, _ = scenes.pack_views(torch.from_numpy(views).cuda(), sel, 0, 'cuda')
        assert torch.equal(again, stacks)
    bad = sel.copy()
    bad[2, 1] = nviews[0] * nviews[1]
    with pytest.raises(ValueError):
        scenes.pack_views(views, bad, 0, 'cuda')
    bad[2, 1] = -1
    with pytest.raises(ValueError):
        scenes.pack_views(views, bad, 0, 'cuda')
    with pytest.raises(ValueError):
        scenes.pack_views(views, sel, 4 * V, 'cuda')


@pytest.mark.parametrize('case', refs.ASSEMBLE_CASES, ids=refs.case_id)
def test_assemble_scene_on_the_device_matches_the_cpu_path(case):
    _, cpu = refs.assemble_case(scenes.assemble_scene, case, 'cpu')
    _, gpu = refs.assemble_case(scenes.assemble_scene, case, 'cuda')
    assert all(t.is_cuda for t in gpu)
    assert [t.dtype for t in gpu] == [t.dtype for t in cpu]
    for k in (0, 1, 2, 3, 4, 5, 6, 8):
        assert torch.equal(gpu[k].cpu(), cpu[k]), k
    # the mask: the band rule around the texture threshold, times the same scene mask on both sides
    center = cpu[4].unsqueeze(0)
    refs.check_mask_band(gpu[7].cpu().unsqueeze(0), cpu[7].unsqueeze(0).numpy(), center, 5, 0.02, refs.case_id(case))


def test_patch_pipeline_takes_device_scenes():
    from mmlf_amd import patches, transforms as T
    H, W, ps, nviews = 48, 56, 8, (3, 3)
    dev_scenes = []
    for seed in (1, 2):
        views, gt, mpi, mask = refs.scene_inputs(nviews, H, W, seed)
        dev_scenes.append(scenes.assemble_scene(views, gt, mpi, mask, index=seed, nviews=nviews, wsize=5))
    assert all(t.is_cuda for s in dev_scenes for t in s)
    assert 0 < int(dev_scenes[0][7].sum()) < H * W
    np_scenes = [tuple(t.cpu().numpy() for t in s) for s in dev_scenes]
    half_cpu = [tuple(t.cpu() if k % 2 else t for k, t in enumerate(s)) for s in dev_scenes]
    chain = [T.DownSampling(2), T.RandomShift(1.0), T.RandomCrop(ps), T.RandomRotate(), T.RedistColor(), T.Brightness(0.3),
             T.Contrast(0.5), T.Noise(0.01)]
    for kw in (dict(max_downscale=1), dict(chain=chain, noise_seed=3)):
        outs = []
        for sc in (np_scenes, dev_scenes, half_cpu):
            pipe = patches.PatchPipeline(sc, ps, **kw)
            random.seed(11)
            outs.append(pipe.sample([0, 1, 1, 0, 1]))
        for other in outs[1:]:
            for k, (a, b) in enumerate(zip(outs[0], other)):
                assert a.dtype == b.dtype and torch.equal(a.cpu(), b.cpu()), (list(kw), k)
        assert outs[0][0].shape == (5, 3, 3, ps, ps) and outs[0][7].dtype == torch.int32
        assert outs[0][8].tolist() == [[1], [2], [2], [1], [2]]
    # the cached scenes are copies: sampling and the pre-shift never write into the caller's tensors
    before = [t.clone() for t in dev_scenes[0]]
    patches.PatchPipeline(dev_scenes, ps, max_downscale=1, train_shift=0.5).sample([0, 1])
    assert all(torch.equal(a, b) for a, b in zip(before, dev_scenes[0]))
    assert 'libmmlf_scene_hip.so' in open('/proc/self/maps').read()
