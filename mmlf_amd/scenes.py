"""Cached training scenes from decoded view images.

``PatchPipeline`` and ``TrainStep`` start from the scene tuple ``(h, v, i, d, center, gt, mpi, mask, index)`` of the
reference's ``HCI4D.load_scene`` (mmlf/data/hci4d.py:124-254).  Apart from reading files that loader picks the four view
stacks out of the camera grid, converts them to float CHW, cuts the centre view, fixes up or synthesises the multi-plane
target and multiplies the scene's mask by ``create_mask_texture(center, 23, 0.02)`` (hci4d.py:38-69, 241): the pixels the
training loss is taken over.  This module is that arithmetic: decoded images in, the scene on the device out.

On CUDA tensors the stacks and the texture mask are kernels of libmmlf_scene_hip.so (include/mmlf_scene_hip.h), with no
fallback; on the CPU the same functions run in plain torch / numpy, accumulating over the window offsets (the reference's
``unfold`` would materialise 3 * wsize^2 * H * W floats, 1.66 GB for one 512 x 512 scene).
"""
import os

import numpy as np
import torch

from . import _lib
from ._lib import ptr


def view_indices(nviews=(9, 9)):
    """(us, vs, ids, dds): the grid images behind the horizontal, vertical, rising and falling diagonal stacks
    (hci4d.py:141-149; all four ranges run over `h`, the rising diagonal is reversed)."""
    w, h = nviews
    us = [int(h / 2) * w + i for i in range(h)]
    vs = [int(w / 2) + w * i for i in range(h)]
    ids = [w - i - 1 + w * i for i in range(h)]
    ids.reverse()
    dds = [i + w * i for i in range(h)]
    return us, vs, ids, dds


def uint8_table():
    """the float32 behind every uint8 image value: float32(float64(x) * (1 / 255))"""
    return (np.arange(256, dtype=np.float64) * (1.0 / 255)).astype(np.float32)


def _check_wsize(wsize):
    wsize = int(wsize)
    if not 1 <= wsize <= _lib.SCENE_MAX_WSIZE or wsize % 2 == 0:
        raise ValueError(f'texture window: wsize {wsize} must be odd and in [1, {_lib.SCENE_MAX_WSIZE}] '
                         '(the reference\'s `view` fails on an even size)')
    return wsize


def _as_center(center):
    if not isinstance(center, torch.Tensor):
        center = torch.from_numpy(np.ascontiguousarray(center))
    if center.dim() != 4 or center.shape[1] != 3 or center.dtype != torch.float32:
        raise ValueError(f'texture window: center must be float32 (B,3,H,W), found {center.dtype} {tuple(center.shape)}')
    return center


def _texture_cpu(center, wsize):
    """float32 sum over the window offsets in the kernel's order (channel, window row, left to right), then one division"""
    B, _, H, W = center.shape
    R = wsize // 2
    pad = torch.nn.functional.pad(center, (R, R, R, R))
    acc = torch.zeros((B, H, W), dtype=torch.float32)
    for ch in range(3):
        c = center[:, ch]
        for dy in range(wsize):
            for dx in range(wsize):
                acc += (pad[:, ch, dy:dy + H, dx:dx + W] - c).abs_()
    return acc / torch.tensor(float(3 * wsize * wsize), dtype=torch.float32)


def _texture(center, wsize, threshold, mask, want_mae, want_mask):
    center = _as_center(center)
    wsize = _check_wsize(wsize)
    B, _, H, W = center.shape
    dev = center.device
    if mask is not None:
        _lib.check(mask, 'texture_mask: mask', dev, torch.int32, (B, H, W))
    if dev.type != 'cuda':
        center = center.contiguous()
        mae = _texture_cpu(center, wsize)
        out = None
        if want_mask:
            R = wsize // 2
            out = (mae >= torch.tensor(float(threshold), dtype=torch.float32)).to(torch.int32)
            if R > 0:
                out[:, :R] = 0
                out[:, max(H - R, 0):] = 0
                out[:, :, :R] = 0
                out[:, :, max(W - R, 0):] = 0
            if mask is not None:
                out = out * mask
        return (mae if want_mae else None), out
    _lib.check(center, 'texture_mask: center', dev, torch.float32, (B, 3, H, W))
    mae = torch.empty((B, H, W), dtype=torch.float32, device=dev) if want_mae else None
    out = torch.empty((B, H, W), dtype=torch.int32, device=dev) if want_mask else None
    with torch.cuda.device(dev):
        _lib.call_scene('mmlf_scene_texture', ptr(center), wsize, float(threshold), ptr(mask), ptr(out), ptr(mae), B, H, W,
                        _lib.stream_ptr())
    return mae, out


def texture_mae(center, wsize=23):
    """float32 (B,H,W): the mean L1 distance of every pixel of `center` (B,3,H,W) to the 3 * wsize^2 values of its
    zero-padded window (hci4d.py:57-61), as a float32 sum divided once by float32(3 * wsize^2)."""
    return _texture(center, wsize, 0.0, None, True, False)[0]


def texture_mask(center, wsize=23, threshold=0.02, mask=None):
    """int32 (B,H,W): hci4d.create_mask_texture(center, wsize, threshold) -- texture_mae >= float32(threshold), zero in
    the wsize // 2 margin -- times `mask` (int32 (B,H,W)) where given."""
    return _texture(center, wsize, threshold, mask, False, True)[1]


def pack_views(views, sel, center_slot, device='cuda'):
    """(stacks (4,V,3,H,W), center (3,H,W)) float32 on `device` from `views` (N,H,W,3), uint8 (through uint8_table) or
    float32, numpy or tensor: stacks[s][k] is image sel[s][k], center is the image of slot `center_slot` of the
    flattened `sel`.  Every entry of `sel` is held to [0, N) here, on the host, ahead of the launch."""
    dev = torch.device(device)
    if not isinstance(views, torch.Tensor):
        views = torch.from_numpy(np.ascontiguousarray(views))
    if views.dim() != 4 or views.shape[3] != 3 or views.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f'pack_views: views must be uint8 or float32 (N,H,W,3), found {views.dtype} {tuple(views.shape)}')
    N, H, W, _ = views.shape
    sel = np.ascontiguousarray(sel, dtype=np.int64)
    if sel.ndim != 2 or sel.shape[0] != 4 or sel.shape[1] < 1:
        raise ValueError(f'pack_views: sel must be (4, V), found {sel.shape}')
    V = sel.shape[1]
    if sel.min() < 0 or sel.max() >= N:
        raise ValueError(f'pack_views: sel names image {int(sel.min() if sel.min() < 0 else sel.max())} of {N}')
    center_slot = int(center_slot)
    if not 0 <= center_slot < 4 * V:
        raise ValueError(f'pack_views: center_slot {center_slot} not in [0, {4 * V})')
    views = views.to(dev)
    if dev.type != 'cuda':
        flat = torch.from_numpy(sel.reshape(-1))
        picked = views[flat]
        if views.dtype == torch.uint8:
            picked = torch.from_numpy(uint8_table())[picked.long()]
        stacks = picked.permute(0, 3, 1, 2).reshape(4, V, 3, H, W).contiguous()
        return stacks, stacks.reshape(4 * V, 3, H, W)[center_slot].clone()
    is_u8 = views.dtype == torch.uint8
    _lib.check(views, 'pack_views: views', views.device, views.dtype, (N, H, W, 3))
    lut = torch.from_numpy(uint8_table()).to(views.device)
    sel_d = torch.from_numpy(sel.reshape(-1).astype(np.int32)).to(views.device)
    stacks = torch.empty((4, V, 3, H, W), dtype=torch.float32, device=views.device)
    center = torch.empty((3, H, W), dtype=torch.float32, device=views.device)
    with torch.cuda.device(views.device):
        _lib.call_scene('mmlf_scene_pack_views', ptr(views) if is_u8 else None, None if is_u8 else ptr(views), ptr(lut),
                        ptr(sel_d), center_slot, N, V, H, W, ptr(stacks), ptr(center), _lib.stream_ptr())
    return stacks, center


def assemble_scene(views, gt=None, mpi=None, mask=None, index=0, nviews=(9, 9), wsize=23, threshold=0.02, device='cuda'):
    """The arithmetic of HCI4D.load_scene after file decoding: (h, v, i, d, center, gt, mpi, mask, index) as tensors on
    `device` -- stacks (V,3,H,W), center (3,H,W), gt (H,W) and mpi (P,5,H,W) float32, mask (H,W) int32, index int64 (1,).

    views: (N,H,W,3) uint8 or float32 in sorted-file order; the centre is view h // 2 of the vertical stack.
    gt:    (H,W), already flipped by the caller (hci4d.py:212); None gives zeros.
    mpi:   (H,W,P,5) as gt_mpi_lowres.npz holds it: rows flipped, (P,5,H,W), NaN -> 0, at most 12 planes
           (hci4d.py:215-221); None gives the one-plane target made from centre and gt (:224-227).
    mask:  (H,W); (mask > 0) times texture_mask(center, wsize, threshold); None gives ones (hci4d.py:233-241)."""
    dev = torch.device(device)
    w, h = nviews
    sel = np.array(view_indices(nviews), dtype=np.int64)
    stacks, center = pack_views(views, sel, 1 * h + int(h / 2), dev)
    dev = stacks.device
    H, W = center.shape[1:]

    def on_dev(a, name, shape):
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
        if tuple(t.shape[:len(shape)]) != tuple(shape):
            raise ValueError(f'assemble_scene: {name} {tuple(t.shape)} does not fit the {H} x {W} frame')
        return t.to(dev)

    if gt is None:
        gt_t = torch.zeros((H, W), dtype=torch.float32, device=dev)
    else:
        gt_t = on_dev(gt, 'gt', (H, W)).to(torch.float32).contiguous()
    if mpi is None:
        mpi_t = torch.empty((1, 5, H, W), dtype=torch.float32, device=dev)
        mpi_t[0, :3] = center
        mpi_t[0, 3] = 1.0
        mpi_t[0, 4] = gt_t
    else:
        mpi_t = on_dev(mpi, 'mpi', (H, W))
        if mpi_t.dim() != 4 or mpi_t.shape[3] != 5:
            raise ValueError(f'assemble_scene: mpi must be (H,W,P,5), found {tuple(mpi_t.shape)}')
        mpi_t = mpi_t.to(torch.float32).flip(0).permute(2, 3, 0, 1)[:12]
        mpi_t = torch.where(torch.isnan(mpi_t), torch.zeros((), dtype=torch.float32, device=dev), mpi_t).contiguous()
    if mask is None:
        mask_t = torch.ones((1, H, W), dtype=torch.int32, device=dev)
    else:
        mask_t = (on_dev(mask, 'mask', (H, W)) > 0).to(torch.int32).reshape(1, H, W).contiguous()
    mask_t = texture_mask(center.unsqueeze(0), wsize, threshold, mask_t)[0]
    index_t = torch.from_numpy(np.atleast_1d(index).astype(np.int64)).to(dev)
    return stacks[0], stacks[1], stacks[2], stacks[3], center, gt_t, mpi_t, mask_t, index_t


def load_scene_dir(scene_dir, index=0, nviews=(9, 9), device='cuda'):
    """One scene directory of the 4D light field benchmark through assemble_scene: the view images by the file filter and
    sort of hci4d.py:134-139, the disparity .pfm chosen as in :196-212, gt_mpi_lowres.npz and mask.png where present."""
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError('load_scene_dir decodes the view images with Pillow, which is not installed; decode them '
                           'yourself and call assemble_scene') from e
    from . import pfm
    files = [f.name for f in os.scandir(scene_dir)]
    skip = ('normals', 'mask', 'objectids', 'unused', 'edges', 'specular')
    imgs = sorted(f for f in files if f.endswith(('.png', '.jpg', '.jpeg')) and not any(s in f for s in skip))
    w, h = nviews
    us = view_indices(nviews)[0]
    if len(imgs) <= max(max(s) for s in view_indices(nviews)):
        raise ValueError(f'{scene_dir}: {len(imgs)} view images, the {w} x {h} grid needs more')

    def decode(name):
        img = Image.open(os.path.join(scene_dir, name))
        a = np.asarray(img)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
            a = np.asarray(img.convert('RGB'))
        return a

    views = np.stack([decode(f) for f in imgs])
    pfms = [f for f in files if f.endswith('.pfm')]
    if len(pfms) > 1:
        pfms = [f for f in pfms if 'disp' in f]
    if len(pfms) > 1:
        pfms = [f for f in pfms if 'lowres' in f]
    if len(pfms) > 1:
        pfms = [f for f in pfms if str(us[int(w / 2)]).zfill(3) in f]
    gt = np.flip(pfm.load(os.path.join(scene_dir, pfms[0])), 0).copy() if pfms else None
    mpi = np.load(os.path.join(scene_dir, 'gt_mpi_lowres.npz'))['mpi'] if 'gt_mpi_lowres.npz' in files else None
    mask = None
    if os.path.exists(os.path.join(scene_dir, 'mask.png')):
        mask = np.asarray(Image.open(os.path.join(scene_dir, 'mask.png')))
        mask = mask[:, :, 0] if mask.ndim == 3 else mask
    return assemble_scene(views, gt, mpi, mask, index, nviews, device=device)


def as_batch(scene):
    """the scene tuple with a batch axis of one on every entry: the shape validate_scenes takes"""
    return tuple(t.unsqueeze(0) for t in scene)
