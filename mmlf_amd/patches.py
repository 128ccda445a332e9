"""On-device training patch pipeline.

The reference produces a training sample on the CPU: ``HCI4D.__getitem__`` deep-copies a cached
512x512 scene and runs the transform chain of mmlf/train/cli.py:72-94 over the whole frame
(mmlf/data/hci4d.py:289-291) -- RandomDownSampling, RandomShift(1.0), RandomCrop(ps+16),
CenterCrop(ps), RandomRotate, RedistColor, Brightness, Contrast -- in 4 DataLoader workers.  At
several hundred patches/s per GPU that is the bottleneck.  Here the scenes stay in HBM and a batch is ONE
fused gather (mmlf_patch_gather) plus the Contrast pass (mmlf_patch_contrast): only the ps x ps output
pixels are computed.

Random parameters are drawn on the host from Python's ``random`` module in exactly the reference's call
order, so with the same seed a sample is the reference's sample (float tolerance: the Contrast mean is
summed in double here, pairwise float32 in numpy).

``PatchPipeline(chain=[...])`` runs any list of ``mmlf_amd.transforms`` objects that fits the slot order there (Zoom,
IntegerShift, Noise and other parameters than the CLI's included) through libmmlf_data_hip.so: mmlf_data_gather reads the
scaled frame through per-sample index tables, mmlf_data_finish applies Contrast and Noise.
"""
import random as _random

import numpy as np
import torch

from . import _lib
from . import transforms as T
from ._lib import call, ptr
from .ensamble import shift_table

FLAG_SHIFT, FLAG_COLOR, FLAG_BRIGHT = 1, 2, 4


def rotation_sources(views):
    """rot_src[r][stack][view] = source stack*views + source view after r x Rotate90
    (hci4d.py:1063-1069: new H = old V, new V = old H with the view order flipped; I/D likewise)."""
    lab = [[(s, n) for n in range(views)] for s in range(4)]
    tabs = []
    for _ in range(4):
        tabs.append([[s * views + n for (s, n) in row] for row in lab])
        lab = [lab[1], lab[0][::-1], lab[3], lab[2][::-1]]
    return np.asarray(tabs, dtype=np.int32)


def draw_sample(frame_hw, ps, max_downscale=4, augment=True, rng=None):
    """The random draws of one sample in the reference's order (train/cli.py:79-88 and the transforms'
    __call__ bodies).  Returns a dict of plain numbers."""
    rng = rng or _random
    H, W = frame_hw
    p = dict(f=1, disp=0.0, rot=0, mat=np.eye(3), bright=1.0, contrast=1.0, augment=bool(augment))
    if augment:
        p['f'] = rng.randint(1, max_downscale)                   # RandomDownSampling, hci4d.py:526
        p['disp'] = rng.uniform(-1.0, 1.0)                       # RandomShift(1.0), hci4d.py:1024
    big = ps + 2 * 4 * 2
    h, w = -(-H // p['f']), -(-W // p['f'])                      # frame[..., ::f, ::f]
    if not (h > big and w > big):
        raise ValueError(f'frame {h}x{w} after downsampling by {p["f"]} is not larger than the {big}-px crop '
                         '(hci4d.py:656-657)')
    y = rng.randint(0, h - big)                                  # RandomCrop, hci4d.py:659-660
    x = rng.randint(0, w - big)
    off = int((big - ps) / 2)                                    # CenterCrop, hci4d.py:617-618
    p['y0'], p['x0'] = y + off, x + off
    if augment:
        p['rot'] = rng.randint(0, 3)                             # RandomRotate, hci4d.py:1082
        mat = np.zeros((3, 3))                                   # RedistColor, hci4d.py:687-697
        mat[0, 0] = rng.uniform(0.0, 1.0)
        mat[0, 1] = rng.uniform(0.0, 1.0 - mat[0, 0])
        mat[1, 0] = rng.uniform(0.0, 1.0 - mat[0, 0])
        mat[1, 1] = rng.uniform(0.0, 1.0 - max(mat[0, 1], mat[1, 0]))
        mat[0, 2] = 1.0 - mat[0, 0] - mat[0, 1]
        mat[1, 2] = 1.0 - mat[1, 0] - mat[1, 1]
        mat[2, 0] = 1.0 - mat[0, 0] - mat[1, 0]
        mat[2, 1] = 1.0 - mat[0, 1] - mat[1, 1]
        mat[2, 2] = mat[0, 0] + mat[0, 1] + mat[1, 0] + mat[1, 1] - 1.0
        p['mat'] = mat
        p['bright'] = rng.uniform(-0.9, 0.9) + 1.0               # Brightness(), hci4d.py:773
        p['contrast'] = rng.uniform(-0.9, 0.9) + 1.0             # Contrast(), hci4d.py:740
    return p


def cli_chain(ps, max_downscale=4, augment=True):
    """The transform list train/cli.py:72-88 composes, as ``PatchPipeline(chain=...)`` takes it (the fixed pre-shift of
    :89-90 stays the pipeline's ``train_shift=``)."""
    crops = [T.RandomCrop(ps + 2 * 4 * 2), T.CenterCrop(ps)]
    if not augment:
        return crops
    return [T.RandomDownSampling(max_downscale), T.RandomShift(1.0), *crops, T.RandomRotate(), T.RedistColor(),
            T.Brightness(), T.Contrast()]


def validate_chain(chain, ps):
    """Hold a transform list to the slot order of mmlf_amd/transforms.py; returns {slot: transform}.  ValueError names the
    offending element."""
    plan, last = {}, -1
    for k, tf in enumerate(chain):
        if not isinstance(tf, T.Transform) or tf.slot not in T.SLOTS:
            raise ValueError(f'chain[{k}] = {tf!r} is not one of the transforms of mmlf_amd.transforms')
        at = T.SLOTS.index(tf.slot)
        if tf.slot in plan:
            raise ValueError(f'chain[{k}] = {tf!r}: the {tf.slot} slot is already taken by {plan[tf.slot]!r}')
        if at < last:
            raise ValueError(f'chain[{k}] = {tf!r} cannot follow {chain[k - 1]!r}: the order is ' + ' '.join(T.SLOTS))
        plan[tf.slot], last = tf, at
    if 'crop' not in plan:
        raise ValueError(f'the chain {list(chain)!r} has no RandomCrop: the pipeline produces patches')
    for slot in ('crop', 'center'):
        if slot in plan and plan[slot].size[0] != plan[slot].size[1]:
            raise ValueError(f'{plan[slot]!r}: tuple sizes are not supported, the patch is square')
    final = plan.get('center', plan['crop'])
    if final.size[0] != ps:
        raise ValueError(f'{final!r}: the last crop must have the pipeline\'s patch size {ps}')
    if 'center' in plan and plan['center'].size[0] > plan['crop'].size[0]:
        raise ValueError(f'{plan["center"]!r} is larger than {plan["crop"]!r} (hci4d.py:613)')
    return plan


def draw_chain_sample(plan, frame_hw, views, rng=None):
    """draw_sample's sibling for a validated chain: the draws of one sample from Python's ``random`` stream in the order
    the reference's transforms would take them (scale, shear, crop y then x, rotation, colour matrix, brightness,
    contrast; Noise takes none), and what follows from them on the host.  Returns a dict of plain numbers:
    hs, ws (the scaled frame), down | zoom, disp | idisp, y0, x0, rot, mat, bright, contrast (absent slots: None)."""
    rng = rng or _random
    H, W = frame_hw
    p = dict(down=None, zoom=None, disp=None, idisp=None, rot=0, mat=None, bright=None, contrast=None)
    for slot in ('scale', 'shear'):
        if slot in plan:
            p.update(plan[slot].draw(rng))
    if p['down'] is not None:
        h, w = -(-H // p['down']), -(-W // p['down'])                # frame[..., ::f, ::f]
    elif p['zoom'] is not None:
        h, w = T.zoom_size(H, p['zoom']), T.zoom_size(W, p['zoom'])
    else:
        h, w = H, W
    p['hs'], p['ws'] = h, w
    if p['idisp'] is not None and not abs(p['idisp']) * (views // 2) < min(h, w):
        raise ValueError(f'{plan["shear"]!r} rolls the outer views by {abs(p["idisp"]) * (views // 2)} px, '
                         f'not less than the {h}x{w} frame')
    crop = plan['crop']
    n, pad = crop.size[0], crop.pad
    if not (h > n and w > n):
        raise ValueError(f'frame {h}x{w} after scaling is not larger than the {n}-px crop (hci4d.py:656-657)')
    if h - n - pad < pad or w - n - pad < pad:
        raise ValueError(f'{crop!r} leaves no position in a {h}x{w} frame (hci4d.py:659-660)')
    y = rng.randint(pad, h - n - pad)                                # RandomCrop, hci4d.py:659-660
    x = rng.randint(pad, w - n - pad)
    off = int((n - plan['center'].size[0]) / 2) if 'center' in plan else 0      # CenterCrop, hci4d.py:610-611
    p['y0'], p['x0'] = y + off, x + off
    for slot in ('rotate', 'color', 'brightness', 'contrast'):
        if slot in plan:
            p.update(plan[slot].draw(rng))
    return p


def integer_shift_table(disp, views):
    """IntegerShift's roll per view, disp * (view - views // 2) (hci4d.py:857-861), in shift_table's layout: one tap"""
    tab_s = np.zeros((views, 2), np.int32)
    tab_s[:, 0] = tab_s[:, 1] = disp * (np.arange(views) - int(views / 2))
    tab_w = np.zeros((views, 2), np.float32)
    tab_w[:, 0] = 1.0
    return tab_s, tab_w


def index_maps(p, frame_hw, cache):
    """(ymap, xmap) of one sample: the cached frame's row / column behind every row / column of the scaled frame (-1:
    scipy.ndimage.zoom's constant, transforms.zoom_map says where).  They depend on the scaled extents alone, so the few
    a chain can draw are kept in `cache`."""
    Hf, Wf = frame_hw
    key = ('down', p['down']) if p['down'] is not None else ('zoom', p['hs'], p['ws']) if p['zoom'] is not None else ()
    maps = cache.get(key)
    if maps is None:
        if p['down'] is not None:
            maps = T.down_map(Hf, p['down']), T.down_map(Wf, p['down'])
        elif p['zoom'] is not None:
            maps = T.zoom_map(Hf, p['hs']), T.zoom_map(Wf, p['ws'])
        else:
            maps = np.arange(Hf, dtype=np.int32), np.arange(Wf, dtype=np.int32)
        if not (len(maps[0]) == p['hs'] and len(maps[1]) == p['ws'] and -1 <= maps[0].min() and maps[0].max() < Hf
                and -1 <= maps[1].min() and maps[1].max() < Wf):
            raise AssertionError(f'index tables {key} do not fit the {p["hs"]}x{p["ws"]} frame scaled from {Hf}x{Wf}')
        if len(cache) < 4096:
            cache[key] = maps
    return maps


def pack_chain_params(draws, scene_ids, frame_hw, views, ps, cache):
    """What mmlf_data_gather / mmlf_data_finish read per sample, in ONE host buffer (one copy to the device): returns
    (uint8 buffer, {name: byte offset}, map_h, map_w) with the sections mat (B,9) float64, ip (B,8) int32, fp (B,4) and
    alpha (B,2) float32, tab_s / tab_w (B,views,2), ymap (B,map_h) and xmap (B,map_w) int32, each 8-byte aligned."""
    F, B, V = _lib.DATA_FLAGS, len(draws), views
    map_h, map_w = max(p['hs'] for p in draws), max(p['ws'] for p in draws)
    sizes = (('mat', np.float64, 9), ('ip', np.int32, 8), ('fp', np.float32, 4), ('alpha', np.float32, 2),
             ('tab_s', np.int32, 2 * V), ('tab_w', np.float32, 2 * V), ('ymap', np.int32, map_h), ('xmap', np.int32, map_w))
    offs, total = {}, 0
    for name, dt, n in sizes:
        offs[name] = total
        total += -(-B * n * np.dtype(dt).itemsize // 8) * 8
    buf = np.zeros(total, np.uint8)
    host = {name: buf[offs[name]:offs[name] + B * n * np.dtype(dt).itemsize].view(dt).reshape(B, n) for name, dt, n in sizes}
    ip, fp, alpha, mat = [], [], [], []
    for sc, p in zip(scene_ids, draws):
        flags, gscale, disp = 0, 1.0, 0.0
        if p['down'] is not None:
            flags, gscale = flags | F['GT_DIV'], float(p['down'])
        elif p['zoom'] is not None:
            flags, gscale = flags | F['GT_MUL'], float(p['zoom'])
        if p['disp'] is not None:
            flags, disp = flags | F['SHEAR'], p['disp']
        elif p['idisp'] is not None:
            flags, disp = flags | F['ROLL'], float(p['idisp'])
        if p['mat'] is not None:
            flags |= F['COLOR']
            mat.append(p['mat'])
        if p['bright'] is not None:
            flags |= F['BRIGHT']
        if p['contrast'] is not None:
            alpha.append((p['contrast'], 1.0 - p['contrast']))
        if not (0 <= p['y0'] and p['y0'] + ps <= p['hs'] and 0 <= p['x0'] and p['x0'] + ps <= p['ws']):
            raise AssertionError(f'crop {p["y0"]},{p["x0"]} + {ps} outside the {p["hs"]}x{p["ws"]} frame')
        ip.append((sc, p['hs'], p['ws'], p['y0'], p['x0'], p['rot'], flags, 0))
        fp.append((gscale, disp, 1.0 if p['bright'] is None else p['bright'], 0.0))
    host['ip'][:], host['fp'][:] = ip, fp
    if mat:                                             # (a slot is taken by every sample or by none)
        host['mat'][:] = np.asarray(mat).reshape(B, 9)
    if alpha:
        host['alpha'][:] = alpha
    if draws[0]['disp'] is not None:
        tab_s, tab_w = shift_table([p['disp'] for p in draws], V)
        host['tab_s'][:], host['tab_w'][:] = tab_s.reshape(B, -1), tab_w.reshape(B, -1)
    elif draws[0]['idisp'] is not None:
        tab_s, tab_w = integer_shift_table(draws[0]['idisp'], V)
        host['tab_s'][:], host['tab_w'][:] = tab_s.reshape(-1), tab_w.reshape(-1)
    rows = {}                                           # samples by scaled extents: a chain draws few distinct tables
    for b, p in enumerate(draws):
        rows.setdefault((p['down'], p['hs'], p['ws']), []).append(b)
    for (_, hs, ws), bs in rows.items():
        ym, xm = index_maps(draws[bs[0]], frame_hw, cache)
        host['ymap'][bs, :hs], host['xmap'][bs, :ws] = ym, xm
    return buf, offs, map_h, map_w


class PatchPipeline:
    """Scenes cached on the GPU + the fused transform chain.

    scenes: list of tuples (h, v, i, d, center, gt, mpi, mask, index) as ``HCI4D.load_scene`` returns
    them (hci4d.py:150-254), all of one frame size: numpy arrays, or torch tensors on the CPU or already on ``device``
    (``mmlf_amd.scenes.assemble_scene``; a device tensor makes no host round trip).  ``train_shift`` is the CLI's fixed pre-shift
    (train/cli.py:93-94), applied once to the cached scenes.

    ``chain``: None runs the CLI's chain with its three knobs (``max_downscale``, ``augment``, ``train_shift``).  A list
    of ``mmlf_amd.transforms`` objects runs that chain instead (``max_downscale`` and ``augment`` are then not used),
    through libmmlf_data_hip.so; ``noise_seed`` keys the generator behind ``Noise`` together with the number of
    ``sample()`` calls made so far.
    """

    def __init__(self, scenes, ps, max_downscale=4, augment=True, train_shift=0.0, device='cuda', chain=None, noise_seed=0):
        if not torch.cuda.is_available():
            raise RuntimeError('PatchPipeline needs the HIP library and an MI355X; use the reference '
                               'DataLoader path on CPU')
        _lib.load()
        self.plan = None
        if chain is not None:
            self.plan = validate_chain(list(chain), int(ps))
            _lib.load_data()
        self.noise_seed, self.calls = int(noise_seed) & (2 ** 63 - 1), 0
        self._maps = {}
        self.ps, self.max_downscale, self.augment = int(ps), int(max_downscale), bool(augment)
        dev = torch.device(device)

        def f32(a):          # a tensor (mmlf_amd.scenes.assemble_scene; CPU or already on `dev`) is taken as it is
            if isinstance(a, torch.Tensor):
                return a.detach().to(device=dev, dtype=torch.float32)
            return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)

        def i32(a):
            if isinstance(a, torch.Tensor):
                return a.detach().to(device=dev, dtype=torch.int32)
            return torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).to(dev)

        def host(a):
            return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
        self.stacks = torch.stack([torch.stack([f32(s[k]) for k in range(4)]) for s in scenes])  # (S,4,V,3,H,W)
        self.center = torch.stack([f32(s[4]) for s in scenes])
        self.gt = torch.stack([f32(s[5]) for s in scenes])
        self.mpi = torch.stack([f32(s[6]) for s in scenes])
        self.mask = torch.stack([i32(s[7]) for s in scenes])
        self.index = [np.atleast_1d(host(s[8])) for s in scenes]
        self.S, _, self.V, _, self.Hf, self.Wf = self.stacks.shape
        self.P = self.mpi.shape[1]
        self.rot_src = torch.from_numpy(rotation_sources(self.V)).to(dev)
        if train_shift != 0.0:
            self._preshift(float(train_shift))

    def _preshift(self, disp):
        """hci4d.Shift(train_shift) on every cached scene (stacks, gt, mpi[:, 4]; hci4d.py:907-990)."""
        tab_s, tab_w = shift_table([disp], self.V)
        dev = self.stacks.device
        ts, tw = torch.from_numpy(tab_s).to(dev), torch.from_numpy(tab_w).to(dev)
        out = torch.empty_like(self.stacks)
        for s in range(self.S):
            src, dst = self.stacks[s], out[s]
            call('mmlf_shift_views', ptr(src[0]), ptr(src[1]), ptr(src[2]), ptr(src[3]), ptr(dst[0]), ptr(dst[1]),
                 ptr(dst[2]), ptr(dst[3]), ptr(ts), ptr(tw), 1, self.V, self.Hf, self.Wf, _lib.stream_ptr())
        self.stacks = out
        self.gt = self.gt - np.float32(disp)
        self.mpi[:, :, 4] -= np.float32(disp)

    def sample(self, scene_indices, rng=None):
        """One batch: (h, v, i, d, center, gt, mpi, mask, index), batch-first like the collated output of
        the reference DataLoader (stacks (B,V,3,ps,ps), ...).  Draws come from `rng` (default: the
        ``random`` module), one sample after the other, in the reference's order."""
        if self.plan is not None:
            return self._sample_chain(scene_indices, rng)
        B, ps, V, dev = len(scene_indices), self.ps, self.V, self.stacks.device
        ip = np.zeros((B, 8), np.int32)
        fp = np.zeros((B, 4), np.float32)
        mat = np.zeros((B, 9), np.float64)
        alpha = np.zeros((B, 2), np.float32)
        disps = []
        for b, sc in enumerate(scene_indices):
            p = draw_sample((self.Hf, self.Wf), ps, self.max_downscale, self.augment, rng)
            flags = (FLAG_SHIFT | FLAG_COLOR | FLAG_BRIGHT) if self.augment else 0
            ip[b, :6] = (int(sc) % self.S, p['f'], p['y0'], p['x0'], p['rot'], flags)
            fp[b, :3] = (float(p['f']), p['disp'], p['bright'])
            mat[b] = p['mat'].reshape(-1)
            alpha[b] = (p['contrast'], 1.0 - p['contrast'])
            disps.append(p['disp'])
        tab_s, tab_w = shift_table(disps, V)
        up = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
        ip_d, fp_d, mat_d, al_d, ts_d, tw_d = up(ip), up(fp), up(mat), up(alpha), up(tab_s), up(tab_w)
        o_st = torch.empty((4, B, V, 3, ps, ps), dtype=torch.float32, device=dev)
        o_c = torch.empty((B, 3, ps, ps), dtype=torch.float32, device=dev)
        o_gt = torch.empty((B, ps, ps), dtype=torch.float32, device=dev)
        o_mpi = torch.empty((B, self.P, 5, ps, ps), dtype=torch.float32, device=dev)
        o_mask = torch.empty((B, ps, ps), dtype=torch.int32, device=dev)
        msum = torch.zeros(B, dtype=torch.float64, device=dev)
        call('mmlf_patch_gather', ptr(self.stacks), ptr(self.center), ptr(self.gt), ptr(self.mpi), ptr(self.mask),
             self.S, V, self.P, self.Hf, self.Wf, ptr(ip_d), ptr(fp_d), ptr(ts_d), ptr(tw_d), ptr(mat_d),
             ptr(self.rot_src), ptr(o_st), ptr(o_c), ptr(o_gt), ptr(o_mpi), ptr(o_mask), ptr(msum), B, ps,
             _lib.stream_ptr())
        if self.augment:
            call('mmlf_patch_contrast', ptr(o_st), ptr(o_c), ptr(msum), ptr(al_d), B, V, ps, _lib.stream_ptr())
        index = torch.from_numpy(np.stack([self.index[int(sc) % self.S] for sc in scene_indices]))
        return o_st[0], o_st[1], o_st[2], o_st[3], o_c, o_gt, o_mpi, o_mask, index

    def _sample_chain(self, scene_indices, rng=None):
        """sample() for a chain of mmlf_amd.transforms objects: the draws and the index tables on the host, one
        mmlf_data_gather, and mmlf_data_finish where the chain has Contrast or Noise."""
        plan = self.plan
        B, ps, V, dev = len(scene_indices), self.ps, self.V, self.stacks.device
        draws = [draw_chain_sample(plan, (self.Hf, self.Wf), V, rng) for _ in scene_indices]
        buf, offs, map_h, map_w = pack_chain_params(draws, [int(sc) % self.S for sc in scene_indices], (self.Hf, self.Wf), V, ps,
                                                    self._maps)
        buf_d = torch.from_numpy(buf).to(dev)
        at = {name: buf_d.data_ptr() + off for name, off in offs.items()}
        o_st = torch.empty((4, B, V, 3, ps, ps), dtype=torch.float32, device=dev)
        o_c = torch.empty((B, 3, ps, ps), dtype=torch.float32, device=dev)
        o_gt = torch.empty((B, ps, ps), dtype=torch.float32, device=dev)
        o_mpi = torch.empty((B, self.P, 5, ps, ps), dtype=torch.float32, device=dev)
        o_mask = torch.empty((B, ps, ps), dtype=torch.int32, device=dev)
        contrast, noise = 'contrast' in plan, plan.get('noise')
        msum = torch.zeros(B, dtype=torch.float64, device=dev) if contrast else None
        _lib.call_data('mmlf_data_gather', ptr(self.stacks), ptr(self.center), ptr(self.gt), ptr(self.mpi), ptr(self.mask),
                       self.S, V, self.P, self.Hf, self.Wf, at['ip'], at['fp'], at['ymap'], map_h, at['xmap'], map_w,
                       at['tab_s'], at['tab_w'], at['mat'], ptr(self.rot_src), ptr(o_st), ptr(o_c), ptr(o_gt), ptr(o_mpi),
                       ptr(o_mask), ptr(msum), B, ps, _lib.stream_ptr())
        if contrast or noise is not None:
            _lib.call_data('mmlf_data_finish', ptr(o_st), ptr(o_c), ptr(msum), at['alpha'] if contrast else None,
                           int(noise is not None), 0.0 if noise is None else noise.stdev, self.noise_seed, self.calls, B, V,
                           ps, _lib.stream_ptr())
        self.calls += 1
        index = torch.from_numpy(np.stack([self.index[int(sc) % self.S] for sc in scene_indices]))
        return o_st[0], o_st[1], o_st[2], o_st[3], o_c, o_gt, o_mpi, o_mask, index
