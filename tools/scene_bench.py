"""What the scene builder costs on the device, in one process:

    python tools/scene_bench.py [--out profiles/scene_texture_ab.log]

1. scenes.texture_mask(center, 23, 0.02) against the stock-torch expression of the reference (hci4d.py:54-67: unfold, view,
   abs, mean, >=, margin) on the same device tensors, at (1,3,512,512) and (16,3,512,512).  Both arms are warmed up at every
   timed shape and then timed in alternating rounds between HIP events; a round is REPS calls of one arm, the figure the
   median over rounds of the time per call.  The stock arm materialises 3 * 529 * H * W floats per image (1.66 GB) and its
   difference again, so its rounds hold fewer calls.
2. scenes.assemble_scene for one 81 x 512 x 512 uint8 grid that is already on the device (the upload of the decoded
   images is the caller's), gt and mask included.

The masks of the two arms are compared and the number of differing pixels is written beside the times.  Exits nonzero if
the kernel is not at least twice as fast as the stock expression at both shapes.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from mmlf_amd import scenes  # noqa: E402
import scene_refs as refs  # noqa: E402

WSIZE, THRESHOLD, SIZE, ROUNDS, WARMUP = 23, 0.02, 512, 7, 3
REPS = {'kernel': {1: 2000, 16: 300}, 'stock': {1: 20, 16: 3}}


def stock_mask(center, wsize, threshold):
    """the reference's expression in stock torch ops, on whatever device `center` lives"""
    b, h, w = center.shape[0], center.shape[-2], center.shape[-1]
    m = torch.nn.functional.unfold(center, kernel_size=wsize, padding=wsize // 2).view(b, 3, -1, h, w)
    m = ((m - center.unsqueeze(2)).abs_().mean((1, 2)) >= threshold).int()        # (abs in place: one copy less)
    r = wsize // 2
    margin = torch.zeros_like(m)
    margin[..., r:h - r, r:w - r] = 1
    return m * margin


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'scene_texture_ab.log'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'scene_bench.py measures on the GPU: there is no CPU figure'
    lines = [f'{torch.cuda.get_device_name(0)}: texture_mask(wsize {WSIZE}, threshold {THRESHOLD}) against the stock unfold '
             f'expression, {WARMUP} warm-up calls per arm and shape, {ROUNDS} alternating rounds, median time per call']
    ok = True
    for B in (1, 16):
        center = torch.from_numpy(np.concatenate([refs.centre(1, SIZE, SIZE, seed=s) for s in range(B)])).cuda()
        arms = {'kernel': lambda: scenes.texture_mask(center, WSIZE, THRESHOLD),
                'stock': lambda: stock_mask(center, WSIZE, THRESHOLD)}
        reps = {'kernel': REPS['kernel'][B], 'stock': REPS['stock'][B]}
        for name, fn in arms.items():
            for _ in range(WARMUP):
                fn()
        torch.cuda.synchronize()
        diff = int((arms['kernel']() != arms['stock']()).sum())
        t = {name: [] for name in arms}
        for _ in range(ROUNDS):
            for name, fn in arms.items():
                t[name].append(timed(fn, reps[name]))
        med = {name: float(np.median(v)) for name, v in t.items()}
        ratio = med['stock'] / med['kernel']
        ok = ok and ratio >= 2.0
        lines.append(f'({B},3,{SIZE},{SIZE}): kernel {med["kernel"] * 1e3:10.1f} us [{min(t["kernel"]) * 1e3:.1f} .. '
                     f'{max(t["kernel"]) * 1e3:.1f}]   stock {med["stock"] * 1e3:10.1f} us [{min(t["stock"]) * 1e3:.1f} .. '
                     f'{max(t["stock"]) * 1e3:.1f}]   ratio {ratio:7.1f}   masks differ at {diff} of {B * SIZE * SIZE} pixels')
        print(lines[-1], flush=True)
        del center, arms
        torch.cuda.empty_cache()
    views, gt, _, mask = refs.scene_inputs((9, 9), SIZE, SIZE, 0)
    views_d = torch.from_numpy(views).cuda()
    build = lambda: scenes.assemble_scene(views_d, gt, None, mask)   # noqa: E731
    for _ in range(WARMUP):
        build()
    torch.cuda.synchronize()
    t = [timed(build, 20) for _ in range(ROUNDS)]
    lines.append(f'assemble_scene, 81 x {SIZE} x {SIZE} uint8 grid on the device (gt and mask from the host): median '
                 f'{float(np.median(t)):.3f} ms per scene [{min(t):.3f} .. {max(t):.3f}]')
    print(lines[-1], flush=True)
    lines.append('kernel at least 2x faster than the stock expression at both shapes: ' + ('yes' if ok else 'NO'))
    print(lines[-1])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
