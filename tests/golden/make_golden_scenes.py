#!/usr/bin/env python3
"""Generate tests/golden/g15_texture_mask.npz by running the REFERENCE's create_mask_texture (imported as
make_golden_chain.py imports the reference; CPU only) over the seeded centres of tests/scene_refs.py GOLDEN_SHAPES.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_scenes.py

Only data is written: per shape and kind (float, dyadic) the reference's mask as uint8.  The centres come from
scene_refs.centre and are not stored.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, '/root/reference')

from mmlf.data import hci4d as ref_hci4d  # noqa: E402

import scene_refs as refs  # noqa: E402


def main():
    rec = {}
    for B, H, W, wsize, thr in refs.GOLDEN_SHAPES:
        for kind in refs.KINDS:
            c = torch.from_numpy(refs.centre(B, H, W, dyadic=kind == 'dyadic'))
            mask = ref_hci4d.create_mask_texture(c, wsize, thr).numpy()
            assert mask.shape == (B, H, W)
            inner = refs.interior(H, W, wsize)
            ref = (refs.window_sum64(c, wsize) / float(3 * wsize * wsize)).numpy()
            band = (np.abs(ref - float(np.float32(thr))) <= refs.rel_bound(wsize) * float(np.float32(thr))) & inner[None]
            ones = float(mask[:, inner].mean()) if inner.any() else 0.0
            print(refs.tag(B, H, W, wsize, kind), 'interior ones %.3f' % ones, 'band %d of %d' % (band.sum(), B * inner.sum()))
            rec[refs.tag(B, H, W, wsize, kind)] = mask.astype(np.uint8)
    out = os.path.join(HERE, 'g15_texture_mask.npz')
    np.savez_compressed(out, **rec)
    print(len(rec), 'arrays,', os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
