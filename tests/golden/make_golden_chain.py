#!/usr/bin/env python3
"""Generate tests/golden/g12_patch_chain.npz by running the REFERENCE's transforms (imported as make_golden.py imports
the reference; CPU only) over the chains of tests/transform_refs.py CASES.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_chain.py

Only data is written: per case and sample the eight output arrays and one `random.random()` taken after the sample (the
state the host draws must leave the stream in).  The scenes come from mmlf_amd.synth and are not stored.
"""
import copy
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, '/root/reference')

from mmlf.data import hci4d as ref_hci4d  # noqa: E402

from mmlf_amd import synth  # noqa: E402
import transform_refs as refs  # noqa: E402


def main():
    rec = {}
    for tag, (scene_seed, (H, W), chain) in refs.CASES.items():
        scene = synth.synth_scene(scene_seed, H, W, views=refs.VIEWS, planes=refs.PLANES)
        tfs = refs.build(ref_hci4d, chain)
        for k in range(refs.SAMPLES):
            random.seed(refs.case_seed(tag, k))
            data = copy.deepcopy(scene)            # hci4d.py:289-291
            for tf in tfs:
                data = tf(data)
            rec[f'{tag}.{k}.after'] = np.float64(random.random())
            for name, arr in zip(refs.NAMES, data):
                arr = np.ascontiguousarray(arr)
                rec[f'{tag}.{k}.{name}'] = arr.astype(np.uint8) if name == 'mask' else arr
            print(tag, k, data[0].shape, data[5].shape, data[7].shape)
    out = os.path.join(HERE, 'g12_patch_chain.npz')
    np.savez_compressed(out, **rec)
    print(len(rec), 'arrays,', os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
