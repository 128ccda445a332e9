"""--model_no_batchnorm: a BASE training step (forward + masked L1 loss + backward + Adam, TrainStep) at bs=64, ps=96 -- the size
at which MIOpen's weight gradient is right -- on the native 2x2 trunk, on the stock-torch path of the same
module (`_native_ok = False`: MIOpen / ATen), and, beside them, the native step of the default BatchNorm net.  Same process,
same device, same inputs; every configuration is warmed up, then the three take turns step by step (what else runs on the
host moves all of them alike), each step between two device synchronisations.  Prints one JSON object; --out also writes it.
    python tools/nobn_bench.py [--batch 64] [--ps 96] [--steps 5] [--warmup 2] [--out profiles/nobn_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmlf_amd import _lib, engine, synth  # noqa: E402
from mmlf_amd.feed_forward import FeedForward  # noqa: E402
from mmlf_amd.train import TrainStep  # noqa: E402

KW = dict(model_ksize=2, model_in_blocks=3, model_out_blocks=8, model_chs=70, model_views=9, model_cross=False,
          model_uncert=False, model_unet=False, model_discrete=False, model_no_batchnorm=True,
          model_batchnorm_momentum=0.1, val_disp_min=-3.5, val_disp_max=3.5)


def make_step(kw, native, dev):
    m = FeedForward(**kw)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_state(synth.param_spec(**kw), 21).items()})
    m.to(dev)
    assert m._native_ok
    m._native_ok = native
    return TrainStep(m, lr=1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--ps', type=int, default=96)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('nobn_bench: no GPU (a time taken anywhere else says nothing)')
    dev = torch.device('cuda:0')
    stacks, gt, mask = synth.synth_inputs(a.batch, a.ps, seed=8)
    data = [torch.from_numpy(s).to(dev) for s in stacks] + [torch.from_numpy(gt).to(dev), torch.from_numpy(mask).to(dev)]
    steps = {'nobn_native': make_step(KW, True, dev), 'nobn_stock': make_step(KW, False, dev),
             'batchnorm_native': make_step(dict(KW, model_no_batchnorm=False), True, dev)}
    times = {k: [] for k in steps}
    losses = {k: [] for k in steps}
    for it in range(a.warmup + a.steps):
        for name, step in steps.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = step(*data, it + 1)
            torch.cuda.synchronize()
            if it >= a.warmup:
                times[name].append(1e3 * (time.perf_counter() - t0))
            losses[name].append(float(loss))
    res = {'config': {'batch': a.batch, 'ps': a.ps, 'steps': a.steps, 'warmup': a.warmup, 'conv_mode': engine.CONV_MODE,
                      'device': torch.cuda.get_device_name(0), 'build': _lib.build_info()}}
    for name in steps:
        res[f'step_{name}'] = {'ms_per_step': times[name], 'ms_median': float(np.median(times[name])), 'losses': losses[name]}
    med = lambda k: res[f'step_{k}']['ms_median']   # noqa: E731
    res['nobn_native_over_stock'] = med('nobn_native') / med('nobn_stock')
    res['nobn_native_over_batchnorm_native'] = med('nobn_native') / med('batchnorm_native')
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
