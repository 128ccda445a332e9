"""TrainStep(micro_batches=n) at the README batch: a BASE training step (forward + masked L1 loss + backward +
Adam) at bs=512, ps=96 for micro_batches 1, 2, 4, 8 -- one TrainStep per setting on weights of its own, taking turns step by
step in one process, each step between two device synchronisations and with the allocator's peak counter reset in front of it.
Per setting: the median step time, patches/s and the largest torch.cuda.max_memory_allocated of its measured steps.  Beside
them the yardstick bench.py --full calls shard64: the same step on 64 patches alone (one replica's share of the batch on 8
GPUs), as patches/s over the n=1 rate -- what eight passes of that size can reach at best.
Prints one JSON object; --out also writes it.  --micro-batches selects the settings (a run of one setting alone gives that
setting's memory in a process that never held a larger step).
    python tools/microbatch_bench.py [--batch 512] [--ps 96] [--steps 10] [--warmup 3] [--micro-batches 1 2 4 8]
                                     [--out profiles/microbatch_bench.json]"""
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
          model_uncert=False, model_unet=False, model_discrete=False, model_no_batchnorm=False,
          model_batchnorm_momentum=0.1, val_disp_min=-3.5, val_disp_max=3.5)


def make_step(dev, n):
    m = FeedForward(**KW)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_state(synth.param_spec(**KW), 21).items()})
    m.to(dev)
    assert m._native_ok
    return TrainStep(m, lr=1e-3, micro_batches=n)


def timed_step(step, data, it):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    loss = step(*data, it)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), torch.cuda.max_memory_allocated(), float(loss)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--ps', type=int, default=96)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--micro-batches', type=int, nargs='*', default=[1, 2, 4, 8])
    ap.add_argument('--shard', type=int, default=64, help='patches of the stand-alone yardstick step (0: none)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('microbatch_bench: no GPU (a time taken anywhere else says nothing)')
    dev = torch.device('cuda:0')
    stacks, gt, mask = synth.synth_inputs(a.batch, a.ps, seed=8)
    data = [torch.from_numpy(s).to(dev) for s in stacks] + [torch.from_numpy(gt).to(dev), torch.from_numpy(mask).to(dev)]
    res = {'config': {'batch': a.batch, 'ps': a.ps, 'steps': a.steps, 'warmup': a.warmup, 'conv_mode': engine.CONV_MODE,
                      'device': torch.cuda.get_device_name(0), 'build': _lib.build_info(),
                      'resident_bytes_before_steps': None}}
    steps = {n: make_step(dev, n) for n in a.micro_batches}
    torch.cuda.synchronize()
    res['config']['resident_bytes_before_steps'] = torch.cuda.memory_allocated()       # inputs, weights, moments
    rows = {n: {'ms': [], 'peak': [], 'loss': []} for n in steps}
    for it in range(a.warmup + a.steps):
        for n, step in steps.items():
            ms, peak, loss = timed_step(step, data, it + 1)
            if it >= a.warmup:
                rows[n]['ms'].append(ms)
                rows[n]['peak'].append(peak)
            rows[n]['loss'].append(loss)
    for n, row in rows.items():
        med = float(np.median(row['ms']))
        res[f'micro_batches_{n}'] = {'chunk': -(-a.batch // n), 'ms_per_step': row['ms'], 'ms_median': med,
                                     'patches_per_s': a.batch / med * 1e3, 'max_memory_allocated': max(row['peak']),
                                     'max_memory_allocated_gib': max(row['peak']) / 2 ** 30, 'losses': row['loss']}
    base = res.get('micro_batches_1')
    if base is not None:
        for n in steps:
            row = res[f'micro_batches_{n}']
            row['rate_vs_n1'] = row['patches_per_s'] / base['patches_per_s']
            row['memory_vs_n1'] = row['max_memory_allocated'] / base['max_memory_allocated']
    del steps
    torch.cuda.empty_cache()
    if a.shard and a.shard < a.batch:
        step = make_step(dev, 1)
        part = [t[:a.shard].contiguous() for t in data]
        ms = [timed_step(step, part, it + 1)[0] for it in range(a.warmup + a.steps)][a.warmup:]
        med = float(np.median(ms))
        res[f'shard{a.shard}'] = {'ms_per_step': ms, 'ms_median': med, 'patches_per_s': a.shard / med * 1e3}
        if base is not None:
            res[f'shard{a.shard}']['vs_n1'] = res[f'shard{a.shard}']['patches_per_s'] / base['patches_per_s']
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
