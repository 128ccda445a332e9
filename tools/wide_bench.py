"""Nets wider than 288 channels (column blocks): a BASE training step (forward + masked L1 loss + backward +
Adam, TrainStep) at model_chs 96 and 128, bs=64, ps=96 -- the size at which MIOpen's weight gradient is right (DESIGN.md
section 2) -- on the native trunk and on the stock-torch path of the same module (`_native_ok = False`: MIOpen / ATen), taking
turns step by step in one process, each step between two device synchronisations.  Then, per net and beside them for a
model_chs=70 net in the same process, the device-event times of the wide launches of one native step (engine.PROFILE): forward,
data gradient and weight gradient of the merge blocks, as algorithmic TFLOP/s, and what the 280-wide launch of this run lets
one expect of the wider ones: its TFLOP/s times the share of computed columns that are live under the block rules
(conv.hip wide_np: 2 x 192 of 384, 2 x 256 of 512; wgrad.hip: 288 + 128 for 384, 288 + 288 for 512).
Prints one JSON object; --out also writes it.
    python tools/wide_bench.py [--batch 64] [--ps 96] [--steps 5] [--warmup 2] [--out profiles/wide_bench.json]"""
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
# computed columns per layer width: (convolution, weight gradient)
COLUMNS = {280: (288, 288), 384: (384, 288 + 128), 512: (512, 288 + 288)}


def make_step(kw, native, dev):
    m = FeedForward(**kw)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_state(synth.param_spec(**kw), 21).items()})
    m.to(dev)
    assert m._native_ok
    m._native_ok = native
    return TrainStep(m, lr=1e-3)


def profile_step(step, data, it):
    """one native step with device events around every wide launch: {kind: (median ms, algorithmic TFLOP/s, launches)} for the
    merge blocks' forward, data-gradient and weight-gradient launches (main stream)"""
    kinds = []
    conv, toc = engine.conv, engine._toc

    def conv_spy(geo, x, cs_in, K, packed, bias, *args, **kwargs):
        kinds.append('dgrad' if bias is None else 'forward')      # (a data gradient is a convolution without bias)
        return conv(geo, x, cs_in, K, packed, bias, *args, **kwargs)

    def toc_spy(events, tag, flops, nbytes):
        toc(events, {'conv': kinds[-1] if kinds else 'forward'}.get(tag, tag), flops, nbytes)

    engine.conv, engine._toc, engine.PROFILE = conv_spy, toc_spy, []
    try:
        step(*data, it)
        torch.cuda.synchronize()
        rows = [(tag, flops, e0.elapsed_time(e1)) for tag, flops, e0, e1, _ in engine.PROFILE]
    finally:
        engine.conv, engine._toc, engine.PROFILE = conv, toc, None
    out = {}
    for kind in ('forward', 'dgrad', 'wgrad', 'wgrad_side'):
        ms = [t for tag, _, t in rows if tag == kind]
        fl = [f for tag, f, _ in rows if tag == kind]
        if ms:
            med = float(np.median(ms))
            out[kind] = {'ms_median': med, 'tflops': float(np.median(fl)) / med * 1e-9, 'launches': len(ms)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--ps', type=int, default=96)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--chs', type=int, nargs='*', default=[96, 128])
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('wide_bench: no GPU (a time taken anywhere else says nothing)')
    dev = torch.device('cuda:0')
    stacks, gt, mask = synth.synth_inputs(a.batch, a.ps, seed=8)
    data = [torch.from_numpy(s).to(dev) for s in stacks] + [torch.from_numpy(gt).to(dev), torch.from_numpy(mask).to(dev)]
    res = {'config': {'batch': a.batch, 'ps': a.ps, 'steps': a.steps, 'warmup': a.warmup, 'conv_mode': engine.CONV_MODE,
                      'device': torch.cuda.get_device_name(0), 'build': _lib.build_info()}}
    launches = {}
    for chs in [70] + list(a.chs):
        kw = dict(KW, model_chs=chs)
        steps = {'native': make_step(kw, True, dev)}
        if chs != 70:
            steps['stock'] = make_step(kw, False, dev)
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
        entry = {name: {'ms_per_step': times[name], 'ms_median': float(np.median(times[name])), 'losses': losses[name]}
                 for name in steps}
        if 'stock' in steps:
            entry['native_over_stock'] = entry['native']['ms_median'] / entry['stock']['ms_median']
        launches[4 * chs] = entry['launches'] = profile_step(steps['native'], data, a.warmup + a.steps + 1)
        res[f'model_chs_{chs}'] = entry
        del steps
        torch.cuda.empty_cache()
    # expectation from the 280-wide launch of this run: its TFLOP/s x the live share of the computed columns
    for width, entry in launches.items():
        if width == 280:
            continue
        for kind, row in entry.items():
            base = launches[280].get('wgrad' if kind.startswith('wgrad') else kind)
            if base is None:
                continue
            if width not in COLUMNS:
                continue
            cols = COLUMNS[width][1 if kind.startswith('wgrad') else 0]
            # (the 280-wide launch's algorithmic rate carries its own live share, 280 of 288 computed columns)
            row['expected_tflops'] = base['tflops'] * (COLUMNS[280][0] / 280) * (width / cols)
            row['measured_over_expected'] = row['tflops'] / row['expected_tflops']
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
