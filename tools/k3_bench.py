"""--model_ksize 3: a BASE training step (forward + masked L1 loss + backward + Adam, TrainStep) at bs=64, ps=96 on the native
3x3 trunk and on the stock-torch path of the same module (`_native_ok = False`: MIOpen), same process, same device, and the
280 -> 280 3x3 forward launch (mmlf_conv3x3) timed with HIP events, as a fraction of the f32 MFMA peak (157.3 TF/s, algorithmic
FLOPs 2 B H W Cin Cout 9).  Prints one JSON object; --out also writes it to a file.
    python tools/k3_bench.py [--batch 64] [--ps 96] [--steps 3] [--warmup 1] [--out profiles/k3_bench.json]"""
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

PEAK_F32_TFLOPS = 157.3
KW = dict(model_ksize=3, model_in_blocks=3, model_out_blocks=8, model_chs=70, model_views=9, model_cross=False,
          model_uncert=False, model_unet=False, model_discrete=False, model_no_batchnorm=False,
          model_batchnorm_momentum=0.1, val_disp_min=-3.5, val_disp_max=3.5)


def k3_state(seed):
    spec = [(n, (s[0], s[1], 3, 3) if kind == 'conv_w' else s, kind) for n, s, kind in synth.param_spec(**KW)]
    return synth.synth_state(spec, seed)


def time_steps(native, state, data, steps, warmup, dev):
    m = FeedForward(**KW)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    m.to(dev)
    m._native_ok = native
    step = TrainStep(m, lr=1e-3)
    times, losses = [], []
    for it in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss = step(*data, it + 1)
        torch.cuda.synchronize()
        if it >= warmup:
            times.append(1e3 * (time.perf_counter() - t0))
        losses.append(float(loss))
    del step, m
    torch.cuda.empty_cache()
    return {'ms_per_step': times, 'ms_median': float(np.median(times)), 'losses': losses}


def time_conv(B, ps, dev, reps=10):
    C = 280
    geo = engine.Geometry(B, ps, ps, 3)
    g = torch.Generator().manual_seed(1)
    x = geo.buf(C, dev)
    nchw = torch.randn((B, C, ps, ps), generator=g).to(dev)
    _lib.call('mmlf_pack_nchw', _lib.ptr(nchw), C, _lib.ptr(x), C, B, ps, ps, _lib.ptr(x.absmax), _lib.stream_ptr())
    del nchw
    w = (torch.randn((C, C, 3, 3), generator=g) / np.sqrt(9 * C)).to(dev)
    b = torch.zeros(C, device=dev)
    pk = engine.pack_filter3(w, engine.VAR_IDENTITY, False)
    out = geo.buf(C, dev)
    run = lambda: engine.conv3(geo, x, C, C, pk, b, C, out, C, True)   # noqa: E731
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    flops = 2.0 * B * ps * ps * C * C * 9
    med = float(np.median(ms))
    return {'shape': f'{C}->{C} 3x3, B={B}, {ps}x{ps}', 'ms': ms, 'ms_median': med, 'tflops': flops / med * 1e-9,
            'fraction_of_f32_peak': flops / med * 1e-9 / PEAK_F32_TFLOPS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--ps', type=int, default=96)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    state = k3_state(21)
    stacks, gt, mask = synth.synth_inputs(a.batch, a.ps, seed=8)
    data = [torch.from_numpy(s).to(dev) for s in stacks] + [torch.from_numpy(gt).to(dev), torch.from_numpy(mask).to(dev)]
    res = {'config': {'batch': a.batch, 'ps': a.ps, 'steps': a.steps, 'warmup': a.warmup, 'device': torch.cuda.get_device_name(0),
                      'build': _lib.build_info()},
           'conv3x3_280': time_conv(a.batch, a.ps, dev)}
    res['step_native'] = time_steps(True, state, data, a.steps, a.warmup, dev)
    res['step_stock'] = time_steps(False, state, data, a.steps, a.warmup, dev)
    res['native_over_stock'] = res['step_native']['ms_median'] / res['step_stock']['ms_median']
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
