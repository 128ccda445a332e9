"""Input gradients and the frozen backward of the native trunk: the default BASE net (bs = 64, ps = 96) through the module
(FeedForward + masked L1 loss + backward, no optimizer), five legs in one process on one device, the same inputs:
  a  parameter gradients only (what a training step differentiates)
  b  the same plus the gradients of the four view stacks
  c  frozen net (no parameter requires a gradient), train mode: input gradients only, no weight-gradient launch
  d  frozen net, eval mode: the folded inference launches under a tape, a ReLU-only backward
  e  the torch.no_grad() eval forward alone
Every leg is warmed up, then the legs take turns repeat by repeat (what else runs on the host moves all of them alike); forward
and backward are timed by device events, the medians are reported.  --legs picks a subset (a tree without input gradients
runs a,e).  Prints one JSON object; --out also writes it.
    python tools/ingrad_bench.py [--batch 64] [--ps 96] [--repeats 7] [--warmup 2] [--legs a,b,c,d,e] [--out profiles/ingrad_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmlf_amd import _lib, engine, loss, synth  # noqa: E402
from mmlf_amd.feed_forward import FeedForward  # noqa: E402

KW = dict(model_ksize=2, model_in_blocks=3, model_out_blocks=8, model_chs=70, model_views=9, model_cross=False,
          model_uncert=False, model_unet=False, model_discrete=False, model_no_batchnorm=False,
          model_batchnorm_momentum=0.1, val_disp_min=-3.5, val_disp_max=3.5)
# leg: (parameters require gradients, stacks require gradients, train mode, backward)
LEGS = {'a': (True, False, True, True), 'b': (True, True, True, True), 'c': (False, True, True, True),
        'd': (False, True, False, True), 'e': (False, False, False, False)}


def make_model(dev, params_grad, train):
    m = FeedForward(**KW)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_state(synth.param_spec(**KW), 21).items()})
    m.to(dev)
    assert m._native_ok
    for p in m.parameters():
        p.requires_grad_(params_grad)
    return m.train(train)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--ps', type=int, default=96)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--legs', default='a,b,c,d,e')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('ingrad_bench: no GPU (a time taken anywhere else says nothing)')
    dev = torch.device('cuda:0')
    stacks, gt, mask = synth.synth_inputs(a.batch, a.ps, seed=8)
    data = [torch.from_numpy(s).to(dev) for s in stacks]
    gt, mask = torch.from_numpy(gt).to(dev), torch.from_numpy(mask).to(dev)
    legs = a.legs.split(',')
    models = {k: make_model(dev, LEGS[k][0], LEGS[k][2]) for k in legs}
    crit = loss.MaskedL1Loss()
    fwd = {k: [] for k in legs}
    bwd = {k: [] for k in legs}
    for it in range(a.warmup + a.repeats):
        for k in legs:
            _, xgrad, _, back = LEGS[k]
            m = models[k]
            m.zero_grad(set_to_none=True)
            xs = [t.detach().requires_grad_(xgrad) for t in data]
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            torch.cuda.synchronize()
            ev[0].record()
            with torch.set_grad_enabled(back):
                out = m(*xs)
                lv = crit(out, gt, mask)
            ev[1].record()
            if back:
                lv.backward()
            ev[2].record()
            torch.cuda.synchronize()
            if back and xgrad:
                assert all(x.grad is not None and x.grad.shape == x.shape for x in xs)
            if it >= a.warmup:
                fwd[k].append(ev[0].elapsed_time(ev[1]))
                bwd[k].append(ev[1].elapsed_time(ev[2]))
    res = {'config': {'batch': a.batch, 'ps': a.ps, 'repeats': a.repeats, 'warmup': a.warmup, 'conv_mode': engine.CONV_MODE,
                      'device': torch.cuda.get_device_name(0), 'build': _lib.build_info()}}
    for k in legs:
        tot = [f + b for f, b in zip(fwd[k], bwd[k])]
        res[f'leg_{k}'] = {'forward_ms_median': float(np.median(fwd[k])), 'backward_ms_median': float(np.median(bwd[k])),
                           'total_ms_median': float(np.median(tot)), 'total_ms': tot}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
