#!/usr/bin/env python3
"""Generate tests/golden/g13_nobn_tiny_{base,upr,dpp}.npz: the G1 tiny net (make_golden.py) with model_no_batchnorm=True
(blocks of conv -> ReLU -> conv -> ReLU, reference feed_forward.py:122-137), run by the REFERENCE on the CPU (the checkout
make_golden.py imports).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_nobn.py

Only data is written: the inputs, the eval- and train-mode outputs (one function without BatchNorm; both are stored so that a
test can hold each mode against the reference's), the loss and every parameter gradient of the variant's loss.  The weights
are not stored: they are synth.synth_state(synth.param_spec(**kw), state_seed), numpy RandomState draws that any test
regenerates bit for bit, with every convolution FILTER multiplied by `state_gain` (float32); `state_checksum` (sum of |w| in
float64 over every tensor) lets a test confirm it did.

Why the gain: torch's default filter bound 1 / sqrt(fan_in) halves the signal's variance six times over at every ReLU-only
block, so without BatchNorm to renormalise it the output of the tiny net varies by 1e-3 and the stream nets' gradients are
1e-5 -- below the ABSOLUTE floor of the G1 gradient bar, which would then pass a wrong mask in the stream chain.  With
sqrt(6) (the bound sqrt(6 / fan_in) that keeps the variance through a ReLU) every gradient tensor stands far above the floor
and the bar is the relative one.

A net of ReLUs alone has units whose pre-activation sits within float32 rounding noise of zero: one
that flips between two float32 implementations moves every gradient underneath.  The seed is therefore chosen HERE, on the
CPU and before any kernel sees the fixture: the first one, counting up from FIRST_SEED, at which the reference's float32 and
float64 runs agree on every gradient tensor within the G1 tolerance the GPU tests apply (tests/test_gpu_model.py:
max |difference| <= 5e-4 max |gradient| + 5e-7), for all three variants, AND every gradient tensor of every variant reaches
MIN_GRAD somewhere (the BASE head's first convolution has ONE output unit: where its ReLU is off over the whole patch, every
gradient underneath is exactly zero and the fixture would check nothing).  `f64_worst` records how much of the bar the
float32 run uses, `grad_smallest` the smallest max |gradient| over the tensors.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import TINY_KW, VARIANTS, loss_for, out_arrays, RefFeedForward, ref_loss  # noqa: E402
from mmlf_amd import synth  # noqa: E402

NOBN_TINY_KW = dict(TINY_KW, model_no_batchnorm=True)
FIRST_SEED = 13
INPUT_SEED = 9
STATE_GAIN = np.float32(np.sqrt(6.0))
MIN_GRAD = 1e-2             # 20 x the G1 bar's absolute floor over its relative factor (5e-7 / 5e-4 = 1e-3), and more


def gained_state(kw, seed, gain=STATE_GAIN):
    spec = synth.param_spec(**kw)
    state = synth.synth_state(spec, seed=seed)
    return {n: (state[n] * np.float32(gain) if kind == 'conv_w' else state[n]) for n, _, kind in spec}


def run(variant, kw, state, dtype):
    B, ps = (1 if variant == 'dpp' else 2), 12
    model = RefFeedForward(**kw)
    sd = model.state_dict()
    spec = synth.param_spec(**kw)
    assert list(sd) == [n for n, _, _ in spec], 'key set drifted'
    assert all(tuple(sd[n].shape) == tuple(s) for n, s, _ in spec), 'shapes drifted'
    assert not any('.3.' in n for n in sd), 'a BatchNorm key in a model_no_batchnorm net'
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    model = model.to(dtype)
    stacks, gt, mask = synth.synth_inputs(B, ps, seed=INPUT_SEED)
    m = torch.from_numpy(mask).int() * ref_loss.create_mask_margin(mask.shape, 3)
    tstacks = [torch.from_numpy(s).to(dtype) for s in stacks]
    rec = {}
    model.eval()
    with torch.no_grad():
        rec.update(out_arrays(model(*tstacks), 'eval_'))
    model.train()
    model.zero_grad()
    out = model(*tstacks)
    rec.update(out_arrays(out, 'train_'))
    loss = loss_for(variant, out, torch.from_numpy(gt).to(dtype), m, kw)
    loss.backward()
    rec['loss'] = loss.detach().numpy()
    for n, p in model.named_parameters():
        rec[f'grad/{n}'] = p.grad.numpy().copy()
    for i, s in enumerate(stacks):
        rec[f'in{i}'] = s
    rec['gt'] = gt
    rec['mask'] = m.numpy()
    return rec


def f64_distance(rec32, rec64):
    """the largest share of the G1 gradient bar that the float32 run's distance from the float64 run takes, over the tensors"""
    worst = 0.0
    for k, ref in rec64.items():
        if k.startswith('grad/'):
            err = np.abs(rec32[k].astype(np.float64) - ref).max()
            worst = max(worst, err / (5e-4 * max(np.abs(ref).max(), 1e-6) + 5e-7))
    return worst


def g13_nobn_tiny():
    # float64 linspace grids differ from the float32 ones inside the heads, not inside the trunk: the gradients compared here
    # are the trunk's, and the heads' values are not compared across the two precisions
    seed = FIRST_SEED
    while True:
        recs, worst, small = {}, 0.0, {}
        for variant, extra in VARIANTS.items():
            kw = dict(NOBN_TINY_KW, **extra)
            state = gained_state(kw, seed)
            recs[variant] = (run(variant, kw, state, torch.float32), state)
            worst = max(worst, f64_distance(recs[variant][0], run(variant, kw, state, torch.float64)))
            small[variant] = min(float(np.abs(v).max()) for k, v in recs[variant][0].items() if k.startswith('grad/'))
        print('G13 seed', seed, 'float32 against float64: worst share of the G1 gradient bar', worst,
              'smallest max |gradient| of a tensor', small)
        if worst <= 1.0 and min(small.values()) >= MIN_GRAD:
            break
        seed += 1
    for variant, (rec, state) in recs.items():
        rec['state_seed'] = np.array(seed)
        rec['state_gain'] = np.array(STATE_GAIN)
        rec['state_checksum'] = np.array(sum(np.abs(np.asarray(v, dtype=np.float64)).sum() for v in state.values()))
        rec['f64_worst'] = np.array(worst)
        rec['grad_smallest'] = np.array(small[variant])
        path = os.path.join(HERE, f'g13_nobn_tiny_{variant}.npz')
        np.savez_compressed(path, **rec)
        print('G13', variant, 'loss', float(rec['loss']), 'std of mean', float(rec['train_mean'].std()), 'arrays', len(rec),
              'bytes', os.path.getsize(path))


if __name__ == '__main__':
    g13_nobn_tiny()
