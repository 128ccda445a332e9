#!/usr/bin/env python3
"""Generate tests/golden/g14_ensamble_grad.npz: the REFERENCE's Ensamble (mmlf/model/ensamble.py:40-118) over its tiny UPR
net on the CPU (the checkout make_golden.py imports), differentiated by autograd in the four view stacks and in the
parameters.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ese_grad.py

Only data is written: the five outputs, the four input gradients and two parameter gradients (the first stream filter and
the head's last bias: the two ends of the net) of the loss tests/ese_grad_refs.py defines -- random-weighted sums of `mean`,
`logvar` and `posterior` -- at the first case of ese_grad_refs.CPU_CASES.  The weights, the inputs and the loss weights are
not stored: numpy RandomState draws that the test regenerates bit for bit (`state_checksum` confirms the weights).  The
reference runs in float64 (`dtype` records it): its own float32 buffers for the disparity grid and the posterior
(ensamble.py:90-96) stay as they are, so `posterior` is the float32 rounding of float64 sums.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import RefEnsamble, RefFeedForward  # noqa: E402
import ese_grad_refs as refs  # noqa: E402
from mmlf_amd import synth  # noqa: E402


def g14_ensamble_grad():
    frame, seed = refs.CPU_CASES[0]
    state = synth.synth_state(synth.param_spec(**refs.KW), seed=seed)
    model = RefFeedForward(**refs.KW)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    model = model.double().eval()
    ens = RefEnsamble(model, *refs.DISP)
    xs = [s.double().requires_grad_(True) for s in refs.case_inputs(frame, seed)]
    out = ens(*xs)
    weights = refs.loss_weights(frame, seed)
    loss = refs.loss_of(out, weights)
    loss.backward()
    rec = {f'out/{k}': v.detach().numpy() for k, v in out.items()}
    rec.update({f'dx/{k}': x.grad.numpy() for k, x in zip('hvid', xs)})
    grads = dict(model.named_parameters())
    rec.update({f'dp/{n}': grads[n].grad.numpy() for n in refs.PARAMS})
    rec['loss'] = loss.detach().numpy()
    rec['frame'], rec['seed'], rec['disp'] = np.array(frame), np.array(seed), np.array(refs.DISP)
    rec['dtype'] = np.array('float64')
    rec['state_checksum'] = np.array(sum(np.abs(np.asarray(v, dtype=np.float64)).sum() for v in state.values()))
    path = os.path.join(HERE, 'g14_ensamble_grad.npz')
    np.savez_compressed(path, **rec)
    print('G14 loss', float(loss.detach()), 'max |dx|', [float(x.grad.abs().max()) for x in xs], 'arrays', len(rec), 'bytes',
          os.path.getsize(path))


if __name__ == '__main__':
    g14_ensamble_grad()
