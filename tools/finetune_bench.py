"""Partial training of the native trunk: the default BASE net (bs = 64, ps = 96) through the module (FeedForward + masked L1
loss + backward, no optimizer), five legs in one process on one device, the same inputs:
  a  all parameters trainable (what a training step differentiates)
  b  out_net only (both stream nets frozen)
  c  the head block only
  d  biases and BatchNorm parameters only (every filter frozen: the bias-only weight-gradient launches)
  e  in_net_hv.0 only (the gradient crosses the whole net, two blocks train)
Every leg is warmed up, then the legs take turns repeat by repeat (what else runs on the host moves all of them alike); forward
and backward are timed by device events, the medians are reported, with the peak of torch's allocator over a repeat.
--kernel also times the bias-only launch on the 280-channel gradient of that step against mmlf_bn_bwd_reduce on the same
tensor (which reads a second tensor beside it).  Prints one JSON object; --out also writes it.
    python tools/finetune_bench.py [--batch 64] [--ps 96] [--repeats 7] [--warmup 2] [--legs a,b,c,d,e] [--kernel]
                                   [--out profiles/finetune_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmlf_amd import _lib, engine, loss, synth  # noqa: E402
from mmlf_amd._lib import call, ptr  # noqa: E402
from mmlf_amd.feed_forward import FeedForward  # noqa: E402

KW = dict(model_ksize=2, model_in_blocks=3, model_out_blocks=8, model_chs=70, model_views=9, model_cross=False,
          model_uncert=False, model_unet=False, model_discrete=False, model_no_batchnorm=False,
          model_batchnorm_momentum=0.1, val_disp_min=-3.5, val_disp_max=3.5)
# leg: which parameter names train
LEGS = {'a': lambda n: True,
        'b': lambda n: n.startswith('out_net.'),
        'c': lambda n: n.startswith('out_net.7.'),
        'd': lambda n: not n.endswith(('.0.weight', '.2.weight')),
        'e': lambda n: n.startswith('in_net_hv.0.')}


def make_model(dev, keep):
    m = FeedForward(**KW)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_state(synth.param_spec(**KW), 21).items()})
    m.to(dev)
    assert m._native_ok
    for n, p in m.named_parameters():
        p.requires_grad_(bool(keep(n)))
    return m.train()


def kernel_times(dev, batch, ps, repeats, warmup):
    """the bias-only launch (mmlf_conv2x2_wgrad_h2 with gw = NULL) and mmlf_bn_bwd_reduce on one 280-channel gradient"""
    C = 280
    geo = engine.Geometry(batch, ps, ps)
    g, z = geo.bufs([C, C], dev)
    interior = torch.zeros(batch, geo.R, geo.P, C, device=dev)
    interior[:, 1:ps + 1, 1:ps + 1] = torch.randn(batch, ps, ps, C, device=dev)
    for t in (g, z):
        t[:geo.NQ * C].copy_(interior.view(-1))
    x = geo.buf(C, dev)
    ws = engine._Workspace.get(dev)
    wsp = ws.wgrad_ws(geo, C, C)
    gb = torch.zeros(C, device=dev)
    one, zero = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    coef = torch.empty(3 * C, device=dev)
    ax, ag = geo.amax_of(x, C), geo.amax_of(g, C)

    def bias_only():
        call('mmlf_conv2x2_wgrad_h2', ptr(x), C, C, ptr(g), C, C, geo.P + 1, None, ptr(gb), 0, 0, ptr(wsp), batch, ps, ps,
             ptr(ax), ptr(ag), _lib.stream_ptr())

    def bn_reduce():
        call('mmlf_bn_bwd_reduce', ptr(g), C, 0, ptr(z), C, C, ptr(one), ptr(zero), ptr(one), ptr(zero), ptr(one), ptr(gb),
             ptr(gb), 0, ptr(coef), ptr(ws.partial), engine.BN_BLOCKS, batch, ps, ps, _lib.stream_ptr())

    times = {'bias_only': [], 'bn_bwd_reduce': []}
    for it in range(warmup + repeats):
        for name, fn in (('bias_only', bias_only), ('bn_bwd_reduce', bn_reduce)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                times[name].append(e0.elapsed_time(e1))
    nbytes = 4.0 * geo.NQ * C                    # one pass over g; mmlf_bn_bwd_reduce reads z as well (interior positions)
    out = {'channels': C, 'bytes_g': nbytes}
    for name, reads in (('bias_only', 1), ('bn_bwd_reduce', 2)):
        ms = float(np.median(times[name]))
        out[name] = {'ms_median': ms, 'ms': times[name], 'tensors_read': reads, 'GBps': reads * nbytes / ms * 1e-6,
                     'share_of_8TBps_HBM': reads * nbytes / ms * 1e-6 / 8000.0}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--ps', type=int, default=96)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--legs', default='a,b,c,d,e')
    ap.add_argument('--kernel', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('finetune_bench: no GPU (a time taken anywhere else says nothing)')
    dev = torch.device('cuda:0')
    stacks, gt, mask = synth.synth_inputs(a.batch, a.ps, seed=8)
    data = [torch.from_numpy(s).to(dev) for s in stacks]
    gt, mask = torch.from_numpy(gt).to(dev), torch.from_numpy(mask).to(dev)
    legs = a.legs.split(',')
    models = {k: make_model(dev, LEGS[k]) for k in legs}
    crit = loss.MaskedL1Loss()
    fwd, bwd, peak = ({k: [] for k in legs} for _ in range(3))
    for it in range(a.warmup + a.repeats):
        for k in legs:
            m = models[k]
            m.zero_grad(set_to_none=True)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            ev[0].record()
            lv = crit(m(*data), gt, mask)
            ev[1].record()
            lv.backward()
            ev[2].record()
            torch.cuda.synchronize()
            assert all((p.grad is not None) == bool(LEGS[k](n)) for n, p in m.named_parameters()), k
            if it >= a.warmup:
                fwd[k].append(ev[0].elapsed_time(ev[1]))
                bwd[k].append(ev[1].elapsed_time(ev[2]))
                peak[k].append(torch.cuda.max_memory_allocated(dev))
            del lv
    res = {'config': {'batch': a.batch, 'ps': a.ps, 'repeats': a.repeats, 'warmup': a.warmup, 'conv_mode': engine.CONV_MODE,
                      'device': torch.cuda.get_device_name(0), 'build': _lib.build_info()}}
    for k in legs:
        tot = [f + b for f, b in zip(fwd[k], bwd[k])]
        res[f'leg_{k}'] = {'forward_ms_median': float(np.median(fwd[k])), 'backward_ms_median': float(np.median(bwd[k])),
                           'step_ms_median': float(np.median(tot)), 'step_ms': tot,
                           'max_memory_allocated_GiB': max(peak[k]) / 2.0 ** 30,
                           'trainable_parameters': sum(p.numel() for p in models[k].parameters() if p.requires_grad)}
    if a.kernel:
        del models
        torch.cuda.empty_cache()
        res['bias_only_kernel'] = kernel_times(dev, a.batch, a.ps, a.repeats, a.warmup)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
