"""What a gradient through the Ensamble costs on one MI355X: a 512 x 512 scene, 70 members, the UPR net,
weights frozen and then trainable.

    python tools/ese_grad_bench.py [--size 512] [--budget 24e9] [--out profiles/ese_grad_bench.json]

Per configuration: the forward under autograd and the backward of a loss over mean, logvar and posterior (host clock around
a device synchronise, second of two scenes), torch's max_memory_allocated over the forward and the backward, and the same
with every second member (35 members: the peak must not depend on the number of members beyond one chunk).  --budget is
the module's `member_budget_bytes` (default: the module's own), which under autograd bounds the tape of the members that share
a trunk pass, in the forward and again in the backward.
The two kernels of libmmlf_ese_hip.so alone, between HIP events, on random data of the scene's shapes: mmlf_ese_reduce_bwd
(S = 70) and mmlf_ese_unshift_sum (70 members, the four kinds), each beside its algorithmic bytes over the copy rate a 1 GiB
torch copy reaches in the same process.  The no_grad scene time is tools/ese_bench.py's.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmlf_amd import _lib, engine                           # noqa: E402
from mmlf_amd.ensamble import Ensamble, shift_table         # noqa: E402
from mmlf_amd.feed_forward import FeedForward               # noqa: E402

KW = dict(model_ksize=2, model_in_blocks=3, model_out_blocks=8, model_chs=70, model_views=9, model_cross=False,
          model_uncert=True, model_unet=False, model_discrete=False, model_no_batchnorm=False, model_batchnorm_momentum=0.1,
          val_disp_min=-3.5, val_disp_max=3.5)
DEV = torch.device('cuda:0')


def event_ms(fn, reps=5):
    """median milliseconds of fn() between HIP events, after one warm-up call"""
    fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def copy_rate():
    """bytes per second (read + written) of a 1 GiB device-to-device torch copy"""
    src = torch.empty(2 ** 28, dtype=torch.float32, device=DEV).normal_()
    dst = torch.empty_like(src)
    ms = event_ms(lambda: dst.copy_(src))
    return 2 * src.numel() * 4 / (ms * 1e-3)


def kernels(size, S, rate):
    res = {}
    H = W = size
    g = torch.Generator(device=DEV).manual_seed(0)
    rnd = lambda *shape: torch.rand(*shape, device=DEV, generator=g) * 2 - 1        # noqa: E731
    means, logvars, g_post = rnd(S, 1, H, W) * 3.5, rnd(S, 1, H, W), rnd(1, S, H, W)
    g_mean, g_logvar = rnd(1, H, W), rnd(1, H, W)
    grid = torch.linspace(-3.5, 3.5, S, device=DEV)
    g_means, g_logvars = torch.empty_like(means), torch.empty_like(means)
    ms = event_ms(lambda: _lib.call_ese('mmlf_ese_reduce_bwd', means.data_ptr(), logvars.data_ptr(), grid.data_ptr(),
                                        g_mean.data_ptr(), g_logvar.data_ptr(), g_post.data_ptr(), g_means.data_ptr(),
                                        g_logvars.data_ptr(), S, 1, H, W, _lib.stream_ptr()))
    nbytes = 4 * (5 * S + 2) * H * W                           # means, logvars, g_posterior read; two gradients written
    res['mmlf_ese_reduce_bwd'] = {'ms': ms, 'algorithmic_bytes': nbytes, 'ms_at_copy_rate': nbytes / rate * 1e3,
                                  'exponentials': S * S * H * W + S * H * W}
    del means, logvars, g_post, g_means, g_logvars
    views = KW['model_views']
    cs = engine.cs_of(3 * views)
    tab_s, tab_w = shift_table(np.arange(-3.5, 3.5, 0.1)[:S], views)
    tab_s, tab_w = torch.from_numpy(tab_s).to(DEV), torch.from_numpy(tab_w).to(DEV)
    gx = rnd(S * (H + 2) * (W + 2) * cs)
    out = torch.zeros((views, 3, H, W), device=DEV)
    nbytes = 4 * (S * (H + 2) * (W + 2) * cs + 2 * 3 * views * H * W)      # the members' gradients read; `out` read and written
    for kind, name in enumerate('hvid'):
        ms = event_ms(lambda: _lib.call_ese('mmlf_ese_unshift_sum', gx.data_ptr(), cs, kind, tab_s.data_ptr(), tab_w.data_ptr(),
                                            S, views, H, W, out.data_ptr(), _lib.stream_ptr()))
        res[f'mmlf_ese_unshift_sum kind {kind} ({name})'] = {'ms': ms, 'algorithmic_bytes': nbytes,
                                                             'ms_at_copy_rate': nbytes / rate * 1e3}
    return res


def scene(model, size, step, budget, frozen):
    """seconds of the forward under autograd and of the backward, and the allocator's peak, for the second of two scenes"""
    for p in model.parameters():
        p.requires_grad_(not frozen)
    ens = Ensamble(model, -3.5, 3.5, step).eval()
    ens.member_budget_bytes = budget
    S = len(ens.members())
    g = torch.Generator(device=DEV).manual_seed(1)
    res = {}
    for it in range(2):
        stacks = [torch.rand(1, 9, 3, size, size, device=DEV, generator=g).requires_grad_(True) for _ in range(4)]
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.time()
        out = ens(*stacks)
        loss = out['mean'].sum() + out['logvar'].sum() + out['posterior'].sum()
        torch.cuda.synchronize()
        t1 = time.time()
        peak_fwd = torch.cuda.max_memory_allocated()
        loss.backward()
        torch.cuda.synchronize()
        t2 = time.time()
        assert all(s.grad is not None for s in stacks) and all((p.grad is None) == frozen for p in model.parameters())
        res = {'finite': all(bool(torch.isfinite(s.grad).all()) for s in stacks),
               'members': S, 'members_per_pass': ens._chunk(model, S, size, size, taped=True), 'member_budget_bytes': ens.member_budget_bytes,
               'forward_s': t1 - t0, 'backward_s': t2 - t1, 'peak_forward_gib': peak_fwd / 2 ** 30,
               'peak_gib': torch.cuda.max_memory_allocated() / 2 ** 30}
        del out, loss, stacks
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--budget', type=float, default=24e9)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'ese_grad_bench.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'ese_grad_bench.py measures on the GPU: there is no CPU figure'
    torch.manual_seed(0)
    model = FeedForward(**KW).to(DEV).eval()
    rate = copy_rate()
    res = {'device': torch.cuda.get_device_name(0), 'build': _lib.build_info(), 'size': args.size,
           'copy_rate_tb_s': rate / 1e12, 'kernels': kernels(args.size, 70, rate)}
    print(json.dumps(res['kernels'], indent=1), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for frozen in (True, False):
        for step in (0.1, 0.2):
            key = f'{"frozen" if frozen else "trainable"} {len(np.arange(-3.5, 3.5, step))} members'
            res[key] = scene(model, args.size, step, args.budget, frozen)
            print(key, json.dumps(res[key]), flush=True)
            with open(args.out, 'w') as f:              # (after every scene: what was measured survives a later failure)
                json.dump(res, f, indent=1, sort_keys=True)
    print(f'copy rate {rate / 1e12:.2f} TB/s -> {args.out}')


if __name__ == '__main__':
    main()
