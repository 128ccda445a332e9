"""Times of the multimodal evaluation on one 512 x 512 scene.

kernels:  each of the three entry points of libmmlf_eval_hip.so between two HIP events (warm-up, then --repeats pairs of
          events around ten launches each), for S = 70 (the Ensamble's mixture) and S = 108 (DPP / UPR), beside its algorithmic
          bytes over the 6.29 TB/s copy rate this project measured (EXPERIMENTS.md): what a pass that only moved
          the data would take.
cpu:      this package's own CPU path on the same tensors (torch threads as the environment sets them): the only host-side
          comparison there is -- the reference's scripts do not run here (removed numpy aliases, skimage not installed).
validate: validate_scenes on the 70-member Ensamble, multimodal=True against multimodal=False taking turns scene by scene.
--root:   import mmlf_amd from another tree (a checkout of the parent commit) and time validate_scenes(multimodal=False
          there: absent) alone -- run both trees in turn to see that the default path did not change.
Prints one JSON object; --out also writes it.
    python tools/multimodal_bench.py [--size 512] [--repeats 20] [--warmup 5] [--scenes 3] [--out profiles/multimodal_bench.json]
    python tools/multimodal_bench.py --root <tree> --validate-default-only"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument('--size', type=int, default=512)
ap.add_argument('--repeats', type=int, default=20)
ap.add_argument('--warmup', type=int, default=5)
ap.add_argument('--scenes', type=int, default=3)
ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--validate-default-only', action='store_true')
ap.add_argument('--no-cpu', action='store_true')
ap.add_argument('--out', default=None)
ARGS = ap.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.root))
from mmlf_amd import synth, validate  # noqa: E402
from mmlf_amd.ensamble import Ensamble  # noqa: E402
from mmlf_amd.feed_forward import FeedForward  # noqa: E402

INNER = 10               # launches between two events
COPY_RATE = 6.29e12      # bytes/s, measured on this part (EXPERIMENTS.md)
KW = dict(model_ksize=2, model_in_blocks=3, model_out_blocks=8, model_chs=70, model_views=9, model_cross=False,
          model_uncert=True, model_unet=False, model_discrete=False, model_no_batchnorm=False,
          model_batchnorm_momentum=0.1, val_disp_min=-3.5, val_disp_max=3.5)


def event_ms(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def summary(ms, nbytes=None):
    row = {'ms': ms, 'ms_median': float(np.median(ms)), 'ms_min': float(min(ms))}
    if nbytes is not None:
        row['algorithmic_bytes'] = int(nbytes)
        row['ms_at_copy_rate'] = nbytes / COPY_RATE * 1e3
        row['median_over_copy_rate'] = row['ms_median'] / row['ms_at_copy_rate']
    return row


def posterior_like(s, n, dev, seed):
    """a Laplace mixture of two components per pixel on s bins, as the Ensamble's posterior is one of seventy"""
    g = torch.Generator().manual_seed(seed)
    bins = torch.linspace(-3.5, 3.5, s).view(1, s, 1, 1)
    p = torch.zeros(1, s, n, n)
    for _ in range(2):
        mu, b = torch.rand(1, 1, n, n, generator=g) * 6 - 3, torch.rand(1, 1, n, n, generator=g) * 0.5 + 0.1
        p += torch.exp(-(bins - mu).abs() / b) / (2 * b)
    return (p / p.sum(1, keepdim=True)).to(dev)


def kernels(dev, n):
    """the entry points themselves on preallocated outputs (no wrapper, no allocation between the events), INNER launches per
    pair of events: at 20-120 us a launch, the host's own time per call would otherwise be part of the figure"""
    from mmlf_amd import _lib, multimodal
    res = {}
    gt = torch.from_numpy(np.asarray(synth.synth_scene(0, n, n)[5])).float().unsqueeze(0).to(dev)
    pred = gt + 0.05 * torch.randn(gt.shape, generator=torch.Generator().manual_seed(1)).to(dev)
    pix = n * n
    stream = torch.cuda.current_stream().cuda_stream
    modes, edges = multimodal.gt_modes(gt, return_edges=True)
    out6 = torch.empty(6, dtype=torch.float64, device=dev)
    partials = torch.empty(multimodal._PARTIALS, dtype=torch.float64, device=dev)

    def timed(name, nbytes, entry, *args):
        def fn():
            for _ in range(INNER):
                _lib.call_eval(entry, *args, stream)
        res[name] = summary([ms / INNER for ms in event_ms(fn, ARGS.warmup, ARGS.repeats)], nbytes)
        res[name]['launches_per_event_pair'] = INNER

    timed('gt_modes', pix * (4 + 16 + 4), 'mmlf_eval_gt_modes', gt.data_ptr(), modes.data_ptr(), edges.data_ptr(), 1, n, n, 2.0, 0.5)
    res['gt_modes']['edge_share'] = float(edges.double().mean())
    cpu = {}
    for s in (70, 108):
        post = posterior_like(s, n, dev, s)
        n_modes, disp, cnt, prop = multimodal.posterior_analysis(post, -3.5, 3.5)
        timed(f'posterior_modes_S{s}', pix * (4 * s + 4 + 16 + 4 + 4), 'mmlf_eval_posterior_modes', post.data_ptr(), n_modes.data_ptr(),
              disp.data_ptr(), cnt.data_ptr(), prop.data_ptr(), 1, s, n, n, -3.5, 3.5, 2.0, 0.1)
        timed(f'two_mode_error_S{s}', pix * (16 + 4 + 16 + 4 + 4), 'mmlf_eval_two_mode_error', disp.data_ptr(), n_modes.data_ptr(),
              modes.data_ptr(), gt.data_ptr(), pred.data_ptr(), 1, n, n, 15, 0, partials.data_ptr(), out6.data_ptr())
        if not ARGS.no_cpu:
            c = [t.cpu() for t in (post, gt, pred)]
            t0 = time.perf_counter()
            m = multimodal.gt_modes(c[1])
            t1 = time.perf_counter()
            nm, d, _, _ = multimodal.posterior_analysis(c[0], -3.5, 3.5)
            t2 = time.perf_counter()
            multimodal.two_mode_error(d, nm, m, c[1], c[2])
            t3 = time.perf_counter()
            cpu[f'S{s}'] = {'gt_modes_ms': 1e3 * (t1 - t0), 'posterior_modes_ms': 1e3 * (t2 - t1), 'two_mode_error_ms': 1e3 * (t3 - t2),
                            'torch_threads': torch.get_num_threads()}
    if cpu:
        res['cpu_path'] = cpu
    return res


def validate_times(dev, n, settings):
    model = FeedForward(**KW)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_state(synth.param_spec(**KW), 4).items()})
    model.to(dev).eval()
    ens = Ensamble(model, -3.5, 3.5, 0.1)
    scenes = [tuple(torch.from_numpy(np.asarray(a)).unsqueeze(0).to(dev) for a in synth.synth_scene(k, n, n)[:8])
              + (torch.tensor([[k]]),) for k in range(ARGS.scenes)]
    times = {name: [] for name in settings}
    for rep in range(2):                                        # the first round warms up
        for scene in scenes:
            for name, kwargs in settings.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                validate.validate_scenes(ens, [scene], margin=15, **kwargs)
                torch.cuda.synchronize()
                if rep:
                    times[name].append(1e3 * (time.perf_counter() - t0))
    return {name: summary(ms) for name, ms in times.items()}


def main():
    if not torch.cuda.is_available():
        raise SystemExit('multimodal_bench: no GPU (a time taken anywhere else says nothing)')
    dev = torch.device('cuda:0')
    res = {'config': {'size': ARGS.size, 'repeats': ARGS.repeats, 'warmup': ARGS.warmup, 'scenes': ARGS.scenes,
                      'device': torch.cuda.get_device_name(0), 'root': os.path.basename(os.path.abspath(ARGS.root))}}
    if ARGS.validate_default_only:
        res['validate_scenes_ms_per_scene'] = validate_times(dev, ARGS.size, {'default': {}})
    else:
        res['kernels'] = kernels(dev, ARGS.size)
        res['validate_scenes_ms_per_scene'] = validate_times(dev, ARGS.size, {'multimodal_false': {'multimodal': False},
                                                                             'multimodal_true': {'multimodal': True}})
    line = json.dumps(res)
    print(line)
    if ARGS.out:
        os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
        with open(ARGS.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
