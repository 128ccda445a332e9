"""What a batch of PatchPipeline(chain=...) costs beside the fixed pipeline: 16 cached 512 x 512 scenes,
batches of 512 patches of 96 x 96, the host's draws and tables included.

    python tools/patch_chain_bench.py [--out profiles/patch_chain_bench.log]

Three arms, each 3 warm-up calls and 20 timed calls of sample() between HIP events (the median and the mean per call):
chain=None, the equivalent patches.cli_chain(96), and [RandomZoom, RandomCrop, Noise].  The cli_chain arm may take at most
the larger of 1.5 x the chain=None arm of the same run (the tables add two index loads per pixel) and 4.4 ms (1 % of the
443 ms BASE step); the script exits nonzero otherwise.
"""
import argparse
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mmlf_amd import patches, synth, transforms as T  # noqa: E402

B, PS, SCENES, SIZE, WARMUP, CALLS = 512, 96, 16, 512, 3, 20


def arm(pipe, idx):
    random.seed(1)
    for _ in range(WARMUP):
        pipe.sample(idx)
    torch.cuda.synchronize()
    times = []
    for _ in range(CALLS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        pipe.sample(idx)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.mean(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'patch_chain_bench.log'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'patch_chain_bench.py measures on the GPU: there is no CPU figure'
    scenes = [synth.synth_scene(s, SIZE, SIZE, planes=1) for s in range(SCENES)]
    random.seed(0)
    idx = [random.randrange(4096) for _ in range(B)]
    arms = (('chain=None', dict()),
            ('cli_chain', dict(chain=patches.cli_chain(PS))),
            ('RandomZoom + Noise', dict(chain=[T.RandomZoom(), T.RandomCrop(PS), T.Noise()], noise_seed=1)))
    lines = [f'{torch.cuda.get_device_name(0)}: {SCENES} scenes of {SIZE} x {SIZE}, bs {B}, ps {PS}, {WARMUP} warm-up and '
             f'{CALLS} timed calls of sample() between HIP events (host draws and tables included)']
    res = {}
    for name, kw in arms:
        res[name] = arm(patches.PatchPipeline(scenes, PS, **kw), idx)
        lines.append(f'{name:<20s} median {res[name][0]:8.3f} ms   mean {res[name][1]:8.3f} ms per call')
        print(lines[-1], flush=True)
    bar = max(1.5 * res['chain=None'][0], 4.4)
    ok = res['cli_chain'][0] <= bar
    lines.append(f'cli_chain {res["cli_chain"][0]:.3f} ms against the bar max(1.5 x {res["chain=None"][0]:.3f}, 4.4) = {bar:.3f} ms: '
                 f'{"within" if ok else "OVER"}')
    print(lines[-1])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
