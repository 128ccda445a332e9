"""The persistent 2x2 convolution walks (csrc/conv.hip conv4tap_x6s_kernel, conv4tap_rs_kernel, thin_rowdot_kernel; csrc/wgrad.hip
thin_wgrad_kernel) under a cap of the compute units.  On 256 compute units every frame of the suite's edge lists is one tile
per workgroup; MMLF_CONV_CUS = 8 | 9 makes the frames of tests/test_conv_walk_cpu.py walk three trips and more, through the
kernels' XCD-ordered branch (8, 16 workgroups) and their linear one (9, 18), which no multi-trip launch ran before.

Three arms -- cap unset, 8, 9 -- one child process each (tests/conv_walk_arm.py; the library reads the cap once per process),
strictly one after another; an arm that does not return 0 ends the sequence and fails every test that needs it or a later one.
Each arm holds every launch to its own float64 reference: exact-integer operands bit for bit, mixed-magnitude operands (the
two tiles of a hand-over 2^10 and more apart) at the shared bars, the BatchNorm sums, the thin kernels, one net.  Between
the arms, here: a tile's result does not depend on which workgroup ran it -- the per-tile digests, the canonical amax arrays and
the ReLU mask words of every forward and data-gradient launch are equal.  Weight gradients and BatchNorm partial sums regroup
their sums under a cap: they are held to their references, not to each other.

Replaces nn.Conv2d(k=2) forward / backward where MMLF_CONV_CUS leaves compute units to a collective under data parallelism
(reference mmlf/model/feed_forward.py:123,125)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_conv_walk_cpu import BN_CASES, CAPS, CASES, F32_CASES, MODES, cap_env, plan, trips

pytestmark = pytest.mark.gpu

ARM = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'conv_walk_arm.py')


@pytest.fixture(scope='module')
def arms(tmp_path_factory):
    """{cap: the arm's .npz, or the text of its failure}; after a failed arm no further arm is started"""
    tmp = tmp_path_factory.mktemp('conv_walk')
    out, failed = {}, None
    for cap in CAPS:
        if failed is not None:
            out[cap] = f'not started: the arm with MMLF_CONV_CUS={failed[0]} failed first\n{failed[1]}'
            continue
        path = str(tmp / f'cap_{cap}.npz')
        try:
            res = subprocess.run([sys.executable, ARM, path, str(tmp)], env=cap_env(cap), capture_output=True, text=True, timeout=600)
            rc, err = res.returncode, res.stderr
        except subprocess.TimeoutExpired as e:
            rc, err = 'timeout', (e.stderr or b'').decode(errors='replace') if isinstance(e.stderr, bytes) else (e.stderr or '')
        if rc != 0:
            failed = (cap, f'MMLF_CONV_CUS={cap}: exit status {rc}\n{err[-3000:]}')
            out[cap] = failed[1]
        else:
            print(res.stdout)
            out[cap] = np.load(path)
    return out


def need(arms, *caps):
    for cap in caps:
        if isinstance(arms[cap], str):
            pytest.fail(arms[cap], pytrace=False)
    return [arms[cap] for cap in caps]


@pytest.mark.parametrize('cap', CAPS)
def test_every_launch_of_the_arm_met_its_float64_reference(arms, cap):
    """the arm's own assertions: exact-integer and mixed-magnitude forward and data gradient, BatchNorm sums, thin kernels, net"""
    a, = need(arms, cap)
    assert json.loads(str(a['failures'])) == []
    assert (int(a['cus']) == cap) if cap else int(a['cus']) > 18
    ratios, times = json.loads(str(a['ratios'])), json.loads(str(a['times']))
    print(f'MMLF_CONV_CUS={cap}: {times["total"]:.1f} s in the arm ' + ' '.join(f'{k} {v:.1f}' for k, v in times.items()))
    for k in sorted(ratios):
        print(f'  largest error / bound, {k}: {ratios[k]:.3g}')
    assert all(v <= 1.0 for v in ratios.values()), ratios
    # every mode and leg left its figures
    for mode in MODES:
        for k in (f'sum_bar mixed forward {mode}', f'sum_bar mixed dgrad {mode}', f'net output {mode}'):
            assert k in ratios, k
    assert 'f16x3_bound mixed forward f16x3' in ratios and 'f16x3_bound mixed dgrad f16x3' in ratios


@pytest.mark.parametrize('cap', CAPS)
def test_the_arm_launched_the_workgroups_the_lists_count_on(arms, cap):
    """what the CPU file derives from the host queries holds on the device: one trip with the cap unset, three and more under
    a cap; the BatchNorm legs saw exactly that many rows (asserted in the arm against the NaN behind them)"""
    a, = need(arms, cap)
    cus = int(a['cus'])
    for frame, (K, N), *_ in CASES:
        _, _, ntiles, blocks = plan('f16x3', K, N, frame, cus)
        assert int(a['blocks %d %d %d %d %d' % (K, N, *frame)]) == blocks, (K, N, frame)
        assert (trips(ntiles, blocks) >= 3) if cap else (trips(ntiles, blocks) == 1)
    assert all('blocks %d %d %d %d %d' % (K, N, *frame) in a.files for frame, (K, N) in BN_CASES)


@pytest.mark.parametrize('cap', [8, 9])
def test_a_tiles_result_does_not_depend_on_the_workgroup_that_ran_it(arms, cap):
    """every forward and data-gradient launch of the tiled and register-streamed kernels, every mode and leg: the digest of
    each 256-position tile of the output buffer, the canonical amax array and the ReLU mask words equal the uncapped arm's"""
    base, a = need(arms, None, cap)
    cus = int(a['cus'])
    keys = [k for k in base.files if k.split(' ')[0] in ('tiles', 'amax', 'mask')]
    assert sorted(keys) == sorted(k for k in a.files if k.split(' ')[0] in ('tiles', 'amax', 'mask'))
    seen = {'tiles': 0, 'amax': 0, 'mask': 0}
    for k in keys:
        kind = k.split(' ')[0]
        seen[kind] += 1
        x, y = base[k], a[k]
        if x.tobytes() == y.tobytes():
            continue
        t = int(np.flatnonzero(x != y)[0]) if x.shape == y.shape else -1
        if kind == 'amax':
            pytest.fail(f'MMLF_CONV_CUS={cap}, {k}: amax entry {t} holds {y[t]!r}, uncapped {x[t]!r}', pytrace=False)
        # '<kind> <leg> <mode> | K->N BxHxW #n'
        mode = k.split(' | ')[0].split(' ')[-1]
        K, N = (int(v) for v in k.split(' | ')[1].split(' ')[0].split('->'))
        frame = tuple(int(v) for v in k.split(' | ')[1].split(' ')[1].split('x'))
        _, tile, _, blocks = plan(mode, K, N, frame, cus) if mode != 'f32' else (None, 256, None, 10 ** 9)
        pytest.fail(f'MMLF_CONV_CUS={cap}, {k}: 256-position tile {t} differs from the uncapped arm: trip {t * 256 // tile // blocks} '
                    f'of its workgroup ({blocks} workgroups, {tile}-position tiles)', pytrace=False)
    # per case the f16 split launches 11 times (forward, the data gradient's three ReLU forms and the forward launch that writes
    # the mask words, its channel slice; the first five again in the other leg), the bf16 split and the control 7 times
    assert seen['tiles'] == len(CASES) * (11 + 7) + len(F32_CASES) * 7 + len(BN_CASES), seen
    assert seen['amax'] == len(CASES) * 10 + len(BN_CASES) and seen['mask'] == len(CASES) * 2, seen


def test_the_net_gives_the_same_bytes_in_every_arm(arms):
    """the 70-channel model_no_batchnorm net at 6 x 33 x 37 on mixed-magnitude stacks, train mode: the output and the four
    input gradients byte for byte (the parameter gradients are held to float64 in each arm)"""
    base, a8, a9 = need(arms, *CAPS)
    keys = [k for k in base.files if k.startswith('net ')]
    assert len(keys) == len(MODES) * 6
    for k in keys:
        for cap, a in ((8, a8), (9, a9)):
            assert base[k].tobytes() == a[k].tobytes(), (cap, k)
