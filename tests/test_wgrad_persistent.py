"""The persistent form of the wide f16 / bf16 weight gradient (csrc/wgrad.hip wgrad4tap_x6w_kernel: one workgroup per compute
unit walks the (slice, split) items of the launch; MMLF_WGRAD_PERSIST=0 launches one workgroup per item as before).

CPU: the listing of a launch by tools/wgrad_items.hip -- a host program on csrc/wgrad_map.h, the functions the kernel maps a
block with and the launch sizes its grid by -- covers every item once, keeps a workgroup's items on one XCD and in the one-shot
launch's order, under a cap of 8 and of 256 compute units.
GPU: the two arms write the same BYTES (the items are run exactly as the one-shot blocks ran them, accumulators zeroed per
item), at six trips under MMLF_CONV_CUS=8 and with the cap unset; the persistent arm against float64; and the batch at which
the full-size launch goes from one trip to three.  The kernel replaces the weight gradient of nn.Conv2d(k=2) under autograd
(reference mmlf/model/feed_forward.py:123,125).  The switches are read once per process: every arm is a child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (Cin, Cout): six slices, two slices, six slices with the ones row in a slice of its own 48th row, the column-block path
PAIRS = [(280, 280), (70, 280), (287, 280), (280, 320)]
# (B, H, W): at six slices 42 splits (one round) | 128 splits (the first batch of 96 x 96 patches with 42 * 1024 chunks) on 256
# compute units; under a cap of 8 the small geometries are cut into 8 splits
GEOMS = [(2, 5, 7), (3, 37, 41), (143, 96, 96), (144, 96, 96)]

def _nchunks(B, H, W):
    """32-position chunks of a launch on a (B, H, W) grid: the positions padded to whole 256-position tiles, as the library pads
    them (mmlf_relu_mask_words: 16 words per position group, tests/test_gpu_backward2x2.py _nqpad)"""
    from mmlf_amd import _lib
    return int(_lib.load().mmlf_relu_mask_words(B, H, W)) // 4096 * 256 // 32


@pytest.fixture(scope='module')
def lister(tmp_path_factory):
    """tools/wgrad_items.hip, compiled for the host: it lists a launch by the functions the kernel and its launch call
    (csrc/wgrad_map.h)"""
    from mmlf_amd.csrc import build
    if not os.path.exists(build.HIPCC):
        pytest.skip('no hipcc')
    exe = str(tmp_path_factory.mktemp('wgrad_items') / 'wgrad_items')
    subprocess.run([build.HIPCC, '--offload-arch=gfx950', '-I', build.HERE, os.path.join(ROOT, 'tools', 'wgrad_items.hip'), '-o', exe],
                   check=True, capture_output=True, text=True, timeout=300)

    def run(cin, nchunks, cus, persist):
        res = subprocess.run([exe, str(cin), str(nchunks), str(cus), str(persist)], check=True, capture_output=True, text=True)
        d = json.loads(res.stdout)
        return d['dims'], [tuple(it) for it in d['items']]
    return run


def test_the_chunk_counts_are_on_both_sides_of_the_three_round_threshold():
    assert _nchunks(143, 96, 96) < 42 * 1024 <= _nchunks(144, 96, 96)
    # 16 chunks: fewer than 42 splits (empty items); 160 chunks: 20 per split at 8 splits, 4 per split and two empty splits at 42
    assert (_nchunks(2, 5, 7), _nchunks(3, 37, 41)) == (16, 160)


@pytest.mark.parametrize('cus', [8, 256])
def test_persistent_launch_walks_every_item_once_in_one_shot_order(lister, cus):
    seen_splits, seen_trips = set(), set()
    for cin, cout in PAIRS:                  # (Cout > 128 selects the wide kernel; of 320 columns it runs the first 288)
        for geom in GEOMS:
            key = (cin, cout, geom)
            n = _nchunks(*geom)
            (grid1, trips1, nslice1, nsplit1), blocks = lister(cin, n, cus, 0)     # the one-shot launch: block b -> item
            (grid, trips, nslice, nsplit), flat = lister(cin, n, cus, 1)
            assert (nslice1, nsplit1) == (nslice, nsplit) and trips1 == 1, key     # the switch changes the grid alone
            assert nslice == {280: 6, 70: 2, 287: 6}[cin]
            assert grid % 8 == 0 and grid <= cus and grid == min(grid1, cus), (key, grid)
            # (csrc/wgrad_map.h wgrad_wide_splits, transcribed: one round of the compute units, or three rounds of 256 from
            # 42 * 1024 chunks on)
            assert nsplit == ((768 // nslice + 7) // 8 * 8 if geom[0] == 144 else max(8, cus // nslice)), (key, nsplit)
            seen_splits.add(nsplit)
            seen_trips.add(trips)
            assert trips * grid >= grid1 > (trips - 1) * grid, (key, grid, trips)
            assert len(flat) == grid * trips and len(blocks) == grid1
            items = [flat[g * trips:(g + 1) * trips] for g in range(grid)]
            # every (slice, split) exactly once
            real = [it for row in items for it in row if it != (-1, -1)]
            assert sorted(real) == [(s, p) for s in range(nslice) for p in range(nsplit)], key
            for g, row in enumerate(items):
                # in the one-shot launch's block order: trip t of workgroup g is block g + t * grid -- hence all on XCD g & 7
                for t, it in enumerate(row):
                    b = g + t * grid
                    assert it == (blocks[b] if b < grid1 else (-1, -1)), (key, g, t)
                    assert b & 7 == g & 7
            xcd_of_split = {}             # the slices of a regular split share an XCD (their gradient reads meet in its L2)
            for g, row in enumerate(items):
                for it in row:
                    if it != (-1, -1) and it[1] < nsplit // 8 * 8:
                        assert xcd_of_split.setdefault(it[1], g & 7) == g & 7, (key, it)
    assert seen_splits == ({42, 128, 384} if cus == 256 else {8, 128, 384}), seen_splits
    assert seen_trips == ({1, 3} if cus == 256 else {2, 6, 96}), seen_trips


# ------------------------------------------------------------------------------------------------ GPU

ARM = r'''
import sys, numpy as np, torch
sys.path.insert(0, %r)
sys.path.insert(0, %r)
from mmlf_amd import engine, _lib
from tests_helpers import unfilter4, wgrad4_ref
dev = torch.device('cuda:0')
assert engine.CONV_MODE == 'f16x3'
out = {}
for B, H, W in ((2, 5, 7), (3, 37, 41)):
    geo = engine.Geometry(B, H, W)
    for cin, cout in ((280, 280), (70, 280)):
        cs_in, cs_g = engine.cs_of(cin), engine.cs_of(cout)
        ws = torch.empty(int(_lib.load().mmlf_wgrad_workspace_floats(cin, cout, B, H, W)), device=dev)
        for pad in (1, 0):
            rs = np.random.RandomState(B + cin + pad)
            ih, iw, ioff = (H, W, 1) if pad else (H + 1, W + 1, 0)
            oh, ow, ooff = (H + 1, W + 1, 0) if pad else (H, W, 1)
            # rows many binades apart in both operands
            xv = rs.standard_normal((B, ih, iw, cin)) * np.exp(rs.uniform(-6, 6, (B, ih, 1, 1)))
            gv = rs.standard_normal((B, oh, ow, cout)) * np.exp(rs.uniform(-6, 6, (B, oh, 1, 1)))
            x, g = torch.zeros(geo.alloc * cs_in, device=dev), torch.zeros(geo.alloc * cs_g, device=dev)
            xg, gg = (t[:geo.NQ * cs].view(B, geo.R, geo.P, cs) for t, cs in ((x, cs_in), (g, cs_g)))
            xg[:, ioff:ioff + ih, ioff:ioff + iw, :cin] = torch.from_numpy(xv.astype(np.float32)).to(dev)
            gg[:, ooff:ooff + oh, ooff:ooff + ow, :cout] = torch.from_numpy(gv.astype(np.float32)).to(dev)
            x.absmax, g.absmax = geo.amax_of(x, cs_in), geo.amax_of(g, cs_g)
            ref_w, ref_b = wgrad4_ref(xg[..., :cin].double(), gg[..., :cout].double(), pad)
            for variant in (0, 2):
                gw, gb = torch.zeros((cout, cin, 2, 2), device=dev), torch.zeros(cout, device=dev)
                engine.wgrad(geo, x, cs_in, cin, g, cs_g, cout, 0 if pad else geo.P + 1, gw, gb, variant, ws)
                key = f'{B}x{H}x{W} {cin}->{cout} pad{pad} v{variant}'
                out['gw ' + key], out['gb ' + key] = gw.cpu().numpy(), gb.cpu().numpy()
                out['rw ' + key], out['rb ' + key] = unfilter4(ref_w, variant).cpu().numpy(), ref_b.cpu().numpy()
torch.cuda.synchronize()
out['cus'] = np.int64(_lib.load().mmlf_conv_cus())
np.savez(sys.argv[1], **out)
''' % (ROOT, os.path.join(ROOT, 'tests'))


@pytest.mark.gpu
@pytest.mark.parametrize('cus', ['8', None])
def test_persistent_and_one_shot_launch_write_the_same_bytes(tmp_path, cus):
    """MMLF_CONV_CUS=8: 8 splits x 6 slices = 48 items on 8 workgroups, six trips (two at the two slices of 70 -> 280); cap
    unset: one trip.  2 x 5 x 7 (16 chunks) has fewer chunks than its 42 splits with the cap unset (empty items write
    zero partial sums), 3 x 37 x 41 (160 chunks) leaves the last two of 42 splits empty and runs 20 chunks per item under the cap.  Both placements of the gradient, variant 0 and a stream variant."""
    arms = []
    for persist in ('0', '1'):
        env = dict(os.environ, MMLF_WGRAD_PERSIST=persist)
        env.pop('MMLF_CONV_CUS', None)
        env.pop('MMLF_CONV_MODE', None)
        if cus:
            env['MMLF_CONV_CUS'] = cus
        out = str(tmp_path / f'persist{persist}.npz')
        res = subprocess.run([sys.executable, '-c', ARM, out], env=env, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stderr[-3000:]
        arms.append(np.load(out))
    a0, a1 = arms
    assert int(a1['cus']) == int(a0['cus']) and (cus is None or int(a1['cus']) == 8)
    keys = [k for k in a1.files if k.startswith('g')]
    assert len(keys) == 2 * 2 * 2 * 2 * 2
    for k in keys:
        assert a0[k].tobytes() == a1[k].tobytes(), k
        ref = a1['r' + k[1:]]                                    # float64, at the tolerance of test_conv_backward
        print(k, 'max |err| / max |ref| =', float(np.abs(a1[k] - ref).max() / np.abs(ref).max()))
        np.testing.assert_allclose(a1[k], ref, rtol=1e-4, atol=2e-5 * np.abs(ref).max(), err_msg=k)


@pytest.mark.gpu
def test_one_trip_and_three_trips_at_the_full_size_threshold():
    """280 -> 280 on 96 x 96 patches: B = 144 is the first batch cut into 128 splits (768 items: three trips on 256 compute
    units), B = 143 beside it into 42 (one trip).  Both against a float64 weight gradient on the GPU (the shared bar:
    2e-5 * sum |a||b| + 1e-6 * max); B = 143 reads the first 143 patches of the same tensors."""
    from mmlf_amd import engine, _lib
    from tests_helpers import check_sum_bar, wgrad4_ref
    dev = torch.device('cuda:0')
    cin = cout = cs = 280
    H = W = 96
    gen = torch.Generator(device=dev).manual_seed(144)
    big = engine.Geometry(144, H, W)
    x, g = torch.zeros(big.alloc * cs, device=dev), torch.zeros(big.alloc * cs, device=dev)
    xg, gg = (t[:big.NQ * cs].view(144, big.R, big.P, cs) for t in (x, g))
    for b0 in range(0, 144, 48):
        xg[b0:b0 + 48, 1:H + 1, 1:W + 1] = torch.rand((48, H, W, cs), device=dev, generator=gen) * 2 - 1
        gg[b0:b0 + 48, :H + 1, :W + 1] = torch.rand((48, H + 1, W + 1, cs), device=dev, generator=gen) * 2 - 1
    # float64 sums over the first 143 patches and over the last one, with the bar's sum of absolute products
    ref = {}
    for name, lo, hi in (('head', 0, 143), ('last', 143, 144)):
        acc = None
        for b0 in range(lo, hi, 13):
            xs, gs = xg[b0:min(hi, b0 + 13)].double(), gg[b0:min(hi, b0 + 13)].double()
            part = [*wgrad4_ref(xs, gs, 1), *wgrad4_ref(xs.abs(), gs.abs(), 1)]
            acc = part if acc is None else [p + q for p, q in zip(acc, part)]
        ref[name] = acc
    lib = _lib.load()
    ws = torch.empty(int(lib.mmlf_wgrad_workspace_floats(cin, cout, 144, H, W)), device=dev)
    for B in (143, 144):
        geo = engine.Geometry(B, H, W)
        assert (_nchunks(B, H, W) >= 42 * 1024) == (B == 144)       # (the CPU test lists both launches: 256 x 3 and 256 x 1)
        xb, gb_ = x[:geo.alloc * cs].clone(), g[:geo.alloc * cs].clone()
        xb[geo.NQ * cs:] = 0                   # (B = 143: the 144th patch lies where this geometry has its zeroed tail)
        gb_[geo.NQ * cs:] = 0
        xb.absmax, gb_.absmax = geo.amax_of(xb, cs), geo.amax_of(gb_, cs)
        gw, gb = torch.zeros((cout, cin, 2, 2), device=dev), torch.zeros(cout, device=dev)
        engine.wgrad(geo, xb, cs, cin, gb_, cs, cout, 0, gw, gb, 0, ws)
        want = ref['head'] if B == 143 else [p + q for p, q in zip(ref['head'], ref['last'])]
        check_sum_bar(gw.double(), want[0], want[2], f'gw B={B}')
        check_sum_bar(gb.double(), want[1], want[3], f'gb B={B}')
