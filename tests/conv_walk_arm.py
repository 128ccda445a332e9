"""One arm of tests/test_gpu_conv_walk.py: every case of tests/test_conv_walk_cpu.py on the GPU, in a process of its own
(MMLF_CONV_CUS is read once per process), each result against its float64 reference.

    python tests/conv_walk_arm.py OUT.npz SHARED_DIR

OUT.npz receives, for every forward and data-gradient launch (in launch order, which the seeds make the same in every arm):
an 8-byte digest per 256-position tile of the output buffer, the canonical amax array, a digest per tile of the ReLU mask words;
the largest error / bound seen per leg and mode; the workgroup counts; the net's digests.  Never the tensors themselves.
SHARED_DIR keeps the float64 CPU run of the net, computed by the first arm that gets there.
A failed comparison does not stop the arm: the failures are listed on stderr and in OUT.npz, and the exit status is 1.

The legs (MMLF_CONV_CUS):
  exact-integer     tests/test_gpu_wide.py _forward and tests/test_gpu_backward2x2.py _Case as they are: bit equality with
                    float64 on every position the launch writes, the fill everywhere else -- a dropped, doubled or misplaced
                    tile, an accumulator that was not cleared;
  mixed-magnitude   operands uniform in [-1, 1), image b scaled by 2^E_CYCLE[b % 6] (bands of four grid rows on frames of
                    fewer than four images), so that the two tiles of a hand-over differ in magnitude: forward and data
                    gradient at check_sum_bar per image and, in the f16 split, at f16x3_bound per output with M the maximum
                    of the rows the wave reads (_row_scale_max) -- an operand scale handed over late costs bits or overflows;
  BatchNorm sums    exactly mmlf_conv2x2_blocks rows under the arm's cap, finalized against bn_stats_ref of the stored output;
  thin kernels      forward on every position of the grid, weight gradient with both legs of _Case.check_wgrad and between
                    guard bands with the workspace sized by the query under the arm's cap;
  net               the 70-channel model_no_batchnorm net of tests/test_gpu_nobn.py on mixed-magnitude stacks."""
import collections
import hashlib
import inspect
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import test_gpu_backward2x2 as b2                                                     # noqa: E402
import test_gpu_wide as wd                                                            # noqa: E402
from test_conv_walk_cpu import (BN_CASES, CASES, E_CYCLE, F32_CASES, MODES, NET_FRAME, THIN_CASES, row_exponents)   # noqa: E402
from test_gpu_backward2x2 import SENTINEL, _Case, _compare, _draw, _fresh, _seed, _view, _written       # noqa: E402
from test_gpu_precision import _row_scale_max, f16x3_bound                            # noqa: E402
from test_gpu_wide import _forward                                                    # noqa: E402
from tests_helpers import bn_stats_ref, check_sum_bar, conv4_ref, dgrad4_ref, filter4   # noqa: E402
from mmlf_amd import _lib, engine                                                     # noqa: E402
from mmlf_amd._lib import call, ptr                                                   # noqa: E402

DEV = torch.device('cuda:0')
OUT = {}                 # what goes into the .npz
RATIO = {}               # 'leg mode' -> largest error / bound
FAILURES = []


def note(key, ratio):
    RATIO[key] = max(RATIO.get(key, 0.0), float(ratio))


# ---------------------------------------------------------------------------------------------- digests of the launches
_MULT = {}


def tile_digest(t, per_position):
    """one int64 per 256-position tile of a float32 / int32 buffer: the sum of its words times fixed odd multipliers, mod 2^64"""
    n = 256 * per_position
    words = t.view(torch.int32).to(torch.int64)
    pad = -words.numel() % n
    if pad:
        words = torch.cat([words, words.new_zeros(pad)])
    if n not in _MULT:
        g = torch.Generator().manual_seed(n)
        _MULT[n] = (torch.randint(-2 ** 62, 2 ** 62, (n,), generator=g, dtype=torch.int64) * 2 + 1).to(DEV)
    return (words.view(-1, n) * _MULT[n]).sum(1).cpu().numpy()


class Recorder:
    """engine.conv, and a record of what every launch left behind (off: the launches pass through unrecorded)"""

    def __init__(self):
        self.real, self.tag, self.n, self.launches, self.on = engine.conv, '', 0, [], True
        self.sig = inspect.signature(engine.conv)

    def start(self, tag):
        self.tag, self.n, self.launches = tag, 0, []

    def __call__(self, *args, **kwargs):
        self.real(*args, **kwargs)
        bound = self.sig.bind(*args, **kwargs)
        bound.apply_defaults()
        kw = bound.arguments
        if not self.on or kw['w_master'] is not None:
            return
        geo, out = kw['geo'], kw['out']
        key = f'{self.tag} #{self.n}'
        self.n += 1
        self.launches.append((out, kw))
        OUT['tiles ' + key] = tile_digest(out, kw['cs_out'])
        if getattr(out, 'absmax', None) is not None:
            OUT['amax ' + key] = geo.amax_canonical(out.absmax).cpu().numpy()
        if kw['mask_out'] is not None:
            OUT['mask ' + key] = tile_digest(kw['mask_out'], 16)


REC = Recorder()
engine.conv = REC

# ---------------------------------------------------------------------------------------------- the mixed-magnitude operands
MIXED = [False]
LEG = ['']
_plain_grid_rand = b2._grid_rand


def _grid_rand(geo, C, cs, off, h, w, gen, integer, values=(-2, -1, 1, 2)):
    """tests/test_gpu_backward2x2.py _grid_rand; in the mixed-magnitude leg every grid row times its power of two"""
    t = _plain_grid_rand(geo, C, cs, off, h, w, gen, integer, values)
    if MIXED[0] and not integer:
        e = row_exponents((geo.B, geo.H, geo.W), 0, geo.R)
        _view(geo, t, cs).mul_(torch.tensor(np.exp2(np.array(e, np.float64)), dtype=torch.float32, device=t.device)
                               .view(geo.B, geo.R, 1, 1))
    return t


def _check_sum_bar(got, ref, bound, what, tol=2e-5):
    """tests_helpers.check_sum_bar, its ratio noted"""
    lim = tol * bound + 1e-6 * float(bound.max()) + 1e-30
    note('sum_bar ' + LEG[0], ((got - ref).abs() / lim).max())
    return check_sum_bar(got, ref, bound, what, tol)


b2._grid_rand = wd._grid_rand = _grid_rand
b2.check_sum_bar = _check_sum_bar


def _images(v):
    """a grid view's extent (B, h, w, C) as the NCHW numpy array _row_scale_max takes"""
    return v.permute(0, 3, 1, 2).cpu().numpy()


def _f16_bound(got, ref, mag, wabs, M, K, what, key):
    bound = f16x3_bound(mag, wabs.view(1, 1, 1, -1) * torch.from_numpy(M).to(DEV)[:, :, None, None], K)
    ratio = float(((got - ref).abs() / bound).max())
    note(key, ratio)
    assert ratio <= 1.0, (what, 'error / f16x3_bound', ratio)


def mixed_forward(mode, frame, K, N, pad, variant, relu, sliced):
    """one forward launch K -> N on mixed-magnitude rows, without a bias (it would carry the small images' outputs)"""
    B, H, W = frame
    engine.CONV_MODE = mode
    geo = engine.Geometry(B, H, W)
    gen = torch.Generator(device=DEV).manual_seed(_seed(B, H, W, K, N, pad, False) + 17)
    cs_in, cs_out = engine.cs_of(K), engine.cs_of(N)
    ih, iw, ioff = (H, W, 1) if pad else (H + 1, W + 1, 0)
    oh, ow, ooff = (H + 1, W + 1, 0) if pad else (H, W, 1)
    shift = 0 if pad else geo.P + 1
    x = _grid_rand(geo, K, cs_in, ioff, ih, iw, gen, False)
    w = _draw((N, K, 2, 2), gen, False) / np.sqrt(4 * K)
    wv = filter4(w.double(), variant)
    xv = _view(geo, x, cs_in)[..., :K]
    what = f'mixed forward {mode} {K}->{N} B={B} {H}x{W} pad={pad} variant={variant} relu={relu} sliced={sliced}'

    def want(b0, b1):
        xd = xv[b0:b1].double()
        val = conv4_ref(xd, wv, None, pad)
        return (val.clamp_min(0) if relu else val), conv4_ref(xd.abs(), wv.abs(), None, pad)

    off, cs_buf, n_store, fill = (8, cs_out + 16, N, SENTINEL) if sliced else (0, cs_out, cs_out, 0.0)
    out = _fresh(geo, cs_out, cs_buf, off, n_store, shift, fill, DEV)
    if mode == 'f16x3':
        out.absmax = torch.zeros(geo.amax_n, device=DEV)
    engine.conv(geo, x, cs_in, K, engine.pack_filter(w, variant, False), None, N, out, cs_buf, shift, oh, ow, relu,
                n_store=n_store, out_off=off)
    assert bool(torch.isfinite(out).all()), (what, 'not finite')
    _written(geo, out, cs_buf, off, n_store, ooff, oh, ow, shift, want, 1, fill, False, what)          # per image
    if mode == 'f16x3':
        got = _view(geo, out, cs_buf)[:, ooff:ooff + oh, ooff:ooff + ow, off:off + N].double()
        ref, mag = want(0, B)
        M = _row_scale_max(_images(xv[:, ioff:ioff + ih, ioff:ioff + iw]), pad)
        _f16_bound(got, ref, mag, wv.abs().sum((1, 2, 3)), M, K, what, 'f16x3_bound ' + LEG[0])


def mixed_dgrad(mode, c):
    """_Case's data gradient on mixed-magnitude rows: its three ReLU forms at check_sum_bar per image, the plain form at
    f16x3_bound per output"""
    c.chunk = 1
    c.check_dgrad(mode)
    out = [o for o, kw in REC.launches if kw['ref'] is None and kw['mask_in'] is None and kw['mask_out'] is None]
    assert len(out) == 1
    assert all(bool(torch.isfinite(o).all()) for o, _ in REC.launches), (c.tag, 'not finite')
    if mode == 'f16x3':
        o = c.ioff
        got = _view(c.geo, out[0], c.cs_in)[:, o:o + c.ih, o:o + c.iw, :c.cin].double()
        gd = c.gv.double()
        ref, mag = dgrad4_ref(gd, c.wv, c.pad), dgrad4_ref(gd.abs(), c.wv.abs(), c.pad)
        M = _row_scale_max(_images(c.gv[:, c.ooff:c.ooff + c.oh, c.ooff:c.ooff + c.ow]), 1 - c.pad)
        _f16_bound(got, ref, mag, c.wv.abs().sum((0, 2, 3)), M, c.cout, f'mixed data gradient {mode} {c.tag}',
                   'f16x3_bound ' + LEG[0])


# ---------------------------------------------------------------------------------------------- the legs
def leg(name, fn, *args):
    LEG[0] = name.split(' | ')[0]
    REC.start(name)
    try:
        fn(*args)
    except AssertionError as e:
        FAILURES.append(f'{name}: {str(e)[:600]}')


def conv_case(modes, frame, layer, pad, variant, relu, sliced):
    (B, H, W), (K, N) = frame, layer
    tag = f'{K}->{N} {B}x{H}x{W}'
    for integer in (True, False):
        MIXED[0] = not integer
        p = pad if integer else 1 - pad
        c = _Case(B, H, W, N, K, p, variant, integer, _seed(B, H, W, N, K, p, integer))      # its data gradient is a K -> N launch
        for mode in modes:
            if integer:
                leg(f'integer forward {mode} | {tag}', _forward, mode, B, H, W, K, N, pad, variant, relu, True, sliced)
                leg(f'integer dgrad {mode} | {tag}', c.check_dgrad, mode)
                leg(f'integer dgrad_slice {mode} | {tag}', c.check_dgrad_slice, mode)
            else:
                leg(f'mixed forward {mode} | {tag}', mixed_forward, mode, frame, K, N, p, variant, not relu, not sliced)
                leg(f'mixed dgrad {mode} | {tag}', mixed_dgrad, mode, c)
    MIXED[0] = False


def bn_case(frame, layer):
    """the f16 split's pad-0 forward with the epilogue's BatchNorm sums (tests/test_gpu_wide.py
    test_wide_epilogue_batchnorm_statistics, through engine.conv): exactly `blocks` rows, the 8 doubles behind them untouched"""
    (B, H, W), (K, N) = frame, layer
    engine.CONV_MODE = 'f16x3'
    geo = engine.Geometry(B, H, W)
    cs_in, cs_out = engine.cs_of(K), engine.cs_of(N)
    gen = torch.Generator(device=DEV).manual_seed(N + W)
    x = _plain_grid_rand(geo, K, cs_in, 0, H + 1, W + 1, gen, False).abs_()
    w = (torch.rand((N, K, 2, 2), device=DEV, generator=gen) - 0.5) * 0.1
    bias = torch.rand(N, device=DEV, generator=gen) - 0.5
    z = geo.buf(cs_out, DEV)
    nblk = int(_lib.load().mmlf_conv2x2_blocks(K, N, B, H, W))
    OUT[f'blocks {K} {N} {B} {H} {W}'] = np.int64(nblk)
    partial = torch.full((nblk * 2 * N + 8,), float('nan'), dtype=torch.float64, device=DEV)
    engine.conv(geo, x, cs_in, K, engine.pack_filter(w, 0, False), bias, N, z, cs_out, geo.P + 1, H, W, False, bn_partial=partial)
    rows = partial[:nblk * 2 * N].view(nblk, 2 * N)
    assert bool(torch.isnan(partial[nblk * 2 * N:]).all()), 'the doubles behind the last row were written'
    assert bool(torch.isfinite(rows).all()), ('rows left unwritten', torch.isnan(rows).any(1).nonzero().flatten().tolist())
    gamma, beta = torch.rand(N, device=DEV, generator=gen) + 0.5, torch.rand(N, device=DEV, generator=gen) - 0.5
    rm, rv = torch.full((N,), 0.25, device=DEV), torch.full((N,), 2.0, device=DEV)
    ref = bn_stats_ref(_view(geo, z, cs_out)[..., :N].double(), gamma.double(), beta.double(), rm.double(), rv.double(), 0.1, 1e-5)
    c = torch.empty(4 * N, device=DEV)
    call('mmlf_bn_stats_finalize', ptr(partial), nblk, N, ptr(gamma), ptr(beta), ptr(rm), ptr(rv), 0.1, 1e-5,
         ptr(c[2 * N:]), ptr(c[3 * N:]), ptr(c), ptr(c[N:]), B, H, W, _lib.stream_ptr())
    for got, want, name in zip((c[2 * N:3 * N], c[3 * N:], c[:N], c[N:2 * N], rm, rv), ref,
                               ('mean', 'invstd', 'scale', 'shift', 'running_mean', 'running_var')):
        g, r = got.double().cpu().numpy(), want.cpu().numpy()
        note('batchnorm f16x3', (np.abs(g - r) / (1e-7 + 2e-6 * np.abs(r))).max())
        np.testing.assert_allclose(g, r, rtol=2e-6, atol=1e-7, err_msg=f'{name} {K}->{N} B={B} {H}x{W}')
    assert torch.equal(geo.amax_canonical(z.absmax)[0], geo.amax_of(z, cs_out)[0])


def thin_case(frame, layer, pad, variant):
    (B, H, W), (K, N) = frame, layer
    geo = engine.Geometry(B, H, W)
    cs_in, cs_out = engine.cs_of(K), engine.cs_of(N)
    ih, iw, ioff = (H, W, 1) if pad else (H + 1, W + 1, 0)
    oh, ow, ooff = (H + 1, W + 1, 0) if pad else (H, W, 1)
    shift = 0 if pad else geo.P + 1
    gen = torch.Generator(device=DEV).manual_seed(_seed(B, H, W, K, N, pad, False) + 5)
    x = _plain_grid_rand(geo, K, cs_in, ioff, ih, iw, gen, False)
    w, bias = _draw((N, K, 2, 2), gen, False) * 0.5, _draw((N,), gen, False) * 0.5
    # forward (bias, ReLU) at the bar of test_thin_convolution_and_weight_gradient, on every position of the grid
    out = geo.buf(cs_out, DEV)
    out.fill_(float('nan'))
    out.absmax.zero_()
    ws = torch.empty(int(_lib.load().mmlf_conv2x2_thin_workspace_floats(B, H, W)), device=DEV)
    call('mmlf_conv2x2_thin', ptr(x), cs_in, K, ptr(w), ptr(bias), N, ptr(out), cs_out, shift, oh, ow, B, H, W, 1, variant,
         ptr(ws), ptr(out.absmax), _lib.stream_ptr())
    want = torch.zeros((B, geo.R, geo.P, cs_out), dtype=torch.float64, device=DEV)
    wv = filter4(w.double(), variant)
    want[:, ooff:ooff + oh, ooff:ooff + ow, :N] = conv4_ref(_view(geo, x, cs_in)[..., :K].double(), wv, bias.double(), pad).clamp_min(0)
    got = _view(geo, out, cs_out).double()
    assert bool(((want != 0) | (got == 0)).all()), 'a position outside the extent is not zero'
    note('thin forward', ((got - want).abs() / (2e-5 + 2e-5 * want.abs())).max())
    np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=2e-5, atol=2e-5)
    assert torch.equal(geo.amax_canonical(out.absmax), geo.amax_of(torch.nan_to_num(out), cs_out))
    # weight and bias gradient: both legs through the engine, then between guard bands with the workspace the query sizes
    G = 256
    for integer in (True, False):
        c = _Case(B, H, W, K, N, pad, variant, integer, _seed(B, H, W, K, N, pad, integer))
        LEG[0] = 'thin wgrad'
        c.check_wgrad('f16x3')
        nws = int(_lib.load().mmlf_conv2x2_wgrad_thin_workspace_floats(K))
        assert nws == 16 * int(_lib.load().mmlf_conv_cus()) * 4 * (K + 1) * 2
        gwr, gbr, gwa, gba = c.wgrad_ref()
        bands = [torch.full((G + n + G,), SENTINEL, device=DEV) for n in (N * K * 4, N, nws)]
        for t in bands:
            t[G:-G] = float('nan')
        gw, gb, wsp = (t[G:-G] for t in bands)
        call('mmlf_conv2x2_wgrad_thin', ptr(c.x), c.cs_in, K, ptr(c.g), c.cs_out, N, c.fwd_shift, ptr(gw), ptr(gb), variant, 0,
             ptr(wsp), B, H, W, _lib.stream_ptr())
        for t, name in zip(bands, ('gw', 'gb', 'workspace')):
            assert bool((t[:G] == SENTINEL).all()) and bool((t[-G:] == SENTINEL).all()), f'{name} guard {c.tag}'
        _compare(gw.view(c.w.shape).double(), gwr, gwa, integer, f'thin weight gradient {c.tag}')
        _compare(gb.double(), gbr, gba, integer, f'thin bias gradient {c.tag}')


def net(shared):
    """tests/test_gpu_nobn.py test_70_channel_net_against_float64 at 6 x 33 x 37, image b of every stack scaled by
    2^E_CYCLE[b]: outputs, loss and parameter gradients at that test's bars; digests of the outputs and the four input gradients"""
    from mmlf_amd import loss, synth
    from test_gpu_nobn import _model
    from test_nobn_cpu import NOBN_TINY_KW, gained_state
    B, H, W = NET_FRAME
    kw = dict(NOBN_TINY_KW, model_chs=70, model_in_blocks=2, model_out_blocks=3, model_uncert=True)
    state = gained_state(kw, 24)
    stacks, gt, mask = synth.synth_inputs(B, H, seed=11, ps_w=W)
    scale = np.exp2(np.array([E_CYCLE[b % 6] for b in range(B)], np.float32))[:, None, None, None, None]
    stacks = [s * scale for s in stacks]
    m_mask = torch.from_numpy(mask).int() * loss.create_mask_margin(mask.shape, 2)

    def run(dev, dt):
        m = _model(kw, state, dev).to(dt)
        assert m._native_ok
        m.train()
        xs = [torch.from_numpy(s).to(dev, dt).requires_grad_(True) for s in stacks]
        out = m(*xs)
        lv = loss.ImprovedUncertaintyL1Loss()(out, torch.from_numpy(gt).to(dev, dt), m_mask.to(dev), None)
        lv.backward()
        return ({k: out[k].detach() for k in ('mean', 'logvar')}, float(lv.detach()), {n: p.grad for n, p in m.named_parameters()},
                [x.grad for x in xs])

    path = os.path.join(shared, 'net_float64.npz')
    if not os.path.exists(path):
        o0, l0, g0, _ = run(torch.device('cpu'), torch.float64)
        np.savez(path + '.tmp.npz', loss=l0, **{'out/' + k: v.numpy() for k, v in o0.items()}, **{'grad/' + n: v.numpy() for n, v in g0.items()})
        os.replace(path + '.tmp.npz', path)
    ref = np.load(path)
    g0 = {k[5:]: torch.from_numpy(ref[k]) for k in ref.files if k.startswith('grad/')}
    assert min(float(v.norm()) for v in g0.values()) >= 1e-1
    for mode in MODES:
        engine.CONV_MODE = mode
        o1, l1, g1, dx = run(DEV, torch.float32)
        for k in o1:
            err = float((o1[k].double().cpu() - torch.from_numpy(ref['out/' + k])).abs().max())
            note(f'net output {mode}', err / 1e-4)
            assert err <= 1e-4, (mode, k, err)
        assert abs(l1 - float(ref['loss'])) <= 1e-4 * abs(float(ref['loss']))
        rels = {n: float((g1[n].double().cpu() - g0[n]).norm()) / (float(g0[n].norm()) + 1e-6 * g0[n].numel() ** 0.5 / 3e-2) for n in g0}
        worst, med = max(rels, key=rels.get), float(np.median(list(rels.values())))
        note(f'net gradient worst {mode}', rels[worst] / 6e-2)
        note(f'net gradient median {mode}', med / 4e-2)
        assert rels[worst] <= 6e-2 and med <= 4e-2, (mode, worst, rels[worst], med)
        assert all(d is not None and bool(torch.isfinite(d).all()) for d in dx)
        for name, t in [*o1.items(), *((f'dx{i}', d) for i, d in enumerate(dx))]:
            OUT[f'net {mode} {name}'] = np.frombuffer(hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).digest(), np.uint8)


def main(out_path, shared):
    t0 = time.time()
    assert engine.CONV_MODE == 'f16x3', 'MMLF_CONV_MODE is set'
    lib = _lib.load()
    OUT['cus'] = np.int64(lib.mmlf_conv_cus())
    times = {}

    def timed(name, fn):
        t = time.time()
        fn()
        torch.cuda.synchronize()
        times[name] = time.time() - t

    timed('cases', lambda: [conv_case(MODES, *c) for c in CASES])
    timed('f32', lambda: [conv_case(('f32',), *c) for c in F32_CASES])
    for frame, (K, N), *_ in CASES:
        OUT['blocks %d %d %d %d %d' % (K, N, *frame)] = np.int64(lib.mmlf_conv2x2_blocks(K, N, *frame))
    timed('batchnorm', lambda: [leg('batchnorm f16x3 | %d->%d %dx%dx%d' % (*c[1], *c[0]), bn_case, *c) for c in BN_CASES])
    timed('thin', lambda: [leg('thin | %d->%d %dx%dx%d' % (*c[1], *c[0]), thin_case, *c) for c in THIN_CASES])
    REC.on = False
    timed('net', lambda: leg('net', net, shared))
    times['total'] = time.time() - t0
    OUT['ratios'] = np.array(json.dumps(RATIO))
    OUT['times'] = np.array(json.dumps(times))
    OUT['failures'] = np.array(json.dumps(FAILURES))
    np.savez(out_path, **OUT)
    print(json.dumps({'cus': int(OUT['cus']), 'times': times, 'ratios': RATIO}, indent=1))
    if FAILURES:          # (the parent shows the end of stderr: the first messages in full, then every failed leg by kind)
        kinds = collections.Counter(f.split(' | ')[0] for f in FAILURES)
        print('\n'.join(FAILURES[:3]) + f'\n{len(FAILURES)} FAILED LEGS under MMLF_CONV_CUS={os.environ.get("MMLF_CONV_CUS")}: '
              + ', '.join(f'{n} x {k}' for k, n in kinds.most_common()), file=sys.stderr)
        return 1
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1], sys.argv[2]))
