"""The BatchNorm, layout and slack kernels of csrc/elementwise.hip -- bn_reduce_kernel<4>, bn_reduce_bwd_kernel, the two
finalize kernels, bn_coeffs_eval_kernel, fold_bn_kernel, bn_rows_kernel<0|1, 4>, bn_apply4_kernel, pack / unpack_nchw_kernel,
zero_slack(4)_kernel -- each called directly through its C entry point and held, element by element, to float64 evaluations
of the same operation on the GPU (tests_helpers.bn_stats_ref / bn_apply_ref / bn_bwd_ref, pinned to torch's batch_norm and
relu under autograd by tests/test_elementwise_cpu.py).  tests/test_elementwise_cpu.py::test_gpu_shape_lists_reach_every_class
holds the lists below to the kernel paths they exist for.

Buffers: every output and scratch buffer lies between two guard bands and is pre-filled -- NaN where the launch must write, a
sentinel where it must not -- and EVERY element is compared afterwards: the values, the exact zeros (border positions, pad
channels up to C_store), the sentinels (other channels of a slice write, slack).  z and gy carry NaN on border positions and in
the slack and a finite junk value in pad channels (the kernels load whole groups of four); mmlf_unpack_nchw's grid carries NaN
on both.

Two legs per kernel:
  * exact: z and gy small integers, scale / invstd from {+-0.25, +-0.5, 1, 2}, shift / mean multiples of 0.25, k1..k3 dyadic --
    float32 arithmetic is exact in any order, so the apply kernels must reproduce the float64 result and the sums must be the
    exact sums; channels with u == 0 at one value of z are included (the gradient there is masked).  Quantities that pass
    through a division or a square root (statistics, k1..k3) are held to 1 float32 ulp of the float64 expression;
  * real-valued: seeded normal values with per-channel scale and offset, held to bars that count the kernel's float32
    roundings (one per fused multiply-add, four in dz, two in zhat) times 2^-24 of the absolute terms -- see each check.
No element is set aside for the ReLU decision: the kernels decide by fmaf(z, scale, shift) > 0, which has the sign of the exact
value, and so has the float64 reference (its product is exact)."""
import ctypes

import pytest
import torch

from tests_helpers import RATIOS, _Pool, _bar, _ints, _pick, _same, _ulp, bn_apply_ref, bn_bwd_ref, bn_stats_ref

pytestmark = pytest.mark.gpu

# (B, H, W): n = 1 | one row | one column: pitch 3, shorter than dx | ... | pitch 127, 128, 129: the pack tile of 128 short,
# exact, one over | pitch 32, 33: the 16-wide pack tile of cs = 280 exact and ragged | a long row | the longest
FRAMES = [(1, 1, 1), (1, 1, 37), (2, 29, 1), (3, 5, 29), (3, 10, 14), (2, 10, 125), (2, 10, 126), (2, 10, 127), (2, 3, 30),
          (2, 3, 31), (2, 3, 300), (1, 2, 514)]
LAYOUT_FRAMES = FRAMES + [(2, 3, 32)]        # pack / unpack: W = 32 is whole unpack tiles (they walk W, not the pitch)
FULL_FRAME, FULL_CH = (64, 96, 96), (70, 72)  # 6144 rows > BN_BLOCKS: the engine's regime
# (C, cs_z): cvn = 1 | tail-only groups | cvn divides 256 | ... | (70, 72): dx = 14, dc = 4 | ... | 512: mmlf_bn_bwd_reduce's last
CHANNELS = [(1, 8), (2, 8), (3, 8), (6, 8), (8, 8), (32, 32), (64, 64), (27, 32), (70, 72), (108, 112), (132, 136), (280, 280),
            (288, 288), (512, 512)]
APPLY_ONLY = (516, 520)                      # dx = 1
STATS_LIMIT, STATS_LIMIT_FRAME = (1024, 1024), (1, 2, 3)
# (C, cs_y, c_off, C_store): slice writes of the apply, slice reads of gy in the backward
SLICES = [(70, 280, 0, 70), (70, 280, 140, 70), (70, 280, 70, 70), (70, 280, 210, 70), (70, 72, 0, 72), (27, 32, 0, 32),
          (6, 8, 2, 6), (2, 8, 6, 2), (8, 32, 24, 8)]
SLICE_FRAMES = [(1, 1, 1), (2, 29, 1), (3, 5, 29), (2, 3, 31)]
APPLY4 = [(2, 8), (6, 8), (70, 72), (6, 6)]  # (C, cs_z); cs_z = 6 is legal here only
NBLOCKS = [1, 3, 63, 64, 65, 1024, 4096]
NBLOCKS_FRAME, NBLOCKS_CH = (3, 23, 5), [(6, 8), (70, 72)]      # 69 rows: more than 3, 63, 64 and 65 blocks, fewer than 1024
FOLD = [(1, 1), (2, 280), (70, 27), (280, 280)]                 # (Cout, Cin)
COEFFS_C = [1, 63, 64, 65, 280]
SLACK_FRAMES = [(1, 1, 1), (2, 29, 1), (2, 3, 300)]
BN_BLOCKS = 1024

SENT, JUNK = 1234.5, 777.25
NAN = float('nan')
E23, E22, E24 = 2.0 ** -23, 2.0 ** -22, 2.0 ** -24
DYADIC = (-0.5, -0.25, 0.25, 0.5, 1.0, 2.0)


def _dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module', autouse=True)
def _report_ratios():
    yield
    for k in sorted(RATIOS):
        print(f'\n[elementwise headroom] {k}: max error / bar = {RATIOS[k]:.4f}', end='')
    print()
    RATIOS.clear()                               # the table is shared with the other modules that use _bar


def _normal(shape, gen, standardize):
    """normal values; standardize: each channel (last axis) brought to mean 0, variance 1 over the other axes, so that a small
    sample keeps mean^2 <= 100 var after the per-channel scale and offset"""
    r = torch.randn(shape, device=gen.device, generator=gen, dtype=torch.float64)
    n = r.numel() // r.shape[-1]
    if standardize and n > 1:
        flat = r.reshape(n, -1)
        flat = (flat - flat.mean(0)) / flat.var(0, unbiased=False).sqrt().clamp_min(1e-3)
        r = flat.reshape(shape)
    return r


def _all_equal(got, exp, cs, what):
    bad = ~(got == exp)
    if bool(bad.any()):
        k = int(bad.reshape(-1).to(torch.uint8).argmax())
        raise AssertionError(f'{what}: position {k // cs} channel {k % cs} holds {float(got.reshape(-1)[k])!r}, expected '
                             f'{float(exp.reshape(-1)[k])!r}')


class _Case:
    """one (frame, C, cs_z, leg): z on the grid, BatchNorm coefficients, and their float64 forms"""

    def __init__(self, frame, C, cs_z, integer, seed):
        from mmlf_amd import engine
        self.dev = dev = _dev()
        self.B, self.H, self.W = B, H, W = frame
        self.geo = geo = engine.Geometry(B, H, W)
        self.C, self.cs_z, self.integer, self.n = C, cs_z, integer, B * H * W
        self.gen = gen = torch.Generator(device=dev).manual_seed(seed)
        self.tag = f'B={B} {H}x{W} C={C} cs_z={cs_z} {"exact" if integer else "real"}'
        small = self.n < 4096
        if integer:
            data = _ints(-4, 4, (B, H, W, C), gen)
        else:
            data = (_normal((B, H, W, C), gen, small) * (0.5 + 1.5 * torch.rand(C, device=dev, generator=gen, dtype=torch.float64))
                    + (6 * torch.rand(C, device=dev, generator=gen, dtype=torch.float64) - 3)).float()
        self.z = self.grid(data, cs_z, 0, NAN, JUNK)
        self.zg = self.view(self.z, cs_z)[..., :C].double()
        if integer:
            self.gamma = _pick((-1.0, 0.5, 1.0, 2.0), (C,), gen)
            self.beta = 0.25 * _ints(-8, 8, (C,), gen)
            self.scale = _pick(DYADIC, (C,), gen)
            zc, j = _ints(-3, 3, (C,), gen), _pick((0.0, 0.0, 0.0, 1.0, -1.0, 2.0), (C,), gen)
            self.shift = -self.scale * zc + 0.25 * j               # u == 0 exactly at z == zc where j == 0
            self.mean = 0.25 * _ints(-8, 8, (C,), gen)
            self.invstd = _pick(DYADIC, (C,), gen)
        else:
            self.gamma = 0.5 + torch.rand(C, device=dev, generator=gen)
            self.beta = torch.rand(C, device=dev, generator=gen) - 0.5
            st = bn_stats_ref(self.zg, self.gamma.double(), self.beta.double(), None, None, 0.1, 1e-5)
            self.mean, self.invstd, self.scale, self.shift = (t.float() for t in st[:4])

    def view(self, t, cs):
        return t[:self.geo.NQ * cs].view(self.B, self.geo.R, self.geo.P, cs)

    def grid(self, data, cs, c_off, outside, pad):
        """a grid buffer with `data` (B, H, W, C) on the interior, channels [c_off, c_off + C); `outside` on the border positions
        of those channels; `pad` on every other channel of positions [0, NQ); `outside` in the tail slack"""
        C = data.shape[-1]
        t = torch.full((self.geo.alloc * cs,), outside, device=self.dev)
        v = self.view(t, cs)
        v[..., :c_off] = pad
        v[..., c_off + C:] = pad
        v[:, 1:self.H + 1, 1:self.W + 1, c_off:c_off + C] = data
        return t

    def draw_gy(self, cs_gy, c_off):
        """the output gradient as a channel slice of a cs_gy-wide buffer (finite junk in the other channels and in the slack:
        the last group of four of a slice reads up to three channels past it)"""
        shape = (self.B, self.H, self.W, self.C)
        data = _pick((-2.0, -1.0, 1.0, 2.0), shape, self.gen) if self.integer else _normal(shape, self.gen, False).float()
        t = self.grid(data, cs_gy, c_off, NAN, JUNK)
        t[self.geo.NQ * cs_gy:] = JUNK
        return t, self.view(t, cs_gy)[..., c_off:c_off + self.C].double()

    def bwd(self, gyg):
        return bn_bwd_ref(self.zg, gyg, self.scale.double(), self.shift.double(), self.gamma.double(), self.mean.double(),
                          self.invstd.double())


def _check_amax(geo, amax, buf, cs, c_off, C_store, what):
    """the canonical amax array equals the row and tensor maxima of what the launch itself wrote (the slice alone)"""
    rows = buf[:geo.NQ * cs].view(geo.B * geo.R, geo.P, cs)[:, :, c_off:c_off + C_store].abs().amax((1, 2))
    exp = torch.zeros(geo.amax_n, device=buf.device)
    exp[0] = rows.max()
    exp[geo.amax_head:geo.amax_head + rows.numel()] = rows
    got = geo.amax_canonical(amax)
    bad = ~(got == exp)
    assert not bool(bad.any()), (what, 'amax entry', int(bad.to(torch.uint8).argmax()), 'of', geo.amax_n, 'rows', rows.numel())
    hd = amax[:geo.amax_head].view(-1, geo.amax_stride)
    assert not bool(hd[:, 1:].any()), (what, 'amax head written between the shards')


def _check_grid(case, buf, cs, c_off, C_store, want, bar, key, what):
    """`buf` after a row kernel wrote channels [c_off, c_off + C_store) of every grid position [0, NQ): `want` (B, H, W, C) on
    the interior (equal in the exact leg, within `bar` otherwise), exactly zero on the border and in channels [C, C_store),
    the sentinel everywhere else"""
    geo, C = case.geo, want.shape[-1]
    got = buf.view(-1, cs)
    inner = case.view(buf, cs)[:, 1:case.H + 1, 1:case.W + 1, c_off:c_off + C]
    if case.integer:
        _same(inner, want, what)
    else:
        _bar((inner.double() - want).abs(), bar, key, what)
    exp = torch.full_like(got, SENT)
    exp[:geo.NQ, c_off:c_off + C_store] = 0
    case.view(exp.view(-1), cs)[:, 1:case.H + 1, 1:case.W + 1, c_off:c_off + C] = inner
    _all_equal(got, exp, cs, what)


def _fresh_grid(case, pool, cs, c_off, C_store):
    y = pool.new(case.geo.alloc * cs, SENT)
    y.view(-1, cs)[:case.geo.NQ, c_off:c_off + C_store] = NAN
    return y


# ------------------------------------------------------------------------------------------------ apply (+ ReLU)
def _run_apply(case, cs_y, c_off, C_store, use_amax=True):
    from mmlf_amd import _lib
    from mmlf_amd._lib import call, ptr
    geo, C = case.geo, case.C
    what = f'mmlf_bn_apply_relu {case.tag} cs_y={cs_y} c_off={c_off} C_store={C_store}'
    pool = _Pool(case.dev)
    y = _fresh_grid(case, pool, cs_y, c_off, C_store)
    amax = pool.new(geo.amax_n, 0.0) if use_amax else None
    call('mmlf_bn_apply_relu', ptr(case.z), case.cs_z, C, ptr(case.scale), ptr(case.shift), ptr(y), cs_y, c_off, C_store,
         case.B, case.H, case.W, ptr(amax), _lib.stream_ptr())
    u, absu = bn_apply_ref(case.zg, case.scale.double(), case.shift.double())
    u, absu = (t[:, 1:case.H + 1, 1:case.W + 1] for t in (u, absu))
    _check_grid(case, y, cs_y, c_off, C_store, u.clamp_min(0), E23 * absu, 'apply: 2^-23 (|z scale| + |shift|)', what)
    got = case.view(y, cs_y)[:, 1:case.H + 1, 1:case.W + 1, c_off:c_off + C]
    assert torch.equal(got > 0, u > 0), (what, 'the ReLU decision differs from the sign of the exact value')
    if use_amax:
        _check_amax(geo, amax, y, cs_y, c_off, C_store, what)
    pool.check(what)
    return got > 0


def _c_stores(C, cs):
    return [C] if C == cs else [C, cs]           # the slice form and the form that zeroes the pad channels


@pytest.mark.parametrize('integer', [True, False], ids=['exact', 'real'])
@pytest.mark.parametrize('C,cs', CHANNELS + [APPLY_ONLY], ids=lambda v: str(v))
def test_bn_apply_relu(C, cs, integer):
    for k, frame in enumerate(FRAMES):
        case = _Case(frame, C, cs, integer, 1000 * C + k)
        for c_store in _c_stores(C, cs):
            _run_apply(case, cs, 0, c_store, use_amax=(k + c_store) % 4 != 3)      # amax_out = NULL now and then


@pytest.mark.parametrize('integer', [True, False], ids=['exact', 'real'])
@pytest.mark.parametrize('C,cs_y,c_off,C_store', SLICES, ids=lambda v: str(v))
def test_bn_apply_relu_slice_write(C, cs_y, c_off, C_store, integer):
    from mmlf_amd import engine
    for k, frame in enumerate(SLICE_FRAMES):
        _run_apply(_Case(frame, C, engine.cs_of(C), integer, 77 * C + c_off + k), cs_y, c_off, C_store)


@pytest.mark.parametrize('integer', [True, False], ids=['exact', 'real'])
@pytest.mark.parametrize('C,cs_z', APPLY4, ids=lambda v: str(v))
def test_bn_apply_relu4(C, cs_z, integer):
    from mmlf_amd import _lib
    from mmlf_amd._lib import call, ptr
    arr = lambda ts: (ctypes.c_void_p * 4)(*[ptr(t) for t in ts])
    for k, frame in enumerate(FRAMES):
        cases = [_Case(frame, C, cs_z, integer, 4000 * C + 10 * k + s) for s in range(4)]
        c0, geo, cs_y = cases[0], cases[0].geo, 4 * C
        what = f'mmlf_bn_apply_relu4 {c0.tag}'
        pool = _Pool(c0.dev)
        y = _fresh_grid(c0, pool, cs_y, 0, cs_y)
        amax = pool.new(geo.amax_n, 0.0) if k % 3 != 2 else None
        call('mmlf_bn_apply_relu4', arr([c.z for c in cases]), cs_z, C, arr([c.scale for c in cases]),
             arr([c.shift for c in cases]), ptr(y), cs_y, c0.B, c0.H, c0.W, ptr(amax), _lib.stream_ptr())
        refs = [bn_apply_ref(c.zg, c.scale.double(), c.shift.double()) for c in cases]
        u, absu = (torch.cat([r[i] for r in refs], -1)[:, 1:c0.H + 1, 1:c0.W + 1] for i in (0, 1))
        _check_grid(c0, y, cs_y, 0, cs_y, u.clamp_min(0), E23 * absu, 'apply4: 2^-23 (|z scale| + |shift|)', what)
        if amax is not None:
            _check_amax(geo, amax, y, cs_y, 0, cs_y, what)
        pool.check(what)


# ------------------------------------------------------------------------------------------------ training statistics
def _check_stats(out, ref, integer, absz_mean, gamma, beta, what, name):
    """out / ref: (mean, invstd, scale, shift, running mean, running variance).  The exact leg: 1 ulp each, of the float64
    expression in the kernel's order -- mean, invstd and the running statistics are rounded from double once; scale and shift
    are float32 expressions of the ROUNDED mean and invstd (scale = gamma * invstd, shift = beta - mean * scale: the library
    is built without contraction), so their reference starts from the rounded values too: gamma is a power of two there (the
    product is exact) and beta has the sign of -mean * scale (the sum does not cancel), which leaves the rounding of
    mean * scale, at most half an ulp of the shift, and the shift's own."""
    mean, invstd, scale, shift, rm, rv = ref
    if integer:
        scale = gamma * invstd.float().double()
        shift = beta - mean.float().double() * scale.float().double()
        for got, want, k in zip(out, (mean, invstd, scale, shift, rm, rv),
                                ('mean', 'invstd', 'scale', 'shift', 'running mean', 'running variance')):
            if want is not None:
                _ulp(got, want, f'{name} exact, {k}: 1 ulp', what)
        return
    _bar((out[0].double() - mean).abs(), E23 * mean.abs() + 1e-12 * absz_mean, f'{name} mean: 2^-23 |ref| + 1e-12 mean|z|', what)
    for got, want, k in ((out[1], invstd, 'invstd'), (out[2], scale, 'scale'), (out[5], rv, 'running variance')):
        if want is not None:
            _bar((got.double() - want).abs(), E22 * want.abs(), f'{name} {k}: 2^-22 relative', what)
    _bar((out[3].double() - shift).abs(), E22 * (beta.abs() + (mean * scale).abs()), f'{name} shift: 2^-22 (|beta| + |mean scale|)', what)
    if rm is not None:
        _bar((out[4].double() - rm).abs(), E23 * rm.abs() + 1e-12 * absz_mean, f'{name} running mean: 2^-23 |ref| + 1e-12 mean|z|', what)


def _stats_inputs(C, integer, gen):
    dev = gen.device
    if integer:                                  # gamma a power of two (and beta on the side of -mean * scale): _check_stats
        gamma = _pick((0.5, 1.0, 2.0), (C,), gen)
        rm, rv = 0.25 * _ints(-8, 8, (C,), gen), 0.25 * _ints(1, 8, (C,), gen)
    else:
        gamma = 0.5 + torch.rand(C, device=dev, generator=gen)
        rm, rv = 2 * torch.rand(C, device=dev, generator=gen) - 1, 0.5 + 1.5 * torch.rand(C, device=dev, generator=gen)
    return gamma, rm, rv


def _run_stats_train(frame, C, cs, integer, nblocks, seed, running=True):
    from mmlf_amd import _lib
    from mmlf_amd._lib import call, ptr
    case = _Case(frame, C, cs, integer, seed)
    gen, dev = case.gen, case.dev
    what = f'mmlf_bn_stats_train {case.tag} nblocks={nblocks}'
    if integer:                                  # integers around a per-channel offset whose sign the mean takes
        off = _pick((-6.0, -5.0, 5.0, 6.0), (C,), gen)
        zi = case.view(case.z, cs)[:, 1:case.H + 1, 1:case.W + 1, :C]
        zi += off
        case.zg = case.view(case.z, cs)[..., :C].double()
    gamma, rm, rv = _stats_inputs(C, integer, gen)
    zi = case.zg[:, 1:case.H + 1, 1:case.W + 1]
    beta = (-torch.sign(zi.sum((0, 1, 2))).float() * 0.25 * _ints(0, 8, (C,), gen)) if integer else case.beta
    mom, eps = (0.25, 1e-5) if integer else (0.1, 1e-5)
    ref = bn_stats_ref(case.zg, gamma.double(), beta.double(), rm.double() if running else None,
                       rv.double() if running else None, mom, eps)
    var = 1 / ref[1] ** 2 - eps
    assert case.n == 1 or integer or bool((ref[0] ** 2 <= 100 * var).all()), (what, 'precondition: mean^2 <= 100 var')
    pool = _Pool(dev)
    outs = [pool.new(C, NAN) for _ in range(4)]
    trm, trv = (pool.of(rm), pool.of(rv)) if running else (None, None)
    part = pool.new(2 * C * nblocks, NAN, torch.float64)
    call('mmlf_bn_stats_train', ptr(case.z), cs, C, ptr(gamma), ptr(beta), ptr(trm), ptr(trv), mom, eps, ptr(outs[0]),
         ptr(outs[1]), ptr(outs[2]), ptr(outs[3]), ptr(part), nblocks, case.B, case.H, case.W, _lib.stream_ptr())
    # every block wrote its partial sums, and they add up to the sums over the tensor
    p = part.view(nblocks, 2, C).sum(0)
    for got, want, k in ((p[0], zi.sum((0, 1, 2)), 'sum z'), (p[1], (zi * zi).sum((0, 1, 2)), 'sum z^2')):
        if integer:
            _same(got, want, what + ' ' + k)
        else:
            _bar((got - want).abs(), 1e-12 * (zi.abs() if k == 'sum z' else zi * zi).sum((0, 1, 2)),
                 f'stats partial {k}: 1e-12 sum |.|', what)
    _check_stats(outs + [trm, trv], ref, integer, zi.abs().mean((0, 1, 2)), gamma.double(), beta.double(), what, 'stats')
    pool.check(what)


@pytest.mark.parametrize('integer', [True, False], ids=['exact', 'real'])
@pytest.mark.parametrize('C,cs', CHANNELS, ids=lambda v: str(v))
def test_bn_stats_train(C, cs, integer):
    for k, frame in enumerate(FRAMES):
        _run_stats_train(frame, C, cs, integer, BN_BLOCKS, 31 * C + k, running=k % 5 != 4)


@pytest.mark.parametrize('integer', [True, False], ids=['exact', 'real'])
def test_bn_stats_train_at_its_channel_limit(integer):
    _run_stats_train(STATS_LIMIT_FRAME, *STATS_LIMIT, integer, BN_BLOCKS, 5)


@pytest.mark.parametrize('integer', [True, False], ids=['exact', 'real'])
@pytest.mark.parametrize('nblocks', NBLOCKS)
def test_bn_stats_train_block_counts(nblocks, integer):
    for C, cs in NBLOCKS_CH:
        _run_stats_train(NBLOCKS_FRAME, C, cs, integer, nblocks, nblocks + C)


@pytest.mark.parametrize('integer', [True, False], ids=['exact', 'real'])
@pytest.mark.parametrize('nblocks', NBLOCKS)
def test_bn_stats_finalize_on_given_partials(nblocks, integer):
    """mmlf_bn_stats_finalize on float64 partial sums made here: four values per block and channel"""
    from mmlf_amd import _lib
    from mmlf_amd._lib import call, ptr
    dev = _dev()
    for C in (1, 70):
        gen = torch.Generator(device=dev).manual_seed(9 * nblocks + C)
        what = f'mmlf_bn_stats_finalize nblocks={nblocks} C={C} {"exact" if integer else "real"}'
        if integer:
            x = (_ints(-4, 4, (nblocks, 4, C), gen) + _pick((-6.0, -5.0, 5.0, 6.0), (C,), gen)).double()
        else:
            x = (_normal((nblocks * 4, C), gen, True) * (0.5 + 1.5 * torch.rand(C, device=dev, generator=gen, dtype=torch.float64))
                 + (6 * torch.rand(C, device=dev, generator=gen, dtype=torch.float64) - 3)).view(nblocks, 4, C)
        gamma, rm, rv = _stats_inputs(C, integer, gen)
        beta = (-torch.sign(x.sum((0, 1))).float() * 0.25 * _ints(0, 8, (C,), gen)) if integer else \
            torch.rand(C, device=dev, generator=gen) - 0.5
        mom, eps = (0.25, 1e-5) if integer else (0.1, 1e-5)
        # the same data as a (nblocks, 2, 2) frame for the reference
        xg = torch.full((nblocks, 4, 4, C), NAN, dtype=torch.float64, device=dev)
        xg[:, 1:3, 1:3] = x.view(nblocks, 2, 2, C)
        ref = bn_stats_ref(xg, gamma.double(), beta.double(), rm.double(), rv.double(), mom, eps)
        assert integer or bool((ref[0] ** 2 <= 100 * (1 / ref[1] ** 2 - eps)).all()), (what, 'precondition: mean^2 <= 100 var')
        pool = _Pool(dev)
        part = pool.of(torch.stack([x.sum(1), (x * x).sum(1)], 1))          # [nblocks][2][C]
        outs = [pool.new(C, NAN) for _ in range(4)]
        trm, trv = pool.of(rm), pool.of(rv)
        call('mmlf_bn_stats_finalize', ptr(part), nblocks, C, ptr(gamma), ptr(beta), ptr(trm), ptr(trv), mom, eps,
             ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), ptr(outs[3]), nblocks, 2, 2, _lib.stream_ptr())
        _check_stats(outs + [trm, trv], ref, integer, x.abs().mean((0, 1)), gamma.double(), beta.double(), what, 'finalize')
        pool.check(what)


# ------------------------------------------------------------------------------------------------ backward
def _run_bwd_reduce(case, cs_gy, c_off, nblocks, accumulate):
    from mmlf_amd import _lib
    from mmlf_amd._lib import call, ptr
    C, n = case.C, case.n
    what = f'mmlf_bn_bwd_reduce {case.tag} cs_gy={cs_gy} c_off={c_off} nblocks={nblocks} accumulate={accumulate}'
    gy, gyg = case.draw_gy(cs_gy, c_off)
    ref = case.bwd(gyg)
    pool = _Pool(case.dev)
    start = _ints(-3, 3, (2, C), case.gen) if accumulate else torch.full((2, C), NAN, device=case.dev)
    dgam, dbet = pool.of(start[0]), pool.of(start[1])
    coef = pool.new(3 * C, NAN)
    part = pool.new(2 * C * nblocks, NAN, torch.float64)
    call('mmlf_bn_bwd_reduce', ptr(gy), cs_gy, c_off, ptr(case.z), case.cs_z, C, ptr(case.scale), ptr(case.shift),
         ptr(case.gamma), ptr(case.mean), ptr(case.invstd), ptr(dgam), ptr(dbet), accumulate, ptr(coef), ptr(part), nblocks,
         case.B, case.H, case.W, _lib.stream_ptr())
    base = start.double() if accumulate else torch.zeros((2, C), dtype=torch.float64, device=case.dev)
    k = coef.view(3, C)
    assert bool(torch.isfinite(part).all()), (what, 'a block left its partial sums unwritten')
    if case.integer:
        assert float((16 * ref.sum_abs_gz + 3).max()) < 2 ** 24 and float((ref.sum_abs_g + 3).max()) < 2 ** 24, \
            (what, 'precondition: the sums are float32 numbers')
        _same(dgam, base[0] + ref.dgamma, what + ' dgamma')
        _same(dbet, base[1] + ref.dbeta, what + ' dbeta')
        for got, want, name in zip(k, (ref.k1, ref.k2, ref.k3), ('k1', 'k2', 'k3')):
            _ulp(got, want, f'bwd_reduce exact, {name}: 1 ulp', what)
    else:
        bar_b = E23 * ref.dbeta.abs() + 1e-12 * ref.sum_abs_g
        bar_g = E23 * ref.dgamma.abs() + E22 * ref.sum_abs_gz
        _bar((dbet.double() - base[1] - ref.dbeta).abs(), bar_b, 'dbeta: 2^-23 |ref| + 1e-12 sum|g|', what)
        _bar((dgam.double() - base[0] - ref.dgamma).abs(), bar_g, 'dgamma: 2^-23 |ref| + 2^-22 sum|g||zhat|', what)
        _ulp(k[0], ref.k1, 'k1: 1 ulp', what)
        _bar((k[1].double() - ref.k2).abs(), (ref.k1 / n).abs() * bar_b, 'k2: |k1 / n| bar(dbeta)', what)
        _bar((k[2].double() - ref.k3).abs(), (ref.k1 * case.invstd.double() / n).abs() * bar_g, 'k3: |k1 invstd / n| bar(dgamma)', what)
    pool.check(what)
    return gy, gyg, ref


def _run_bwd_apply(case, gy, gyg, cs_gy, c_off, use_amax=True, relu_mask=None):
    from mmlf_amd import _lib
    from mmlf_amd._lib import call, ptr
    C, cs, gen = case.C, case.cs_z, case.gen
    what = f'mmlf_bn_bwd_apply {case.tag} cs_gy={cs_gy} c_off={c_off}'
    if case.integer:                             # dyadic coefficients of their own
        k = torch.stack([_pick(DYADIC, (C,), gen), 0.25 * _ints(-4, 4, (C,), gen), _pick(DYADIC + (0.0,), (C,), gen)])
    else:
        r = case.bwd(gyg)
        k = torch.stack([r.k1, r.k2, r.k3]).float()
    k64, mean64 = k.double(), case.mean.double()
    z, g = case.zg[:, 1:case.H + 1, 1:case.W + 1], gyg[:, 1:case.H + 1, 1:case.W + 1]
    mask = z * case.scale.double() + case.shift.double() > 0
    want = k64[0] * g * mask - k64[1] - k64[2] * (z - mean64)
    bound = (k64[0] * g * mask).abs() + k64[1].abs() + k64[2].abs() * (z - mean64).abs()
    pool = _Pool(case.dev)
    dz = _fresh_grid(case, pool, cs, 0, cs)
    amax = pool.new(case.geo.amax_n, 0.0) if use_amax else None
    k = k.contiguous()
    call('mmlf_bn_bwd_apply', ptr(gy), cs_gy, c_off, ptr(case.z), cs, C, ptr(case.scale), ptr(case.shift), ptr(case.mean),
         ptr(k), ptr(dz), cs, case.B, case.H, case.W, ptr(amax), _lib.stream_ptr())
    _check_grid(case, dz, cs, 0, cs, want, E22 * bound, 'dz: 2^-22 (|k1 g| + |k2| + |k3||z - mean|)', what)
    if relu_mask is not None:
        # the mask this launch used, read back from dz where k1 * gy stands clear of the bar: the forward's (y > 0)
        got = case.view(dz, cs)[:, 1:case.H + 1, 1:case.W + 1, :C].double()
        rest = -k64[1] - k64[2] * (z - mean64)
        clear = (k64[0] * g).abs() > 8 * E22 * (bound + (k64[0] * g).abs())
        used = (got - rest).abs() > (k64[0] * g).abs() / 2
        assert bool(clear.any()) and torch.equal(used[clear], relu_mask[clear]), (what, 'mask differs from (y > 0) of the apply')
        assert torch.equal(relu_mask, mask), what
    if use_amax:
        _check_amax(case.geo, amax, dz, cs, 0, cs, what)
    pool.check(what)


@pytest.mark.parametrize('integer', [True, False], ids=['exact', 'real'])
@pytest.mark.parametrize('C,cs', CHANNELS, ids=lambda v: str(v))
def test_bn_backward(C, cs, integer):
    """mmlf_bn_bwd_reduce (accumulate 0 and 1) and mmlf_bn_bwd_apply, and one ReLU mask for them and the forward apply"""
    for i, frame in enumerate(FRAMES):
        case = _Case(frame, C, cs, integer, 500 * C + i)
        relu_mask = _run_apply(case, cs, 0, C)
        gy, gyg, _ = _run_bwd_reduce(case, cs, 0, BN_BLOCKS, accumulate=i % 2 if integer else 0)
        _run_bwd_apply(case, gy, gyg, cs, 0, use_amax=i % 4 != 1, relu_mask=relu_mask)
    if integer:
        _run_bwd_reduce(_Case(FRAMES[4], C, cs, True, C), cs, 0, BN_BLOCKS, accumulate=1)
        _run_bwd_reduce(_Case(FRAMES[3], C, cs, True, C), cs, 0, BN_BLOCKS, accumulate=0)


@pytest.mark.parametrize('integer', [True, False], ids=['exact', 'real'])
@pytest.mark.parametrize('C,cs_gy,c_off,C_store', SLICES, ids=lambda v: str(v))
def test_bn_backward_slice_read(C, cs_gy, c_off, C_store, integer):
    from mmlf_amd import engine
    for i, frame in enumerate(SLICE_FRAMES):
        case = _Case(frame, C, engine.cs_of(C), integer, 13 * C + c_off + i)
        gy, gyg, _ = _run_bwd_reduce(case, cs_gy, c_off, BN_BLOCKS, accumulate=i % 2 if integer else 0)
        _run_bwd_apply(case, gy, gyg, cs_gy, c_off)


@pytest.mark.parametrize('integer', [True, False], ids=['exact', 'real'])
@pytest.mark.parametrize('nblocks', NBLOCKS)
def test_bn_bwd_reduce_block_counts(nblocks, integer):
    for C, cs in NBLOCKS_CH:
        _run_bwd_reduce(_Case(NBLOCKS_FRAME, C, cs, integer, nblocks + C), cs, 0, nblocks, accumulate=int(integer))


# ------------------------------------------------------------------------------------------------ the engine's regime
@pytest.fixture(scope='module')
def full_case():
    case = _Case(FULL_FRAME, *FULL_CH, False, 64)
    yield case
    del case
    torch.cuda.empty_cache()


def test_full_frame_stats_train():
    _run_stats_train(FULL_FRAME, *FULL_CH, False, BN_BLOCKS, 64)
    torch.cuda.empty_cache()


def test_full_frame_apply(full_case):
    _run_apply(full_case, FULL_CH[1], 0, FULL_CH[1])


def test_full_frame_bwd_reduce_and_apply(full_case):
    gy, gyg, _ = _run_bwd_reduce(full_case, FULL_CH[1], 0, BN_BLOCKS, 0)
    _run_bwd_apply(full_case, gy, gyg, FULL_CH[1], 0)


# ------------------------------------------------------------------------------------------------ layout
@pytest.mark.parametrize('C,cs', CHANNELS, ids=lambda v: str(v))
def test_pack_and_unpack_nchw(C, cs):
    from mmlf_amd import engine, _lib
    from mmlf_amd._lib import call, ptr
    dev = _dev()
    for k, (B, H, W) in enumerate(LAYOUT_FRAMES):
        geo = engine.Geometry(B, H, W)
        gen = torch.Generator(device=dev).manual_seed(C + k)
        what = f'pack / unpack B={B} {H}x{W} C={C} cs={cs}'
        x = torch.randn((B, C, H, W), device=dev, generator=gen)
        pool = _Pool(dev)
        g = pool.new(geo.alloc * cs, SENT)
        g[:geo.NQ * cs] = NAN
        amax = pool.new(geo.amax_n, 0.0) if k % 3 != 1 else None
        call('mmlf_pack_nchw', ptr(x), C, ptr(g), cs, B, H, W, ptr(amax), _lib.stream_ptr())
        exp = torch.full((geo.alloc, cs), SENT, device=dev)              # the tail slack keeps its sentinel
        exp[:geo.NQ] = 0
        exp[:geo.NQ].view(B, geo.R, geo.P, cs)[:, 1:H + 1, 1:W + 1, :C] = x.permute(0, 2, 3, 1)
        _all_equal(g.view(-1, cs), exp, cs, 'mmlf_pack_nchw ' + what)
        if amax is not None:
            _check_amax(geo, amax, g, cs, 0, cs, what)
        # unpack reads interior positions and channels below C only: NaN everywhere else
        src = torch.full((geo.alloc, cs), NAN, device=dev)
        src[:geo.NQ].view(B, geo.R, geo.P, cs)[:, 1:H + 1, 1:W + 1, :C] = x.permute(0, 2, 3, 1)
        back = pool.new(B * C * H * W, NAN)
        call('mmlf_unpack_nchw', ptr(src), cs, ptr(back), C, B, H, W, _lib.stream_ptr())
        _all_equal(back, x.reshape(-1), 1, 'mmlf_unpack_nchw ' + what)
        pool.check(what)


@pytest.mark.parametrize('k3', [False, True], ids=['2x2', '3x3'])
@pytest.mark.parametrize('B,H,W', SLACK_FRAMES)
def test_zero_slack(B, H, W, k3):
    """only the head [0, (P + 1) cs), the tail [NQ cs, end of the allocation) and the amax array change"""
    from mmlf_amd import engine, _lib
    from mmlf_amd._lib import call, ptr
    dev = _dev()
    geo = engine.Geometry(B, H, W, 3 if k3 else 2)
    sfx = '_k3' if k3 else ''

    def expect(cs):
        e = torch.full((geo.alloc * cs,), SENT, device=dev)
        e[:(geo.P + 1) * cs] = 0
        e[geo.NQ * cs:] = 0
        return e

    def check(bufs, css, amaxes, what):
        for t, cs, a in zip(bufs, css, amaxes):
            if t is not None:
                _all_equal(t, expect(cs), cs, f'{what} cs={cs}')
            if a is not None:
                want = 0.0 if t is not None else 7.0
                assert bool((a == want).all()), (what, cs, 'amax array')

    for cs, with_amax in ((8, True), (72, False), (280, True)):
        pool = _Pool(dev)
        t, a = pool.new(geo.alloc * cs, SENT), pool.new(geo.amax_n, 7.0) if with_amax else None
        call('mmlf_zero_slack' + sfx, ptr(t), cs, B, H, W, ptr(a), _lib.stream_ptr())
        check([t], [cs], [a], f'mmlf_zero_slack{sfx} B={B} {H}x{W}')
        pool.check(f'mmlf_zero_slack{sfx} cs={cs}')
    # four at once: a NULL grid in the middle of the table (its cs and amax are not looked at), NULL amax arrays
    pool = _Pool(dev)
    css = [8, 280, 0, 72]
    bufs = [pool.new(geo.alloc * cs, SENT) if cs else None for cs in css]
    amaxes = [pool.new(geo.amax_n, 7.0), None, pool.new(geo.amax_n, 7.0), pool.new(geo.amax_n, 7.0)]
    arr = lambda ts: (ctypes.c_void_p * 4)(*[ptr(t) for t in ts])
    call('mmlf_zero_slack4' + sfx, arr(bufs), (ctypes.c_int * 4)(*css), arr(amaxes), B, H, W, _lib.stream_ptr())
    check(bufs, css, amaxes, f'mmlf_zero_slack4{sfx} B={B} {H}x{W}')
    pool.check('mmlf_zero_slack4' + sfx)
    bufs = [None, pool.new(geo.alloc * 32, SENT), None, None]             # one buffer, no amax
    call('mmlf_zero_slack4' + sfx, arr(bufs), (ctypes.c_int * 4)(0, 32, 0, 0), arr([None] * 4), B, H, W, _lib.stream_ptr())
    check(bufs, [0, 32, 0, 0], [None] * 4, f'mmlf_zero_slack4{sfx} (one buffer) B={B} {H}x{W}')
    pool.check('mmlf_zero_slack4' + sfx)


# ------------------------------------------------------------------------------------------------ eval-mode coefficients
@pytest.mark.parametrize('bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('taps', [4, 9], ids=['2x2', '3x3'])
@pytest.mark.parametrize('cout,cin', FOLD, ids=lambda v: str(v))
def test_fold_bn_eval(cout, cin, taps, bias):
    from mmlf_amd import _lib
    from mmlf_amd._lib import call, ptr
    dev = _dev()
    gen = torch.Generator(device=dev).manual_seed(cout + cin + taps)
    what = f'mmlf_fold_bn_eval{"3x3" if taps == 9 else ""} {cin}->{cout} bias={bias}'
    w = torch.randn(cout * cin * taps, device=dev, generator=gen)
    b = torch.randn(cout, device=dev, generator=gen) if bias else None
    scale = (0.5 + torch.rand(cout, device=dev, generator=gen)) * _pick((-1.0, 1.0), (cout,), gen)
    shift = torch.randn(cout, device=dev, generator=gen)
    pool = _Pool(dev)
    w_out, b_out = pool.new(w.numel(), NAN), pool.new(cout, NAN)
    call('mmlf_fold_bn_eval3x3' if taps == 9 else 'mmlf_fold_bn_eval', ptr(w), ptr(b), ptr(scale), ptr(shift), ptr(w_out),
         ptr(b_out), cout, cin, _lib.stream_ptr())
    want = w.double().view(cout, -1) * scale.double()[:, None]
    _bar((w_out.double().view(cout, -1) - want).abs(), E24 * want.abs(), 'fold w scale: 2^-24 relative', what)
    bs = b.double() * scale.double() if bias else torch.zeros(cout, dtype=torch.float64, device=dev)
    _bar((b_out.double() - (bs + shift.double())).abs(), E23 * (bs.abs() + shift.double().abs()),
         'fold bias: 2^-23 (|b scale| + |shift|)', what)
    pool.check(what)


@pytest.mark.parametrize('affine', ['gamma+beta', 'gamma', 'beta', 'none'])
@pytest.mark.parametrize('C', COEFFS_C)
def test_bn_coeffs_eval(C, affine):
    from mmlf_amd import _lib
    from mmlf_amd._lib import call, ptr
    dev = _dev()
    gen = torch.Generator(device=dev).manual_seed(C)
    what = f'mmlf_bn_coeffs_eval C={C} {affine}'
    gamma = (0.5 + torch.rand(C, device=dev, generator=gen)) if 'gamma' in affine else None
    beta = (torch.rand(C, device=dev, generator=gen) - 0.5) if 'beta' in affine else None
    rm, rv = 2 * torch.rand(C, device=dev, generator=gen) - 1, 0.5 + 1.5 * torch.rand(C, device=dev, generator=gen)
    pool = _Pool(dev)
    scale, shift = pool.new(C, NAN), pool.new(C, NAN)
    call('mmlf_bn_coeffs_eval', ptr(gamma), ptr(beta), ptr(rm), ptr(rv), 1e-5, ptr(scale), ptr(shift), C, _lib.stream_ptr())
    sc = 1 / (rv.double() + 1e-5).sqrt() * (gamma.double() if gamma is not None else 1)
    b64 = beta.double() if beta is not None else torch.zeros(C, dtype=torch.float64, device=dev)
    _ulp(scale, sc, 'coeffs_eval scale: 1 ulp', what)
    _bar((shift.double() - (b64 - rm.double() * sc)).abs(), E23 * (b64.abs() + (rm.double() * sc).abs()),
         'coeffs_eval shift: 2^-23 (|beta| + |rm scale|)', what)
    pool.check(what)


# ------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks_refuse_before_any_launch():
    """every call below fails a host check that stands in front of the wrapper's first launch: nonzero return and a message"""
    from mmlf_amd import _lib
    dev = _dev()
    L = _lib.load()
    t = torch.zeros(4096, device=dev)
    d = torch.zeros(4096, dtype=torch.float64, device=dev)
    p, dp, st = t.data_ptr(), d.data_ptr(), _lib.stream_ptr()

    def refused(name, *args):
        rc = getattr(L, name)(*args)
        msg = _lib.last_error()
        assert rc != 0 and name.replace('_k3', '').replace('3x3', '') in msg, (name, args, rc, msg)

    refused('mmlf_bn_bwd_apply', p, 8, 0, p, 8, 12, p, p, p, p, p, 16, 1, 1, 1, None, st)            # C > cs_z
    refused('mmlf_bn_bwd_apply', p, 8, 0, p, 8, 0, p, p, p, p, p, 8, 1, 1, 1, None, st)              # C = 0
    refused('mmlf_bn_bwd_apply', p, 8, 0, p, 8, 8, p, p, p, p, p, 8, 1, 0, 1, None, st)              # H = 0
    refused('mmlf_bn_apply_relu', p, 8, 0, p, p, p, 8, 0, 0, 1, 1, 1, None, st)                      # C = 0
    refused('mmlf_bn_apply_relu', p, 8, -4, p, p, p, 8, 0, 4, 1, 1, 1, None, st)                     # C < 0
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, -1)):
        refused('mmlf_bn_apply_relu', p, 8, 8, p, p, p, 8, 0, 8, *bad, None, st)
        refused('mmlf_bn_stats_train', p, 8, 8, None, None, None, None, 0.1, 1e-5, p, p, p, p, dp, 4, *bad, st)
        refused('mmlf_bn_stats_finalize', dp, 4, 8, None, None, None, None, 0.1, 1e-5, p, p, p, p, *bad, st)
        refused('mmlf_bn_bwd_reduce', p, 8, 0, p, 8, 8, p, p, None, p, p, None, None, 0, p, dp, 4, *bad, st)
        refused('mmlf_pack_nchw', p, 8, p, 8, *bad, None, st)
        refused('mmlf_unpack_nchw', p, 8, p, 8, *bad, st)
    refused('mmlf_unpack_nchw', p, 6, p, 6, 1, 1, 1, st)                                             # cs % 4
    refused('mmlf_bn_bwd_reduce', p, 520, 0, p, 520, 513, p, p, None, p, p, None, None, 0, p, dp, 1, 1, 1, 1, st)   # 129 groups
    refused('mmlf_bn_bwd_reduce', p, 8, 0, p, 8, 0, p, p, None, p, p, None, None, 0, p, dp, 1, 1, 1, 1, st)         # C = 0
    refused('mmlf_bn_stats_train', p, 1032, 1025, None, None, None, None, 0.1, 1e-5, p, p, p, p, dp, 1, 1, 1, 1, st)  # 257 groups
    torch.cuda.synchronize()
