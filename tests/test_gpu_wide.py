"""The 2x2 kernels on layers wider than one launch (288 < N <= 512, column blocks: csrc/conv.hip wide_np, csrc/wgrad.hip
wgrad_col_blocks), kernel level, in the three arithmetic modes: forward and data gradient of every width at
which the block rule changes, the ReLU mask words and the epilogue's BatchNorm statistics across the blocks, the weight and
bias gradient of wide gradient tensors and of wide inputs.  The references are the float64 per-tap matmuls of tests_helpers
(conv4_ref / dgrad4_ref / wgrad4_ref on the transformed filter, pinned to nn.Conv2d and its autograd by
tests/test_backward2x2_cpu.py), the operands, legs and bars those of tests/test_gpu_backward2x2.py (its _Case is reused as it
is): real-valued operands at 2e-5 * sum|a||b| + 1e-6 * max, exact-integer operands bit for bit.  The forward pass is also held
to tests/test_gpu_kernels.py's rtol = atol = 2e-5 and, in the f16 split, to the derived per-output bound of
tests/test_gpu_precision.py.  Every one of these launches is refused ("not supported (max 288)") by a library without the
column blocks.

Replaces nn.Conv2d(k=2) forward / backward at --model_chs above 72 (reference mmlf/model/feed_forward.py:123,125)."""
import numpy as np
import pytest
import torch

from test_gpu_backward2x2 import (SENTINEL, _Case, _compare, _dev, _draw, _fresh, _grid_rand, _seed, _view, _written)
from test_gpu_precision import f16x3_bound
from tests_helpers import bn_stats_ref, conv4_ref, filter4

pytestmark = pytest.mark.gpu

MODES = ['f32', 'bf16x6', 'f16x3']
# 289: the first wide width (an odd channel count: no 16-byte stores); 296, 304: model_chs 74 and 76; 320 | 321, 384 | 385: the
# last width of the 2 x 160 (2 x 192) column rule and the first of the next -- the last live column is the last column of the
# second block | an early column of a block most of which is padding; 500: a ragged second block of 2 x 256; 512: every column
# live.  The first and the last column of every block are live in each of them (the blocks split the layer at column 160, 192
# or 256 < 289) and are compared like every other column.
WIDTHS = [289, 296, 304, 320, 321, 384, 385, 500, 512]
DEPTHS = [8, 72, 296, 512]
# B x frame: one pixel; 3 x 5 and 9 x 7 (several patches in one tile, a ragged last tile); 5 x 130 (pitch above 127: no
# sixteen-wave kernel anywhere); 2 x 400 (pitch above 383: the two-segment activation window).  With (variant, pad, relu):
FRAMES = [((1, 1, 1), 0, 1, False), ((3, 3, 5), 1, 0, True), ((3, 9, 7), 2, 1, True), ((1, 5, 130), 0, 0, False),
          ((1, 2, 400), 1, 1, True), ((3, 3, 5), 2, 0, False)]


@pytest.fixture(autouse=True)
def _mode():
    from mmlf_amd import engine
    keep = engine.CONV_MODE
    yield
    engine.CONV_MODE = keep


def _forward(mode, B, H, W, K, N, pad, variant, relu, integer, sliced):
    """one forward launch K -> N against float64: every position and channel of the buffer"""
    from mmlf_amd import engine
    engine.CONV_MODE = mode
    dev = _dev()
    geo = engine.Geometry(B, H, W)
    gen = torch.Generator(device=dev).manual_seed(_seed(B, H, W, K, N, pad, integer))
    cs_in, cs_out = engine.cs_of(K), engine.cs_of(N)
    ih, iw, ioff = (H, W, 1) if pad else (H + 1, W + 1, 0)
    oh, ow, ooff = (H + 1, W + 1, 0) if pad else (H, W, 1)
    shift = 0 if pad else geo.P + 1
    x = _grid_rand(geo, K, cs_in, ioff, ih, iw, gen, integer)
    w = _draw((N, K, 2, 2), gen, integer)
    w = w if integer else w / np.sqrt(4 * K)
    bias = _draw((N,), gen, integer, (-3, -2, -1, 0, 1, 2, 3))
    wv = filter4(w.double(), variant)
    xv = _view(geo, x, cs_in)[..., :K]
    what = f'forward {mode} {K}->{N} B={B} {H}x{W} pad={pad} variant={variant} relu={relu} {"integer" if integer else "real"}'

    def want(b0, b1):
        xd = xv[b0:b1].double()
        val = conv4_ref(xd, wv, bias.double(), pad)
        return (val.clamp_min(0) if relu else val), conv4_ref(xd.abs(), wv.abs(), bias.double().abs(), pad)

    if sliced:          # N channels at offset 8 of a wider, sentinel-filled buffer: the neighbouring channels keep the sentinel
        off, cs_buf, n_store, fill = 8, cs_out + 16, N, SENTINEL
    else:
        off, cs_buf, n_store, fill = 0, cs_out, cs_out, 0.0
    out = _fresh(geo, cs_out, cs_buf, off, n_store, shift, fill, dev)
    if mode == 'f16x3':
        out.absmax = torch.zeros(geo.amax_n, device=dev)
    engine.conv(geo, x, cs_in, K, engine.pack_filter(w, variant, False), bias, N, out, cs_buf, shift, oh, ow, relu,
                n_store=n_store, out_off=off)
    _written(geo, out, cs_buf, off, n_store, ooff, oh, ow, shift, want, max(1, 150_000 // (geo.R * geo.P)), fill, integer, what)
    if integer:
        return
    got = _view(geo, out, cs_buf)[:, ooff:ooff + oh, ooff:ooff + ow, off:off + N].double()
    ref, mag = want(0, B)
    assert torch.allclose(got, ref, rtol=2e-5, atol=2e-5), (what, float((got - ref).abs().max()))
    if mode == 'f16x3':
        # a wave's scale maximum is at most the tensor's; the bias is added in float32 behind the sum (half an ulp of the result)
        wabs = wv.abs().sum((1, 2, 3))
        bound = f16x3_bound(mag, wabs * float(x.abs().max()), K) + 2.0 ** -24 * (mag + ref.abs())
        err = (got - ref).abs()
        assert bool((err <= bound).all()), (what, float((err / bound).max()))


@pytest.mark.parametrize('N', WIDTHS)
@pytest.mark.parametrize('mode', MODES)
def test_wide_forward_and_data_gradient(mode, N):
    """K -> N forward (whole rows and a channel slice) and the data gradient of an N -> K layer (plain, ReLU by reference, ReLU
    by the mask words a wide forward launch left, and a channel slice), on every frame, both placements, the three variants,
    with and without ReLU; the depths K and the two legs rotate over the frames and widths so that every width meets every
    depth class and both legs"""
    i = WIDTHS.index(N)
    for j, ((B, H, W), variant, pad, relu) in enumerate(FRAMES):
        K = DEPTHS[(i + j) % len(DEPTHS)]
        integer = (i + j) % 2 == 0
        _forward(mode, B, H, W, K, N, pad, variant, relu, integer, sliced=False)
        _forward(mode, B, H, W, K, N, 1 - pad, variant, not relu, not integer, sliced=True)
        c = _Case(B, H, W, N, K, pad, variant, integer, _seed(B, H, W, N, K, pad, integer))
        c.check_dgrad(mode)
        if j % 2 == 0:
            c.check_dgrad_slice(mode)


@pytest.mark.parametrize('N', [296, 512])
@pytest.mark.parametrize('B,H,W', [(3, 9, 7), (1, 2, 400)])
def test_wide_relu_mask_words_across_the_column_blocks(N, B, H, W):
    """conv1's forward launch leaves (out > 0) of both column blocks in one tile's mask words; conv2's data gradient reads them:
    the same bits as with the activations as reference, and the float64 gradient with the ReLU applied"""
    from mmlf_amd import engine
    engine.CONV_MODE = 'f16x3'
    for pad in (1, 0):
        c = _Case(B, H, W, N, N, pad, 0, False, _seed(B, H, W, N, N, pad, False))
        geo, cs, dev = c.geo, c.cs_in, c.dev
        y, mask = c.relu_mask('f16x3')
        frac = float((_view(geo, y, cs)[:, c.ioff:c.ioff + c.ih, c.ioff:c.ioff + c.iw, :N] > 0).float().mean())
        assert 0.05 < frac < 0.95, frac                  # a real mix of kept and dropped elements
        a, b = geo.buf(cs, dev), geo.buf(cs, dev)
        c.launch_dgrad('f16x3', a, cs, 0, cs, ref=y)
        c.launch_dgrad('f16x3', b, cs, 0, cs, mask_in=mask)
        assert torch.equal(a, b)
        assert torch.equal(geo.amax_canonical(a.absmax), geo.amax_canonical(b.absmax))
        d_shift = geo.P + 1 - c.fwd_shift
        _written(geo, b, cs, 0, cs, c.ioff, c.ih, c.iw, d_shift, c.dgrad_want(c.keep_of(y, cs)), c.chunk, 0.0, False,
                 f'data gradient by mask words {c.tag}')


@pytest.mark.parametrize('N', [296, 512])
@pytest.mark.parametrize('B,H,W', [(3, 9, 7), (1, 5, 130)])
def test_wide_epilogue_batchnorm_statistics(N, B, H, W):
    """the statistics both column blocks leave in one [workgroup][2][N] array, finalized, against a float64 reduction of the
    stored output (and the two-pass kernel on it) at the bar of test_fused_batchnorm_statistics_match_the_two_pass_form"""
    from mmlf_amd import engine, _lib
    from mmlf_amd._lib import call, ptr
    dev = _dev()
    geo = engine.Geometry(B, H, W)
    K = 296
    cs_in, cs_out = engine.cs_of(K), engine.cs_of(N)
    gen = torch.Generator(device=dev).manual_seed(N + W)
    x = _grid_rand(geo, K, cs_in, 0, H + 1, W + 1, gen, False)
    w = (torch.rand((N, K, 2, 2), device=dev, generator=gen) - 0.5) * 0.1
    bias = torch.rand(N, device=dev, generator=gen) - 0.5
    pk = torch.empty(int(_lib.load().mmlf_packed_filter_h2_bytes(cs_in, N)) // 4, device=dev)
    call('mmlf_pack_filter_h2', ptr(w), ptr(pk), N, K, 0, 0, _lib.stream_ptr())
    z = geo.buf(cs_out, dev)
    nblk = int(_lib.load().mmlf_conv2x2_blocks(K, N, B, H, W))
    partial = torch.full((nblk * 2 * N + 8,), float('nan'), dtype=torch.float64, device=dev)
    call('mmlf_conv2x2_h2', ptr(x), cs_in, K, ptr(pk), ptr(bias), N, ptr(z), cs_out, cs_out, geo.P + 1, H, W,
         B, H, W, 0, None, 0, ptr(geo.amax_of(x, cs_in)), ptr(z.absmax), ptr(partial), None, None, _lib.stream_ptr())
    assert bool(torch.isnan(partial[nblk * 2 * N:]).all()) and bool(torch.isfinite(partial[:nblk * 2 * N]).all())
    gamma, beta = torch.rand(N, device=dev, generator=gen) + 0.5, torch.rand(N, device=dev, generator=gen) - 0.5
    rm0, rv0 = torch.full((N,), 0.25, device=dev), torch.full((N,), 2.0, device=dev)
    zg = _view(geo, z, cs_out)[..., :N].double()
    ref = bn_stats_ref(zg, gamma.double(), beta.double(), rm0.double(), rv0.double(), 0.1, 1e-5)
    for form in ('fused', 'two_pass'):
        rm, rv = rm0.clone(), rv0.clone()
        c = torch.empty(4 * N, device=dev)
        if form == 'fused':
            call('mmlf_bn_stats_finalize', ptr(partial), nblk, N, ptr(gamma), ptr(beta), ptr(rm), ptr(rv), 0.1, 1e-5,
                 ptr(c[2 * N:]), ptr(c[3 * N:]), ptr(c), ptr(c[N:]), B, H, W, _lib.stream_ptr())
        else:
            part = torch.empty(2 * N * 1024, dtype=torch.float64, device=dev)
            call('mmlf_bn_stats_train', ptr(z), cs_out, N, ptr(gamma), ptr(beta), ptr(rm), ptr(rv), 0.1, 1e-5,
                 ptr(c[2 * N:]), ptr(c[3 * N:]), ptr(c), ptr(c[N:]), ptr(part), 1024, B, H, W, _lib.stream_ptr())
        mean, invstd, scale, shift, new_rm, new_rv = ref
        for got, want, name in ((c[2 * N:3 * N], mean, 'mean'), (c[3 * N:], invstd, 'invstd'), (c[:N], scale, 'scale'),
                                (c[N:2 * N], shift, 'shift'), (rm, new_rm, 'running_mean'), (rv, new_rv, 'running_var')):
            np.testing.assert_allclose(got.double().cpu().numpy(), want.cpu().numpy(), rtol=2e-6, atol=1e-7,
                                       err_msg=f'{form} {name} N={N} B={B} {H}x{W}')
    assert torch.equal(geo.amax_canonical(z.absmax)[0], geo.amax_of(z, cs_out)[0])      # both blocks raised the tensor maximum


# (Cin, Cout): the widest stream layers of model_chs 96 and 128 (inputs of the wide nets, one launch each); 296, 384, 512 square
# (a second block of 8, 96 and 224 columns: the 32-column, the 128-column and the 288-column kernels behind the first 288); a
# wide input under the DPP head's 108 columns and under the thin head; a narrow input under the widest gradient
WGRAD_PAIRS = [(96, 96), (128, 128), (296, 296), (384, 384), (512, 512), (512, 108), (512, 2), (8, 512)]
WGRAD_FRAMES = [((3, 9, 7), 0, 1, True), ((1, 5, 130), 1, 0, False), ((1, 2, 400), 2, 1, False), ((1, 1, 1), 1, 0, True),
                ((3, 3, 5), 2, 0, True)]


@pytest.mark.parametrize('cin,cout', WGRAD_PAIRS)
@pytest.mark.parametrize('mode', MODES)
def test_wide_weight_and_bias_gradient(mode, cin, cout):
    """through the engine (accumulating into drawn gw / gb) and through the C entry points with accumulate = 0 (gw / gb
    prefilled with NaN: overwritten, not read) and 1, between guard bands, the three variants, both placements and legs"""
    from mmlf_amd import _lib, engine
    from mmlf_amd._lib import call, ptr
    dev = _dev()
    G = 256

    def guarded(n, inner):
        t = torch.full((G + n + G,), SENTINEL, device=dev)
        t[G:G + n] = inner
        return t, t[G:G + n]

    thin = cout <= engine.THIN_MAX_N and cin >= engine.THIN_MIN_K
    for (B, H, W), variant, pad, integer in WGRAD_FRAMES:
        c = _Case(B, H, W, cin, cout, pad, variant, integer, _seed(B, H, W, cin, cout, pad, integer))
        c.check_wgrad(mode)
        geo = c.geo
        nws = int(_lib.load().mmlf_conv2x2_wgrad_thin_workspace_floats(cin) if thin else
                  _lib.load().mmlf_wgrad_workspace_floats(cin, cout, B, H, W))
        assert nws > 0
        gwr, gbr, gwa, gba = c.wgrad_ref()
        gw0 = _draw(c.w.shape, c.gen, integer, (-3, -2, -1, 0, 1, 2, 3))
        gb0 = _draw((cout,), c.gen, integer, (-3, -2, -1, 0, 1, 2, 3))
        ax, ag = geo.amax_of(c.x, c.cs_in), geo.amax_of(c.g, c.cs_out)
        for acc in (0, 1):
            gw_t, gw = guarded(gw0.numel(), gw0.reshape(-1) if acc else float('nan'))
            gb_t, gb = guarded(cout, gb0 if acc else float('nan'))
            ws_t, ws = guarded(nws, float('nan'))
            args = (ptr(c.x), c.cs_in, cin, ptr(c.g), c.cs_out, cout, c.fwd_shift, ptr(gw), ptr(gb), variant, acc, ptr(ws), B, H, W)
            if thin:
                call('mmlf_conv2x2_wgrad_thin', *args, _lib.stream_ptr())
            elif mode == 'f16x3':
                call('mmlf_conv2x2_wgrad_h2', *args, ptr(ax), ptr(ag), _lib.stream_ptr())
            else:
                call('mmlf_conv2x2_wgrad_split' if mode == 'bf16x6' else 'mmlf_conv2x2_wgrad', *args, _lib.stream_ptr())
            for t, what in ((gw_t, 'gw'), (gb_t, 'gb'), (ws_t, 'workspace')):
                assert bool((t[:G] == SENTINEL).all()) and bool((t[-G:] == SENTINEL).all()), f'{what} guard, accumulate={acc} {c.tag}'
            base_w, base_b = (gw0.double(), gb0.double()) if acc else (0, 0)
            _compare(gw.view(gw0.shape).double(), base_w + gwr, gwa + (gw0.double().abs() if acc else 0), integer,
                     f'weight gradient accumulate={acc} {mode} {c.tag}')
            _compare(gb.double(), base_b + gbr, gba + (gb0.double().abs() if acc else 0), integer,
                     f'bias gradient accumulate={acc} {mode} {c.tag}')
