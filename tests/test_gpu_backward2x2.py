"""The 2x2 backward kernels -- data gradient (mmlf_conv2x2 / _split / _h2 on a dgrad-packed filter) and weight + bias gradient
(mmlf_conv2x2_wgrad / _split / _h2 / _thin) -- against float64 per-tap matmuls on the GPU (tests_helpers.conv4_ref / dgrad4_ref /
wgrad4_ref, pinned to nn.Conv2d by tests/test_backward2x2_cpu.py), element by element, in the three arithmetic modes, both
placements (pad 1 / pad 0) and the stream variants, over every weight-gradient layout and the frames at which the
convolution kernels change path.  tests/test_backward2x2_cpu.py::test_backward2x2_gpu_shapes_cover_the_kernel_edges holds the
lists below to what they are for.

Two legs per check:
  * real-valued: uniform values in [-1, 1), weights scaled by 1 / sqrt(4 Cin), held to 2e-5 * sum|a||b| + 1e-6 * max
    (tests_helpers.check_sum_bar) -- rounding;
  * exact-integer: activations and weights from {-2, -1, 1, 2}, gradients from {-1, 1}, gw0 / gb0 and biases small integers.
    Every product and every partial sum is an integer below 2^24; the two f16 halves of the f16 split and the three bf16 parts
    of the bf16 split carry such values exactly under any power-of-two scale (the low parts are zero), so float32 accumulation is
    exact in every order and the result must equal the float64 reference BIT FOR BIT -- one dropped, doubled or misplaced
    product moves an element by at least 1, at any size.  Each comparison first asserts sum|a||b| + |gw0| < 2^24 on the
    reference."""
import numpy as np
import pytest
import torch

from tests_helpers import check_sum_bar, dgrad4_ref, filter4, unfilter4, wgrad4_ref

pytestmark = pytest.mark.gpu

MODES = ['f32', 'bf16x6', 'f16x3']
# (Cin, Cout): every (mb, nb) layout of the split weight gradient (csrc/wgrad.hip wgrad16_cfg: 22, 52, 25, 55, 28, 38, wide; wide
# again with column blocks partly and wholly past Cout), every pick_nt class of the exact-f32 one (1, 3, 4, 9), the smallest
# layer, and the thin kernel's three shapes.  The ABI rejects Cout > 288 (pick_nt < 0): no such pair can be swept.
PAIRS = [(2, 2), (32, 8), (27, 70), (70, 70), (108, 108), (280, 108), (280, 280), (280, 132), (1, 1),
         (280, 1), (280, 2), (70, 2)]
STREAM_PAIRS = [(27, 70), (70, 70)]                  # the layers that run under the stream variants
# one pixel, one row, one column; 3 x 5 x 29 (a tile of pure padding; fewer chunks than splits in every layout); pitch 127 / 128
# (sixteen-wave kernel | eight-wave and register-streamed kernels); 302; 383 / 384 (one window | two segments); 516;
# 5 x 96 x 96 = 1504 chunks: 3 / 12 / 19 / 36 chunks per split in the 512 / 128 / 80 / 42-split layouts, the last split ragged
GEOMS = [(1, 1, 1), (1, 1, 40), (1, 40, 1), (3, 5, 29), (2, 3, 125), (2, 3, 126), (2, 2, 300), (1, 2, 381), (1, 2, 382),
         (1, 3, 514), (5, 96, 96)]
VARIANT1_GEOM = (3, 5, 29)                           # where the stream pairs run variant 1 (0 / 2 alternate elsewhere)
GUARD_GEOMS = [(2, 7, 45), (1, 3, 200), (1, 2, 400)]   # sixteen-wave | eight-wave, register-streamed | two-segment window
FULL_PAIRS = [(280, 280), (70, 70), (27, 70)]
BS64, BS160, BS512 = (64, 96, 96), (160, 96, 96), (512, 96, 96)
BS512_CASES = [(280, 280, 1, 0), (70, 70, 0, 2)]     # (Cin, Cout, pad, variant)
SENTINEL = 1234.5
EXACT = float(2 ** 24)


def _dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def variant_of(pair, geom, pad):
    if pair not in STREAM_PAIRS:
        return 0
    if geom == VARIANT1_GEOM:
        return 1
    return (0, 2)[(GEOMS.index(geom) + pad + STREAM_PAIRS.index(pair)) % 2] if geom in GEOMS else 2 * pad


def _nqpad(geo):
    from mmlf_amd import _lib
    return int(_lib.load().mmlf_relu_mask_words(geo.B, geo.H, geo.W)) // 4096 * 256      # whole 256-position tiles


def _view(geo, t, cs):
    return t[:geo.NQ * cs].view(geo.B, geo.R, geo.P, cs)


def _draw(shape, gen, integer, values=(-2, -1, 1, 2)):
    """uniform in [-1, 1), or -- the exact-integer leg -- a uniform pick of `values`"""
    if not integer:
        return torch.rand(shape, device=gen.device, generator=gen) * 2 - 1
    v = torch.tensor(values, dtype=torch.float32, device=gen.device)
    return v[torch.randint(0, len(values), shape, device=gen.device, generator=gen)]


def _grid_rand(geo, C, cs, off, h, w, gen, integer, values=(-2, -1, 1, 2)):
    """a zeroed grid buffer of the 2x2 allocation with drawn values on the extent (h, w) at grid offset (off, off), channels
    [0, C), generated patch by patch (a bs = 512 tensor of 280 channels holds 5.5 GB)"""
    t = torch.zeros(geo.alloc * cs, device=gen.device)
    v = _view(geo, t, cs)
    for b0 in range(0, geo.B, 32):
        n = min(32, geo.B - b0)
        v[b0:b0 + n, off:off + h, off:off + w, :C] = _draw((n, h, w, C), gen, integer, values)
    return t


def _compare(got, ref, bound, integer, what):
    """real-valued leg: the shared float64 bar.  Exact-integer leg: the precondition on the reference, then equality of bits."""
    if not integer:
        return check_sum_bar(got, ref, bound, what)
    assert float(bound.max()) < EXACT, (what, 'precondition: sum|a||b| + |gw0| < 2^24', float(bound.max()))
    bad = got != ref
    if bool(bad.any()):
        k = int(bad.reshape(-1).to(torch.uint8).argmax())
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} elements differ from the exact result; flat index {k} '
                             f'holds {float(got.reshape(-1)[k])!r}, exact {float(ref.reshape(-1)[k])!r}')


def _fresh(geo, cs, cs_buf, off, n_store, out_shift, fill, dev):
    """a buffer as the engine hands it to a launch (zeroed slack: fill = 0) or a wider sentinel-filled one, with NaN on every
    element the launch must write: positions [out_shift, NQpad + out_shift), channels [off, off + n_store)"""
    t = torch.full((geo.alloc * cs_buf,), float(fill), device=dev)
    t.view(-1, cs_buf)[out_shift:_nqpad(geo) + out_shift, off:off + n_store] = float('nan')
    return t


def _written(geo, buf, cs_buf, off, n_store, place, h, w, out_shift, want_fn, chunk, fill, integer, what):
    """`buf` after a 2x2 launch that stores channels [off, off + n_store) of extent (h, w) at grid offset (place, place): on the
    extent what want_fn(b0, b1) returns for images [b0, b1) -- (value, bound) of the first channels, zero behind them; exactly
    zero on every other position the epilogue writes (q + out_shift, q < NQpad: border, pad channels, tile padding); `fill`
    everywhere else (other channels, head, tail slack)"""
    B = geo.B
    got = buf.view(-1, cs_buf)
    gv = got[:geo.NQ].view(B, geo.R, geo.P, cs_buf)
    sl = (slice(None), slice(place, place + h), slice(place, place + w), slice(off, off + n_store))
    for b0 in range(0, B, chunk):
        want, bound = want_fn(b0, min(B, b0 + chunk))
        pad = (0, n_store - want.shape[-1])
        _compare(gv[b0:b0 + chunk][sl].double(), torch.nn.functional.pad(want, pad), torch.nn.functional.pad(bound, pad),
                 integer, what)
    exp = torch.full_like(got, fill)
    exp[out_shift:_nqpad(geo) + out_shift, off:off + n_store] = 0
    ev = exp[:geo.NQ].view(B, geo.R, geo.P, cs_buf)
    ev[sl] = gv[sl]
    bad = (got != exp).view(-1)
    if bool(bad.any()):
        k = int(bad.to(torch.uint8).argmax())
        raise AssertionError(f'{what}: position {k // cs_buf} channel {k % cs_buf} holds {float(got.view(-1)[k])!r}, expected '
                             f'{float(exp.view(-1)[k])!r} (P={geo.P} NQ={geo.NQ} NQpad={_nqpad(geo)} alloc={geo.alloc})')


def _amax_rule(geo, buf, cs, what):
    """the project's rule for a producer's amax array (tests/test_gpu_kernels.py): the head holds the tensor's true maximum,
    a row entry is no smaller than the row's true maximum"""
    true = geo.amax_of(buf, cs)
    got = geo.amax_canonical(buf.absmax)
    assert float(got[0]) == float(true[0]), (what, float(got[0]), float(true[0]))
    assert bool((got >= true).all()), what


class _Case:
    """one (geometry, layer, placement, variant, leg): operands and float64 references, shared by the modes that run on it"""

    def __init__(self, B, H, W, cin, cout, pad, variant, integer, seed):
        from mmlf_amd import engine
        self.dev = dev = _dev()
        self.geo = geo = engine.Geometry(B, H, W)
        self.cin, self.cout, self.pad, self.variant, self.integer = cin, cout, pad, variant, integer
        self.cs_in, self.cs_out = engine.cs_of(cin), engine.cs_of(cout)
        self.gen = gen = torch.Generator(device=dev).manual_seed(seed)
        # forward input x: extent (ih, iw) at (ioff, ioff); output gradient g: extent (oh, ow) at (ooff, ooff)
        self.ih, self.iw, self.ioff = (H, W, 1) if pad else (H + 1, W + 1, 0)
        self.oh, self.ow, self.ooff = (H + 1, W + 1, 0) if pad else (H, W, 1)
        self.fwd_shift = 0 if pad else geo.P + 1
        self.x = _grid_rand(geo, cin, self.cs_in, self.ioff, self.ih, self.iw, gen, integer)
        self.g = _grid_rand(geo, cout, self.cs_out, self.ooff, self.oh, self.ow, gen, integer, (-1, 1))
        # the ReLU reference of dx: a tensor of its own, or -- at 160 patches and more, to bound memory -- the layer input itself
        self.rf = self.x if B >= 160 else _grid_rand(geo, cin, self.cs_in, self.ioff, self.ih, self.iw, gen, integer)
        w = _draw((cout, cin, 2, 2), gen, integer)
        self.w = w if integer else w / np.sqrt(4 * cin)
        self.wv = filter4(self.w.double(), variant)
        self.xv = _view(geo, self.x, self.cs_in)[..., :cin]
        self.gv = _view(geo, self.g, self.cs_out)[..., :cout]
        self.tag = f'{cin}->{cout} B={B} {H}x{W} pad={pad} variant={variant} {"integer" if integer else "real"}'
        self.chunk = max(1, 150_000 // (geo.R * geo.P))               # images per float64 reference

    # ---- weight + bias gradient
    def wgrad_ref(self):
        if not hasattr(self, '_wref'):
            gwr, gbr, gwa, gba = 0, 0, 0, 0
            for b0 in range(0, self.geo.B, self.chunk):
                xd, gd = self.xv[b0:b0 + self.chunk].double(), self.gv[b0:b0 + self.chunk].double()
                r, s = wgrad4_ref(xd, gd, self.pad)
                a, c = wgrad4_ref(xd.abs(), gd.abs(), self.pad)
                gwr, gbr, gwa, gba = gwr + r, gbr + s, gwa + a, gba + c
            self._wref = (unfilter4(gwr, self.variant), gbr, unfilter4(gwa, self.variant), gba)
        return self._wref

    def check_wgrad(self, mode):
        from mmlf_amd import _lib, engine
        engine.CONV_MODE = mode                                   # (restored by the _mode fixture)
        gw0 = _draw(self.w.shape, self.gen, self.integer, (-3, -2, -1, 0, 1, 2, 3))
        gb0 = _draw((self.cout,), self.gen, self.integer, (-3, -2, -1, 0, 1, 2, 3))
        gw, gb = gw0.clone(), gb0.clone()
        geo = self.geo
        ws = torch.empty(int(_lib.load().mmlf_wgrad_workspace_floats(self.cin, self.cout, geo.B, geo.H, geo.W)), device=self.dev)
        engine.wgrad(geo, self.x, self.cs_in, self.cin, self.g, self.cs_out, self.cout, self.fwd_shift, gw, gb, self.variant, ws)
        gwr, gbr, gwa, gba = self.wgrad_ref()
        _compare(gw.double(), gw0.double() + gwr, gw0.double().abs() + gwa, self.integer, f'weight gradient {mode} {self.tag}')
        _compare(gb.double(), gb0.double() + gbr, gb0.double().abs() + gba, self.integer, f'bias gradient {mode} {self.tag}')

    # ---- data gradient: out[q + d_shift] on the forward input's extent
    def dgrad_want(self, keep_of):
        def want(b0, b1):
            gd = self.gv[b0:b1].double()
            keep = keep_of(b0, b1)
            return dgrad4_ref(gd, self.wv, self.pad) * keep, dgrad4_ref(gd.abs(), self.wv.abs(), self.pad)
        return want

    def keep_of(self, ref, cs_ref):
        if ref is None:
            return lambda b0, b1: 1
        rv = _view(self.geo, ref, cs_ref)
        o = self.ioff
        return lambda b0, b1: rv[b0:b1, o:o + self.ih, o:o + self.iw, :self.cin] > 0

    def launch_dgrad(self, mode, out, cs_buf, off, n_store, ref=None, mask_in=None):
        from mmlf_amd import engine
        engine.CONV_MODE = mode
        geo = self.geo
        pk = engine.pack_filter(self.w, self.variant, True)
        engine.conv(geo, self.g, self.cs_out, self.cout, pk, None, self.cin, out, cs_buf, geo.P + 1 - self.fwd_shift, self.ih,
                    self.iw, False, ref=ref, cs_ref=self.cs_in if ref is not None else 0, n_store=n_store, out_off=off,
                    mask_in=mask_in)

    def relu_mask(self, mode):
        """a ReLU mask as bits, written by a forward launch of this geometry, width and placement (what the data gradient's
        launch is, seen as a convolution): its ReLU output y and the mask of (y > 0)"""
        from mmlf_amd import engine
        engine.CONV_MODE = mode
        geo = self.geo
        w2 = _draw((self.cin, self.cout, 2, 2), self.gen, self.integer)
        src = _grid_rand(geo, self.cout, self.cs_out, self.ooff, self.oh, self.ow, self.gen, self.integer)
        bias = _draw((self.cin,), self.gen, self.integer, (-3, -2, -1, 0, 1, 2, 3))
        y, mask = geo.buf(self.cs_in, self.dev), geo.relu_mask(self.dev)
        mask.fill_(-1)
        engine.conv(geo, src, self.cs_out, self.cout, engine.pack_filter(w2 if self.integer else w2 / np.sqrt(4 * self.cout), 0, False),
                    bias, self.cin, y, self.cs_in, geo.P + 1 - self.fwd_shift, self.ih, self.iw, True, mask_out=mask)
        return y, mask

    def check_dgrad(self, mode, whole=True, patches=None):
        """the three ReLU forms.  whole: every position of the buffer; patches: these images' extents only (full size)"""
        geo, cs, dev = self.geo, self.cs_in, self.dev
        d_shift = geo.P + 1 - self.fwd_shift
        forms = [('plain', None), ('relu_ref', self.rf)]
        if mode == 'f16x3':
            forms.append(('relu_mask_in', None))
        for name, ref in forms:
            what = f'data gradient {name} {mode} {self.tag}'
            mask = None
            if name == 'relu_mask_in':
                y, mask = self.relu_mask(mode)
                keep = self.keep_of(y, cs)
            else:
                keep = self.keep_of(ref, cs)
            out = _fresh(geo, cs, cs, 0, cs, d_shift, 0.0, dev)
            if mode == 'f16x3':
                out.absmax = torch.zeros(geo.amax_n, device=dev)
            self.launch_dgrad(mode, out, cs, 0, cs, ref=ref, mask_in=mask)
            want = self.dgrad_want(keep)
            if whole:
                _written(geo, out, cs, 0, cs, self.ioff, self.ih, self.iw, d_shift, want, self.chunk, 0.0, self.integer, what)
            else:
                ov = _view(geo, out, cs)
                o = self.ioff
                for b in patches:
                    val, bound = want(b, b + 1)
                    _compare(ov[b:b + 1, o:o + self.ih, o:o + self.iw, :self.cin].double(), val, bound, self.integer,
                             f'{what} patch {b}')
            if mode == 'f16x3':
                _amax_rule(geo, out, cs, what)
            del out

    def check_dgrad_slice(self, mode):
        """a channel slice of a wider sentinel-filled buffer (N_store = Cin < cs_out, at an offset): the other channels and
        every position the launch does not write keep the sentinel"""
        geo, dev = self.geo, self.dev
        off, cs_buf = 8, self.cs_in + 16
        d_shift = geo.P + 1 - self.fwd_shift
        out = _fresh(geo, self.cs_in, cs_buf, off, self.cin, d_shift, SENTINEL, dev)
        self.launch_dgrad(mode, out, cs_buf, off, self.cin, ref=self.rf)
        _written(geo, out, cs_buf, off, self.cin, self.ioff, self.ih, self.iw, d_shift, self.dgrad_want(self.keep_of(self.rf, self.cs_in)),
                 self.chunk, SENTINEL, self.integer, f'data gradient channel slice {mode} {self.tag}')


@pytest.fixture(autouse=True)
def _mode():
    from mmlf_amd import engine
    keep = engine.CONV_MODE
    yield
    engine.CONV_MODE = keep


def _seed(B, H, W, cin, cout, pad, integer):
    return B * 100003 + H * 1009 + W * 101 + cin * 7 + cout * 3 + pad * 2 + int(integer)


# ------------------------------------------------------------------------------------------------ the sweep
@pytest.mark.parametrize('B,H,W', GEOMS)
@pytest.mark.parametrize('cin,cout', PAIRS)
@pytest.mark.parametrize('pad', [1, 0])
@pytest.mark.parametrize('mode', MODES)
def test_backward2x2_exact_integer_sweep(mode, pad, cin, cout, B, H, W):
    """the exact-integer leg: weight, bias and data gradient (three ReLU forms, every position of the buffer) equal the
    float64 reference bit for bit"""
    c = _Case(B, H, W, cin, cout, pad, variant_of((cin, cout), (B, H, W), pad), True, _seed(B, H, W, cin, cout, pad, True))
    c.check_wgrad(mode)
    c.check_dgrad(mode)


@pytest.mark.parametrize('B,H,W', GEOMS)
@pytest.mark.parametrize('cin,cout', PAIRS)
@pytest.mark.parametrize('pad', [1, 0])
@pytest.mark.parametrize('mode', MODES)
def test_backward2x2_real_valued_sweep(mode, pad, cin, cout, B, H, W):
    """the real-valued leg at the shared float64 bar: the same three checks"""
    c = _Case(B, H, W, cin, cout, pad, variant_of((cin, cout), (B, H, W), pad), False, _seed(B, H, W, cin, cout, pad, False))
    c.check_wgrad(mode)
    c.check_dgrad(mode)


@pytest.mark.parametrize('cin,cout', PAIRS)
@pytest.mark.parametrize('mode', MODES)
def test_backward2x2_accumulate_flag_guard_bands_and_channel_slices(mode, cin, cout):
    """Through the C entry points with accumulate = 0 (gw / gb prefilled with NaN: overwritten, not read) and 1; gw, gb and
    the workspace -- sized by mmlf_wgrad_workspace_floats / mmlf_conv2x2_wgrad_thin_workspace_floats, NaN-filled -- sit between
    sentinel guard bands that must come back unchanged.  Then the data gradient as a channel slice of a wider buffer, on a
    frame per kernel family.  Exact-integer inputs on the first frame, real-valued ones on the others."""
    from mmlf_amd import _lib, engine
    from mmlf_amd._lib import call, ptr
    dev = _dev()
    G = 256                                            # guard floats on either side (keeps 16-byte alignment)

    def guarded(n, inner):
        t = torch.full((G + n + G,), SENTINEL, device=dev)
        t[G:G + n] = inner
        return t, t[G:G + n]

    for k, (B, H, W) in enumerate(GUARD_GEOMS):
        pad, integer = (k + 1) % 2, k == 0
        variant = variant_of((cin, cout), (B, H, W), pad)
        c = _Case(B, H, W, cin, cout, pad, variant, integer, _seed(B, H, W, cin, cout, pad, integer))
        c.check_dgrad_slice(mode)
        geo = c.geo
        thin = cout <= engine.THIN_MAX_N and cin >= engine.THIN_MIN_K
        nws = int(_lib.load().mmlf_conv2x2_wgrad_thin_workspace_floats(cin) if thin else
                  _lib.load().mmlf_wgrad_workspace_floats(cin, cout, B, H, W))
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


# ------------------------------------------------------------------------------------------------ full size: 96 x 96 patches
@pytest.mark.timeout(600)
@pytest.mark.parametrize('integer', [True, False], ids=['integer', 'real'])
@pytest.mark.parametrize('pad', [1, 0])
@pytest.mark.parametrize('cin,cout', FULL_PAIRS)
def test_backward2x2_bs64(cin, cout, pad, integer):
    """64 patches (the measured batch per GPU; 19 216 chunks): weight, bias and data gradient of the three modes, element by
    element, on one set of operands and references"""
    B, H, W = BS64
    c = _Case(B, H, W, cin, cout, pad, variant_of((cin, cout), BS64, pad), integer, _seed(B, H, W, cin, cout, pad, integer))
    for mode in MODES:
        c.check_wgrad(mode)
        c.check_dgrad(mode)


@pytest.mark.timeout(600)
@pytest.mark.parametrize('integer', [True, False], ids=['integer', 'real'])
def test_backward2x2_bs160_wide_kernel_three_rounds(integer):
    """160 patches are 48 128 chunks, past the 42 * 1024 at which the wide split kernel takes 128 position splits (three rounds
    of workgroups) instead of 42: the whole 280 -> 280 weight gradient"""
    B, H, W = BS160
    c = _Case(B, H, W, 280, 280, 1, 0, integer, _seed(B, H, W, 280, 280, 1, integer))
    for mode in MODES:
        c.check_wgrad(mode)


@pytest.mark.timeout(900)
@pytest.mark.parametrize('cin,cout,pad,variant', BS512_CASES)
def test_backward2x2_bs512_exact_integer(cin, cout, pad, variant):
    """bs = 512, the benchmark's size (byte offsets pass 4 GiB at 280 channels), exact-integer leg: the whole weight and bias
    gradient in the three modes -- worst case 512 * 97 * 97 * 2 * 1 = 9.6e6 < 2^24 -- and the data gradient on the first and
    the last patch and one seeded patch of every 64"""
    B, H, W = BS512
    c = _Case(B, H, W, cin, cout, pad, variant, True, _seed(B, H, W, cin, cout, pad, True))
    rs = np.random.RandomState(cin + pad)
    patches = sorted({0, B - 1} | {b0 + int(rs.randint(64)) for b0 in range(0, B, 64)})
    for mode in MODES:
        c.check_wgrad(mode)
        c.check_dgrad(mode, whole=False, patches=patches)
