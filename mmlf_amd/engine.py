"""Host-side orchestration of the HIP kernels for the FeedForward trunk
(reference mmlf/model/feed_forward.py:206-269 forward; autograd backward reached from
mmlf/train/cli.py:257).  PyTorch supplies device memory and streams only; every arithmetic
step is a call through the C ABI (include/mmlf_hip.h).

Layout and indexing are described in include/mmlf_hip.h and DESIGN.md section 3.
"""
import contextlib
import ctypes
import os
import threading
from collections import namedtuple

import torch

from . import _lib
from ._lib import call, check, ptr

VAR_IDENTITY, VAR_TRANSPOSE, VAR_TRANSPOSE_FLIPH = 0, 1, 2
BN_BLOCKS = 1024
LOSS_BLOCKS = 1024


# widest layer (output channels) of the convolution and weight-gradient entry points, by filter size: one launch holds 288
# packed columns; the 2x2 entry points run wider layers as column blocks.  The head's oc stays within one launch.
MAX_WIDTH = {2: 512, 3: 288}
MAX_OC = 288
# widest layer whose first convolution's weight gradient may go to the side stream (OVERLAP_WGRAD below)
MAX_OVERLAP_WIDTH = 288


def cs_of(c):
    """channel stride (floats) used for a c-channel grid tensor: multiple of 8."""
    return (c + 7) // 8 * 8


class Geometry:
    """ksize 3: buffers sized and zeroed for the 3x3 kernels, whose taps reach 2P + 2 positions past a tile
    (mmlf_grid_alloc_positions_k3; the 2x2 allocation does not grow)"""

    def __init__(self, B, H, W, ksize=2):
        self.B, self.H, self.W = B, H, W
        self.ksize = ksize
        # pitch W + 2, H + 2 rows (the library reports its constant; csrc/common.h has the measured alternatives)
        self.P, self.R = W + int(_lib.load().mmlf_grid_pad_w()), H + int(_lib.load().mmlf_grid_pad_h())
        self.G = self.P * self.R
        self.NQ = B * self.G
        self.alloc = int(_lib.load().mmlf_grid_alloc_positions_k3(B, H, W) if ksize == 3
                         else _lib.load().mmlf_grid_alloc_positions(B, H, W))
        self.amax_n = int(_lib.load().mmlf_amax_entries(B, H, W))
        self.amax_head = int(_lib.load().mmlf_amax_head())             # tensor-maximum shards, then one entry per grid row
        self.amax_stride = int(_lib.load().mmlf_amax_shard_stride())
        if self.alloc * MAX_WIDTH[2] * 4 >= 2 ** 63 or self.NQ + 2 * self.P + 600 >= 2 ** 31:
            raise ValueError('batch x image too large for 32-bit grid positions')

    def buf(self, cs, device):
        """Grid buffer with zeroed head/tail slack (the kernels write everything else) and its zeroed amax
        array: a head of 64 partial maxima of |x| over the tensor (`amax_stride` floats apart), then
        [amax_head + r] = max |x| of grid row r; the tensor's producers raise the entries by atomic max and the
        f16-split kernels derive their power-of-two operand scales from them (include/mmlf_hip.h)."""
        t = torch.empty(self.alloc * cs, dtype=torch.float32, device=device)
        t.absmax = torch.empty(self.amax_n, dtype=torch.float32, device=device)
        call('mmlf_zero_slack_k3' if self.ksize == 3 else 'mmlf_zero_slack', ptr(t), cs, self.B, self.H, self.W, ptr(t.absmax),
             _lib.stream_ptr())
        return t

    def bufs(self, css, device):
        """several grid buffers (channel strides `css`, at most four) whose slack and amax arrays ONE launch zeroes"""
        assert 1 <= len(css) <= 4
        ts = []
        for cs in css:
            t = torch.empty(self.alloc * cs, dtype=torch.float32, device=device)
            t.absmax = torch.empty(self.amax_n, dtype=torch.float32, device=device)
            ts.append(t)
        n = len(ts)
        grid = (ctypes.c_void_p * 4)(*([ptr(t) for t in ts] + [None] * (4 - n)))
        amax = (ctypes.c_void_p * 4)(*([ptr(t.absmax) for t in ts] + [None] * (4 - n)))
        csa = (ctypes.c_int * 4)(*(list(css) + [0] * (4 - n)))
        call('mmlf_zero_slack4_k3' if self.ksize == 3 else 'mmlf_zero_slack4', grid, csa, amax, self.B, self.H, self.W,
             _lib.stream_ptr())
        return ts

    def relu_mask(self, device):
        """words for the bit form of one layer's ReLU mask (mmlf_conv2x2_h2 relu_mask_out / relu_mask_in)"""
        n = int(_lib.load().mmlf_relu_mask_words(self.B, self.H, self.W))
        return torch.empty(n, dtype=torch.int32, device=device)

    def amax_of(self, t, cs):
        """amax array of a grid tensor that did not come from buf() (tests, tools): computed with torch ops."""
        rows = t[:self.NQ * cs].view(self.B * self.R, self.P * cs).abs().amax(1)
        out = torch.zeros(self.amax_n, dtype=torch.float32, device=t.device)
        out[0] = rows.max()                # one shard holds it all
        out[self.amax_head:self.amax_head + rows.numel()] = rows
        return out

    def amax_canonical(self, a):
        """an amax array with the tensor maximum collapsed into shard 0 (what amax_of builds): kernels spread it over
        the shards by wave / row, so two arrays that describe the same tensor compare equal in this form only"""
        out = a.clone()
        out[:self.amax_head] = 0
        out[0] = a[:self.amax_head].max()
        return out


class _Workspace:
    """Scratch that is reused across calls (stream-ordered: one stream at a time, `enter_stream` orders a change of
    stream), one per (device, calling thread):
    nn.DataParallel drives replicas from one thread per device -- and nothing stops two of them from sharing a
    device -- while autograd's backward runs on its own thread per device.  Kept in thread-local storage, so a
    workspace (an 8 MB partial-sum buffer, a side stream, up to a few hundred MB of weight-gradient scratch) dies
    with its thread: DataParallel.parallel_apply starts fresh threads on every forward."""
    _tls = threading.local()

    @classmethod
    def get(cls, device):
        table = getattr(cls._tls, 'table', None)
        if table is None:
            table = cls._tls.table = {}
        key = (device.type, device.index)
        ws = table.get(key)
        if ws is None:
            ws = table[key] = cls(device)
        return ws

    def __init__(self, device):
        self.device = device
        self.side = torch.cuda.Stream(device=device) if device.type == 'cuda' else None
        self.partial = torch.empty(2 * 512 * max(BN_BLOCKS, LOSS_BLOCKS) + 8, dtype=torch.float64, device=device)
        self._packs = {}                 # packed_filters: signature -> (signature, table, store, views, columns)
        self._last_stream = None         # enter_stream
        self._scratch = {}               # scratch: (name, side) -> float32 buffer

    def packed_filters(self, items):
        """f16-split packed forms of many filters from ONE launch (mmlf_pack_filters_h2).  items: list of
        (key, weight tensor (Cout, Cin, 2, 2), variant, dgrad).  The descriptor table and the packed buffers persist
        across steps as long as the same weight storage is passed (Adam updates weights in place); the contents are
        re-made on every call.  Returns {key: packed tensor}.

        Conditions of use (the views are handed to the tape and read again by backward):
          * the weights must not change between a forward pass and its backward pass (the packed data-gradient forms
            were made from the forward's weights; the reference's loop and TrainStep step the optimizer after backward);
          * one (thread, device) workspace serves ONE stream at a time: the store is overwritten in stream order by the
            next forward.  If the calling thread switches streams, the new stream first waits for an event recorded on the
            old one behind this workspace's last use (`_last_use`), so a repack cannot overtake convolutions still reading
            the store;
          * one cache entry per signature (training packs forward + data-gradient forms, evaluation forward forms only):
            alternating train and eval steps re-uses both instead of re-allocating and re-uploading the table."""
        import numpy as np
        lib = _lib.load()
        sig = tuple((w.data_ptr(), w.shape[0], w.shape[1], int(var), int(dg)) for _, w, var, dg in items)
        self.enter_stream()
        caches = self._packs
        cache = caches.get(sig)
        if cache is None:
            if len(caches) >= 4:                       # (weights re-allocated: drop the stale entries)
                caches.clear()
            desc = np.zeros(len(items), dtype=np.dtype([('w', '<u8'), ('packed', '<u8'), ('Cout', '<i4'), ('Cin', '<i4'),
                                                         ('variant', '<i4'), ('dgrad', '<i4'), ('col0', '<i4'), ('np', '<i4')]))
            offs, total, col = [], 0, 0
            for i, (_, w, var, dg) in enumerate(items):
                cout, cin = w.shape[0], w.shape[1]
                K, N = (cout, cin) if dg else (cin, cout)
                nbytes = int(lib.mmlf_packed_filter_h2_bytes(cs_of(K), N))
                npk = int(lib.mmlf_packed_filter_h2_columns(N))
                if nbytes < 0 or npk < 0:
                    raise RuntimeError(f'pack_filters: unsupported channels K={K} N={N}')
                offs.append((total, nbytes))
                desc[i] = (w.data_ptr(), 0, cout, cin, int(var), int(dg), col, npk)
                total += (nbytes + 255) // 256 * 256
                col += npk
            store = torch.empty(total, dtype=torch.uint8, device=self.device)
            for i, (o, _) in enumerate(offs):
                desc['packed'][i] = store.data_ptr() + o
            table = torch.from_numpy(desc.view(np.uint8).copy()).to(self.device)
            views = [store[o:o + n].view(torch.float32) for o, n in offs]
            cache = caches[sig] = (sig, table, store, views, col)
        _, table, _, views, col = cache
        call('mmlf_pack_filters_h2', ptr(table), len(items), col, _lib.stream_ptr())
        return {key: v for (key, _, _, _), v in zip(items, views)}

    def enter_stream(self):
        """Orders a change of stream for EVERY buffer this workspace owns (the packed-filter store, `partial`, the
        scratch and weight-gradient buffers): if the calling thread has moved to another stream since the workspace was
        last used, the new stream first waits for the work the previous one had enqueued.  Called from the places that hand
        out or overwrite those buffers -- packed_filters(), scratch(), wgrad_ws() -- and at the entry of Trunk.forward /
        Trunk.backward (which use `partial` directly); one comparison per call when the stream has not changed."""
        if self.device.type != 'cuda':
            return
        cur = torch.cuda.current_stream(self.device)
        last = self._last_stream
        if last is not None and last != cur:
            cur.wait_event(last.record_event())
        self._last_stream = cur

    def scratch(self, name, n, side=False):
        """a float32 scratch buffer of at least n elements, reused across calls of this thread on this stream.  side: the one
        of that name for side-stream launches, which share no scratch with the main stream's and are ordered by their events"""
        if not side:
            self.enter_stream()
        t = self._scratch.get((name, side))
        if t is None or t.numel() < n:
            t = self._scratch[name, side] = torch.empty(n, dtype=torch.float32, device=self.device)
        return t

    def wgrad_ws(self, geo, cin, cout, side=False):
        query = _lib.load().mmlf_wgrad3x3_workspace_floats if geo.ksize == 3 else _lib.load().mmlf_wgrad_workspace_floats
        n = int(query(cin, cout, geo.B, geo.H, geo.W))
        if n < 0:
            raise RuntimeError(f'wgrad: unsupported channels {cin}->{cout}')
        return self.scratch('wgrad', n, side)


# 'f16x3': 2-way f16 split of power-of-two-scaled operands, 3 MFMA passes (f32-equivalent accuracy, 5.3x the
# f32 MFMA rate); 'bf16x6': 3-way bf16 split, 6 passes (no operand scaling needed); 'f32': exact-f32 MFMA
CONV_MODE = os.environ.get('MMLF_CONV_MODE', 'f16x3')
# per mode: the size query of a packed filter, the bytes per unit of its answer (the split forms count bytes, the f32 one
# floats) and the packing entry point; any other mode string runs the f32 kernels
_PACK = {'f16x3': ('mmlf_packed_filter_h2_bytes', 1, 'mmlf_pack_filter_h2'),
         'bf16x6': ('mmlf_packed_filter_split_bytes', 1, 'mmlf_pack_filter_split'),
         'f32': ('mmlf_packed_filter_floats', 4, 'mmlf_pack_filter')}
_PACK3 = ('mmlf_packed_filter3x3_floats', 4, 'mmlf_pack_filter3x3')


def _pack(who, query, unit, entry, w, variant, dgrad):
    cout, cin = w.shape[0], w.shape[1]
    K, N = (cout, cin) if dgrad else (cin, cout)
    # the kernels walk K in chunks of 8 over the channel stride of their input and only fill ceil(K/8) chunks;
    # cs_of(K)/8 == ceil(K/8)
    n = int(getattr(_lib.load(), query)(cs_of(K), N))
    if n < 0:
        raise RuntimeError(f'{who}: unsupported channels K={K} N={N}')
    out = torch.empty(n * unit // 4, dtype=torch.float32, device=w.device)
    call(entry, ptr(w), ptr(out), cout, cin, variant, int(dgrad), _lib.stream_ptr())
    return out


def pack_filter(w, variant, dgrad):
    return _pack('pack_filter', *_PACK.get(CONV_MODE, _PACK['f32']), w, variant, dgrad)


PROFILE = None   # bench.py sets this to a list to time the 280-wide conv / weight-gradient launches with HIP events


def _tic():
    """PROFILE: two timing events, the first recorded on the current stream (the stream the launch goes to: the side
    stream for the overlapped weight gradients)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    return e0, e1


def _toc(events, tag, flops, nbytes):
    events[1].record()
    PROFILE.append((tag, flops, events[0], events[1], nbytes))


@contextlib.contextmanager
def _timed(tag, flops, nbytes):
    """PROFILE: the launches inside the `with` block between two events, as one entry"""
    events = _tic()
    yield
    _toc(events, tag, flops, nbytes)


_UNTIMED = contextlib.nullcontext()      # what a launch that PROFILE does not time runs under


def _amax_of(geo, t, cs):
    """The amax array (tensor and grid-row maxima of |t|) the f16-split kernels scale by.  Grid tensors made
    by Geometry.buf carry it (their producers maintain it); for any other tensor it is computed here."""
    a = getattr(t, 'absmax', None)
    if a is None:
        return geo.amax_of(t, cs)
    if CHECK_ABSMAX:       # test hook: the producers' running maxima must be the tensor's true maxima
        true = geo.amax_of(t, cs)
        c = geo.amax_canonical(a)
        exact = geo.P >= 32                 # smaller pitches: rows behind a wave's first get an upper bound
        bad = (c != true) if exact else (c < true)
        bad[0] = c[0] != true[0]
        if bool(bad.any()):
            k = int(bad.nonzero()[0])
            raise AssertionError(f'amax entry {k} holds {float(c[k])!r}, true max |x| is {float(true[k])!r}')
    return a


CHECK_ABSMAX = bool(os.environ.get('MMLF_CHECK_ABSMAX'))
# MMLF_OVERLAP_WGRAD (default 1 since round 6; 0 switches it off): conv1's weight gradient of the wide blocks runs on a side
# stream beside the BatchNorm-backward kernels of the block underneath (which only need the data gradient).  It pays since the
# weight gradient is down to 2 x 232 registers per SIMD and both BatchNorm-backward kernels fit the 48 left (round 5:
# +0.9...1.1 % on two boxes, gradients bit-identical, profiles/r05_overlap_modes.log; round 6's same-box A/B:
# profiles/r06_ab_overlap_wgrad.log).  The side-stream launch takes ~11.3 ms instead of 7.6 (it shares the CUs) while 4.7 ms of
# BatchNorm kernels hide behind it; +5.5 GiB stay alive (x and dy of one block, until the main stream has waited for the launch).
# The events around a side-stream launch do not time the kernel alone: bench.py's roofline_wgrad is taken on the main-stream
# launches (conv2's gradients: same kernel, same shape).  History of the rejected forms: EXPERIMENTS.md 4.9.
OVERLAP_WGRAD = os.environ.get('MMLF_OVERLAP_WGRAD', '1') not in ('', '0')


# MMLF_CHECK_EXTENTS=1 (debug; the f16-split launches): before every convolution / weight-gradient launch the host compares
# the audited END of what the launch may touch behind each pointer (mmlf_audit_conv_h2 / mmlf_audit_wgrad_h2: derived from the
# launch geometry) with the bytes the tensor behind that pointer really has, and raises instead of launching.  The product
# kernels' range-checked descriptors DROP a stray access (conv_device.h: mmlf_records_left), so a wrong extent would be a quietly
# wrong result; this is the product-build signal for it (the -DMMLF_BOUNDS_DEBUG build counts accesses on the GPU instead).
CHECK_EXTENTS = bool(os.environ.get('MMLF_CHECK_EXTENTS'))
EXTENT_CHECKS = 0         # launches checked so far (tests)


def _audit(entry, scalars, n_ends, kind, have):
    """One launch against MMLF_CHECK_EXTENTS: `entry(*scalars, ends)` fills the n_ends audited ends; have maps the name of
    a pointer argument to (its index in ends, the tensor behind it or None, the pointer's offset in floats)."""
    global EXTENT_CHECKS
    ends = (ctypes.c_int64 * n_ends)()
    call(entry, *scalars, ends)
    for name, (k, t, off) in have.items():
        if t is None:
            continue
        # bytes from the tensor's first element (+ the offset) to the end of its storage
        got = t.untyped_storage().nbytes() - t.storage_offset() * t.element_size() - 4 * off
        if ends[k] > got:
            raise RuntimeError(f'MMLF_CHECK_EXTENTS: {kind}: the launch may touch {ends[k]} bytes behind `{name}`, '
                               f'the tensor has {got}')
    EXTENT_CHECKS += 1


def relu_bwd_slice(geo, src, cs_src, c_off, ref, cs_ref, ref_off, C, dst, cs_dst):
    """dst = src[..., c_off:c_off + C] where ref[..., ref_off:ref_off + C] > 0, zero elsewhere, as a compact grid tensor"""
    amax = getattr(dst, 'absmax', None)
    if CHECK_EXTENTS:
        _audit('mmlf_audit_relu_bwd_slice', (cs_src, c_off, cs_ref, ref_off, C, cs_dst, geo.B, geo.H, geo.W), 4,
               f'relu_bwd_slice C={C} {cs_src}+{c_off} B={geo.B} {geo.H}x{geo.W}',
               {'src': (0, src, 0), 'ref': (1, ref, 0), 'dst': (2, dst, 0), 'amax': (3, amax, 0)})
    call('mmlf_relu_bwd_slice', ptr(src), cs_src, c_off, ptr(ref), cs_ref, ref_off, C, ptr(dst), cs_dst, geo.B, geo.H, geo.W,
         ptr(amax), _lib.stream_ptr())


THIN_MAX_N, THIN_MIN_K = 2, 64     # mmlf_conv2x2_thin: at most 2 output channels over at least 64 input channels


def wgrad(geo, x, cs_in, cin, g, cs_g, cout, g_shift, gw, gb, variant, workspace, side=False):
    """weight + bias gradient, accumulated into gw / gb (side: the launch goes to the side stream and must not share
    scratch with main-stream launches).  gw None: the bias gradient alone, one pass over g (the entry points' bias-only
    form; x is not read); gb None: the weight gradient alone."""
    if cout <= THIN_MAX_N and cin >= THIN_MIN_K and cs_in <= 512:
        # a matrix-vector product (the BASE / UPR head): plain float32 FMAs, bound by reading x once
        ws = _Workspace.get(x.device).scratch('thin_wgrad', int(_lib.load().mmlf_conv2x2_wgrad_thin_workspace_floats(cin)), side)
        call('mmlf_conv2x2_wgrad_thin', ptr(x), cs_in, cin, ptr(g), cs_g, cout, g_shift, ptr(gw), ptr(gb), variant, 1,
             ptr(ws), geo.B, geo.H, geo.W, _lib.stream_ptr())
        return
    args = (ptr(x), cs_in, cin, ptr(g), cs_g, cout, g_shift, ptr(gw), ptr(gb), variant, 1, ptr(workspace),
            geo.B, geo.H, geo.W)
    timed = _UNTIMED
    if PROFILE is not None and cin >= 256 and cout >= 256 and gw is not None:
        # algorithmic FLOPs: the convolution's valid output positions x Cout x 4 taps x Cin, 2 FLOP per MAC (the
        # gradient of a pad-1 convolution lives at grid offset 0 with extent (H+1, W+1), of a pad-0 one at (1, 1))
        vh, vw = (geo.H + 1, geo.W + 1) if g_shift == 0 else (geo.H, geo.W)
        nbytes = 4.0 * geo.B * (cin * (geo.H * geo.W if g_shift == 0 else (geo.H + 1) * (geo.W + 1)) + cout * vh * vw)
        timed = _timed('wgrad_side' if side else 'wgrad', 2.0 * geo.B * vh * vw * cout * 4 * cin, nbytes)
    with timed:
        if CONV_MODE == 'f16x3':
            ax, ag = _amax_of(geo, x, cs_in), _amax_of(geo, g, cs_g)
            if CHECK_EXTENTS:
                _audit('mmlf_audit_wgrad_h2', (cs_in, cin, cs_g, cout, g_shift, geo.B, geo.H, geo.W), 7,
                       f'wgrad {cin}->{cout} B={geo.B} {geo.H}x{geo.W} g_shift={g_shift}',
                       {'in': (0, x, 0), 'g': (1, g, 0), 'gw': (2, gw, 0), 'gb': (3, gb, 0), 'workspace': (4, workspace, 0),
                        'in_amax': (5, ax, 0), 'g_amax': (6, ag, 0)})
            call('mmlf_conv2x2_wgrad_h2', *args, ptr(ax), ptr(ag), _lib.stream_ptr())
        else:
            call('mmlf_conv2x2_wgrad_split' if CONV_MODE == 'bf16x6' else 'mmlf_conv2x2_wgrad', *args, _lib.stream_ptr())


def conv(geo, x, cs_in, K, packed, bias, N, out, cs_out, out_shift, vh, vw, relu, ref=None, cs_ref=0,
         n_store=None, out_off=0, bn_partial=None, mask_out=None, mask_in=None, w_master=None, variant=0):
    """bn_partial (f16x3 only): a float64 buffer that receives per-workgroup sums of the output and its
    square per channel -- BatchNorm's training statistics without another pass over the output.
    mask_out / mask_in (f16x3 only): the ReLU mask of the output as bits (Geometry.relu_mask), written by the
    forward launch and read by the data gradient of the layer above instead of `ref`."""
    aout = getattr(out, 'absmax', None)
    if (w_master is not None and N <= THIN_MAX_N and K >= THIN_MIN_K and cs_in <= 512 and ref is None and mask_in is None
            and mask_out is None and bn_partial is None and out_off == 0 and n_store in (None, cs_out)):
        # a matrix-vector product (the BASE / UPR head): straight from the OIHW master filter
        ws = _Workspace.get(x.device).scratch('thin_fwd', int(_lib.load().mmlf_conv2x2_thin_workspace_floats(geo.B, geo.H, geo.W)))
        call('mmlf_conv2x2_thin', ptr(x), cs_in, K, ptr(w_master), ptr(bias), N, ptr(out), cs_out, out_shift, vh, vw,
             geo.B, geo.H, geo.W, int(relu), variant, ptr(ws), ptr(aout), _lib.stream_ptr())
        return
    n_store = cs_out if n_store is None else n_store
    # bench.py's per-launch timing: the 280-wide launches (tag 'conv') and the 70 -> 70 stream-layer launches ('conv70')
    timed = _UNTIMED
    if PROFILE is not None and ((K >= 256 and N >= 256) or (K == N and 64 <= K < 128)):
        # algorithmic FLOPs of this launch: valid output positions x N x 4 taps x K, 2 FLOP per MAC; algorithmic BYTES: the
        # input's and the output's stored extents once each (a pad-1 convolution reads (H, W) and writes (H+1, W+1), a pad-0
        # one the other way round), float32, unpadded channels
        nbytes = 4.0 * geo.B * (K * (geo.H * geo.W if out_shift == 0 else (geo.H + 1) * (geo.W + 1)) + N * vh * vw)
        timed = _timed('conv' if K >= 256 else 'conv70', 2.0 * geo.B * vh * vw * N * 4 * K, nbytes)
    args = (ptr(x), cs_in, K, ptr(packed), ptr(bias), N, ptr(out) + 4 * out_off, cs_out, n_store, out_shift, vh, vw,
            geo.B, geo.H, geo.W, int(relu), ptr(ref), cs_ref)
    with timed:
        if CONV_MODE == 'f16x3':
            ax = _amax_of(geo, x, cs_in)
            if CHECK_EXTENTS:
                _audit('mmlf_audit_conv_h2', (cs_in, K, N, cs_out, n_store, out_shift, cs_ref, geo.B, geo.H, geo.W), 9,
                       f'conv {K}->{N} B={geo.B} {geo.H}x{geo.W} shift={out_shift}',
                       {'in': (0, x, 0), 'packed': (1, packed, 0), 'bias': (2, bias, 0), 'out': (3, out, out_off),
                        'ref': (4, ref, 0), 'in_amax': (5, ax, 0), 'out_amax': (6, aout, 0), 'bn_partial': (7, bn_partial, 0),
                        'mask_out': (8, mask_out, 0), 'mask_in': (8, mask_in, 0)})
            call('mmlf_conv2x2_h2', *args, ptr(ax), ptr(aout), ptr(bn_partial), ptr(mask_out), ptr(mask_in), _lib.stream_ptr())
        else:
            call('mmlf_conv2x2_split' if CONV_MODE == 'bf16x6' else 'mmlf_conv2x2', *args, _lib.stream_ptr())


# ---------------------------------------------------------------------------------------------- 3x3 filters (--model_ksize 3)
# Exact-f32 MFMA kernels whatever MMLF_CONV_MODE says (include/mmlf_hip.h): both convolutions of a block are "same"
# convolutions, input and output at grid offset (1, 1) with extent (H, W).

def pack_filter3(w, variant, dgrad):
    return _pack('pack_filter3', *_PACK3, w, variant, dgrad)


def conv3(geo, x, cs_in, K, packed, bias, N, out, cs_out, relu, ref=None, cs_ref=0, n_store=None, out_off=0):
    """3x3 forward (or, on a dgrad-packed filter, data gradient): out[q + P + 1] from x[q + dy*P + dx]"""
    n_store = cs_out if n_store is None else n_store
    if CHECK_EXTENTS:
        _audit('mmlf_audit_conv3x3', (cs_in, K, N, cs_out, n_store, cs_ref if ref is not None else 0, geo.B, geo.H, geo.W), 5,
               f'conv3x3 {K}->{N} B={geo.B} {geo.H}x{geo.W}',
               {'in': (0, x, 0), 'packed': (1, packed, 0), 'bias': (2, bias, 0), 'out': (3, out, out_off), 'ref': (4, ref, 0)})
    prof = PROFILE is not None and K >= 256 and N >= 256
    with _timed('conv3x3', 2.0 * geo.B * geo.H * geo.W * N * 9 * K, 4.0 * geo.B * geo.H * geo.W * (K + N)) if prof else _UNTIMED:
        call('mmlf_conv3x3', ptr(x), cs_in, K, ptr(packed), ptr(bias), N, ptr(out) + 4 * out_off, cs_out, n_store,
             geo.B, geo.H, geo.W, int(relu), ptr(ref), cs_ref, _lib.stream_ptr())


def wgrad3(geo, x, cs_in, cin, g, cs_g, cout, gw, gb, variant, workspace):
    """3x3 weight + bias gradient, accumulated into gw / gb (gw None: the bias gradient alone, as in wgrad)"""
    if CHECK_EXTENTS:
        _audit('mmlf_audit_wgrad3x3', (cs_in, cin, cs_g, cout, geo.B, geo.H, geo.W), 5,
               f'wgrad3x3 {cin}->{cout} B={geo.B} {geo.H}x{geo.W}',
               {'in': (0, x, 0), 'g': (1, g, 0), 'gw': (2, gw, 0), 'gb': (3, gb, 0), 'workspace': (4, workspace, 0)})
    call('mmlf_conv3x3_wgrad', ptr(x), cs_in, cin, ptr(g), cs_g, cout, ptr(gw), ptr(gb), variant, 1, ptr(workspace),
         geo.B, geo.H, geo.W, _lib.stream_ptr())


class BlockSpec:
    """bn, like feed_forward._conv_block's argument: True = BatchNorm + ReLU behind the second convolution, False = the ReLU
    alone (model_no_batchnorm), None = nothing (the head block)"""

    def __init__(self, prefix, cin, cout, bn):
        self.prefix, self.cin, self.cout, self.bn = prefix, cin, cout, bn


# One block of the trunk, as Trunk.sites lists them in forward order.  chain: 0 ... 3 a stream (H, V, I, D), 4 out_net; k: the
# block's position in its chain; var: the stream's filter variant; last: the chain's last block.
Site = namedtuple('Site', 'index chain k spec var last')

# A grid activation: tensor, channel stride; relu: a ReLU wrote it, which the data gradient of the convolution that reads it
# applies (conv1's output; the output of a block without BatchNorm), mask: the bits of that ReLU if its launch left any.
_Act = namedtuple('_Act', 't cs relu mask')
# Channels [off, off + C) of a grid tensor of channel stride cs: a gradient on its way down, or where a block's output goes.
_Slice = namedtuple('_Slice', 't cs off')
# A convolution of a block: second: its pad-0 one (False: its pad-1 one), K -> N channels, the stream's variant, the packed
# filter, the bias and, for the thin kernels, the OIHW master filter.  A weight gradient is described by the first four.
_Filter = namedtuple('_Filter', 'second K N var packed bias master', defaults=(None, None, None))


class _Rec:
    """What a block's forward leaves on the tape for its backward.  x: the block's input (x.relu: the output of a block
    without BatchNorm, whose trailing ReLU the data gradient of conv1 applies); y: conv1's output behind its ReLU; z: conv2's
    output where BatchNorm or nothing follows; scale ... sinv: BatchNorm's coefficients and saved statistics; eval: they are
    the RUNNING statistics.  bn: backward goes through BatchNorm (spec.bn, unless the forward folded it into conv2: a frozen
    evaluation, whose block is then a ReLU-only one with the filter whose data-gradient form is pk2d)."""
    __slots__ = ('spec', 'var', 'x', 'y', 'z', 'scale', 'shift', 'smean', 'sinv', 'eval', 'bn', 'pk2d')

    def __init__(self, site, x, y, z):
        self.spec, self.var, self.x, self.y, self.z = site.spec, site.var, x, y, z
        self.scale = self.shift = self.smean = self.sinv = None
        self.eval, self.bn, self.pk2d = False, site.spec.bn, None


class _Tape:
    """One pass over the trunk: what its blocks share and what forward leaves for backward (Trunk.forward returns it).  plan:
    the forward's Plan (None: nothing is saved); packs: the step's prepacked filters; running: a train-mode pass moves
    BatchNorm's running statistics and counters (False: a later micro-batch of a step); tracked: the counters the pass moves;
    deferred: (z, scale, shift) of the streams' last blocks, whose BatchNorm-apply runs as ONE pass (None: each block
    applies its own); concat: kept behind forward for mmlf_relu_bwd_slice only; recs[site.index]: a live block's record."""
    __slots__ = ('geo', 'device', 'p', 'train', 'fold', 'plan', 'packs', 'running', 'tracked', 'deferred', 'concat', 'recs')

    def __init__(self, geo, device, p=None, train=False, fold=False, plan=None, packs=None, sites=0, running=True):
        self.geo, self.device, self.p, self.train, self.fold, self.plan, self.running = geo, device, p, train, fold, plan, running
        self.packs, self.tracked, self.deferred, self.concat, self.recs = packs or {}, [], None, None, [None] * sites


class _SideWgrad:
    """The weight gradient that one backward pass runs on the workspace's side stream (OVERLAP_WGRAD), and the pass's on_done
    hook.  A wide block's first convolution's weight gradient is launched there AFTER the block's data gradient is enqueued,
    which is all the BatchNorm-backward kernels of the block underneath need.  At most one launch is pending; settle() makes
    the main stream wait for it.  A workspace without a side stream (no CUDA device) overlaps nothing and touches no stream."""
    __slots__ = ('main', 'side', 'pending', 'kept', 'on_done')

    def __init__(self, ws, on_done, enabled):
        self.side = ws.side if enabled else None
        self.main = torch.cuda.current_stream() if self.side is not None else None
        self.pending, self.kept, self.on_done = None, None, on_done      # pending: (the launch's end, its on_done key)

    def takes(self, cin):
        # (wider layers run as column blocks, on kernels outside the overlap's register budget: main stream)
        return self.side is not None and 128 <= cin <= MAX_OVERLAP_WIDTH

    def launch(self, key, keep, run):
        """run() on the side stream, behind everything the main stream has enqueued; settle() reports key.  keep: the
        tensors it reads, held (no record_stream: deferred reuse makes the caching allocator grow and stall) until the next
        out_net block has enqueued its launches (_block_bwd) -- one block longer than settle() needs, and where the
        allocator's peak has always been."""
        ready = self.main.record_event()
        with torch.cuda.stream(self.side):
            self.side.wait_event(ready)
            run()
            self.pending, self.kept = (self.side.record_event(), key), keep

    def settle(self):
        """the main stream waits for the pending launch, whose key is complete then"""
        if self.pending is not None:
            self.main.wait_event(self.pending[0])
            if self.on_done:
                self.on_done(self.pending[1])
            self.pending = None

    def done(self, key):
        """every gradient of `key` is enqueued -- unless its weight gradient is the pending launch: settle() says so then"""
        if self.on_done and (self.pending is None or self.pending[1] != key):
            self.on_done(key)


class BlockPlan:
    """The backward launches of one live block, in backward order (Trunk.plan).  want: the wanted
    parameters of the block, as suffixes ('0.weight', '0.bias', '2.weight', '2.bias', '3.weight', '3.bias').
    reduce / apply: mmlf_bn_bwd_reduce / mmlf_bn_bwd_apply; wgrad2 / wgrad1: the weight-gradient launch of conv2 / conv1 (the
    bias gradient alone where the filter itself is not wanted: gw = NULL); dgrad2 / dgrad1: the data gradient of conv2 (-> dy)
    / conv1 (-> dx)."""
    LAUNCHES = ('reduce', 'apply', 'wgrad2', 'dgrad2', 'wgrad1', 'dgrad1')
    __slots__ = ('prefix', 'want') + LAUNCHES

    def __init__(self, prefix, want, bn, train, need_dx):
        self.prefix, self.want = prefix, frozenset(want)
        want_bn = bn and bool(self.want & {'3.weight', '3.bias'})
        self.wgrad1 = bool(self.want & {'0.weight', '0.bias'})
        self.wgrad2 = bool(self.want & {'2.weight', '2.bias'})
        self.dgrad1 = bool(need_dx)
        self.dgrad2 = self.wgrad1 or self.dgrad1                    # dy
        need_dz = self.wgrad2 or self.dgrad2
        self.apply = bool(bn) and need_dz
        # the batch sums feed dgamma / dbeta and, where the statistics were the batch's, the coefficients of dz
        self.reduce = bool(bn) and (want_bn or (need_dz and bool(train)))

    def launches(self):
        return [k for k in self.LAUNCHES if getattr(self, k)]

    def __eq__(self, other):
        return isinstance(other, BlockPlan) and all(getattr(self, k) == getattr(other, k) for k in self.__slots__)

    def __repr__(self):
        return f'BlockPlan({self.prefix}: {" ".join(self.launches())}; {sorted(self.want)})'


class Plan:
    """Which backward launches a step runs (Trunk.plan): a value, computed on the host without a library call.
    trainable: the wanted parameter names; input_grads: four bools; fold: BatchNorm is folded into conv2 (blocks below the
    head are ReLU-only ones); streams[s][k] / out[k]: the BlockPlan of a live block, None for a block that launches nothing;
    slices[s]: stream s's mmlf_relu_bwd_slice runs (ReLU-only blocks of a live stream)."""

    def __init__(self, trainable, input_grads, train, fold, streams, out, relu_only):
        self.trainable, self.input_grads, self.train, self.fold = trainable, input_grads, train, fold
        self.streams, self.out = streams, out
        self.stream_live = [any(b is not None for b in blocks) for blocks in streams]
        self.slices = [relu_only and live for live in self.stream_live]

    def of(self, site):
        """the BlockPlan of a Site, None where the block launches nothing"""
        return self.out[site.k] if site.chain == 4 else self.streams[site.chain][site.k]

    def blocks(self):
        """the live blocks in backward order"""
        return ([b for b in reversed(self.out) if b is not None]
                + [b for s in reversed(range(4)) for b in reversed(self.streams[s]) if b is not None])

    def counts(self):
        """launches of the backward pass by kind: {'wgrad', 'reduce', 'apply', 'dgrad', 'slice', 'bias_only'}; bias_only: the
        weight-gradient launches among 'wgrad' that form a bias gradient alone"""
        live = self.blocks()
        n = {'wgrad': sum(b.wgrad1 + b.wgrad2 for b in live), 'reduce': sum(b.reduce for b in live),
             'apply': sum(b.apply for b in live), 'dgrad': sum(b.dgrad1 + b.dgrad2 for b in live), 'slice': sum(self.slices)}
        n['bias_only'] = sum((b.wgrad1 and '0.weight' not in b.want) + (b.wgrad2 and '2.weight' not in b.want) for b in live)
        return n

    def __eq__(self, other):
        return (isinstance(other, Plan) and (self.trainable, self.input_grads, self.train, self.fold, self.streams, self.out)
                == (other.trainable, other.input_grads, other.train, other.fold, other.streams, other.out))


class Trunk:
    """Native forward/backward of in_net_hv / in_net_id / out_net (non-cross) with 2x2 or 3x3 filters, and, with 2x2
    filters, with or without BatchNorm (batchnorm=False: model_no_batchnorm, reference feed_forward.py:122-137 -- both ReLUs
    of a block ride in the convolutions' epilogues, training and inference take the same launches, and the gradient behind a
    block's trailing ReLU comes out of the data gradient of the convolution above it: _block_fwd, _block_bwd).
    `params` maps state_dict keys to device tensors.
    ksize 3 runs the exact-f32 3x3 kernels (conv3 / wgrad3): filters packed per layer, BatchNorm statistics by
    mmlf_bn_stats_train, the data gradient's ReLU by `ref`, inference with BatchNorm folded into conv2."""

    def __init__(self, chs, in_blocks, out_blocks, views, oc, momentum, eps=1e-5, ksize=2, batchnorm=True):
        if ksize not in (2, 3):
            raise ValueError(f'native trunk: ksize {ksize} (2 or 3)')
        if not batchnorm and ksize != 2:
            raise ValueError('native trunk: blocks without BatchNorm run on the 2x2 kernels only')
        self.batchnorm = bn = bool(batchnorm)
        self.ksize = ksize
        self.chs, self.views, self.oc = chs, views, oc
        self.momentum, self.eps = float(momentum), float(eps)
        cin0 = views * 3
        self.streams = []
        for key, net, var in (('h', 'in_net_hv', VAR_TRANSPOSE), ('v', 'in_net_hv', VAR_IDENTITY),
                              ('i', 'in_net_id', VAR_TRANSPOSE_FLIPH), ('d', 'in_net_id', VAR_IDENTITY)):
            blocks = [BlockSpec(f'{net}.0', cin0, chs, bn)]
            blocks += [BlockSpec(f'{net}.{k}', chs, chs, bn) for k in range(1, in_blocks)]
            self.streams.append((key, var, blocks))
        c = 4 * chs
        self.out_blocks = [BlockSpec(f'out_net.{k}', c, c, bn) for k in range(out_blocks - 1)]
        self.out_blocks.append(BlockSpec(f'out_net.{out_blocks - 1}', c, oc, None))
        if chs % 2 or cs_of(c) != c:
            raise ValueError('native trunk needs an even model_chs with 4*model_chs a multiple of 8')
        if c > MAX_WIDTH[ksize] or oc > MAX_OC:
            raise ValueError(f'native trunk: 4*model_chs = {c} (max {MAX_WIDTH[ksize]} with {ksize}x{ksize} filters), '
                             f'{oc} output channels (max {MAX_OC})')
        # every block once, in forward order (streams H, V, I, D, then out_net); reversed: backward's order.  The ONE listing
        # that _numel, plan, _prepack, forward and backward walk
        chains = [(var, blocks) for _, var, blocks in self.streams] + [(VAR_IDENTITY, self.out_blocks)]
        sites = [(c, k, spec, var, k == len(blocks) - 1) for c, (var, blocks) in enumerate(chains) for k, spec in enumerate(blocks)]
        self.sites = tuple(Site(i, *site) for i, site in enumerate(sites))
        # state_dict key -> element count of every parameter and BatchNorm buffer the blocks read through raw pointers
        # (check_params); h / v and i / d share their nets' keys
        self._numel = {}
        for spec in (site.spec for site in self.sites):
            n = {'0.weight': spec.cout * spec.cin * ksize * ksize, '0.bias': spec.cout,
                 '2.weight': spec.cout * spec.cout * ksize * ksize, '2.bias': spec.cout}
            if spec.bn is True:
                n.update({f'3.{k}': spec.cout for k in ('weight', 'bias', 'running_mean', 'running_var')})
                n['3.num_batches_tracked'] = 1
            self._numel.update({f'{spec.prefix}.{k}': v for k, v in n.items()})
        self._grad_names = [n for n in self._numel if n.endswith(('.weight', '.bias'))]     # what backward accumulates into
        self._checked, self._plans = {}, {}

    def _check_dict(self, what, d, names, dev):
        """every d[name]: present, on `dev`, contiguous, float32 (the BatchNorm counter int64), of the element count its block
        implies.  Once per (data_ptr, device) signature, as _Workspace.packed_filters keeps its table: a training run's
        parameters and gradient views keep their storage (Adam updates in place), so a step pays one pointer read per tensor."""
        ts = [d.get(name) for name in names]
        sig = (dev, *[t if t is None else (t.data_ptr(), t.device) for t in ts])
        if self._checked.get(what) != sig:
            for name, t in zip(names, ts):
                check(t, f'{what}[{name!r}]', dev, torch.int64 if name.endswith('num_batches_tracked') else torch.float32,
                      numel=self._numel[name])
            self._checked[what] = sig

    def check_params(self, p, dev):
        """every parameter and buffer the trunk will read -- the pack kernels read an OIHW master filter through its raw
        pointer, so a channels_last model is refused, like one on another device"""
        self._check_dict('parameters', p, self._numel, dev)

    # ------------------------------------------------------------------ the plan of a backward pass
    def plan(self, trainable=None, input_grads=None, train=True, fold=None):
        """Which backward launches run when the gradients of the parameters `trainable` (state_dict names; None: all of
        _grad_names) and of the stacks `input_grads` (four bools; None: none) are asked for.  Both passes follow it and
        nothing else decides a launch: forward keeps a record for the live blocks only, backward runs the listed launches.
        A block is live if the gradient must reach its output: it has a wanted parameter, or a block beneath it in its chain
        has one (the stream blocks are beneath out_net.0; H and V share in_net_hv's names, I and D in_net_id's), or, in a
        stream, its stack's gradient is wanted.  train: BatchNorm's statistics are the batch's.  fold: BatchNorm is folded
        into conv2; None: as forward decides under a tape (a 2x2 trunk in eval mode of which no parameter is wanted)."""
        names = set(self._grad_names)
        wanted = frozenset(names if trainable is None else trainable)
        if not wanted <= names:
            raise ValueError(f'Trunk.plan: {sorted(wanted - names)[0]!r} is no parameter of this trunk')
        want_x = tuple(bool(w) for w in input_grads) if input_grads is not None else (False,) * 4
        if len(want_x) != 4:
            raise ValueError('Trunk.plan: input_grads takes four bools (streams H, V, I, D)')
        if fold is None:
            fold = self.batchnorm and not train and not wanted and self.ksize == 2
        if fold and wanted:
            raise ValueError('Trunk.plan: a folded BatchNorm has no parameter gradients')
        key = (wanted, want_x, bool(train), bool(fold))
        cached = self._plans.get(key)                # (a training run asks for the same plan twice per step)
        if cached is not None:
            return cached
        if len(self._plans) >= 64:
            self._plans.clear()
        chains = [[] for _ in range(5)]
        for site in self.sites:
            spec = site.spec
            if site.k == 0:
                # a chain's first block needs dx where its stack's gradient is wanted (a stream) or a stream is live (out_net)
                live = want_x[site.chain] if site.chain < 4 else any(b is not None for blocks in chains for b in blocks)
            want = {n[len(spec.prefix) + 1:] for n in wanted if n.startswith(spec.prefix + '.')}
            need_dx = live                           # the block beneath is live, or the stack's gradient is wanted
            live = live or bool(want)
            chains[site.chain].append(BlockPlan(spec.prefix, want, spec.bn is True and not fold, train, need_dx) if live else None)
        made = self._plans[key] = Plan(wanted, want_x, bool(train), bool(fold), chains[:4], chains[4],
                                       not self.batchnorm or bool(fold))
        return made

    # ------------------------------------------------------------------ filters
    def _prepack(self, p, dev, plan, fold=False):
        """every packed filter a step needs -- forward and the data-gradient forms of the launches `plan` contains (None: no
        backward follows) -- from ONE launch (f16 split only; the other modes pack per layer).  fold: BatchNorm is folded
        into conv2 (_block_fwd packs the folded filter itself), so conv2's master filter is not packed.
        Keys: (parameter name, variant, dgrad)."""
        if CONV_MODE != 'f16x3' or dev.type != 'cuda' or self.ksize != 2:
            return {}
        items = []
        add = lambda name, var, dgrad: items.append(((name, var, dgrad), p[name], var, dgrad))       # noqa: E731
        for site in self.sites:
            spec, var, bp = site.spec, site.var, plan.of(site) if plan else None
            thin = spec.cout <= THIN_MAX_N and spec.cin >= THIN_MIN_K      # the head's first conv runs from the master filter
            own2 = not (fold and spec.bn is True)
            if not thin:
                add(f'{spec.prefix}.0.weight', var, False)
            if own2:
                add(f'{spec.prefix}.2.weight', var, False)
            if bp is not None and own2 and bp.dgrad2:
                add(f'{spec.prefix}.2.weight', var, True)
            if bp is not None and bp.dgrad1:
                add(f'{spec.prefix}.0.weight', var, True)
        return _Workspace.get(dev).packed_filters(items)

    def _pack(self, w, var, dgrad):
        return (pack_filter3 if self.ksize == 3 else pack_filter)(w, var, dgrad)

    def _packed(self, tape, name, var, dgrad):
        """the packed form of filter `name`: from the step's prepack, or else packed now"""
        pk = tape.packs.get((name, var, dgrad))
        return pk if pk is not None else self._pack(tape.p[name], var, dgrad)

    def _f16(self):
        return CONV_MODE == 'f16x3' and self.ksize == 2      # ReLU bits, BatchNorm sums from conv2: the f16-split 2x2 kernels'

    # ------------------------------------------------------------------ the two convolutions of a block, by kernel size
    # 2x2: conv1 (pad 1) takes extent (H, W) at grid offset (1, 1) to (H+1, W+1) at offset 0, conv2 (pad 0) takes it back; a
    # data gradient goes the way of the other convolution's forward: _extent[second] is the launch's (out_shift, vh, vw).
    # 3x3: "same" convolutions, one geometry for all.
    _extent = (lambda geo: (0, geo.H + 1, geo.W + 1), lambda geo: (geo.P + 1, geo.H, geo.W))

    def _conv(self, geo, x, f, out, off=None, stats=None):
        """forward of the convolution f (_Filter) from the activation x into `out` (_Act: its ReLU rides in the epilogue and
        leaves out.mask).  off: `out` is shared with other blocks and channels [off, off + f.N) of it are stored; None: the
        block's own buffer, stored at its whole channel stride.  stats: the float64 buffer for BatchNorm's per-workgroup sums.
        The 3x3 kernels have no mask, sums or thin form (the callers' capability conditions leave them None there)."""
        n_store, out_off = (out.cs, 0) if off is None else (f.N, off)
        if self.ksize == 3:
            assert out.mask is None and stats is None and f.master is None, (f, out.mask, stats)
            conv3(geo, x.t, x.cs, f.K, f.packed, f.bias, f.N, out.t, out.cs, out.relu, n_store=n_store, out_off=out_off)
            return
        conv(geo, x.t, x.cs, f.K, f.packed, f.bias, f.N, out.t, out.cs, *self._extent[f.second](geo), out.relu,
             n_store=n_store, out_off=out_off, bn_partial=stats, mask_out=out.mask, w_master=f.master, variant=f.var)

    def _dgrad(self, geo, g, f, dx, x):
        """data gradient of the convolution f (f.packed: its dgrad form) from the gradient g of its output into dx (_Slice,
        both at offset 0).  x: the activation the convolution read; the ReLU behind it, if any, is applied in the epilogue: by
        x itself or, in the f16 split, by the bits the launch that wrote x left -- that launch and this one have the same
        (B, H, W), N, out_shift and a buffer of channel stride x.cs of their own, so they run the same kernel and epilogue
        orientation and agree on the private word layout."""
        relu = {}
        if x.relu:
            relu = {'mask_in': x.mask} if x.mask is not None and self._f16() else {'ref': x.t, 'cs_ref': x.cs}
        if self.ksize == 3:
            conv3(geo, g.t, g.cs, f.N, f.packed, None, f.K, dx.t, dx.cs, False, **relu)
            return
        conv(geo, g.t, g.cs, f.N, f.packed, None, f.K, dx.t, dx.cs, *self._extent[not f.second](geo), False, **relu)

    def _wgrad(self, geo, f, x, g, into, side=False):
        """weight + bias gradient of the convolution f from its input x and the gradient g of its output, accumulated into
        the pair `into` = (gw, gb)"""
        ws = _Workspace.get(x.t.device).wgrad_ws(geo, f.K, f.N, side=side)
        if self.ksize == 3:
            wgrad3(geo, x.t, x.cs, f.K, g.t, g.cs, f.N, *into, f.var, ws)
        else:
            wgrad(geo, x.t, x.cs, f.K, g.t, g.cs, f.N, geo.P + 1 if f.second else 0, *into, f.var, ws, side=side)

    # ------------------------------------------------------------------ forward
    def _bn_fwd(self, tape, spec, z, rec):
        """(scale, shift, smean, sinv) of a block's BatchNorm.  Train mode: the batch statistics of z (conv2's output) --
        from the sums conv2's epilogue left (f16 split) or a pass over z -- which also move the running statistics (unless
        tape.running is False: NULL running pointers, the statistics and coefficients alone, no counter tracked); eval
        mode: the running statistics' coefficients, and under a tape (rec: the block's record) the statistics themselves.
        z None: the eval coefficients alone, for the fold into conv2 (smean, sinv: None)."""
        geo, p, pre, C, sp = tape.geo, tape.p, spec.prefix, spec.cout, _lib.stream_ptr
        coef = torch.empty((2 if z is None else 4) * C, dtype=torch.float32, device=tape.device)
        scale, shift = coef[:C], coef[C:2 * C]
        smean, sinv = (None, None) if z is None else (coef[2 * C:3 * C], coef[3 * C:])
        g, bt, rm, rv = (p[f'{pre}.3.{k}'] for k in ('weight', 'bias', 'running_mean', 'running_var'))
        if tape.train:
            partial = _Workspace.get(tape.device).partial
            moved = (rm, rv) if tape.running else (None, None)
            if self._f16():
                nblk = int(_lib.load().mmlf_conv2x2_blocks(C, C, geo.B, geo.H, geo.W))
                call('mmlf_bn_stats_finalize', ptr(partial), nblk, C, ptr(g), ptr(bt), ptr(moved[0]), ptr(moved[1]),
                     self.momentum, self.eps, ptr(smean), ptr(sinv), ptr(scale), ptr(shift), geo.B, geo.H, geo.W, sp())
            else:
                call('mmlf_bn_stats_train', ptr(z), cs_of(C), C, ptr(g), ptr(bt), ptr(moved[0]), ptr(moved[1]), self.momentum,
                     self.eps, ptr(smean), ptr(sinv), ptr(scale), ptr(shift), ptr(partial), BN_BLOCKS, geo.B, geo.H, geo.W, sp())
            if tape.running:
                tape.tracked.append(p[f'{pre}.3.num_batches_tracked'])
        else:
            call('mmlf_bn_coeffs_eval', ptr(g), ptr(bt), ptr(rm), ptr(rv), self.eps, ptr(scale), ptr(shift), C, sp())
            if rec is not None:
                # eval-mode BatchNorm under autograd (reference train/cli.py:227-230, --train_eval_mode): the
                # statistics are constants, so backward is dz = g * gamma * invstd with the RUNNING statistics
                smean.copy_(rm)
                sinv.copy_(torch.rsqrt(rv.double() + self.eps).float())
                rec.eval = True
        if rec is not None:
            rec.scale, rec.shift, rec.smean, rec.sinv = scale, shift, smean, sinv
        return scale, shift, smean, sinv

    def _block_fwd(self, tape, site, x, dest=None):
        """One block: conv1 (pad 1) -> ReLU -> conv2 (pad 0), then BatchNorm -> ReLU (bn True), ReLU (bn False) or nothing (the
        head).  conv1's ReLU always rides in its epilogue; conv2's does where conv2 is the block's last operation: a block
        without BatchNorm, or one whose eval-mode BatchNorm is folded into conv2 (tape.fold: inference, and the saving forward
        of a frozen net).  x: the input (_Act; extent H,W at (1,1)).  A live block of tape.plan leaves its record in tape.recs.
        dest (a stream's last block): the slice of the concat buffer the output goes to; with tape.deferred the BatchNorm-apply
        + ReLU pass into it is NOT launched but left to Trunk.forward's one pass for all four streams.  Returns the output."""
        geo, p, dev, spec, var = tape.geo, tape.p, tape.device, site.spec, site.var
        C, cs_mid, pre = spec.cout, cs_of(spec.cout), spec.prefix
        w1, b1, w2, b2 = p[f'{pre}.0.weight'], p[f'{pre}.0.bias'], p[f'{pre}.2.weight'], p[f'{pre}.2.bias']
        save = tape.plan is not None and tape.plan.of(site) is not None
        f16 = self._f16()
        thin = C <= THIN_MAX_N and spec.cin >= THIN_MIN_K and self.ksize == 2     # the head: matrix-vector kernels, y is tiny
        bits = save and f16 and not thin
        folded = spec.bn is True and tape.fold                     # BatchNorm folded into conv2
        relu2 = spec.bn is False or folded                         # conv2 is the block's last operation: it writes the output
        fused_stats = spec.bn is True and tape.train and f16       # BatchNorm's statistics from conv2's epilogue
        new_out = spec.bn is not None and dest is None             # the block output is a buffer of its own
        pk1 = None if thin else self._packed(tape, f'{pre}.0.weight', var, False)
        if spec.bn is False:      # (these blocks pack conv2's filter ahead of conv1's launch)
            pk2 = self._packed(tape, f'{pre}.2.weight', var, False)
        got = geo.bufs([cs_mid] * ((1 if relu2 else 2) + (1 if new_out else 0)), dev)   # one zeroing launch for all
        z = None if relu2 else got[1]
        off = None if dest is None else dest.off                   # (None: a buffer of the block's own, stored at its whole stride)
        if new_out:
            dest = _Slice(got[-1], cs_mid, 0)
        ymask = geo.relu_mask(dev) if bits else None
        # the mask of the block's output is read by the data gradient of the NEXT block's first convolution (_block_bwd):
        # a slice of the concat buffer has no such consumer (mmlf_relu_bwd_slice reads the activations)
        omask = geo.relu_mask(dev) if bits and relu2 and new_out else None
        y = _Act(got[0], cs_mid, True, ymask)
        self._conv(geo, x, _Filter(False, spec.cin, C, var, pk1, b1, w1 if thin else None), y)   # (thin: from the master filter)
        if folded:
            # BatchNorm(eval) is a per-channel affine map -> fold it into conv2 and fuse the ReLU
            scale, shift, _, _ = self._bn_fwd(tape, spec, None, None)
            w2f, b2f = torch.empty_like(w2), torch.empty_like(b2)
            call('mmlf_fold_bn_eval3x3' if self.ksize == 3 else 'mmlf_fold_bn_eval', ptr(w2), ptr(b2), ptr(scale), ptr(shift),
                 ptr(w2f), ptr(b2f), C, C, _lib.stream_ptr())
            pk2, b2 = self._pack(w2f, var, False), b2f
        elif spec.bn is not False:
            pk2 = self._packed(tape, f'{pre}.2.weight', var, False)
        rec = None
        if save:
            rec = tape.recs[site.index] = _Rec(site, x, y, z)
            if folded:
                # backward is the ReLU-only block's, through the FOLDED filter (the weights are frozen: no gradient of theirs)
                rec.bn, rec.pk2d = False, self._pack(w2f, var, True)
        conv2 = _Filter(True, C, C, var, pk2, b2)
        if relu2:
            out = _Act(dest.t, dest.cs, True, omask)
            self._conv(geo, y, conv2, out, off)
            return out
        self._conv(geo, y, conv2, _Act(z, cs_mid, False, None), stats=_Workspace.get(dev).partial if fused_stats else None)
        if spec.bn is None:
            return _Act(z, cs_mid, False, None)
        scale, shift, _, _ = self._bn_fwd(tape, spec, z, rec)
        if tape.deferred is not None and off is not None:
            tape.deferred.append((z, scale, shift))
        else:
            call('mmlf_bn_apply_relu', ptr(z), cs_mid, C, ptr(scale), ptr(shift), ptr(dest.t), dest.cs, dest.off,
                 dest.cs if new_out else C, geo.B, geo.H, geo.W, ptr(dest.t.absmax), _lib.stream_ptr())
        return _Act(dest.t, dest.cs, False, None)

    def forward(self, p, stacks, train, save, packed=None, input_grads=None, frozen=False, trainable=None,
                update_running=True, packs=None):
        """stacks: four (B, views, 3, H, W) contiguous float32 device tensors.  They, the grid tensors of `packed` and every
        entry of `p` the blocks read are validated here (_lib.check), ahead of the first call into the library.
        packed (instead of stacks): (Geometry, [four grid tensors of channel stride cs_of(3 views), with their amax arrays]) --
        inputs some other kernel already wrote in the grid layout (the Ensamble's mmlf_shift_pack).
        input_grads (with save): four bools, the streams whose input gradient backward will be asked for -- their first
        filters' data-gradient forms join the step's one packing launch (backward packs them itself otherwise).
        frozen (with save): backward will be called with grads=None (no parameter wants a gradient).  In eval mode a 2x2 trunk
        with BatchNorm then runs the inference launches (BatchNorm folded into conv2) and keeps what a model_no_batchnorm
        forward keeps: the same output bits as without a tape, and a backward without any BatchNorm launch.
        trainable (with save): the parameter names whose gradient backward will be asked for (None: all; frozen=True means
        the empty set).  Together with input_grads it makes the step's plan (Trunk.plan): blocks that are not live leave no
        record and write no ReLU bits, the concat buffer is kept only for a live stream, and only the planned data gradients'
        filter forms are packed.  BatchNorm's running statistics move in train mode whatever is frozen, as in torch.
        update_running (train mode): False leaves every BatchNorm buffer -- running statistics and counters -- untouched; the
        batch statistics and the coefficients are formed as ever (a later micro-batch of a train step: device 0's buffers
        persist under nn.DataParallel).  Eval mode reads the running statistics whatever it says.
        packs: the `packs` of an earlier pass's tape, used instead of packing the filters again.  The caller vouches that
        nothing has changed since that pass: the weights, the plan (train, trainable, input_grads, frozen), the thread and the
        stream (_Workspace.packed_filters: the store behind the views is overwritten by the next packing launch).
        Returns (output NCHW (B,oc,H,W), tape or None)."""
        cin0 = self.views * 3
        if packed is not None:
            geo, xs_in = packed
            B, H, W = geo.B, geo.H, geo.W
            dev = xs_in[0].device
            if geo.ksize != self.ksize or len(xs_in) != 4:
                raise ValueError(f'Trunk.forward: packed= needs four grid tensors of a ksize {self.ksize} geometry')
            for k, t in enumerate(xs_in):
                check(t, f'packed[{k}]', dev, min_numel=geo.alloc * cs_of(cin0))
        else:
            shape = tuple(getattr(stacks[0], 'shape', ()))
            if len(stacks) != 4 or len(shape) != 5 or shape[1:3] != (self.views, 3):
                raise ValueError(f'Trunk.forward: four (B, {self.views}, 3, H, W) stacks required, the first has shape {shape}')
            B, _, _, H, W = shape
            dev = stacks[0].device
            for name, t in zip('hvid', stacks):
                check(t, f'{name}_views', dev, shape=shape)
        self.check_params(p, dev)
        if packed is None:
            geo = Geometry(B, H, W, self.ksize)
        _Workspace.get(dev).enter_stream()
        # BatchNorm folded into conv2: inference, and the frozen evaluation that is differentiated in its inputs (3x3 trunks
        # have no ReLU-only backward and keep the unfolded form under a tape)
        plan = self.plan(() if frozen else trainable, input_grads, train) if save else None
        fold = self.batchnorm and not train and (not save or plan.fold)
        tape = _Tape(geo, dev, p, train, fold, plan, self._prepack(p, dev, plan, fold) if packs is None else packs,
                     len(self.sites), bool(update_running))
        cs_in, cs_cat = cs_of(cin0), 4 * self.chs
        if packed is not None:
            tape.concat, xs = geo.buf(cs_cat, dev), list(xs_in)
        else:
            tape.concat, *xs = geo.bufs([cs_cat] + [cs_in] * 3, dev)
            xs.append(geo.buf(cs_in, dev))
        # the four streams' last BatchNorm-apply passes write quarter rows of the concat buffer: one pass for all four
        # (whole rows) when they are real passes (not folded into conv2)
        if self.batchnorm and not fold:
            tape.deferred = []
        for site in self.sites:
            s = site.chain
            if site.k == 0 and s < 4:
                x = _Act(xs[s], cs_in, False, None)
                if packed is None:
                    call('mmlf_pack_nchw', ptr(stacks[s]), cin0, ptr(x.t), cs_in, B, H, W, ptr(x.t.absmax), _lib.stream_ptr())
            elif site.k == 0:
                if tape.deferred:
                    arr = lambda k: (ctypes.c_void_p * 4)(*[ptr(d[k]) for d in tape.deferred])
                    call('mmlf_bn_apply_relu4', arr(0), cs_of(self.chs), self.chs, arr(1), arr(2), ptr(tape.concat), cs_cat,
                         B, H, W, ptr(tape.concat.absmax), _lib.stream_ptr())
                tape.deferred = None
                # (no trailing ReLU: mmlf_relu_bwd_slice applies the concat buffer's per stream in backward)
                x = _Act(tape.concat, cs_cat, False, None)
            x = self._block_fwd(tape, site, x, _Slice(tape.concat, cs_cat, s * self.chs) if site.last and s < 4 else None)
        if tape.tracked:
            # the shared stream nets' counters appear twice: two forwards per pass, as in the reference
            # (feed_forward.py:222-235 calls in_net_hv for h and v) -- one entry per tensor with its count, since a
            # multi-tensor launch must not hold the same tensor twice
            counts = {}
            for t in tape.tracked:
                counts.setdefault(t.data_ptr(), [t, 0])[1] += 1
            torch._foreach_add_([t for t, _ in counts.values()], [n for _, n in counts.values()])
        out = torch.empty((B, self.oc, H, W), dtype=torch.float32, device=dev)
        call('mmlf_unpack_nchw', ptr(x.t), x.cs, ptr(out), self.oc, B, H, W, _lib.stream_ptr())
        if not (save and any(plan.slices)):
            tape.concat = None               # (kept for mmlf_relu_bwd_slice alone)
        return out, (tape if save else None)

    # ------------------------------------------------------------------ backward
    def _bn_bwd(self, tape, rec, bp, grads, g, dz):
        """BatchNorm's part of a block's backward, as bp lists it: the batch sums with dgamma / dbeta (mmlf_bn_bwd_reduce), the
        coefficients of dz, and dz itself, the gradient behind BatchNorm, written to the grid buffer `dz` (mmlf_bn_bwd_apply).
        g: the gradient of the block's output.  Returns (dz as a _Slice or None, the coefficients: held by the caller)."""
        geo, p, pre, C = tape.geo, tape.p, rec.spec.prefix, rec.spec.cout
        cs_mid, sp, ws = cs_of(C), _lib.stream_ptr, _Workspace.get(tape.device)
        g3w, g3b = (grads[f'{pre}.{k}'] if k in bp.want else None for k in ('3.weight', '3.bias'))
        coef = None
        if bp.reduce:
            coef = torch.empty(3 * C, dtype=torch.float32, device=tape.device)
            # an unwanted dgamma / dbeta goes to scratch: the batch sums still feed the coefficients (or the other of the two)
            dgb = ws.scratch('bn_dgamma_dbeta', 2 * C) if g3w is None or g3b is None else None
            dgamma, dbeta = (dgb[:C] if g3w is None else g3w), (dgb[C:2 * C] if g3b is None else g3b)
            acc = int(g3w is not None or g3b is not None)
            call('mmlf_bn_bwd_reduce', ptr(g.t), g.cs, g.off, ptr(rec.z), cs_mid, C, ptr(rec.scale), ptr(rec.shift),
                 ptr(p[f'{pre}.3.weight']), ptr(rec.smean), ptr(rec.sinv), ptr(dgamma), ptr(dbeta), acc, ptr(coef),
                 ptr(ws.partial), BN_BLOCKS, geo.B, geo.H, geo.W, sp())
            if rec.eval and bp.apply:
                coef[C:].zero_()        # no batch-statistics terms: dz = k1 * g (dgamma / dbeta sums are the same)
        elif bp.apply:
            # running statistics and nobody reads dgamma / dbeta: dz = k1 * g with k1 = gamma * invstd, formed as
            # mmlf_bn_bwd_reduce forms it (the float64 product of gamma and the saved float32 invstd, rounded once), so that
            # a frozen block hands down the bits the full backward does
            assert rec.eval, (pre, bp)
            coef = torch.zeros(3 * C, dtype=torch.float32, device=tape.device)
            coef[:C].copy_((p[f'{pre}.3.weight'].double() * rec.sinv.double()).float())
        if not bp.apply:
            return None, coef
        call('mmlf_bn_bwd_apply', ptr(g.t), g.cs, g.off, ptr(rec.z), cs_mid, C, ptr(rec.scale), ptr(rec.shift),
             ptr(rec.smean), ptr(coef), ptr(dz), cs_mid, geo.B, geo.H, geo.W, ptr(dz.absmax), sp())
        return _Slice(dz, cs_mid, 0), coef

    def _block_bwd(self, tape, rec, bp, grads, g, side=None):
        """g: the gradient w.r.t. the block output (_Slice; extent (H,W)).  Returns the gradient w.r.t. the block input
        (_Slice) or None.  bp: the block's BlockPlan -- the launches that run, and nothing else decides one; grads holds the
        tensors of bp.want.  The unwanted partner of a wanted tensor goes nowhere (gw / gb = NULL).  side (an out_net block):
        the pass's _SideWgrad, settled once this block's BatchNorm-backward kernels are enqueued; a wide block's first weight
        gradient goes to it behind the data gradient.  None (a stream block): all on the main stream, nothing is settled."""
        if rec is None:
            raise ValueError(f'Trunk.backward: the forward pass kept no record of {bp.prefix} (its trainable= / '
                             'input_grads= did not ask for what this backward needs)')
        spec, var, x, y, geo = rec.spec, rec.var, rec.x, rec.y, tape.geo
        C, cs_mid, pre = spec.cout, cs_of(spec.cout), spec.prefix
        assert not bp.want or rec.pk2d is None, 'a frozen forward (BatchNorm folded) has no parameter gradients'
        assert bool(rec.bn) or not (bp.reduce or bp.apply), (pre, bp)
        need_dx = bp.dgrad1
        gw1, gb1, gw2, gb2 = (grads[f'{pre}.{k}'] if k in bp.want else None for k in ('0.weight', '0.bias', '2.weight', '2.bias'))
        conv1, conv2 = _Filter(False, spec.cin, C, var), _Filter(True, C, C, var)
        # this block's gradient buffers, one zeroing launch: dz (behind BatchNorm), dy, dx
        css = ([cs_mid] if bp.apply else []) + ([cs_mid] if bp.dgrad2 else []) + ([x.cs] if need_dx else [])
        got = geo.bufs(css, tape.device) if css else []
        dy = _Slice(got[1 if bp.apply else 0], cs_mid, 0) if bp.dgrad2 else None
        dx = _Slice(got[-1], x.cs, 0) if need_dx else None
        if rec.bn:         # (False where a frozen evaluation folded BatchNorm into conv2: ReLU-only backward)
            dz, coef = self._bn_bwd(tape, rec, bp, grads, g, got[0] if bp.apply else None)   # (coef: held until the return)
        else:
            assert g.off == 0 and g.cs == cs_mid
            dz = g
        if side is not None:
            side.settle()
        # conv2: weight / bias gradient, then data gradient fused with the ReLU of y
        if bp.wgrad2:
            self._wgrad(geo, conv2, y, dz, (gw2, gb2))
        if bp.dgrad2:
            pk2d = rec.pk2d if rec.pk2d is not None else self._packed(tape, f'{pre}.2.weight', var, True)
            self._dgrad(geo, dz, conv2._replace(packed=pk2d), dy, y)
        del dz, got
        # conv1: the same, with the ReLU (if any) of the block underneath: x is then the output of a block without BatchNorm,
        # and what comes out is already the gradient behind that block's trailing ReLU (its dz) at no pass of its own
        overlap = side is not None and side.takes(spec.cin) and need_dx and bp.wgrad1
        if bp.wgrad1 and not overlap:
            self._wgrad(geo, conv1, x, dy, (gw1, gb1))
        if need_dx:
            self._dgrad(geo, dy, conv1._replace(packed=self._packed(tape, f'{pre}.0.weight', var, True)), dx, x)
        if overlap:
            side.launch(pre, (x.t, dy.t), lambda: self._wgrad(geo, conv1, x, dy, (gw1, gb1), side=True))
        elif side is not None:
            side.kept = None                         # (no launch of this block's: the last launch's tensors go, see launch())
        return dx

    def backward(self, p, tape, grad_output, grads, on_done=None, input_grads=None, packed_grads=False):
        """grad_output: (B,oc,H,W) NCHW.  grads: dict name -> tensor, ACCUMULATED into
        (the caller zeroes them), or None: no parameter gradient is formed (no weight-gradient launch at all; required
        for a tape of forward(frozen=True)).  The dict holds the names the forward pass was given as trainable= (all of
        _grad_names by default; a name of that set that is missing is an error, other names are not looked at).  The launches
        are those of Trunk.plan for these names and input_grads.  on_done(key) is called exactly once per key, in the order
        'out_net.k' ..., 'in_net_id', 'in_net_hv', when every gradient of the key has been enqueued -- for a key whose blocks
        launch nothing, as soon as nothing more can come for it (gradient-bucket all-reduce hook).
        input_grads: four bools (streams H, V, I, D), the view stacks whose gradient is wanted; default none.  Returns a list
        of four entries: the (B, views, 3, H, W) float32 gradient of a wanted stack, None for the others.  The parameter
        gradients do not depend on it: the same weight-gradient launches in the same order.  The tape is used up: a block's
        record is released as soon as its launches are enqueued, the concat buffer at the end.
        packed_grads (the mirror of forward's packed=): a wanted stack's entry is (grid tensor, cs) instead -- the data
        gradient of the stream's first convolution as the kernel wrote it, extent (H, W) at (1, 1), 3 views channels of
        channel stride cs -- and no mmlf_unpack_nchw runs (the Ensamble's mmlf_ese_unshift_sum reads that layout)."""
        geo, dev = tape.geo, tape.device
        check(grad_output, 'grad_output', dev, shape=(geo.B, self.oc, geo.H, geo.W), contiguous=False)
        fplan = tape.plan
        if grads is not None:
            wanted = self._grad_names if fplan is None else [n for n in self._grad_names if n in fplan.trainable]
            self._check_dict('grads', grads, wanted, dev)
        ws = _Workspace.get(dev)
        ws.enter_stream()
        B, H, W = geo.B, geo.H, geo.W
        g = _Slice(geo.buf(cs_of(self.oc), dev), cs_of(self.oc), 0)
        call('mmlf_pack_nchw', ptr(grad_output.contiguous()), self.oc, ptr(g.t), g.cs, B, H, W, ptr(g.t.absmax),
             _lib.stream_ptr())
        want = [bool(w) for w in input_grads] if input_grads is not None else [False] * 4
        assert len(want) == 4
        # this pass's plan: the forward's wanted names (none with grads=None) and the stacks asked for HERE; it may ask for
        # less than the forward recorded for, never for more
        bplan = self.plan(fplan.trainable if grads is not None else (), want, fplan.train, fplan.fold)
        tape.p = p
        side =_SideWgrad(ws, on_done, OVERLAP_WGRAD and self.ksize == 2)
        dstacks = [None] * 4
        for site in reversed(self.sites):
            rec, tape.recs[site.index] = tape.recs[site.index], None
            bp, s = bplan.of(site), site.chain
            if s == 4:
                if bp is None:
                    # the block and everything beneath it launch nothing: its key is complete as soon as the block above is
                    g = None
                    side.settle()
                else:
                    g = self._block_bwd(tape, rec, bp, grads, g, side)
                side.done(site.spec.prefix)
                continue
            if site.last:
                # g is the gradient w.r.t. the concat buffer (cs = 4*chs); a stream reads its channel slice
                if s == 2:
                    side.settle()            # (out_net.0's weight gradient ran beside the D stream's BatchNorm kernels)
                gs = None if g is None else _Slice(g.t, g.cs, s * self.chs)
                if bplan.slices[s]:
                    if tape.concat is None:
                        raise ValueError('Trunk.backward: the forward pass kept no concat buffer for this backward')
                    # the stream's last ReLU wrote its slice of the concat buffer: the gradient behind it, as a compact tensor
                    gs = _Slice(geo.buf(cs_of(self.chs), dev), cs_of(self.chs), 0)
                    relu_bwd_slice(geo, g.t, g.cs, s * self.chs, tape.concat, g.cs, s * self.chs, self.chs, gs.t, gs.cs)
            if bp is not None:               # (live blocks sit on top of a chain: nothing beneath a block without a plan runs)
                gs = self._block_bwd(tape, rec, bp, grads, gs)
            if site.k == 0:
                if want[s] and packed_grads:
                    assert gs.off == 0
                    dstacks[s] = (gs.t, gs.cs)
                elif want[s]:
                    # gs: the gradient of the stream's packed input, extent (H, W) at (1, 1), 3 views channels of gs.cs
                    dstacks[s] = torch.empty((B, self.views, 3, H, W), dtype=torch.float32, device=dev)
                    call('mmlf_unpack_nchw', ptr(gs.t), gs.cs, ptr(dstacks[s]), 3 * self.views, B, H, W, _lib.stream_ptr())
                if s in (2, 0):              # shared stream nets: complete after the I (resp. H) stream
                    side.done('in_net_id' if s == 2 else 'in_net_hv')
        tape.concat = None
        return dstacks
