"""Nets wider than 288 channels (model_chs up to 128 with 2x2 filters: column blocks in the convolution and weight-gradient
entry points), the part that needs no GPU: which constructor flags take the native trunk, the size queries
(unchanged up to 288 columns, blocked above), the audited extents of every wide launch against what the ABI tells a caller to
allocate (after tests/test_bounds_audit.py), and the compiler's resource figures of the instantiations a wide training step
launches (after tests/test_kernel_resources.py).

Replaces nothing in the reference; the kernels replace nn.Conv2d forward / backward (reference
mmlf/model/feed_forward.py:123-125) at --model_chs above 72."""
import ctypes

import pytest

from conftest import TINY_KW
from mmlf_amd import _lib

FRAMES = [(1, 1, 1), (3, 1, 1), (1, 3, 5), (3, 3, 5), (1, 9, 7), (3, 9, 7), (1, 5, 130), (3, 5, 130), (1, 2, 400), (3, 2, 400)]
WIDE_LAYERS = [(8, 296), (296, 296), (384, 384), (512, 512), (512, 108), (112, 512)]
CONV = dict(IN=0, PACKED=1, BIAS=2, OUT=3, REF=4, IN_AMAX=5, OUT_AMAX=6, BN_PARTIAL=7, MASK=8)
WG = dict(IN=0, G=1, GW=2, GB=3, WORKSPACE=4, IN_AMAX=5, G_AMAX=6)
PARTIAL_BYTES = (2 * 512 * 1024 + 8) * 8          # engine._Workspace.partial (tests/test_bounds_audit.py holds the engine to it)


def cs_of(c):
    return (c + 7) // 8 * 8


def lib():
    return _lib.load()


# ------------------------------------------------------------------ which nets run on the kernels
@pytest.mark.parametrize('head', [{}, {'model_uncert': True}, {'model_discrete': True}], ids=['base', 'upr', 'dpp'])
@pytest.mark.parametrize('nobn', [False, True])
def test_native_predicate_admits_2x2_nets_up_to_512_channels(head, nobn):
    from mmlf_amd.feed_forward import FeedForward
    kw = dict(TINY_KW, model_no_batchnorm=nobn, **head)
    for chs in (74, 96, 128):
        m = FeedForward(**dict(kw, model_chs=chs))
        assert m._native_ok and m._trunk is not None, chs
        assert m._trunk.chs == chs and m._trunk.batchnorm == (not nobn)
    assert not FeedForward(**dict(kw, model_chs=130))._native_ok
    assert not FeedForward(**dict(kw, model_chs=96, model_ksize=3, model_no_batchnorm=False))._native_ok
    assert FeedForward(**dict(kw, model_chs=72, model_ksize=3, model_no_batchnorm=False))._native_ok      # (as before)


def test_trunk_refuses_what_the_kernels_do_not_take():
    from mmlf_amd.engine import Trunk
    Trunk(128, 2, 3, 9, 1, 0.1, ksize=2)
    with pytest.raises(ValueError, match='max 288'):
        Trunk(96, 2, 3, 9, 1, 0.1, ksize=3)
    with pytest.raises(ValueError, match='max 512'):
        Trunk(130, 2, 3, 9, 1, 0.1, ksize=2)


# ------------------------------------------------------------------ size queries
def _np_one_launch(N):
    """packed columns of the split kernels up to 288 output channels, as before the column blocks"""
    return 32 if N <= 32 else 80 if N <= 80 else (N + 15) // 16 * 16 if N <= 128 else 288


def _nt(N):
    n = (N + 31) // 32
    return 1 if n <= 1 else 3 if n <= 3 else 4 if n <= 4 else 9


def _wgrad_partial_one_launch(Cin, Cout):
    """partial sums of the largest weight-gradient layout of a layer of at most 288 output channels, as before"""
    def nsplit(nslice):
        return max(8, 512 // nslice // 8 * 8)
    nslice = (Cin + 1 + 31) // 32
    n = nsplit(nslice) * 4 * (nslice * 32) * (_nt(Cout) * 32)
    nb = 2 if Cout <= 32 else 5 if Cout <= 80 else 8 if Cout <= 128 else 18
    if nb == 18:
        mb, ns = 3, (Cin + 1 + 47) // 48
        split = max(8, 256 // ns, (768 // ns + 7) // 8 * 8)
    else:
        mb = 5 if (nb <= 5 and 32 < Cin + 1 <= 80) else 2
        if nb == 8 and Cin + 1 >= 128:
            mb = 3
        ns = (Cin + 1 + 16 * mb - 1) // (16 * mb)
        split = nsplit(ns)
    return (max(n, split * 4 * (ns * 16 * mb) * (16 * nb)) + 3) // 4 * 4


# forward and data-gradient (K, N) of the BASE and DPP nets' layers
NET_PAIRS = [(27, 70), (70, 70), (280, 280), (280, 1), (1, 1), (280, 108), (108, 108), (70, 27), (108, 280)]


@pytest.mark.parametrize('K,N', NET_PAIRS)
def test_size_queries_up_to_288_columns_are_unchanged(K, N):
    L = lib()
    np_, nchunk = _np_one_launch(N), (K + 7) // 8
    assert L.mmlf_packed_filter_h2_columns(N) == np_
    assert L.mmlf_packed_filter_h2_bytes(K, N) == nchunk * 8 * np_ * 16 + 4 * np_
    assert L.mmlf_packed_filter_split_bytes(K, N) == nchunk * 12 * np_ * 16
    assert L.mmlf_packed_filter_floats(K, N) == nchunk * 4 * 2 * (_nt(N) * 32) * 4
    for B, H, W in ((1, 1, 1), (3, 9, 7), (64, 96, 96)):
        nqpad = L.mmlf_relu_mask_words(B, H, W) // 4096 * 256
        assert nqpad % 512 == 0
        assert L.mmlf_wgrad_workspace_floats(K, N, B, H, W) == _wgrad_partial_one_launch(K, N) + 2 * (nqpad // 32) + 4


def test_size_queries_of_the_column_blocks():
    """two blocks of 160, 192 or 256 packed columns: never more than an eighth of the packed columns wasted at the widths of
    model_chs 80, 96, 112, 128, and never fewer columns than channels; each block a packed filter of its own"""
    L = lib()
    for N, np_ in ((289, 320), (296, 320), (320, 320), (321, 384), (384, 384), (385, 512), (448, 512), (512, 512)):
        assert L.mmlf_packed_filter_h2_columns(N) == np_
        for K in (8, 296, 512):
            nchunk = (K + 7) // 8
            blk = np_ // 2
            assert L.mmlf_packed_filter_h2_bytes(K, N) == 2 * (nchunk * 8 * blk * 16 + 4 * blk)
            assert L.mmlf_packed_filter_split_bytes(K, N) == 2 * nchunk * 12 * blk * 16
            assert L.mmlf_packed_filter_floats(K, N) == 2 * nchunk * 4 * 2 * blk * 4
    for N in (320, 384, 448, 512):
        assert 8 * (L.mmlf_packed_filter_h2_columns(N) - N) <= L.mmlf_packed_filter_h2_columns(N)
    for N in (513, 600):
        assert L.mmlf_packed_filter_h2_columns(N) == -1 and L.mmlf_packed_filter_h2_bytes(8, N) == -1
        assert L.mmlf_packed_filter_split_bytes(8, N) == -1 and L.mmlf_packed_filter_floats(8, N) == -1
    assert L.mmlf_packed_filter3x3_floats(8, 296) == -1               # 3x3 filters stay within one launch
    assert L.mmlf_wgrad_workspace_floats(8, 513, 1, 1, 1) == -1
    # a wide gradient tensor: the larger of its two column blocks' partial sums (they run one after the other)
    for Cin, Cout in ((296, 296), (512, 512), (8, 512)):
        want = max(_wgrad_partial_one_launch(Cin, 288), _wgrad_partial_one_launch(Cin, Cout - 288))
        assert L.mmlf_wgrad_workspace_floats(Cin, Cout, 1, 1, 1) == want + 2 * (512 // 32) + 4


# ------------------------------------------------------------------ audited extents
@pytest.mark.parametrize('B,H,W', FRAMES)
def test_wide_conv_launch_extents_fit_the_allocations_the_abi_prescribes(B, H, W):
    L = lib()
    P = W + L.mmlf_grid_pad_w()
    alloc = L.mmlf_grid_alloc_positions(B, H, W)
    amax = L.mmlf_amax_entries(B, H, W) * 4
    mask = L.mmlf_relu_mask_words(B, H, W) * 4
    wide = 0
    for cin, cout in WIDE_LAYERS:
        for dgrad in (False, True):
            K, N = (cout, cin) if dgrad else (cin, cout)
            cs_in, cs_out = cs_of(K), cs_of(N)
            wide += N > 288
            assert L.mmlf_packed_filter_h2_columns(N) > 0
            nblk = L.mmlf_conv2x2_blocks(K, N, B, H, W)
            assert nblk > 0
            for out_shift in (0, P + 1):
                for n_store, c_off in ((cs_out, 0), (N, 0), (N, cs_out - N)):       # whole rows / exact channels / a channel slice
                    e = (ctypes.c_int64 * 9)()
                    assert L.mmlf_audit_conv_h2(cs_in, K, N, cs_out, n_store, out_shift, cs_out, B, H, W, e) == 0, _lib.last_error()
                    tag = f'{K}->{N} B={B} {H}x{W} shift={out_shift} n_store={n_store}'
                    assert 0 < e[CONV['IN']] <= alloc * cs_in * 4, tag
                    assert e[CONV['PACKED']] == L.mmlf_packed_filter_h2_bytes(cs_in, N), tag
                    assert e[CONV['BIAS']] == N * 4, tag
                    assert 0 < e[CONV['OUT']] <= alloc * cs_out * 4 - c_off * 4, tag
                    assert 0 < e[CONV['REF']] <= alloc * cs_out * 4, tag
                    assert e[CONV['IN_AMAX']] <= amax and e[CONV['OUT_AMAX']] <= amax, tag
                    assert e[CONV['BN_PARTIAL']] == nblk * 2 * N * 8 <= PARTIAL_BYTES, tag
                    assert e[CONV['MASK']] == mask, tag
    assert wide == 9


@pytest.mark.parametrize('B,H,W', FRAMES)
def test_wide_weight_gradient_launch_extents_fit_the_allocations_the_abi_prescribes(B, H, W):
    L = lib()
    P = W + L.mmlf_grid_pad_w()
    alloc = L.mmlf_grid_alloc_positions(B, H, W)
    amax = L.mmlf_amax_entries(B, H, W) * 4
    for pair in WIDE_LAYERS:
        for cin, cout in (pair, pair[::-1]):
            cs_in, cs_g = cs_of(cin), cs_of(cout)
            ws = L.mmlf_wgrad_workspace_floats(cin, cout, B, H, W) * 4
            assert ws > 0
            for g_shift in (0, P + 1):
                e = (ctypes.c_int64 * 7)()
                assert L.mmlf_audit_wgrad_h2(cs_in, cin, cs_g, cout, g_shift, B, H, W, e) == 0, _lib.last_error()
                tag = f'{cin}->{cout} B={B} {H}x{W} g_shift={g_shift}'
                assert 0 < e[WG['IN']] <= alloc * cs_in * 4, tag
                assert 0 < e[WG['G']] <= alloc * cs_g * 4, tag
                assert e[WG['GW']] == cout * cin * 16 and e[WG['GB']] == cout * 4, tag
                assert 0 < e[WG['WORKSPACE']] <= ws, tag
                assert e[WG['IN_AMAX']] <= amax and e[WG['G_AMAX']] <= amax, tag


def test_the_extent_check_of_the_engine_covers_wide_geometries():
    """engine.Geometry sizes its overflow guard by the widest layer the entry points take.  A wide gradient tensor runs on the
    instantiations the narrower layers pin (tests/test_kernel_resources.py): the 288-column kernel on its first 288 channels,
    whatever a layer of that width takes on the rest -- a pair the side-stream register budget was not drawn up for, so
    Trunk.backward keeps it on the main stream."""
    from mmlf_amd import engine
    assert engine.MAX_WIDTH == {2: 512, 3: 288} and engine.MAX_OC == 288
    assert engine.MAX_OVERLAP_WIDTH == 288          # wide nets' weight gradients stay on the main stream


# ------------------------------------------------------------------ resources, from the compiler
@pytest.fixture(scope='module')
def usage():
    import os
    import test_kernel_resources as tkr
    if not os.path.exists(tkr.HIPCC):
        pytest.skip('no hipcc')
    return tkr._resource_usage()


# (G, planes, epilogue kind, waves, transposed) of a wide net's f16-split training step: per column block G = 10 (model_chs 74
# - 80), 12 (- 96) or 16 (- 128): plain and mask-in data gradients, ReLU and ReLU + mask-out forward launches (transposed),
# the statistics launch of a BatchNorm block and the data gradient under a reference tensor (the other orientation)
WIDE_CONV_KINDS = [(g, 2, kind, 8, tr) for g in (10, 12, 16) for kind, tr in ((0, True), (1, True), (17, True), (4, True),
                                                                               (2, False), (8, False))]


@pytest.mark.parametrize('args', WIDE_CONV_KINDS)
def test_wide_conv_launch_kinds_of_a_training_step_do_not_spill(usage, args):
    from test_kernel_resources import _demangled
    vgprs, agprs, scratch, waves = _demangled(usage, 'conv4tap_x6s_kernel', args)
    assert scratch == 0, (args, vgprs, scratch)
    assert waves >= 2 and vgprs <= 256, (args, vgprs, waves)         # __launch_bounds__(512, 2): one 512-thread workgroup per CU


def test_wide_exact_f32_column_blocks_do_not_spill(usage):
    from test_kernel_resources import _demangled
    for nt in (5, 6, 8):
        v = _demangled(usage, 'conv4tap_kernel', (nt,))
        assert v[2] == 0 and v[3] >= 2, (nt, v)


# ------------------------------------------------------------------ the wide nets' float64 reference (tests/test_gpu_wide_nets.py)
# model_chs 74 (4 x 74 = 296: the narrowest width above one launch; column blocks of 160), 96 (384: blocks of 192) and 128 (512:
# blocks of 256): two stream blocks, three merge blocks, UPR head unless told otherwise, bs = 3; 9 x 7 and 5 x 130 (pitch > 127)
WIDE_CHS = [74, 96, 128]
WIDE_FRAMES = [(9, 7), (5, 130)]
WIDE_SEED = 24                # (of the weights; at seeds 24 and 25 the float32 stock run sits within a tenth of every bar below)
OUT_BAR, LOSS_BAR, GRAD_WORST, GRAD_MEDIAN = 1e-4, 1e-4, 6e-2, 4e-2     # tests/test_gpu_nobn.py::test_70_channel_net_against_float64


def wide_kw(chs, bn, **head):
    return dict(TINY_KW, model_chs=chs, model_in_blocks=2, model_out_blocks=3, model_no_batchnorm=not bn,
                **(head or {'model_uncert': True}))


def wide_state(kw, seed=WIDE_SEED):
    """variance-preserving filters without BatchNorm (tests/test_nobn_cpu.py gained_state), synth.synth_state with it"""
    from mmlf_amd import synth
    from test_nobn_cpu import gained_state
    return gained_state(kw, seed) if kw['model_no_batchnorm'] else synth.synth_state(synth.param_spec(**kw), seed=seed)


def wide_model(kw, state, dev='cpu', dtype=None):
    import numpy as np
    import torch
    from mmlf_amd.feed_forward import FeedForward
    m = FeedForward(**kw)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    m = m.to(dev)
    return m.to(dtype) if dtype is not None else m


def wide_variant(kw):
    return 'upr' if kw['model_uncert'] else 'dpp' if kw['model_discrete'] else 'base'


def wide_run(m, kw, H, W, dev, dtype, B=3):
    """one training-mode forward + loss + backward: (outputs, loss, parameter gradients) as float64 CPU tensors"""
    import torch
    from mmlf_amd import loss, synth
    from test_nobn_cpu import loss_of
    stacks, gt, mask = synth.synth_inputs(B, H, seed=11, ps_w=W)
    m_mask = (torch.from_numpy(mask).int() * loss.create_mask_margin(mask.shape, 2)).to(dev)
    m.train()
    out = m(*[torch.from_numpy(s).to(dev, dtype) for s in stacks])
    lv = loss_of(wide_variant(kw), out, torch.from_numpy(gt).to(dev, dtype), m_mask)
    lv.backward()
    # what is compared element by element: the regression outputs; of the DPP head the softmax (its mean is an arg-max)
    keys = {'upr': ['mean', 'logvar'], 'base': ['mean'], 'dpp': ['posterior']}[wide_variant(kw)]
    return ({k: out[k].detach().double().cpu() for k in keys}, float(lv.detach()),
            {n: p.grad.double().cpu() for n, p in m.named_parameters()})


def grad_rels(got, ref):
    """relative L2 error per tensor with the absolute floor of tests/test_gpu_nobn.py::test_70_channel_net_against_float64"""
    return {n: float((got[n] - ref[n]).norm()) / (float(ref[n].norm()) + 1e-6 * ref[n].numel() ** 0.5 / 3e-2) for n in ref}


def compare_runs(tag, got, ref, out_bar, loss_bar, worst_bar, median_bar):
    import numpy as np
    (o1, l1, g1), (o0, l0, g0) = got, ref
    for k in o0:
        err = float((o1[k] - o0[k]).abs().max())
        print(f'{tag} {k}: max |error| {err:.3e} (bar {out_bar:g})')
        assert err <= out_bar, (tag, k, err)
    assert abs(l1 - l0) <= loss_bar * abs(l0), (tag, l1, l0)
    rels = grad_rels(g1, g0)
    worst = max(rels, key=rels.get)
    med = float(np.median(list(rels.values())))
    print(f'{tag}: gradient relative L2 per tensor: median {med:.3e}, worst {worst} {rels[worst]:.3e}')
    assert rels[worst] <= worst_bar and med <= median_bar, (tag, worst, rels[worst], med)


_WIDE_REF = {}


def wide_reference(chs, bn, H, W, **head):
    """(kw, state, float64 run) of one net and frame on the CPU's stock path, computed once and shared by the modes; the
    float32 stock run is first held to a TENTH of every bar: what the GPU tests then measure is the kernels, not the seed"""
    import torch
    key = (chs, bn, H, W, tuple(sorted(head.items())))
    if key not in _WIDE_REF:
        kw = wide_kw(chs, bn, **head)
        state = wide_state(kw)
        runs = {dt: wide_run(wide_model(kw, state, dtype=dt), kw, H, W, torch.device('cpu'), dt) for dt in (torch.float64, torch.float32)}
        compare_runs(f'float32 stock run, model_chs={chs} bn={bn} {H}x{W} {wide_variant(kw)}', runs[torch.float32], runs[torch.float64],
                     OUT_BAR / 10, LOSS_BAR / 10, GRAD_WORST / 10, GRAD_MEDIAN / 10)
        _WIDE_REF[key] = (kw, state, runs[torch.float64])
    return _WIDE_REF[key]


@pytest.mark.parametrize('H,W', WIDE_FRAMES)
@pytest.mark.parametrize('bn', [True, False], ids=['bn', 'nobn'])
@pytest.mark.parametrize('chs', WIDE_CHS)
def test_wide_net_cases_are_well_conditioned(chs, bn, H, W):
    kw, state, (out, lv, grads) = wide_reference(chs, bn, H, W)
    assert set(out) == {'mean', 'logvar'} and lv == lv
    if not bn:            # (with BatchNorm the bias in front of it has a zero gradient, which the measure's floor covers)
        for n, v in grads.items():          # every tensor stands clear of the measure's absolute floor: the bar is a relative one
            assert float(v.norm()) >= 2 * 1e-6 * v.numel() ** 0.5 / 3e-2, (n, float(v.norm()))
