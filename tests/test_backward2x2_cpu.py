"""The 2x2 backward tests without a GPU: the float64 references tests/test_gpu_backward2x2.py holds the kernels against are
nn.Conv2d(k=2) and its gradients, and that file's shape lists reach every kernel path they exist for."""
import ctypes

import pytest
import torch
import torch.nn.functional as F


@pytest.mark.parametrize('variant', [0, 1, 2])
@pytest.mark.parametrize('pad', [0, 1])
def test_grid_float64_references_of_the_2x2_kernels_match_torch_conv2d(pad, variant):
    """tests_helpers.conv4_ref / dgrad4_ref / wgrad4_ref (per-tap matmuls on the grid layout, both placements) are
    nn.Conv2d(k=2, padding=pad) on the stream's transformed image, and its data, weight and bias gradients"""
    from tests_helpers import conv4_ref, dgrad4_ref, filter4, unfilter4, wgrad4_ref

    def stock(x, w, b):          # feed_forward.py _torch_trunk: the H / I streams run on the transposed (and flipped) image
        if variant == 0:
            return F.conv2d(x, w, b, padding=pad)
        if variant == 1:
            return F.conv2d(x.transpose(2, 3), w, b, padding=pad).transpose(2, 3)
        return F.conv2d(x.transpose(2, 3).flip(-1), w, b, padding=pad).flip(-1).transpose(2, 3)

    gen = torch.Generator().manual_seed(7 + 3 * pad + variant)
    B, K, N, H, W = 2, 5, 6, 4, 7
    ih, iw, ioff = (H, W, 1) if pad else (H + 1, W + 1, 0)          # the input's extent and grid offset
    oh, ow, ooff = (H + 1, W + 1, 0) if pad else (H, W, 1)          # the output's
    x = torch.randn((B, K, ih, iw), generator=gen, dtype=torch.float64, requires_grad=True)
    w = torch.randn((N, K, 2, 2), generator=gen, dtype=torch.float64, requires_grad=True)
    b = torch.randn((N,), generator=gen, dtype=torch.float64, requires_grad=True)
    g = torch.randn((B, N, oh, ow), generator=gen, dtype=torch.float64)
    z = stock(x, w, b)
    assert z.shape == g.shape
    z.backward(g)

    def grid(t, h, w_, off):                                       # NCHW -> the (B, H + 2, W + 2, C) grid view
        out = torch.zeros((B, H + 2, W + 2, t.shape[1]), dtype=torch.float64)
        out[:, off:off + h, off:off + w_] = t.detach().permute(0, 2, 3, 1)
        return out

    xg, gg = grid(x, ih, iw, ioff), grid(g, oh, ow, ooff)
    wv = filter4(w.detach(), variant)
    torch.testing.assert_close(conv4_ref(xg, wv, b.detach(), pad), z.detach().permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(dgrad4_ref(gg, wv, pad), x.grad.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    gw, gb = wgrad4_ref(xg, gg, pad)
    torch.testing.assert_close(unfilter4(gw, variant), w.grad, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(gb, b.grad, rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------ the GPU shapes hit what they exist for
# csrc/wgrad.hip wgrad_nsplit / wgrad16_cfg and csrc/common.h pick_nt, transcribed: the library exposes the layout only through
# the workspace size and the audit (both pinned below)
def _nsplit(nslice):
    return max(8, 512 // nslice // 8 * 8)


def _split_cfg(cin, cout, nchunks, cus=256):
    """(mb, nb, nslice, nsplit) of the split-arithmetic weight gradient; nchunks < 0: the layout the workspace is sized by"""
    nb = 2 if cout <= 32 else 5 if cout <= 80 else 8 if cout <= 128 else 18
    if nb == 18:
        mb, nslice = 3, (cin + 1 + 47) // 48
        one, three = cus // nslice, (768 // nslice + 7) // 8 * 8
        nsplit = max(8, max(one, three) if nchunks < 0 else three if nchunks >= 42 * 1024 else one)
    else:
        mb = 5 if nb <= 5 and 32 < cin + 1 <= 80 else 2
        if nb == 8 and cin + 1 >= 128:
            mb = 3
        nslice = -(-(cin + 1) // (16 * mb))
        nsplit = _nsplit(nslice)
    return mb, nb, nslice, nsplit


def _f32_cfg(cin, cout):
    """(nt, nslice, nsplit) of the exact-f32 weight gradient"""
    n = (cout + 31) // 32
    nt = 1 if n <= 1 else 3 if n <= 3 else 4 if n <= 4 else 9
    nslice = (cin + 1 + 31) // 32
    return nt, nslice, _nsplit(nslice)


def _partial_floats(cin, cout):
    nt, nslice, nsplit = _f32_cfg(cin, cout)
    mb, nb, ns16, nsp16 = _split_cfg(cin, cout, -1)
    return (max(nsplit * 4 * nslice * 32 * nt * 32, nsp16 * 4 * ns16 * 16 * mb * 16 * nb) + 3) // 4 * 4


def test_backward2x2_gpu_shapes_cover_the_kernel_edges():
    """tests/test_gpu_backward2x2.py's lists must reach: every (mb, nb) layout of the split weight gradient and every pick_nt
    class of the exact-f32 one; in each of them a frame with three or more chunks per split and a ragged last split (the
    prefetch and the two stages of the chunk loop) and one with empty splits; both split counts of the wide kernel; the
    thin kernel; pitches on both sides of 127 | 128 (sixteen-wave kernel) and 383 | 384 (one-window | two-segment); a frame of one
    row and one of one column; a tile of pure padding.  The transcription above is pinned to the library through
    mmlf_wgrad_workspace_floats and mmlf_audit_wgrad_h2."""
    import test_gpu_backward2x2 as t
    from mmlf_amd import _lib
    L = _lib.load()
    pw, tile = L.mmlf_grid_pad_w(), 256

    def grid(B, H, W):
        NQpad = L.mmlf_relu_mask_words(B, H, W) // 4096 * tile
        return W + pw, B * (H + L.mmlf_grid_pad_h()) * (W + pw), NQpad

    thin = [(ci, co) for ci, co in t.PAIRS if co <= 2 and ci >= 64]
    pairs = [p for p in t.PAIRS if p not in thin]
    assert sorted(thin) == [(70, 2), (280, 1), (280, 2)]
    assert {_split_cfg(ci, co, 0)[:2] for ci, co in pairs} == {(2, 2), (5, 2), (2, 5), (5, 5), (2, 8), (3, 8), (3, 18)}
    assert {_f32_cfg(ci, co)[0] for ci, co in pairs} == {1, 3, 4, 9}
    assert (1, 1) in pairs
    wide = [(ci, co) for ci, co in pairs if _split_cfg(ci, co, 0)[1] == 18]
    assert any(co % 16 and co + 16 <= 288 for _, co in wide), 'a 16-column block partly and one wholly past Cout'
    assert set(t.STREAM_PAIRS) <= set(pairs) and set(t.FULL_PAIRS) <= set(pairs)

    # the transcription is the library's: workspace size (the larger layout), and the audited workspace end of every launch
    for ci, co in pairs:
        assert L.mmlf_wgrad_workspace_floats(ci, co, 1, 1, 1) == _partial_floats(ci, co) + 2 * (grid(1, 1, 1)[2] // 32) + 4, (ci, co)
        for B, H, W in t.GEOMS + t.GUARD_GEOMS + [t.BS64, t.BS160, t.BS512]:
            P, NQ, NQpad = grid(B, H, W)
            e = (ctypes.c_int64 * 7)()
            assert L.mmlf_audit_wgrad_h2((ci + 7) // 8 * 8, ci, (co + 7) // 8 * 8, co, 0, B, H, W, e) == 0, _lib.last_error()
            assert e[4] != -4, (ci, co, B, H, W)
            assert e[4] == (_partial_floats(ci, co) + 2 * (NQpad // 32) + 2) * 4

    # chunks per split in every layout of either kernel family, over the sweep's frames
    for ci, co in pairs:
        for nsplit in (_split_cfg(ci, co, 0)[3], _f32_cfg(ci, co)[2]):
            deep = empty = False
            for B, H, W in t.GEOMS:
                nchunks = grid(B, H, W)[2] // 32
                per = -(-nchunks // nsplit)
                deep |= per >= 3 and nchunks % per != 0
                empty |= -(-nchunks // per) < nsplit
            assert deep and empty, (ci, co, nsplit)
    # both split counts of the wide kernel
    counts = {(B, H, W): _split_cfg(280, 280, grid(B, H, W)[2] // 32)[3] for B, H, W in (t.BS64, t.BS160, t.BS512)}
    assert counts[t.BS64] == 42 and counts[t.BS160] == 128 and counts[t.BS512] == 128, counts
    assert grid(*t.BS160)[2] // 32 >= 42 * 1024 > grid(*t.BS64)[2] // 32

    pitches = {grid(*g)[0] for g in t.GEOMS}
    assert {127, 128, 383, 384} <= pitches and max(pitches) > 384 and min(pitches) < 127
    gp = [grid(*g)[0] for g in t.GUARD_GEOMS]
    assert any(p <= 127 for p in gp) and any(127 < p <= 383 for p in gp) and any(p > 383 for p in gp)
    assert any(H == 1 and W > 1 for _, H, W in t.GEOMS) and any(W == 1 and H > 1 for _, H, W in t.GEOMS)
    assert (1, 1, 1) in t.GEOMS
    assert any(grid(*g)[2] - grid(*g)[1] >= tile and g[0] > 1 for g in t.GEOMS)
    # variants: 0, 1 and 2 all occur on the stream pairs, in every mode (the sweep is a full product over MODES)
    seen = {t.variant_of(p, g, pad) for p in t.STREAM_PAIRS for g in t.GEOMS for pad in (0, 1)}
    assert seen == {0, 1, 2}
    # the sampled patches of the bs = 512 test: the rule in its body picks one per 64
    assert t.BS512[0] == 512 and {(c[0], c[1]) for c in t.BS512_CASES} == {(280, 280), (70, 70)}
