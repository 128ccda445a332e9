"""The BatchNorm / layout tests without a GPU: the float64 references tests/test_gpu_elementwise.py holds the kernels against
are nn.BatchNorm2d + nn.ReLU and their gradients, the grid <-> NCHW helpers invert each other, and that file's shape lists
reach every kernel path they exist for."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests_helpers import bn_apply_ref, bn_bwd_ref, bn_stats_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _grid(t, fill=float('nan')):
    """NCHW -> the (B, H + 2, W + 2, C) grid view; the border holds `fill` (the references must not use it)"""
    B, C, H, W = t.shape
    out = torch.full((B, H + 2, W + 2, C), fill, dtype=t.dtype)
    out[:, 1:H + 1, 1:W + 1] = t.detach().permute(0, 2, 3, 1)
    return out


@pytest.mark.parametrize('shape', [(2, 5, 4, 7), (1, 3, 1, 1), (1, 2, 1, 2), (3, 70, 2, 3)])
def test_grid_float64_references_of_batchnorm_match_torch(shape):
    """tests_helpers.bn_stats_ref / bn_apply_ref / bn_bwd_ref against F.batch_norm + relu under autograd, float64, to 1e-12:
    training statistics, running update, train and eval output, dz, dgamma, dbeta"""
    B, C, H, W = shape
    gen = torch.Generator().manual_seed(B + C + H + W)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    z = (rnd(B, C, H, W) * (0.5 + torch.rand(C, generator=gen, dtype=torch.float64)).view(1, C, 1, 1)
         + rnd(C).view(1, C, 1, 1)).requires_grad_()
    gamma, beta = (0.5 + torch.rand(C, generator=gen, dtype=torch.float64)).requires_grad_(), rnd(C).requires_grad_()
    rm0, rv0 = rnd(C), 0.5 + torch.rand(C, generator=gen, dtype=torch.float64)
    mom, eps = 0.1, 1e-5
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12)
    n = B * H * W
    mean, invstd, scale, shift, rm, rv = bn_stats_ref(_grid(z), gamma.detach(), beta.detach(), rm0, rv0, mom, eps)
    if n == 1:          # torch refuses one value per channel in training mode: the header's kernel gives var = 0
        close(mean, z.detach().reshape(C))
        close(invstd, torch.full((C,), eps ** -0.5, dtype=torch.float64))
        close(rm, 0.9 * rm0 + 0.1 * mean)
        close(rv, 0.9 * rv0)
        return
    trm, trv = rm0.clone(), rv0.clone()
    y = F.relu(F.batch_norm(z, trm, trv, gamma, beta, True, mom, eps))
    gy = rnd(B, C, H, W)
    y.backward(gy)
    close(rm, trm)
    close(rv, trv)
    zd = z.detach()
    close(mean, zd.mean((0, 2, 3)))
    close(invstd, 1 / (zd.var((0, 2, 3), unbiased=False) + eps).sqrt())
    u, absu = bn_apply_ref(_grid(z), scale, shift)
    close(u.clamp_min(0)[:, 1:H + 1, 1:W + 1], y.detach().permute(0, 2, 3, 1))
    assert bool((absu[:, 1:H + 1, 1:W + 1] >= u[:, 1:H + 1, 1:W + 1].abs() * (1 - 1e-15)).all())
    r = bn_bwd_ref(_grid(z), _grid(gy), scale, shift, gamma.detach(), mean, invstd)
    assert torch.equal(r.mask, (y.detach() > 0).permute(0, 2, 3, 1))
    close(r.dz, z.grad.permute(0, 2, 3, 1))
    close(r.dgamma, gamma.grad)
    close(r.dbeta, beta.grad)
    assert bool((r.dz_abs >= r.dz.abs() * (1 - 1e-15)).all()) and bool((r.sum_abs_g >= r.dbeta.abs() * (1 - 1e-15)).all())
    assert bool((r.sum_abs_gz >= r.dgamma.abs() * (1 - 1e-15)).all())
    # eval mode: coefficients from the running statistics
    esc = gamma.detach() / (rv0 + eps).sqrt()
    ue, _ = bn_apply_ref(_grid(z), esc, beta.detach() - rm0 * esc)
    close(ue.clamp_min(0)[:, 1:H + 1, 1:W + 1],
          F.relu(F.batch_norm(zd, rm0, rv0, gamma.detach(), beta.detach(), False, mom, eps)).permute(0, 2, 3, 1))
    # without affine parameters and running statistics
    st = bn_stats_ref(_grid(z), None, None, None, None, mom, eps)
    close(st[2], invstd)
    close(st[3], -mean * invstd)
    assert st[4] is None and st[5] is None


@pytest.mark.parametrize('offset', [0, 1])
def test_grid_from_nchw_and_nchw_from_grid_invert_each_other(offset):
    from mmlf_amd import engine
    from test_gpu_kernels import grid_from_nchw, nchw_from_grid
    B, C, H, W, cs = 2, 5, 3, 4, 8
    geo = engine.Geometry(B, H, W)
    h, w = (H, W) if offset else (H + 1, W + 1)
    x = np.random.RandomState(offset).normal(size=(B, C, h, w)).astype(np.float32)
    buf = grid_from_nchw(x, cs, geo, offset=offset)
    assert buf.shape == (geo.alloc * cs,)
    back, g = nchw_from_grid(buf, cs, C, geo, h, w, offset)
    np.testing.assert_array_equal(back, x)
    assert g.shape == (B, geo.R, geo.P, cs)
    assert np.count_nonzero(buf) == np.count_nonzero(x) and not buf[geo.NQ * cs:].any() and not g[..., C:].any()
    assert g[1, offset + 1, offset + 2, 3] == x[1, 3, 1, 2]
    again = grid_from_nchw(back, cs, geo, offset=offset)
    np.testing.assert_array_equal(again, buf)


# ------------------------------------------------------------------ the GPU shapes hit what they exist for
# the walk and the tile sizes come from the kernels' own functions (csrc/row_walk.h), listed by tools/row_walk.hip
@pytest.fixture(scope='module')
def lister(tmp_path_factory):
    """tools/row_walk.hip, compiled for the host: (walk(cvn, limits), sizes(n)), both cached"""
    from mmlf_amd.csrc import build
    if not os.path.exists(build.HIPCC):
        pytest.skip('no hipcc')
    exe = str(tmp_path_factory.mktemp('row_walk') / 'row_walk')
    subprocess.run([build.HIPCC, '--offload-arch=gfx950', '-I', build.HERE, os.path.join(ROOT, 'tools', 'row_walk.hip'), '-o', exe],
                   check=True, capture_output=True, text=True, timeout=300)

    @functools.lru_cache(maxsize=None)
    def run(*args):
        return json.loads(subprocess.run([exe, *map(str, args)], check=True, capture_output=True, text=True, timeout=60).stdout)

    def walk(cvn, limits):
        """(cvn, dx, dc), {limit: row}: per row the 256 threads' [pairs visited, carries, left through the carry], the hits
        of every (x, cg) and the visits outside the row"""
        out = run('walk', cvn, *limits)
        assert [r['limit'] for r in out['rows']] == list(limits) and all(len(r['threads']) == 256 for r in out['rows'])
        return tuple(out['walk']), {r['limit']: r for r in out['rows']}

    return walk, lambda n: run('sizes', n)


def _covers_once(walk, cvn, limits):
    """the walk reaches every (position, group) of a row exactly once and nothing else"""
    for P, row in walk(cvn, tuple(limits))[1].items():
        assert len(row['hits']) == P * cvn and set(row['hits']) == {1} and row['outside'] == 0, (cvn, P)


def _aligned16(cs, c_off):
    """every group of four of a channel slice starts on 16 bytes (the buffer does); otherwise on 8"""
    assert cs % 2 == 0 and c_off % 2 == 0
    return cs % 4 == 0 and c_off % 4 == 0


def test_gpu_shape_lists_reach_every_class(lister):
    import test_gpu_elementwise as t
    from mmlf_amd import engine
    walk, sizes = lister
    rows_walk = lambda c_store: walk(sizes(c_store)['groups'], ())[0]      # bn_rows_kernel: (cvn, dx, dc) at a store width
    ppi_of = lambda C: tuple(sizes(C)['reduce'])
    pack_xt, unpack_xt = (lambda cs: sizes(cs)['pack_xt']), (lambda C: sizes(C)['unpack_xt'])
    # the lists hold what they were given
    assert set(t.FRAMES) >= {(1, 1, 1), (1, 1, 37), (2, 29, 1), (3, 5, 29), (3, 10, 14), (2, 10, 125), (2, 10, 126), (2, 10, 127),
                             (2, 3, 30), (2, 3, 31), (2, 3, 300), (1, 2, 514)}
    assert set(t.LAYOUT_FRAMES) >= set(t.FRAMES) and set(t.SLACK_FRAMES) >= {(1, 1, 1), (2, 29, 1), (2, 3, 300)}
    assert set(t.CHANNELS) >= {(1, 8), (2, 8), (3, 8), (6, 8), (8, 8), (32, 32), (64, 64), (27, 32), (70, 72), (108, 112),
                               (132, 136), (280, 280), (288, 288), (512, 512)}
    assert t.APPLY_ONLY == (516, 520) and t.STATS_LIMIT == (1024, 1024) and t.STATS_LIMIT_FRAME == (1, 2, 3)
    assert set(t.SLICES) >= {(70, 280, 0, 70), (70, 280, 140, 70), (70, 280, 70, 70), (70, 280, 210, 70), (70, 72, 0, 72),
                             (27, 32, 0, 32), (6, 8, 2, 6), (2, 8, 6, 2), (8, 32, 24, 8)}
    assert set(t.APPLY4) >= {(2, 8), (6, 8), (70, 72), (6, 6)}
    assert set(t.NBLOCKS) >= {1, 3, 63, 64, 65, 1024, 4096} and max(t.NBLOCKS) == 4096
    assert set(t.FOLD) >= {(1, 1), (2, 280), (70, 27), (280, 280)} and set(t.COEFFS_C) >= {1, 63, 64, 65, 280}
    assert t.FULL_FRAME == (64, 96, 96) and t.FULL_CH == (70, 72) and t.BN_BLOCKS == engine.BN_BLOCKS
    for C, cs in t.CHANNELS + [t.APPLY_ONLY, t.STATS_LIMIT, t.FULL_CH]:
        assert C <= cs and cs % 4 == 0
    for C, cs_y, c_off, c_store in t.SLICES:
        assert C <= c_store and c_off + c_store <= cs_y

    pitches = [W + 2 for _, _, W in t.FRAMES]
    assert (1, 1, 1) in t.FRAMES                                            # n = 1
    assert any(H == 1 and W > 1 for _, H, W in t.FRAMES) and any(W == 1 and H > 1 for _, H, W in t.FRAMES)

    # ---- bn_rows_kernel: the stores of the apply (C and cs_z, the slices) and of the backward apply (cs_z)
    stores = {c for C, cs in t.CHANNELS + [t.APPLY_ONLY] for c in t._c_stores(C, cs)} | {s[3] for s in t.SLICES}
    walks = {c: rows_walk(c) for c in stores}
    assert any(cvn == 1 for cvn, _, _ in walks.values())                    # cvn = 1
    assert {2, 8, 16} <= {cvn for cvn, _, dc in walks.values() if dc == 0}  # cvn divides 256: no carry ever
    assert walks[70] == (18, 14, 4) and walks[72] == (18, 14, 4)
    assert rows_walk(t.APPLY_ONLY[0])[1] == 1 and rows_walk(t.APPLY_ONLY[1])[1] == 1      # dx = 1
    assert max(cvn for cvn, _, _ in walks.values()) <= 256
    assert any(c % 4 for c in stores) and any(c % 4 == 0 for c in stores)   # the scalar tail store | whole groups only
    assert any(c_store > C for C, cs in t.CHANNELS for c_store in t._c_stores(C, cs))       # pad channels written as zeros
    assert any(s[3] > s[0] for s in t.SLICES)
    assert min(pitches) == 3 and any(dx > 3 for _, dx, _ in walks.values())                 # a pitch shorter than dx
    upitches = tuple(sorted(set(pitches)))
    for c in stores:                                                        # every walk with a carry: taken in mid-row, and
        cvn, dx, dc = walks[c]                                              # taken as the way out of the row
        if dc == 0:
            continue
        ev = [e for row in walk(cvn, upitches)[1].values() for e in row['threads']]
        assert any(carries and not left for _, carries, left in ev), c
        assert any(left for _, _, left in ev), c
        assert any(seen >= 3 for seen, _, _ in ev), c
    # the kernels' walk reaches every (position, group) of a row exactly once, at every store width and pitch in use
    for c in stores:
        _covers_once(walk, walks[c][0], upitches)
    # mmlf_bn_apply_relu4 walks channel PAIRS: cvn = 2 C
    for C, cs_z in t.APPLY4:
        assert C % 2 == 0 and cs_z % 2 == 0 and 8 * C * 4 <= 48 * 1024
        _covers_once(walk, 2 * C, upitches)
    assert any(cs_z % 4 for _, cs_z in t.APPLY4) and {256 % (2 * C) == 0 for C, _ in t.APPLY4} == {True, False}
    assert {walk(2 * C, ())[0][2] == 0 for C, _ in t.APPLY4} == {True, False}                # the pair walk with and without a carry
    # shift_pack_kernel's write-out walks the pieces of a row, nx = min(xt, P - x0), in groups of four: cvn = cs / 4
    import test_ensamble as te
    for views in te.SHIFT_PACK_VIEWS:
        cs = engine.cs_of(views * 3)
        xt = pack_xt(cs)
        pieces = {min(xt, W + 2 - x0) for _, W in te.SHIFT_PACK_FRAMES for x0 in range(0, W + 2, xt)}
        _covers_once(walk, cs // 4, sorted(pieces))
    assert set(te.SHIFT_PACK_VIEWS) >= {9, 7} and set(te.SHIFT_PACK_FRAMES) >= {(24, 24), (9, 40), (33, 17), (3, 2)}
    assert set(te.SHIFT_PACK_VIEWS) >= {1, 2} and set(te.SHIFT_PACK_FRAMES) >= {(1, 300), (300, 1)}
    # the pieces of every pitch here at xt = 128: a pitch below 128 is one piece, the pitch of 302 is two whole pieces and 46
    sp = tuple(sorted({min(128, W + 2 - x0) for _, W in te.SHIFT_PACK_FRAMES for x0 in range(0, W + 2, 128)}))
    assert walk(8, ())[0] == (8, 32, 0) and pack_xt(32) == 128 and pack_xt(24) == 128 and pack_xt(8) == 128
    assert max(sp) == 128 and 302 % 128 in sp and 3 in sp
    w7, rows7 = walk(6, sp)
    assert w7 == (6, 42, 4) and 4 in rows7                                  # a carry | a pitch below dx: one pair per thread
    assert {seen for seen, _, _ in rows7[4]['threads']} == {0, 1}
    ev = [e for row in rows7.values() for e in row['threads']]
    assert any(carries and not left for _, carries, left in ev) and any(left for _, _, left in ev)

    # ---- VecIO<4>: one 16-byte access or two 8-byte ones
    cls = {s: _aligned16(s[1], s[2]) for s in t.SLICES}
    assert cls[(70, 280, 0, 70)] and cls[(70, 280, 140, 70)] and not cls[(70, 280, 70, 70)] and not cls[(70, 280, 210, 70)]
    assert not cls[(6, 8, 2, 6)] and not cls[(2, 8, 6, 2)] and cls[(8, 32, 24, 8)]
    assert set(t.SLICE_FRAMES) <= set(t.FRAMES) and (1, 1, 1) in t.SLICE_FRAMES and len(t.SLICE_FRAMES) >= 3

    # ---- bn_reduce_body: positions per iteration against the row, blocks against the rows
    ppis = {C: ppi_of(C) for C, _ in t.CHANNELS}
    assert ppis[1] == (1, 256) and ppis[512] == (128, 2) and ppi_of(t.STATS_LIMIT[0]) == (256, 1)
    assert ppi_of(513)[0] > 128 and ppi_of(1025)[0] > 256                       # what the wrappers refuse
    assert any(256 % cvn for cvn, _ in ppis.values()) and any(256 % cvn == 0 for cvn, _ in ppis.values())    # idle threads
    widths = [W for _, _, W in t.FRAMES]
    for C, (cvn, ppi) in ppis.items():
        assert any(W >= 2 * ppi for W in widths), C                          # the x loop takes a further step
        assert ppi == 1 or (any(W < ppi for W in widths) and any(W % ppi and W > ppi for W in widths)), C   # idle | ragged
    rows = t.NBLOCKS_FRAME[0] * t.NBLOCKS_FRAME[1]
    assert all(nb < rows for nb in (1, 3, 63, 64, 65)) and all(nb > rows for nb in (1024, 4096))
    assert rows % 3 == 0 and rows % 65 and rows % 64 and rows // 3 >= 3     # whole strides | a ragged last stride
    assert all(B * H < t.BN_BLOCKS for B, H, _ in t.FRAMES)                 # blocks without a row, everywhere else ...
    assert t.FULL_FRAME[0] * t.FULL_FRAME[1] > t.BN_BLOCKS and (t.FULL_FRAME[0] * t.FULL_FRAME[1]) % t.BN_BLOCKS == 0
    # ... and the finalize kernels' 64 lanes over the partials: fewer, as many, one more, many times as many
    assert {nb < 64 for nb in t.NBLOCKS} == {True, False} and {63, 64, 65} <= set(t.NBLOCKS)
    assert any(nb % 64 == 0 and nb >= 1024 for nb in t.NBLOCKS)
    assert {C for C, _ in t.NBLOCKS_CH} == {6, 70}

    # ---- pack: the tile walks the PITCH; unpack: the tile walks W
    lp = [W + 2 for _, _, W in t.LAYOUT_FRAMES]
    lw = [W for _, _, W in t.LAYOUT_FRAMES]
    xts = {cs: pack_xt(cs) for _, cs in t.CHANNELS}
    assert set(xts.values()) == {128, 64, 32, 16, 8} and xts[280] == 16 and xts[8] == 128
    assert pack_xt(1024) == 4 and 1024 * 5 * 4 <= 64 * 1024
    for xt in set(xts.values()):
        assert any(P < xt for P in lp) and any(P % xt == 0 for P in lp) and any(P % xt == 1 and P > xt for P in lp), xt
        assert any(1 < P % xt < xt for P in lp if P > xt), xt
    assert {127, 128, 129, 32, 33} <= set(lp)
    uxt = {C: unpack_xt(C) for C, _ in t.CHANNELS}
    assert set(uxt.values()) == {32, 16, 8}
    for xt in set(uxt.values()):
        assert any(W < xt for W in lw) and any(W % xt == 0 and W >= xt for W in lw) and any(W % xt and W > xt for W in lw), xt
