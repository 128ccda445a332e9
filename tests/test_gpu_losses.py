"""The kernels that close a training step -- loss_partial / loss_finalize / loss_grad (mmlf_loss_fwd_bwd, kinds 0-2), the four
loss_multi_* kernels (mmlf_loss_multi_fwd_bwd, kinds 3-6) and adam_kernel (mmlf_adam_step) of csrc/elementwise.hip -- each
called directly through its C entry point and held, element by element, to the float64 references of tests_helpers
(loss_ref, adam_ref; pinned to autograd of the CPU branches of mmlf_amd/loss.py and to torch.optim.Adam by
tests/test_loss_head_cpu.py, which also holds the shape lists to the classes they exist for).  The conventions are those of
tests/test_gpu_elementwise.py: every output and scratch buffer lies between guard bands and is pre-filled -- NaN where the
launch must write, a sentinel where it must not (the gradient channels a loss does not use, the aux part of the scratch of
kinds 3 and 5 and under aux_override) -- and every element is compared afterwards.

Decisions (|grid_k - gt| < half_step, tot < 0.01f, raw > 0, the sign of out - gt) are float32 expressions in the kernels and
are taken from the same float32 torch expressions in the references; everything after them is float64.

Two legs:
  * exact: small integers, dyadic alphas, logvar = 0 (the exponential is exactly 1), a mask with a power-of-two count and, for
    kinds 4 and 6, aux_override sums that make both factors powers of two: the block partials add up to the exact sums, the
    gradient equals the float64 result, the loss is held to 1 ulp.  Kinds 4 and 6 without aux_override (their factors are
    quotients then) and the cross-entropy kinds (an exponential at every pixel; their exact leg has scores <= 0, a gradient of
    exactly 0) go through the bars below on the same inputs, and the whole-batch sums of the aux pass are exact;
  * real-valued: seeded normal values, scores and logvars within +-6, held to bars that count the float32 roundings on the
    kernel's path times U = 2^-24 of the absolute terms; the derivation stands in _loss_bars / _adam_bars.  The double
    accumulation adds 1e-12 of the sum of absolute terms.

EXPLOG_ULPS = 2 is the accuracy this module ASSUMES of the device expf and logf, in float32 ulps (c = 2 EXPLOG_ULPS units of U
in the bars).  It is an assumption, not a measurement: nothing in this project records it.

Headroom of the first run on an MI355X (largest error / bar per bar; 0 where every comparison was exact):
  kind           0       1       2       3       4       5       6
  gradient       0.7500  0.6539  0.5507  0.7252  0.4380  0.5446  0.4570
  loss           0.4372  0.1518  0.1436  0.2425  0.1272  0.1212  0.1756
  block partials 0.1289  0.1178  0.1333  0.0498  0.0898  0.1333  0.1458
  exact, loss    0.0000  0.0000  -       0.0000  0.4399  -       0.0000      (1 ulp)
  kind 4 aux sum of alpha 0.0708; adam m 0.9943, v 0.7187, p 0.9970, exact p 0.9814.
The bars that hold EXPLOG_ULPS are those of kinds 1, 2, 4, 5 and 6: the worst ratio seen is 0.6539 (kind 1, gradient), so the
assumed 2 ulps were not needed in that run; the Adam bars hold no such constant and are nearly used up, as a bar that counts
every rounding once should be.
"""
import pytest
import torch

from tests_helpers import (ADAM_N, LOSS_FRAMES, LOSS_NBLOCKS, LOSS_NBLOCKS_FRAMES, LOSS_STRIDE_FRAME, RATIOS, Ref, _Pool, _bar,
                           _close, _ints, _pick, _same, _ulp, adam_ref, loss_ref)

pytestmark = pytest.mark.gpu

FRAMES, STRIDE_FRAME, NBLOCKS, NBLOCKS_FRAMES = LOSS_FRAMES, LOSS_STRIDE_FRAME, LOSS_NBLOCKS, LOSS_NBLOCKS_FRAMES
LOSS_BLOCKS = 1024                           # engine.LOSS_BLOCKS: what loss.py always passes
MIN_OC = {0: 1, 1: 2, 2: 1, 3: 1, 4: 2, 5: 1, 6: 2}
OC = {0: [1, 2], 1: [2, 3], 2: [1, 3, 108], 3: [1, 2], 4: [2, 3], 5: [1, 3, 108], 6: [2, 3]}
THIN_OC = {0: 1, 1: 2, 2: 2, 3: 1, 4: 2, 5: 2, 6: 2}             # the stride frame: the thinnest form of each kind
PLANES = {0: [0], 1: [0], 2: [0], 3: [1, 3], 4: [1, 3], 5: [1, 3], 6: [0]}
KINDS = list(range(7))
LEGS = pytest.mark.parametrize('integer', [True, False], ids=['exact', 'real'])

EXPLOG_ULPS = 2.0                            # assumed accuracy of the device expf / logf (see the docstring)
SENT, NAN, JUNK = 1234.5, float('nan'), 777.25
U = 2.0 ** -24
DISP = (-3.5, 3.5)


def _dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module', autouse=True)
def _report_ratios():
    yield
    for k in sorted(RATIOS):
        print(f'\n[loss headroom] {k}: max error / bar = {RATIOS[k]:.4f}', end='')
    print()
    RATIOS.clear()


def _edge_pixels(n, count):
    return [(37 * j) % n for j in range(count)]


def half_step_edge(grid, half_step):
    """(gt, k): a float32 gt whose float32 difference to the centre of bin k equals the float32 half_step exactly (it belongs
    to neither bin)"""
    half = torch.tensor(half_step, dtype=torch.float64).float()
    g = grid.float().cpu()
    for k in range(g.numel()):
        for s in (1.0, -1.0):
            gt = g[k] + s * half
            if bool(torch.abs(g[k] - gt) == half) and not bool((torch.abs(g - gt) < half).any()):
                return float(gt), k
    raise AssertionError('precondition: no float32 value lies exactly half a step from a bin centre')


def make_inputs(kind, frame, oc, P, integer, seed, dev, mask_mode='some', mp_mode='some', surfaceless='some',
                alpha_edge=True):
    """inputs of one loss call, with the constructed edges at pixels 0, 37, 74, ... (mod n):
    kinds 0, 1, 3, 4, 6: out == gt exactly (the L1 gradient is exactly 0); kind 4: a pixel whose total alpha is the float32
    0.01 exactly (it HAS a surface: tot < 0.01f is strict); kinds 2, 5: raw scores negative, exactly 0 and positive at one
    pixel | gt outside every bin | gt exactly half a step from a bin centre."""
    B, H, W = frame
    n, HW = B * H * W, H * W
    gen = torch.Generator(device=dev).manual_seed(seed)
    r = Ref(kind=kind, frame=frame, oc=oc, P=P, integer=integer, n=n, grid=None, half=0.0, mp=None,
            tag=f'kind={kind} B={B} {H}x{W} oc={oc} P={P} {"exact" if integer else "real"}')
    ce = kind in (2, 5)
    if ce:
        r.grid = torch.linspace(DISP[0], DISP[1], oc).to(dev)                     # dl.reg_to_class / dl.mpi_to_weights
        r.half = (DISP[1] - DISP[0]) / oc / 2.0
    if integer:
        out = _ints(-3, 0, (B, oc, H, W), gen) if ce else _ints(-4, 4, (B, oc, H, W), gen)
        if kind in (1, 4, 6):
            out[:, 1] = 0.0
    else:
        out = (2.5 * torch.randn((B, oc, H, W), device=dev, generator=gen)).clamp(-6, 6)
    out = out.contiguous().view(B, oc, HW)

    def disparity(shape):
        if ce:
            return 7.2 * torch.rand(shape, device=dev, generator=gen) - 3.6
        return _ints(-4, 4, shape, gen) if integer else 1.5 * torch.randn(shape, device=dev, generator=gen)

    edges = _edge_pixels(n, 3 if ce else 2)
    if P == 0:
        tgt = disparity((B, HW))
        disp = tgt
    else:
        tgt = torch.full((B, P, 5, HW), JUNK, device=dev)
        if integer:
            tgt[:, :, 3] = _pick((0.25, 0.5, 1.0) if surfaceless == 'none' else (0.0, 0.25, 0.5, 1.0), (B, P, HW), gen)
        else:
            tgt[:, :, 3] = 0.05 + 0.95 * torch.rand((B, P, HW), device=dev, generator=gen)
        if surfaceless != 'none':
            none = torch.rand((B, 1, HW), device=dev, generator=gen) < 0.25
            none.view(-1)[n - 1] = True
            tgt[:, :, 3] = torch.where(none, torch.zeros_like(tgt[:, :, 3]), tgt[:, :, 3])
        tgt[:, :, 4] = disparity((B, P, HW))
        disp = tgt[:, 0, 4]
    # the edges
    b0, p0 = divmod(edges[0], HW)
    if ce:
        for c, v in zip(range(min(3, oc)), (-1.5, 0.0, 2.25)):
            out[b0, c, p0] = v if not integer else min(v, 0.0)
        b1, p1 = divmod(edges[1], HW)
        b2, p2 = divmod(edges[2], HW)
        if P:                                      # every plane outside; then plane 0 alone on the edge
            tgt[b1, :, 4, p1] = 50.0
            tgt[b2, :, 4, p2] = 50.0
        disp[b1, p1] = 50.0
        disp[b2, p2], k_edge = half_step_edge(r.grid, r.half)
        if not integer:                            # a positive score on that bin: a target of 1 there would show
            out[b2, k_edge, p2] = 1.5
    else:
        out[b0, 0, p0] = disp[b0, p0]
        if kind == 4 and alpha_edge:
            b1, p1 = divmod(edges[1], HW)
            tgt[b1, :, 3, p1] = 0.0
            tgt[b1, 0, 3, p1] = torch.tensor(0.01, dtype=torch.float32)
            if integer:                            # |out - gt| = 2: the products with this alpha stay exact
                out[b1, 0, p1] = tgt[b1, 0, 4, p1] + 2.0
    # the mask: a power-of-two count in the exact leg (1 / count is exact), the edge pixels first
    mask = torch.zeros(n, dtype=torch.int32, device=dev)
    if mask_mode == 'some':
        rest = torch.randperm(n, device=dev, generator=gen).tolist() if n < 4096 else None
        if integer or rest is None:
            count = 1 << (max(n // 2, 1).bit_length() - 1)
            if rest is None:                       # a large frame: a random subset, then the edge pixels swapped in
                perm = torch.randperm(n, device=dev, generator=gen)
                mask[perm[:count]] = 1
                spare = [j for j in perm[:2 * len(edges)].tolist() if j not in edges]
                for e in edges:
                    if not int(mask[e]):
                        mask[e], mask[spare.pop()] = 1, 0
            else:
                order = list(dict.fromkeys(edges + rest))
                mask[torch.tensor(order[:count], device=dev)] = 1
        else:
            mask[:] = (torch.rand(n, device=dev, generator=gen) < 0.7).int()
            mask[torch.tensor(edges, device=dev)] = 1
    r.mask = mask.view(B, H, W)
    if kind == 6:
        if mp_mode == 'some':
            r.mp = (torch.rand((B, H, W), device=dev, generator=gen) < 0.6).int()
        else:
            r.mp = torch.full((B, H, W), 1 if mp_mode == 'ones' else 0, dtype=torch.int32, device=dev)
    r.out = out.view(B, oc, H, W)
    r.target = tgt.view(B, H, W) if P == 0 else tgt.view(B, P, 5, H, W)
    return r


def exact_aux(inp):
    """aux_override sums that make the factors of kinds 4 and 6 powers of two: f0 = s0 / n = 2, f1 = n / s1 = 4 |
    f0 = n / s0 = 2, f1 = n / (n - s0) = 2"""
    n = float(inp.n)
    v = [2 * n, n / 4] if inp.kind == 4 else [n / 2, 0.0]
    return torch.tensor(v, dtype=torch.float64, device=inp.out.device)


def reference(inp, den_override=None, aux_override=None):
    return loss_ref(inp.kind, inp.out, inp.target, inp.mask, inp.mp, inp.grid, inp.half, den_override, aux_override)


def _loss_bars(inp, r):
    """(bar of the per-pixel loss (B, H, W), bar of the gradient (B, c, H, W)), U = 2^-24, c = 2 EXPLOG_ULPS (an expf / logf
    result is within EXPLOG_ULPS ulps <= c U relative).  mkd = mask / den; mk = (float)mask * (float)(1 / den) carries ONE
    rounding (the cast of 1 / den), a product with it a second.
    kind 0: l = fabsf(out - gt): U l.  grad = sgn mk: the product is exact: U |grad|.
    kind 1: e = expf(-lv): c U; d: U; e |d|: U -> (c + 2) U e|d|; + lv: U |l|.  grad0 = e sgn mk: (c + 2) U |grad0|;
            grad1 = (1 - e|d|) mk: (c + 2) U e|d| + U |1 - e|d|| for the difference, 2 U relative for mk and the product.
    kinds 2, 5: t_k sums P alphas: (P - 1) U t_k (kind 2: exact); v_k t_k: U (kind 2: exact); dot sums K = oc terms:
            (K - 1) U -> dot within nd U dot, nd = K - 1 | P + K - 1; expf(dot): c U and nd U dot for its argument; z sums K
            expf: (c + K - 1) U; the quotient: U -> (2 c + K + nd dot) U relative, which logf turns absolute, plus its own
            c U |l|.  grad_k = (expf(raw) / z - t_k) mk for raw > 0: p_k within (c + c + K - 1 + 1) U p_k, t_k as above, the
            difference U, mk and the product 2 U; exactly 0 for raw <= 0.
    kind 3: d: U; |d| w: U; P terms: (P - 1) U -> (P + 1) U l.  dm = sum sgn w: (P - 1) U sum w; times mk: 2 U |dm|.
    kind 4: term_k = (e|d_k| + lv) w_k: (c + 2) U e|d_k| w_k + 2 U |term_k|; acc: (P - 1) U sum |term| -> A = (c + 2) sE +
            (P + 1) sT.  f0 = (float)(s0 / n), s0 a double sum of float32 totals ((P - 1) U each): P U; acc / f0: U ->
            A / f0 + (P + 1) |acc| / f0.  l_oor = (-lv oor) f1, f1 = (float)n / (float)s1: 2 U |l_oor|; the sum: U; / 2 exact.
            dm = gm / f0 / 2, gm = sum (e sgn) w: (c + 1 + P - 1) U sum e w, / f0: (P + 1) U -> (c + 2 P + 1) U sum e w / (2 f0);
            dlv = (glv / f0 - oor f1) / 2, glv = sum (1 - e|d|) w: (c + 2) sE + (P + 1) sG, / f0: (P + 1) |glv| / f0,
            oor f1: U, the difference: U; times mk: 2 U more each.
    kind 6: l_in = (e|d| + lv) mp f0, f0 = (float)n / (float)s0 (U) -> ((c + 2) e|d| + 3 |e|d| + lv|) mp f0 U;
            l_oor: 2 U; the sum: U.  dm = e sgn mp f0 / 2: (c + 2) U, times mk: 2 U.  dlv = ((1 - e|d|) mp f0 - oor f1) / 2:
            ((c + 2) e|d| + 3 |1 - e|d||) mp f0 U, oor f1: U, the difference: U; times mk: 2 U."""
    kind, P, K, p = inp.kind, inp.P, inp.oc, r.parts
    c = 2 * EXPLOG_ULPS
    mkd = (inp.mask.double() / r.den_used).unsqueeze(1)
    g, grad = r.g, r.grad.abs()
    if kind == 0:
        return U * r.l.abs(), U * grad
    if kind == 1:
        return U * ((c + 2) * p['ed'] + r.l.abs()), torch.stack(
            [(c + 2) * U * grad[:, 0], ((c + 2) * U * p['ed'] + 3 * U * (1 - p['ed']).abs()) * mkd[:, 0]], 1)
    if kind in (2, 5):
        nd = K - 1 if kind == 2 else P + K - 1
        bl = U * (2 * c + K + nd * p['dot'].abs() + c * r.l.abs())
        bg = U * ((2 * c + K) * p['pk'] + max(P - 1, 0) * p['t'] + 3 * (p['pk'] - p['t']).abs()) * mkd
        return bl, torch.where(inp.out > 0, bg, torch.zeros_like(bg))
    if kind == 3:
        return (P + 1) * U * r.l.abs(), U * ((P - 1) * p['sw'].unsqueeze(1) + 2 * g.abs()) * mkd
    if kind == 4:
        f0 = p['f0']
        A = (c + 2) * p['sE'] + (P + 1) * p['sT']
        bl = U * (A / f0 + (P + 1) * p['acc'].abs() / f0 + 2 * p['l_oor'].abs() + (p['acc'] / f0 + p['l_oor']).abs()) / 2
        b0 = U * ((c + 2 * P + 1) * p['sew'] / (2 * f0) + 2 * g[:, 0].abs())
        of1 = p['oor'] * p['f1']
        b1 = U * (((c + 2) * p['sE'] + (P + 1) * p['sG']) / f0 + (P + 1) * p['glv'].abs() / f0 + of1
                  + (p['glv'] / f0 - of1).abs()) / 2 + 2 * U * g[:, 1].abs()
        return bl, torch.stack([b0, b1], 1) * mkd
    ed, mp, f0, of1 = p['ed'], p['mp'], p['f0'], p['oor'] * p['f1']
    bl = U * (((c + 2) * ed + 3 * p['nll'].abs()) * mp * f0 + 2 * p['l_oor'].abs() + (p['l_in'] + p['l_oor']).abs()) / 2
    b1 = U * (((c + 2) * ed + 3 * (1 - ed).abs()) * mp * f0 + of1 + 2 * g[:, 1].abs()) / 2 + 2 * U * g[:, 1].abs()
    return bl, torch.stack([(c + 4) * U * g[:, 0].abs(), b1], 1) * mkd


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def run_loss(inp, nblocks=LOSS_BLOCKS, den_override=None, aux_override=None, with_grad=True, exact=None):
    """one call, every buffer checked; returns (loss_out, scratch, reference)"""
    from mmlf_amd import _lib
    from mmlf_amd._lib import call, ptr
    kind, oc, (B, H, W), n = inp.kind, inp.oc, inp.frame, inp.n
    dev = inp.out.device
    multi, used = kind >= 3, 1 if kind in (0, 3) else oc if kind in (2, 5) else 2
    if exact is None:
        exact = inp.integer and (kind in (0, 1, 3) or (kind in (4, 6) and aux_override is not None))
    what = (f'mmlf_loss{"_multi" if multi else ""}_fwd_bwd {inp.tag} nblocks={nblocks} den={den_override is not None} '
            f'aux={aux_override is not None} grad={with_grad}')
    key = f'kind {kind}'
    pool = _Pool(dev)
    loss_out = pool.new(1, NAN)
    grad = pool.new(B * oc * H * W, SENT)
    gv = grad.view(B, oc, H, W)
    if with_grad:
        gv[:, :used] = NAN
    nd = int(_lib.load().mmlf_loss_multi_scratch_doubles(nblocks)) if multi else 2 * nblocks + 2
    assert nd == (4 * nblocks + 4 if multi else 2 * nblocks + 2)
    scratch = pool.new(nd, NAN, torch.float64)
    has_aux = kind in (4, 6)
    if multi and not has_aux:
        scratch[2 + 2 * nblocks:] = SENT
    elif has_aux and aux_override is not None:
        scratch[4 + 2 * nblocks:] = SENT
    g_arg = ptr(grad) if with_grad else None
    if multi:
        call('mmlf_loss_multi_fwd_bwd', kind, ptr(inp.out), oc, ptr(inp.target), inp.P, ptr(inp.mask), ptr(inp.mp),
             ptr(inp.grid), float(inp.half), ptr(loss_out), g_arg, ptr(scratch), nblocks, ptr(den_override), ptr(aux_override),
             B, H, W, _lib.stream_ptr())
    else:
        call('mmlf_loss_fwd_bwd', kind, ptr(inp.out), oc, ptr(inp.target), ptr(inp.mask), ptr(inp.grid), float(inp.half),
             ptr(loss_out), g_arg, ptr(scratch), nblocks, ptr(den_override), B, H, W, _lib.stream_ptr())
    r = reference(inp, den_override, aux_override)
    bar_l, bar_g = _loss_bars(inp, r)
    mk = inp.mask.double()
    # the finalize: 1 / den and the count (or den_override)
    assert float(scratch[1]) == float(r.den) and float(scratch[0]) == 1.0 / float(r.den_used), (what, scratch[:2].tolist())
    # every block wrote its partials, and they add up
    part = scratch[2:2 + 2 * nblocks].view(nblocks, 2)
    assert float(part[:, 0].sum()) == float(r.count), (what, 'block counts', float(part[:, 0].sum()), float(r.count))
    assert not bool(torch.isnan(part[:, 0]).any()), (what, 'a block left its count unwritten')
    psum = part[:, 1].sum()
    bar_sum = (mk * bar_l).sum() + 1e-12 * (mk * r.l.abs()).sum()
    if exact:
        assert bool(torch.isfinite(part).all()) and float(psum) == float(r.sum), (what, 'block sums', float(psum), float(r.sum))
        _ulp(loss_out, r.loss.reshape(1), f'{key} exact, loss: 1 ulp', what)
    else:
        assert bool(torch.isfinite(r.sum)) != bool(torch.isnan(part[:, 1]).any()), (what, 'a block sum is NaN / is not')
        _close(psum, r.sum, bar_sum, f'{key} sum of block partials', what)
        _close(loss_out, r.loss.reshape(1), (U * r.loss.abs() + bar_sum / r.den_used).reshape(1), f'{key} loss', what)
    # the whole-batch sums of the aux pass
    if has_aux:
        fin = scratch[2 + 2 * nblocks:4 + 2 * nblocks]
        if aux_override is not None:
            assert torch.equal(fin, aux_override), (what, 'aux sums under aux_override')
        else:
            aux = scratch[4 + 2 * nblocks:].view(nblocks, 2)
            assert bool(torch.isfinite(aux).all()), (what, 'a block left its aux sums unwritten')
            s0, s1 = r.aux[0], r.aux[1] if kind == 4 else torch.zeros((), dtype=torch.float64, device=dev)
            assert float(fin[1]) == float(s1) and float(aux[:, 1].sum()) == float(s1), (what, 'aux count', float(fin[1]))
            if inp.integer or kind == 6:
                assert float(fin[0]) == float(s0) and float(aux[:, 0].sum()) == float(s0), (what, 'aux sum', float(fin[0]))
            else:            # float32 totals of P alphas, then double
                _close(fin[0], s0, (max(inp.P - 1, 0) * U + 1e-12) * s0, 'kind 4 aux sum of alpha', what)
    if multi and (not has_aux or aux_override is not None):
        assert bool((scratch[(4 if has_aux else 2) + 2 * nblocks:] == SENT).all()), (what, 'aux scratch written')
    # the gradient: the channels the loss uses, the sentinel everywhere else
    if with_grad:
        if exact:
            _same(gv[:, :used], r.grad, what + ' gradient')
        else:
            _close(gv[:, :used], r.grad, bar_g, f'{key} gradient', what)
        if kind in (2, 5):
            assert bool((gv[inp.out <= 0] == 0).all()), (what, 'a nonzero gradient at a score <= 0')
    assert bool((gv[:, used if with_grad else 0:] == SENT).all()), (what, 'a gradient channel the loss does not use changed')
    edge = (37 * 0) % n
    if with_grad and kind in (0, 1, 3) and (kind != 3 or inp.P == 1) and int(inp.mask.view(-1)[edge]):
        b0, p0 = divmod(edge, H * W)
        assert float(gv.view(B, oc, -1)[b0, 0, p0]) == 0.0, (what, 'gradient at out == gt')
    pool.check(what)
    return loss_out, scratch, r


def _oc_p(kind):
    return [(oc, P) for oc in OC[kind] for P in PLANES[kind]]


# ------------------------------------------------------------------------------------------------ the seven kinds
@LEGS
@pytest.mark.parametrize('kind', KINDS)
def test_loss_frames(kind, integer):
    dev = _dev()
    for i, frame in enumerate(FRAMES):
        for j, (oc, P) in enumerate(_oc_p(kind)):
            inp = make_inputs(kind, frame, oc, P, integer, 100 * kind + 10 * i + j, dev)
            run_loss(inp)
            if integer and kind in (4, 6):
                run_loss(inp, aux_override=exact_aux(inp))


@LEGS
@pytest.mark.parametrize('nblocks', NBLOCKS)
def test_loss_block_counts(nblocks, integer):
    """with 4096 blocks and 105 pixels every block must still write its partial: the one-wave finalize sums them all"""
    dev = _dev()
    for i, frame in enumerate(NBLOCKS_FRAMES):
        for kind in KINDS:
            oc, P = OC[kind][1 if kind in (2, 5) else 0], PLANES[kind][-1]
            inp = make_inputs(kind, frame, oc, P, integer, nblocks + 7 * kind + i, dev)
            run_loss(inp, nblocks)
            if integer and kind in (4, 6):
                run_loss(inp, nblocks, aux_override=exact_aux(inp))


@LEGS
@pytest.mark.parametrize('kind', KINDS)
def test_loss_stride_frame(kind, integer):
    """more than 8192 * 256 pixels: the gradient kernels' capped launch takes a second turn of the grid-stride loop"""
    inp = make_inputs(kind, STRIDE_FRAME, THIN_OC[kind], PLANES[kind][0], integer, 900 + kind, _dev())
    run_loss(inp, aux_override=exact_aux(inp) if integer and kind in (4, 6) else None)
    del inp
    torch.cuda.empty_cache()


@LEGS
@pytest.mark.parametrize('kind', KINDS)
def test_loss_den_override(kind, integer):
    """loss = sum / den_override; scratch[0..1] and the gradient scale follow it.  den_override = 0 takes the count-0 rule."""
    dev = _dev()
    inp = make_inputs(kind, (3, 5, 7), MIN_OC[kind] + (kind in (2, 5)), PLANES[kind][-1], integer, 300 + kind, dev)
    aux = exact_aux(inp) if integer and kind in (4, 6) else None
    for den in (8.0, 0.0) if integer else (7.0, 0.0):
        _, _, r = run_loss(inp, den_override=torch.tensor([den], dtype=torch.float64, device=dev), aux_override=aux)
        assert float(r.den) == den and float(r.den_used) == (den or 1.0)


@pytest.mark.parametrize('kind', [4, 6])
def test_loss_aux_override(kind):
    """the whole-batch sums of another (larger) batch: the factors come from aux_override and the aux pass writes nothing"""
    dev = _dev()
    for frame in ((3, 5, 7), (1, 1, 257)):
        for integer in (True, False):
            inp = make_inputs(kind, frame, 2, PLANES[kind][-1], integer, 400 + kind, dev)
            own = reference(inp)
            s0, s1 = float(own.aux[0]), float(own.aux[1]) if kind == 4 else 0.0
            for aux in ([s0, s1], [1.5 * s0 + 1.0, s1 + 3.0]):
                run_loss(inp, aux_override=torch.tensor(aux, dtype=torch.float64, device=dev), exact=False)


@pytest.mark.parametrize('kind', KINDS)
def test_loss_without_gradient(kind):
    """grad = NULL: the same value, bit for bit, the same scratch, and nothing else is written"""
    dev = _dev()
    for frame in ((3, 5, 7), (1, 1, 257)):
        inp = make_inputs(kind, frame, MIN_OC[kind] + 1, PLANES[kind][-1], False, 500 + kind, dev)
        with_g, scr_g, _ = run_loss(inp)
        without, scr, _ = run_loss(inp, with_grad=False)
        assert torch.equal(_bits(with_g), _bits(without)) and torch.equal(_bits(scr_g), _bits(scr)), (kind, frame)


@LEGS
@pytest.mark.parametrize('kind', KINDS)
def test_loss_with_a_mask_that_is_zero_everywhere(kind, integer):
    """count 0 -> denominator 1: the loss is 0 and the gradient is exactly 0 (kind 4: without a surface-less pixel both are
    NaN, 0 * NaN, so its case keeps them)"""
    dev = _dev()
    for frame in ((1, 1, 1), (3, 5, 7), (1, 1, 257)):
        inp = make_inputs(kind, frame, MIN_OC[kind] + 1, PLANES[kind][-1], integer, 600 + kind, dev, mask_mode='zero')
        loss, scratch, r = run_loss(inp, exact=False)
        if bool(torch.isfinite(r.loss)):
            assert float(loss) == 0.0 and float(r.loss) == 0.0 and float(scratch[1]) == 0.0 and float(scratch[0]) == 1.0
            assert not bool(r.grad.any())           # run_loss held the gradient to a bar of exactly 0


@LEGS
def test_multi_upr_without_a_surfaceless_pixel_is_nan(integer):
    """kind 4 divides by the number of pixels without a surface: with none the loss is NaN (0 * inf), in the kernel, in
    loss_ref and in the CPU module (tests/test_loss_head_cpu.py holds the last two together)"""
    dev = _dev()
    for frame in ((3, 5, 7), (1, 1, 257)):
        for P in PLANES[4]:
            inp = make_inputs(4, frame, 2, P, integer, 700 + P, dev, surfaceless='none')
            loss, _, r = run_loss(inp)
            assert float(r.aux[1]) == 0.0 and bool(torch.isnan(r.loss)) and bool(torch.isnan(loss).all())


@LEGS
@pytest.mark.parametrize('mp_mode', ['ones', 'zeros'])
def test_padded_upr_with_a_uniform_mask_padding(mp_mode, integer):
    """kind 6: no out-of-range pixel (f1 stays 1) | no in-range pixel (f0 stays 1)"""
    dev = _dev()
    for frame in ((3, 5, 7), (1, 1, 257)):
        for oc in OC[6]:
            inp = make_inputs(6, frame, oc, 0, integer, 800 + oc, dev, mp_mode=mp_mode)
            _, _, r = run_loss(inp, exact=integer)             # both factors are 1: exact without aux_override too
            assert float(r.parts['f0']) == 1.0 and float(r.parts['f1']) == 1.0


# ------------------------------------------------------------------------------------------------ Adam
def _adam_bars(g, m, v, p, lr, beta1, beta2, eps, step, gs, ref):
    """gi = g grad_scale: exact (grad_scale is a power of two).  c1 = 1 - (float)beta1 is an exact difference (Sterbenz) of a
    rounded beta: beta1 U absolute; likewise c2.
    m' = m + (gi - m) c1: the difference U, the product U, c1: -> |gi - m| (beta1 + 2 c1) U; the sum U |m'|.
    v' = v beta2 + gi gi c2: the cast of beta2 and the product: 2 U v beta2; gi gi: U, times c2: U, c2: beta2 U ->
         gi^2 (beta2 + 2 c2) U; the sum U v'.
    denom = sqrtf(v') / (float)sqrt(bc2) + (float)eps: bar(v') / (2 sqrt v') for the argument, U for the root, U for the cast
         of sqrt(bc2), U for the quotient: 3 U sqrt(v') / sqrt(bc2); U eps; the sum U denom.  (v' = 0: sqrtf(0) = 0 exactly.)
    p' = p - (float)(lr / bc1) (m' / denom): bar(m') / denom + |m'| bar(denom) / denom^2, the quotient U, the cast U, the
         product U: 3 U |m' / denom|; all times lr / bc1; the difference U |p'|."""
    p2, m2, v2 = ref
    gi = g.double() * gs
    c1, c2 = 1 - beta1, 1 - beta2
    bc1, bc2s = 1 - beta1 ** step, (1 - beta2 ** step) ** 0.5
    bm = U * ((gi - m.double()).abs() * (beta1 + 2 * c1) + m2.abs())
    bv = U * (2 * v.double() * beta2 + gi * gi * (beta2 + 2 * c2) + v2)
    root = v2.sqrt()
    denom = root / bc2s + eps
    bden = torch.where(v2 > 0, bv / (2 * root.clamp_min(1e-300)), torch.zeros_like(bv)) / bc2s + 3 * U * root / bc2s \
        + U * eps + U * denom
    q = m2 / denom
    bp = lr / bc1 * (bm / denom + m2.abs() * bden / denom ** 2 + 3 * U * q.abs()) + U * p2.abs()
    return bp, bm, bv


@pytest.mark.parametrize('gs', [1.0, 0.125])
@pytest.mark.parametrize('step', [1, 2, 1000])
@LEGS
def test_adam_step(integer, step, gs):
    from mmlf_amd import _lib
    from mmlf_amd._lib import call, ptr
    dev = _dev()
    lr = 0.0078125 if integer else 1e-3
    beta1, beta2, eps = (0.5, 0.75, 1e-8) if integer else (0.9, 0.999, 1e-8)
    for n in ADAM_N:
        gen = torch.Generator(device=dev).manual_seed(n + step)
        what = f'mmlf_adam_step n={n} step={step} grad_scale={gs} {"exact" if integer else "real"}'
        if integer:
            g, m = 0.25 * _ints(-8, 8, (n,), gen) / gs, 0.25 * _ints(-8, 8, (n,), gen)
            v = 0.0625 * _ints(0, 16, (n,), gen)
            still = torch.rand(n, device=dev, generator=gen) < 0.25           # g = m = v = 0: p must not move
            still[0] = n > 1
            g, m, v = (torch.where(still, torch.zeros_like(t), t) for t in (g, m, v))
        else:
            g, m = torch.randn(n, device=dev, generator=gen) / gs, 0.3 * torch.randn(n, device=dev, generator=gen)
            v = 0.1 * torch.rand(n, device=dev, generator=gen) ** 2
        p = torch.randn(n, device=dev, generator=gen)
        pool = _Pool(dev)
        tp, tg, tm, tv = pool.of(p), pool.of(g), pool.of(m), pool.of(v)
        call('mmlf_adam_step', ptr(tp), ptr(tg), ptr(tm), ptr(tv), n, lr, beta1, beta2, eps, step, gs, _lib.stream_ptr())
        ref = adam_ref(p, g, m, v, lr, beta1, beta2, eps, step, gs)
        bp, bm, bv = _adam_bars(g, m, v, p, lr, beta1, beta2, eps, step, gs, ref)
        if integer:
            _same(tm, ref[1], what + ' m')
            _same(tv, ref[2], what + ' v')
            _bar((tp.double() - ref[0]).abs(), bp, 'adam exact, p', what)
            assert torch.equal(_bits(tp[still]), _bits(p[still])), (what, 'p moved where g = m = v = 0')
        else:
            _bar((tm.double() - ref[1]).abs(), bm, 'adam m', what)
            _bar((tv.double() - ref[2]).abs(), bv, 'adam v', what)
            _bar((tp.double() - ref[0]).abs(), bp, 'adam p', what)
        assert torch.equal(_bits(tg), _bits(g)), (what, 'the gradient changed')
        pool.check(what)
        del pool, tp, tg, tm, tv, ref, bp, bm, bv


# ------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks_refuse_before_any_launch():
    """every call below fails a host check that stands in front of the wrapper's first launch: nonzero return and a message
    naming the function"""
    from mmlf_amd import _lib
    dev = _dev()
    L = _lib.load()
    t = torch.zeros(4096, device=dev)
    d = torch.zeros(4 * 4096 + 4, dtype=torch.float64, device=dev)
    i = torch.zeros(4096, dtype=torch.int32, device=dev)
    p, dp, ip, st = t.data_ptr(), d.data_ptr(), i.data_ptr(), _lib.stream_ptr()

    def refused(name, *args):
        rc = getattr(L, name)(*args)
        msg = _lib.last_error()
        assert rc != 0 and name in msg, (name, args, rc, msg)

    def single(kind=0, out=p, oc=2, gt=p, mask=ip, grid=p, loss=p, scratch=dp, nblocks=4, frame=(1, 1, 1)):
        refused('mmlf_loss_fwd_bwd', kind, out, oc, gt, mask, grid, 0.5, loss, p, scratch, nblocks, None, *frame, st)

    def multi(kind=3, out=p, oc=2, tgt=p, P=1, mask=ip, mp=ip, grid=p, loss=p, scratch=dp, nblocks=4, frame=(1, 1, 1)):
        refused('mmlf_loss_multi_fwd_bwd', kind, out, oc, tgt, P, mask, mp, grid, 0.5, loss, p, scratch, nblocks, None, None,
                *frame, st)

    for kind in (-1, 3, 7):
        single(kind=kind)
    for kind in (-1, 2, 7):
        multi(kind=kind)
    for arg in ('out', 'gt', 'mask', 'loss', 'scratch'):
        single(**{arg: None})
    for arg in ('out', 'tgt', 'mask', 'loss', 'scratch'):
        multi(**{arg: None})
    single(kind=2, grid=None)
    multi(kind=5, grid=None)
    multi(kind=6, mp=None)
    multi(kind=3, P=0)
    for kind, oc in ((0, 0), (1, 1), (2, 0)):
        single(kind=kind, oc=oc)
    for kind, oc in ((3, 0), (4, 1), (5, 0), (6, 1)):
        multi(kind=kind, oc=oc)
    for nblocks in (0, 4097, -1):
        single(nblocks=nblocks)
        multi(nblocks=nblocks)
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, -1)):
        single(frame=bad)
        multi(frame=bad)
        refused('mmlf_head_upr', p, p, p, 2, *bad, st)
        refused('mmlf_head_dpp', p, p, p, p, p, p, p, 2, *bad, st)
        refused('mmlf_head_upr_bwd', p, p, p, p, 2, *bad, st)
        refused('mmlf_head_dpp_bwd', p, p, p, p, p, p, 2, *bad, st)
    refused('mmlf_head_upr', p, p, p, 0, 1, 1, 1, st)
    refused('mmlf_head_upr', p, p, None, 2, 1, 1, 1, st)
    refused('mmlf_head_dpp', p, p, p, p, p, p, None, 2, 1, 1, 1, st)
    refused('mmlf_head_upr_bwd', p, p, None, p, 2, 1, 1, 1, st)
    refused('mmlf_head_dpp_bwd', p, p, p, None, None, p, 2, 1, 1, 1, st)       # neither gradient
    refused('mmlf_head_dpp_bwd', p, p, None, p, p, p, 2, 1, 1, 1, st)
    refused('mmlf_adam_step', p, p, p, p, 0, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, st)
    refused('mmlf_adam_step', p, p, p, p, 16, 1e-3, 0.9, 0.999, 1e-8, 0, 1.0, st)
    refused('mmlf_adam_step', p, None, p, p, 16, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, st)
    torch.cuda.synchronize()
    assert not bool(t.any()) and not bool(d.any()) and not bool(i.any())
