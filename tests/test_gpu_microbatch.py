"""TrainStep(micro_batches=n) on the native path: the chunks of a step through the HIP kernels -- BatchNorm statistics per chunk
with NULL running pointers behind chunk 0, the whole batch's denominators through den_override / aux_override, gradients
accumulated by the weight-gradient and BatchNorm-backward launches themselves, one packing launch and one Adam launch per step."""
import numpy as np
import pytest
import torch

from mmlf_amd import synth
from test_microbatch_cpu import LR, PS, _data, _make, _mpi, _sizes, chunk_invariance_bound

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _cuda(*ts):
    return [t.to(DEV) for t in ts]


def _net(variant='base', **extra):
    return _make(variant, **extra).to(DEV)


def _step(variant='base', model_kw=None, **kw):
    from mmlf_amd.train import TrainStep
    step = TrainStep(_net(variant, **(model_kw or {})), lr=LR, loss_margin=3, **kw)
    assert step.model._native_ok
    return step


def _state(step):
    return [step.flat, step.exp_avg, step.exp_avg_sq] + [b for _, b in step.model.named_buffers()]


@pytest.mark.parametrize('B,n', [(2, 1), (1, 4)])
def test_a_single_chunk_is_bit_identical_to_the_step_without_the_argument(B, n):
    """(the default conversion mode, f16x3, unless MMLF_CONV_MODE says otherwise)"""
    stacks, gt, mask = (torch.from_numpy(np.asarray(x)).to(DEV) for x in synth.synth_inputs(B, PS, seed=6))
    a, b = _step('upr', micro_batches=n), _step('upr')
    for it in (1, 2):
        assert torch.equal(a(*stacks, gt, mask, it), b(*stacks, gt, mask, it))
    for x, y in zip(_state(a), _state(b)):
        assert torch.equal(x, y)
    assert float(a.flat.abs().sum()) > 0 and bool(torch.isfinite(a.flat).all())


@pytest.mark.parametrize('variant', ['base', 'upr', 'dpp'])
@pytest.mark.parametrize('B,n', [(4, 2), (5, 4)])
def test_step_equals_the_chunk_by_chunk_emulation(B, n, variant):
    """The emulation: a fresh native TrainStep per chunk, driven through _native_fwd_bwd with the whole batch's count as the
    denominator, the replicas' gradients summed in float64, one Adam launch on the sum.

    Step 1's gradient, per tensor.  The chunked step and the emulation run the same launches on the same bits, so every
    weight-gradient / BatchNorm-backward launch produces the same value `a` for an element; what differs is how the values are
    joined.  wgrad_reduce_kernel, wgrad_reduce_wave_kernel and bn_bwd_finalize_kernel store `old + (float)a`: the launch's float64 sum is
    rounded to float32 and added in float32, an error of at most 2^-24 of the partial result per join (bias_grad_finish_kernel
    joins in float64 and rounds once: no worse).  The chunked step makes m joins into one buffer, m = n for out_net and 2 n for
    the shared stream nets (two streams per pass); the emulation makes the m / n joins of a replica in float32 and the rest in
    float64.  Both stay within m * 2^-24 * M of the exact sum, M bounding the partial results: the largest sum over the replicas
    of |gradient| in the tensor (the two streams' values of a shared net are taken not to exceed the tensor's M).  Bound on the
    difference: 2 m 2^-24 M.

    Weights after two steps: the bars of tests/test_gpu_ddp.py's two-rank native run."""
    sizes = _sizes(B, n)
    stacks, gt, mask = _data(B, n)
    stacks, gt, mask = _cuda(*stacks), *_cuda(gt, mask)
    step = _step(variant, micro_batches=n)
    reps = [_step(variant) for _ in sizes]
    margin = reps[0]._mask(mask)
    den = margin.sum().double().reshape(1)
    assert float(margin[B - sizes[-1]:].sum()) == 0 and float(den) > 0      # a chunk without a valid pixel
    bounds = np.cumsum([0] + sizes)
    solid = None
    for it in (1, 2):
        loss = step(*stacks, gt, mask, it)
        want = []
        for r, st in enumerate(reps):
            lo, hi = int(bounds[r]), int(bounds[r + 1])
            st.grad.zero_()
            st.model.train()
            want.append(st._native_fwd_bwd(*[s[lo:hi] for s in stacks], gt[lo:hi], margin[lo:hi], den))
        np.testing.assert_allclose(float(loss), sum(float(w) for w in want), rtol=1e-5)
        summed = sum(st.grad.double() for st in reps)
        if it == 1:
            mag = sum(st.grad.double().abs() for st in reps)
            for name, o, cnt in step.layout:
                m = n * (2 if name.startswith('in_net') else 1)
                tol = 2 * m * 2.0 ** -24 * float(mag[o:o + cnt].max())
                worst = float((step.grad[o:o + cnt].double() - summed[o:o + cnt]).abs().max())
                assert worst <= tol, (name, worst, tol)
            assert float(mag.max()) > 0
        ok = summed.abs() > 1e-5
        solid = ok if solid is None else solid & ok
        for st in reps:
            st.grad.copy_(summed)
            st.adam_steps += 1
            st._adam(st.current_lr(it), 1.0)
    assert step.adam_steps == 2
    torch.testing.assert_close(step.flat[solid], reps[0].flat[solid], rtol=1e-4, atol=1e-4 if variant == 'dpp' else 3e-5)
    assert float(solid.float().mean()) > (0.5 if variant == 'dpp' else 0.9)       # (tests/test_microbatch_cpu.py's floors)


LOSS_KW = {'upr': {}, 'multi_upr': {'loss_multimodal': True}, 'upr_padded': {'loss_padding': 1.5},
           'multi_upr_padded': {'loss_multimodal': True, 'loss_padding': 1.5}}


@pytest.mark.parametrize('net', ['eval_mode', 'no_batchnorm'])
@pytest.mark.parametrize('name', list(LOSS_KW))
def test_chunks_change_nothing_where_batchnorm_cannot_differ(name, net):
    """n = 3 on B = 5 (chunks of 2, 2 and 1 samples) against n = 1: the loss to rtol 1e-5, every gradient tensor within
    test_microbatch_cpu.chunk_invariance_bound.  The kernels add to that bound's reasons a power-of-two operand scale taken from
    the tensor's largest magnitude (the chunk's, not the batch's), which moves the f16 split's rounding at the 2^-22 level.
    The padded forms (+-1.5: every sample of either target has values on both sides) take the per-chunk in-range masks and the
    whole batch's sums through the chunks."""
    kw, B, n = LOSS_KW[name], 5, 3
    stacks, gt, mask = (torch.from_numpy(np.asarray(x)) for x in synth.synth_inputs(B, PS, seed=6))
    mask[0, :, :9] = 0
    mask[3] = 0
    target = _mpi(B) if kw.get('loss_multimodal') else gt          # (pixels without a surface in sample 0 alone: the other chunks' own count is 0)
    stacks, target, mask = _cuda(*stacks), *_cuda(target, mask)
    model_kw, step_kw = ({'model_no_batchnorm': True}, {}) if net == 'no_batchnorm' else ({}, {'train_eval_mode': True})

    def run(n):
        step = _step('upr', model_kw, micro_batches=n, **kw, **step_kw)
        return float(step(*stacks, target, mask, 1)), step
    loss1, one = run(1)
    loss, step = run(n)
    assert np.isfinite(loss1) and float(one.grad.abs().max()) > 0
    print(f'{name}, {net}: loss {loss!r} in {n} chunks, {loss1!r} in one')
    np.testing.assert_allclose(loss, loss1, rtol=1e-5)
    for pname, o, cnt in step.layout:
        g, g1 = step.grad[o:o + cnt], one.grad[o:o + cnt]
        worst, tol = float((g - g1).abs().max()), chunk_invariance_bound(g1, n)
        print(f'  {pname}: worst {worst:.3e}, bound {tol:.3e}')
        assert worst <= tol, (pname, worst, tol)


def test_later_chunks_leave_the_buffers_alone():
    """against a step on chunk 0 alone: the same launches on the same bits, so the buffers are compared exactly"""
    B, n = 5, 4
    stacks, gt, mask = _data(B, n)
    stacks, gt, mask = _cuda(*stacks), *_cuda(gt, mask)
    step, ref = _step(micro_batches=n), _step()
    before = {k: v.clone() for k, v in step.model.named_buffers()}
    step(*stacks, gt, mask, 1)
    ref.model.train()
    margin, k0 = ref._mask(mask), _sizes(B, n)[0]
    ref._native_fwd_bwd(*[s[:k0] for s in stacks], gt[:k0], margin[:k0], margin.sum().double().reshape(1))
    moved = 0
    for (k, got), (_, want) in zip(step.model.named_buffers(), ref.model.named_buffers()):
        assert torch.equal(got, want), k
        if k.endswith('num_batches_tracked'):
            assert int(got) == (2 if k.startswith('in_net') else 1), (k, int(got))
        else:
            moved += int(not torch.equal(got, before[k]))
    assert moved > 0


@pytest.mark.parametrize('B,H,W,C', [(1, 1, 1, 2), (3, 9, 7, 70)])
def test_bn_statistics_with_null_running_pointers(B, H, W, C):
    """mmlf_bn_stats_train / mmlf_bn_stats_finalize with running_mean = running_var = NULL: status 0 (call raises otherwise), the
    bits of the call with buffers in save_mean, save_invstd, scale and shift, and a pair of buffers that was not passed unchanged"""
    from mmlf_amd import _lib, engine
    from mmlf_amd._lib import call, ptr
    gen = torch.Generator(device=DEV).manual_seed(B * 100 + C)
    rand = lambda *shape: torch.rand(*shape, device=DEV, generator=gen)      # noqa: E731
    geo, cs = engine.Geometry(B, H, W), engine.cs_of(C)
    z = geo.buf(cs, torch.device(DEV))
    z[:geo.NQ * cs].zero_()
    z[:geo.NQ * cs].view(B, geo.R, geo.P, cs)[:, 1:H + 1, 1:W + 1, :C] = 4 * rand(B, H, W, C) - 1.5
    gamma, beta = rand(C) + 0.5, rand(C) - 0.5
    nblk = 24
    x = (4 * rand(nblk, 4, C) - 1.5).double()
    part_fin = torch.stack([x.sum(1), (x * x).sum(1)], 1).contiguous()       # [nblk][2][C], as conv2's epilogue leaves them
    sentinel = 12345.0
    torch.cuda.synchronize()

    def run(entry, with_buffers):
        rm, rv = torch.full((C,), sentinel, device=DEV), torch.full((C,), sentinel, device=DEV)
        outs = [torch.full((C,), float('nan'), device=DEV) for _ in range(4)]
        passed = (ptr(rm), ptr(rv)) if with_buffers else (None, None)
        if entry == 'mmlf_bn_stats_train':
            part = torch.empty(2 * C * 16, dtype=torch.float64, device=DEV)
            call(entry, ptr(z), cs, C, ptr(gamma), ptr(beta), *passed, 0.1, 1e-5, *[ptr(o) for o in outs], ptr(part), 16,
                 B, H, W, _lib.stream_ptr())
        else:
            call(entry, ptr(part_fin), nblk, C, ptr(gamma), ptr(beta), *passed, 0.1, 1e-5, *[ptr(o) for o in outs],
                 nblk, 2, 2, _lib.stream_ptr())
        torch.cuda.synchronize()
        return outs, rm, rv

    for entry in ('mmlf_bn_stats_train', 'mmlf_bn_stats_finalize'):
        with_b, rm, rv = run(entry, True)
        assert not bool((rm == sentinel).any()) and not bool((rv == sentinel).any()), entry      # (the buffers do move when passed)
        null, rm, rv = run(entry, False)
        assert bool((rm == sentinel).all()) and bool((rv == sentinel).all()), entry
        for a, b, what in zip(with_b, null, ('save_mean', 'save_invstd', 'scale', 'shift')):
            assert bool(torch.isfinite(a).all()) and torch.equal(a, b), (entry, what)


@pytest.mark.parametrize('n', [1, 3])
def test_a_step_packs_its_filters_once(n, monkeypatch):
    from mmlf_amd import engine
    assert engine.CONV_MODE == 'f16x3', 'the one packing launch belongs to the f16-split kernels: run without MMLF_CONV_MODE'
    stacks, gt, mask = _data(5, n)
    stacks, gt, mask = _cuda(*stacks), *_cuda(gt, mask)
    step = _step(micro_batches=n)
    calls, orig = [], engine.call
    monkeypatch.setattr(engine, 'call', lambda name, *a: (calls.append(name), orig(name, *a))[1])
    step(*stacks, gt, mask, 1)
    assert calls.count('mmlf_pack_filters_h2') == 1
    assert calls.count('mmlf_unpack_nchw') == n                         # one forward pass per chunk
    assert not any(name in ('mmlf_pack_filter_h2', 'mmlf_pack_filter') for name in calls)


def test_frozen_parameters_stay_put_over_the_chunks():
    from mmlf_amd.train import TrainStep
    stacks, gt, mask = _data(4, 2)
    stacks, gt, mask = _cuda(*stacks), *_cuda(gt, mask)
    model = _net()
    model.in_net_hv.requires_grad_(False)
    step = TrainStep(model, lr=LR, loss_margin=3, micro_batches=2)
    start = step.flat.clone()
    for it in (1, 2):
        step(*stacks, gt, mask, it)
    frozen = torch.zeros_like(step.flat, dtype=torch.bool)
    for name, o, cnt in step.layout:
        if name.startswith('in_net_hv'):
            frozen[o:o + cnt] = True
    assert 0 < int(frozen.sum()) < frozen.numel()
    assert torch.equal(step.flat[frozen], start[frozen])
    assert not bool(step.exp_avg[frozen].any()) and not bool(step.exp_avg_sq[frozen].any()) and not bool(step.grad[frozen].any())
    moved = (step.flat != start) & ~frozen
    assert bool(moved.any())


def test_four_chunks_need_at_most_half_the_step_memory():
    """What a step allocates beyond what persists between steps is per sample, so four chunks should need a quarter; the factor
    two leaves room for allocator granularity at this size (B = 8, 32 x 32)."""
    stacks, gt, mask = (torch.from_numpy(np.asarray(x)).to(DEV) for x in synth.synth_inputs(8, 32, seed=2))
    peak = {}
    for n in (1, 4):
        step = _step(micro_batches=n)
        step(*stacks, gt, mask, 1)                      # warm-up: workspaces, packed-filter store, margin mask
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step(*stacks, gt, mask, 2)
        torch.cuda.synchronize()
        peak[n] = torch.cuda.max_memory_allocated() - base
        del step
    print(f'step peak above the pre-step level: n=1 {peak[1]} B, n=4 {peak[4]} B, ratio {peak[4] / peak[1]:.3f}')
    assert peak[1] > 0 and peak[4] <= 0.5 * peak[1], peak
