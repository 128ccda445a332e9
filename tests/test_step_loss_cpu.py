"""train.StepLoss: which loss a step takes, on which target, divided by what.  The resolution of every combination of the loss
options against a literal restatement of the reference's loop body (mmlf/train/cli.py:190-225,247-255) on the stock modules, and
the whole-batch sums the object hands to the loss kernel in each regime (one rank, rank of a group, chunk)."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from mmlf_amd import dl, loss, synth
from mmlf_amd.train import TrainStep
from test_ddp_gloo import _free_port
from test_microbatch_cpu import LR, PS, _make, _mpi

B, MARGIN, PAD = 3, 3, 1.5
COMBOS = ([(v, m, p, False) for v in ('base', 'upr', 'dpp') for m in (False, True) for p in (None, PAD)]
          + [(v, False, p, True) for v in ('base', 'upr', 'dpp') for p in (None, PAD)])


def _inputs():
    stacks, gt, mask = (torch.from_numpy(np.asarray(x)) for x in synth.synth_inputs(B, PS, seed=6))
    in_range = (torch.abs(gt) < PAD).sum((1, 2))
    assert bool(((in_range > 0) & (in_range < PS * PS)).all())          # both sides of the padding in every sample
    return stacks, gt, _mpi(B), mask


def _restatement(variant, multimodal, padding, strongest, stacks, gt, mpi, mask):
    """the loop body, line by line, with kwargs[...] spelled as the arguments: (loss, flat gradient)"""
    model = _make(variant)
    model_uncert, model_discrete = variant == 'upr', variant == 'dpp'
    if multimodal:                                                                  # :120-128
        loss_fn, loss_uncert_fn = loss.MultiMaskedL1Loss(), loss.ImprovedMultiUncertaintyL1Loss()
    else:
        loss_fn, loss_uncert_fn = loss.MaskedL1Loss(), loss.ImprovedUncertaintyL1Loss()
    loss_discrete_fn = loss.MaskedCrossEntropy()
    mpi = mpi.clone()
    if strongest:                                                                   # :190-192
        inds = torch.max(mpi[:, :, 3, :, :], dim=1)[1].unsqueeze(1)
        gt = torch.gather(mpi[:, :, 4, :, :], dim=1, index=inds).squeeze()
    mask = mask.int() * loss.create_mask_margin(mask.shape, MARGIN)                # :194
    dims = 4 * 9 * 3                                                                # :196-199
    if model_discrete:                                                              # :201-206
        if multimodal:
            gt_classes = dl.mpi_to_weights(mpi, -3.5, 3.5, dims)
        else:
            gt_classes = dl.reg_to_class(gt, -3.5, 3.5, dims)
    mask_padding = None                                                             # :217-222
    if padding is not None:
        if multimodal:
            mpi[:, :, 3, :, :] *= (torch.abs(mpi[:, :, 4, :, :]) < padding).float()
        else:
            mask_padding = (torch.abs(gt) < padding).int()
    if multimodal:                                                                  # :224-225
        gt = mpi
    model.train()
    output = model(*stacks)                                                         # :245
    if model_uncert:                                                                # :247-255
        loss_train = loss_uncert_fn(output, gt, mask, mask_padding)
    elif model_discrete:
        loss_train = loss_discrete_fn(output, gt_classes, mask)
    else:
        loss_train = loss_fn(output, gt, mask)
    loss_train.backward()
    return loss_train.detach(), torch.cat([p.grad.reshape(-1) for p in model.parameters()])


@pytest.mark.parametrize('variant,multimodal,padding,strongest', COMBOS)
def test_every_combination_resolves_as_the_reference_loop(variant, multimodal, padding, strongest):
    """rtol = atol = 0: the step's stock path runs the restatement's operations on the restatement's bits.  (The restatement
    agrees with itself run twice at the suite's thread count: asserted first.)"""
    stacks, gt, mpi, mask = _inputs()
    want, want_grad = _restatement(variant, multimodal, padding, strongest, stacks, gt, mpi, mask)
    again, again_grad = _restatement(variant, multimodal, padding, strongest, stacks, gt, mpi, mask)
    assert torch.equal(want, again) and torch.equal(want_grad, again_grad)
    assert bool(torch.isfinite(want)) and bool(torch.isfinite(want_grad).all()) and float(want_grad.abs().max()) > 0
    step = TrainStep(_make(variant), lr=LR, loss_margin=MARGIN, loss_multimodal=multimodal, loss_padding=padding,
                     loss_strongest=strongest)
    kept = mpi.clone()
    got = step(*stacks, mpi if multimodal or strongest else gt, mask, 1)
    assert torch.equal(mpi, kept)                                                   # the caller's planes keep their alpha
    assert torch.equal(got, want), (float(got), float(want))
    assert torch.equal(step.grad, want_grad), float((step.grad - want_grad).abs().max())


def test_the_kinds_of_the_combinations():
    kinds = {c: TrainStep(_make(c[0]), lr=LR, loss_multimodal=c[1], loss_padding=c[2], loss_strongest=c[3]).loss.kind for c in COMBOS}
    for (variant, multimodal, padding, strongest), kind in kinds.items():
        base = {'base': loss.KIND_L1, 'upr': loss.KIND_UPR, 'dpp': loss.KIND_CE}[variant]
        if multimodal:
            assert kind == base + 3
        else:                                   # the UPR loss without a padding stays kind 1
            assert kind == (loss.KIND_UPR_PADDED if variant == 'upr' and padding is not None else base)


# ---------------------------------------------------------------------------------------------- the normaliser regimes
AUX_CASES = {loss.KIND_MULTI_UPR: {'loss_multimodal': True}, loss.KIND_UPR_PADDED: {'loss_padding': PAD}}
N_CHUNKS = 2        # B = 3 per rank: chunks of 2 and 1 samples, n / pixels = 1 / 3 and 1 / 6


def _own_sums(kind, target):
    """the two sums over a rank's tensors, as the losses define them (loss.py:336-372, 264-294)"""
    if kind == loss.KIND_MULTI_UPR:
        tot = target[:, :, 3].sum(1)
        return torch.stack([tot.sum().double(), (tot < 0.01).sum().double()])
    return torch.stack([(torch.abs(target) < PAD).int().sum().double(), torch.zeros((), dtype=torch.float64)])


def _rank_data(rank):
    _, gt, mask = (torch.from_numpy(np.asarray(x)) for x in synth.synth_inputs(2 * B, PS, seed=6))
    lo, hi = B * rank, B * rank + B
    return gt[lo:hi], _mpi(2 * B)[lo:hi], mask[lo:hi]


def _aux_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    torch.set_num_threads(2)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        out = {}
        gt, mpi, mask = _rank_data(rank)
        for kind, kw in AUX_CASES.items():
            step = TrainStep(_make('upr'), lr=LR, loss_margin=MARGIN, micro_batches=N_CHUNKS, **kw)
            assert step.loss.kind == kind and step.loss.distributed and step.loss.world == world
            target = mpi if kind == loss.KIND_MULTI_UPR else gt
            sums = _own_sums(kind, target)
            dist.all_reduce(sums)
            _, mask_padding = step.loss._pass_target(target, None)
            whole = step.loss.kernel_aux(target, mask_padding, mask.numel())
            share = step.loss.chunks(N_CHUNKS, N_CHUNKS, target, mask, None)
            chunk = {n: step.loss.kernel_aux(None, None, n, share) for n in (2 * PS * PS, PS * PS)}
            out[kind] = {'sums': sums, 'whole': whole, 'chunk': chunk, 'pixels': share.pixels}
        torch.save(out, os.path.join(out_dir, f'r{rank}.pt'))
    finally:
        dist.destroy_process_group()


def test_aux_of_a_rank_and_of_a_chunk(tmp_path):
    """bit for bit: (all-reduced sums) / world for an un-chunked pass of a rank, (all-reduced sums) * n / pixels for a chunk of n
    pixels -- two float64 values that differ for a sum of alphas"""
    world = 2
    mp.spawn(_aux_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    ranks = [torch.load(tmp_path / f'r{r}.pt') for r in range(world)]
    for kind in AUX_CASES:
        local = [_own_sums(kind, _rank_data(r)[1 if kind == loss.KIND_MULTI_UPR else 0]) for r in range(world)]
        for rk in ranks:
            got, sums = rk[kind], rk[kind]['sums']
            assert torch.equal(sums, local[0] + local[1]) and not torch.equal(local[0], local[1])
            assert got['pixels'] == world * B * PS * PS
            assert got['whole'].dtype == torch.float64 and torch.equal(got['whole'], sums / world)
            for n, aux in got['chunk'].items():
                assert aux.dtype == torch.float64 and torch.equal(aux, sums * n / got['pixels'])
    s = ranks[0][loss.KIND_MULTI_UPR]['sums']
    assert float(s[0]) != round(float(s[0])) and float(s[1]) > 0            # a sum of alphas; some pixels lack a surface


@pytest.mark.parametrize('kind', list(AUX_CASES))
def test_one_rank_leaves_the_sums_to_the_kernel(kind):
    gt, mpi, mask = _rank_data(0)
    step = TrainStep(_make('upr'), lr=LR, loss_margin=MARGIN, **AUX_CASES[kind])
    target = mpi if kind == loss.KIND_MULTI_UPR else gt
    target, mask_padding = step.loss._pass_target(target, None)
    assert (mask_padding is not None) == (kind == loss.KIND_UPR_PADDED)
    assert step.loss.kernel_aux(target, mask_padding, mask.numel()) is None
