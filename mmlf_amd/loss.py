"""Losses and masks of the train / validate step, reference mmlf/model/loss.py.

Each module takes ``(output_dict, target, mask[, mask_padding])`` like the reference.  On CUDA
tensors the training losses -- single-mode, multimodal and padded -- run fused HIP kernels (value +
gradient in one call, ``mmlf_loss_fwd_bwd`` / ``mmlf_loss_multi_fwd_bwd``) behind a small autograd node;
on CPU they are plain torch expressions.  ``LOSSES`` lists the seven kinds: what ``native_loss`` and the
node know about a kind is its row.
"""
import functools
from typing import NamedTuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._lib import call, check, ptr
from .engine import LOSS_BLOCKS

KIND_L1, KIND_UPR, KIND_CE = 0, 1, 2                                         # mmlf_loss_fwd_bwd
KIND_MULTI_L1, KIND_MULTI_UPR, KIND_MULTI_CE, KIND_UPR_PADDED = 3, 4, 5, 6   # mmlf_loss_multi_fwd_bwd


def create_mask_margin(shape, margin=0):
    """Boolean mask that is False in a `margin`-wide frame of the last two dims (loss.py:6-26)."""
    assert margin >= 0
    mask = torch.ones(shape, dtype=torch.bool)
    if margin > 0:
        mask[..., :margin, :] = False
        mask[..., -margin:, :] = False
        mask[..., :margin] = False
        mask[..., -margin:] = False
    return mask


def _masked_mean(loss, mask):
    count = mask.int().sum()
    loss = loss * mask.float()
    if count == 0:
        return loss.sum()
    return loss.sum() / count


def _fused(kind, target, mask, mask_padding, *heads):
    return _NativeLossFn.apply(kind, target, mask, mask_padding, None, 0.0, None, *heads)


class MaskedL1Loss(nn.Module):
    """loss.py:29-77"""

    def forward(self, input, target, mask):
        if input['mean'].is_cuda:
            return _fused(KIND_L1, target, mask, None, input['mean'])
        return _masked_mean(torch.abs(input['mean'] - target), mask)


class MaskedMSELoss(nn.Module):
    """loss.py:106-122"""

    def forward(self, input, target, mask):
        return _masked_mean((input['mean'] - target) ** 2.0, mask)


class MaskedBadPix(nn.Module):
    """loss.py:163-187"""

    def __init__(self, t=0.07):
        super().__init__()
        self.t = t

    def forward(self, input, target, mask):
        bad = (torch.abs(input['mean'] - target) > self.t).int() * mask.int()
        count = mask.int().sum()
        if count == 0:
            return bad.sum()
        return bad.sum().float() / count


class ImprovedUncertaintyL1Loss(nn.Module):
    """loss.py:254-294"""

    def forward(self, input, target, mask, mask_padding=None):
        mean, logvar = input['mean'], input['logvar']
        if mean.is_cuda:        # without a mask_padding this is kind 1, not kind 6 with a mask of ones
            return _fused(KIND_UPR if mask_padding is None else KIND_UPR_PADDED, target, mask, mask_padding, mean, logvar)
        loss = torch.exp(-logvar) * torch.abs(mean - target) + logvar
        if mask_padding is not None:
            mp = mask_padding.float()
            loss = loss * mp
            if mp.sum() > 0:
                loss = loss * (mp.numel() / mp.sum())
            oor = 1.0 - mp
            loss_oor = -logvar * oor
            if oor.sum() > 0:
                loss_oor = loss_oor * (oor.numel() / oor.sum())
            loss = (loss + loss_oor) / 2.0
        return _masked_mean(loss, mask)


class MaskedCrossEntropy(nn.Module):
    """loss.py:137-160: relu(scores), -log(exp(<s,t>) / sum exp(s)), masked mean."""

    def forward(self, input, target, mask):
        s = F.relu(input['scores'])
        loss = -torch.log(torch.exp(torch.sum(s * target, 1)) / torch.sum(torch.exp(s), 1))
        return _masked_mean(loss, mask)


# ------------------------------------------------------------------ multimodal training losses
# (reached with --train_loss_multimodal, reference train/cli.py:120-123,224-225).
# `target` is the multi-plane tensor (B, P, 5, H, W): channel 3 = alpha, channel 4 = disparity.
class MultiMaskedL1Loss(nn.Module):
    """loss.py:80-103: alpha-weighted L1 to every plane, masked mean."""

    def forward(self, input, target, mask):
        if input['mean'].is_cuda:
            return _fused(KIND_MULTI_L1, target, mask, None, input['mean'])
        weights, targets = target[:, :, 3], target[:, :, 4]
        diff = (torch.abs(input['mean'].unsqueeze(1) - targets) * weights).sum(1)
        return _masked_mean(diff, mask)


class ImprovedMultiUncertaintyL1Loss(nn.Module):
    """loss.py:336-372: alpha-weighted Laplace NLL normalised by the mean total alpha, plus a
    -logvar term on pixels without any surface (total alpha < 0.01), each side rescaled; masked mean."""

    def forward(self, input, target, mask, mask_padding=None):
        mean, logvar = input['mean'], input['logvar']
        if mean.is_cuda:
            return _fused(KIND_MULTI_UPR, target, mask, None, mean, logvar)
        weights, targets = target[:, :, 3], target[:, :, 4]
        loss = torch.exp(-logvar).unsqueeze(1) * torch.abs(mean.unsqueeze(1) - targets) + logvar.unsqueeze(1)
        total = weights.sum(1)
        loss = (loss * weights).sum(1) / torch.mean(total)
        oor = (total < 0.01).float()
        loss_oor = -logvar * oor * (oor.numel() / torch.sum(oor))
        return _masked_mean((loss + loss_oor) / 2.0, mask)


# ------------------------------------------------------------------ the seven fused kinds
class LossKind(NamedTuple):
    entry: str              # the C entry point
    heads: tuple            # the heads it consumes, in the channel order of the trunk output
    written: int            # gradient channels the kernel writes (0: all of them); the rest must be zeroed
    target: str             # 'gt': (B, H, W) depths, 'mpi': (B, P, 5, H, W) planes
    mask_padding: bool      # takes the in-range mask
    grid: bool              # takes the disparity grid and half a step of it (the cross-entropy target is built in the kernel)
    aux: bool               # normalises by whole-batch sums (aux_override; NULL: the tensor's own)
    module: type            # the nn.Module that states it on CPU (the cross-entropy kinds: on reg_to_class / mpi_to_weights targets)


_SINGLE, _MULTI = 'mmlf_loss_fwd_bwd', 'mmlf_loss_multi_fwd_bwd'
LOSSES = {
    KIND_L1:         LossKind(_SINGLE, ('mean',), 1, 'gt', False, False, False, MaskedL1Loss),
    KIND_UPR:        LossKind(_SINGLE, ('mean', 'logvar'), 2, 'gt', False, False, False, ImprovedUncertaintyL1Loss),
    KIND_CE:         LossKind(_SINGLE, ('scores',), 0, 'gt', False, True, False, MaskedCrossEntropy),
    KIND_MULTI_L1:   LossKind(_MULTI, ('mean',), 1, 'mpi', False, False, False, MultiMaskedL1Loss),
    KIND_MULTI_UPR:  LossKind(_MULTI, ('mean', 'logvar'), 2, 'mpi', False, False, True, ImprovedMultiUncertaintyL1Loss),
    KIND_MULTI_CE:   LossKind(_MULTI, ('scores',), 0, 'mpi', False, True, False, MaskedCrossEntropy),
    KIND_UPR_PADDED: LossKind(_MULTI, ('mean', 'logvar'), 2, 'gt', True, False, True, ImprovedUncertaintyL1Loss),
}


@functools.lru_cache(maxsize=None)
def _scratch_doubles(entry):
    return 2 * LOSS_BLOCKS + 2 if entry == _SINGLE else int(_lib.load().mmlf_loss_multi_scratch_doubles(LOSS_BLOCKS))


def native_loss(kind, output, target, mask, mask_padding=None, grid_torch=None, half_step=0.0, want_grad=True,
                den_override=None, aux_override=None):
    """Fused loss of LOSSES[kind] on the raw trunk output (B,oc,H,W).  The kernels walk n = B*H*W pixels of mask, mask_padding
    and a gt target (any dtype, any strides: converted here), oc grid entries, one float64 denominator and two float64 sums --
    a shorter tensor, or one of another device, is read past its end.  Returns (loss scalar tensor, grad or None)."""
    row = LOSSES[kind]
    B, oc, H, W = output.shape
    dev, n = output.device, B * H * W
    check(mask, 'loss: mask', dev, None, numel=n, contiguous=False)
    if grid_torch is not None:
        check(grid_torch, 'loss: grid', dev, min_numel=oc)
    if den_override is not None:
        check(den_override, 'loss: den_override', dev, torch.float64, min_numel=1)
    check(target, 'loss: target', dev, None, numel=n if row.target == 'gt' else None, contiguous=False)
    if mask_padding is not None:
        check(mask_padding, 'loss: mask_padding', dev, None, numel=n, contiguous=False)
    if aux_override is not None:
        check(aux_override, 'loss: aux_override', dev, torch.float64, min_numel=2)
    if row.target == 'mpi' and (target.dim() != 5 or target.shape[0] != B or target.shape[2] != 5
                                or tuple(target.shape[3:]) != (H, W)):
        raise ValueError(f'multimodal loss: target must be (B, P, 5, H, W), got {tuple(target.shape)}')
    if row.mask_padding and (tuple(target.shape) != (B, H, W) or mask_padding is None):
        raise ValueError('padded loss: target (B, H, W) and mask_padding required')
    output = output.contiguous()
    target = target.contiguous().float()
    mask = mask.contiguous().to(torch.int32)
    if mask_padding is not None:
        mask_padding = mask_padding.contiguous().to(torch.int32)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    grad = None
    if want_grad:
        grad = torch.zeros_like(output) if 0 < row.written < oc else torch.empty_like(output)
    scratch = torch.empty(_scratch_doubles(row.entry), dtype=torch.float64, device=dev)
    if row.entry == _SINGLE:
        call(_SINGLE, kind, ptr(output), oc, ptr(target), ptr(mask), ptr(grid_torch), float(half_step), ptr(loss), ptr(grad),
             ptr(scratch), LOSS_BLOCKS, ptr(den_override), B, H, W, _lib.stream_ptr())
    else:
        call(_MULTI, kind, ptr(output), oc, ptr(target), target.shape[1] if row.target == 'mpi' else 0, ptr(mask),
             ptr(mask_padding), ptr(grid_torch), float(half_step), ptr(loss), ptr(grad), ptr(scratch), LOSS_BLOCKS,
             ptr(den_override), ptr(aux_override), B, H, W, _lib.stream_ptr())
    return loss, grad


native_multi_loss = native_loss


class _NativeLossFn(torch.autograd.Function):
    """autograd node of the fused losses for callers that go through the loss modules.  heads: LOSSES[kind].heads; aux: the
    kernel's aux_override (a micro-batch of a train step hands in the whole batch's sums), None: the tensor's own sums"""

    @staticmethod
    def forward(ctx, kind, target, mask, mask_padding, grid, half_step, aux, *heads):
        if LOSSES[kind].heads == ('scores',):
            out = heads[0]
        else:
            out = heads[0].unsqueeze(1) if len(heads) == 1 else torch.stack(heads, 1)
        loss, grad = native_loss(kind, out.detach(), target, mask, mask_padding, grid, half_step, aux_override=aux)
        ctx.stacked = out is not heads[0]
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, gl):
        (grad,) = ctx.saved_tensors
        g = grad * gl
        return (None,) * 7 + (tuple(g[:, k] for k in range(g.shape[1])) if ctx.stacked else (g,))
