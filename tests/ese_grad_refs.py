"""float64 restatements for the Ensamble's gradients (tests/test_ese_grad_cpu.py, tests/test_gpu_ese_grad.py), and the
cases both files share.

  * shift_f64 / ensamble_f64 / fuse_f64: reference mmlf/model/ensamble.py:58-101 with hci4d.Shift (hci4d.py:907-990) written
    out of place in torch ops, so that autograd differentiates it in the stacks and in the model's parameters; held to the
    reference's own autograd by tests/golden/g14_ensamble_grad.npz (tests/golden/make_golden_ese_grad.py).
  * reduce_bwd_f64: float64 autograd of the fusion alone, with the arg-min index handed in (kernel (a)'s reference).
  * unshift_f64: the float64 adjoint of the shear of ONE stack for a list of members, and the sum of |w g| over the terms of
    every element (kernel (b)'s reference and the bound's data term).
  * the end-to-end cases: net, frames, seeds, members, loss weights, the power-of-two loss scale.
"""
import functools
import math

import numpy as np
import torch

from conftest import TINY_KW
from mmlf_amd import synth
from mmlf_amd.ensamble import shift_table

KW = dict(TINY_KW, model_uncert=True)
DISP = (-1.0, 1.0, 0.5)                       # members arange(-1, 1, 0.5)
# (frame, seed of the weights and of the inputs); (1, 7, 130): pitch 132, the register-streamed narrow kernel (GPU only)
# ((1, 5, 29) with seed 2 has 11.7 % of its pixels inside tau: over the cap of the masked share, so that frame takes seed 1)
CPU_CASES = [((2, 9, 13), 0), ((2, 9, 13), 2), ((1, 5, 29), 1)]
GPU_CASES = CPU_CASES + [((1, 7, 130), 0)]
GRAD_FLOOR = 1e-2                             # every stack's max |gradient| is lifted to it (tests/test_input_grad_cpu.py)
# tests/test_gpu_model.py holds the tiny UPR net's eval-mode logvar at atol 5e-6 (rtol 5e-5); ten times the absolute part
LOGVAR_ATOL, LOGVAR_RTOL = 5e-6, 5e-5
TAU = 10 * LOGVAR_ATOL
MASK_CAP = 0.10
ALL_KEYS = ('mean', 'logvar', 'posterior', 'means', 'logvars')
PARAMS = ['in_net_hv.0.0.weight', 'out_net.2.2.bias']        # the two parameter gradients the fixture keeps


def bar(ref):
    """the project's gradient bar per tensor"""
    return 5e-4 * float(ref.abs().max()) + 5e-7


def ratio(got, ref):
    return float((got.detach().double().cpu() - ref).abs().max()) / bar(ref)


# ------------------------------------------------------------------------------------------------ the restatement
def _roll(x, s, dim):
    """cat([x[-s:], x[:-s]]) along dim with Python's slice clamping: |s| >= the extent leaves x as it is"""
    return x if abs(s) >= x.shape[dim] else torch.roll(x, s, dim)


def shift_f64(stacks, disp):
    """hci4d.Shift(disp) on (..., views, 3, H, W) tensors, out of place; the weights are the float32 table's (shift_table)"""
    views = stacks[0].shape[-4]
    tab_s, tab_w = shift_table([disp], views)
    outs = [[], [], [], []]
    for k in range(views):
        (s0, s1), (w0, w1) = (int(s) for s in tab_s[0, k]), (float(w) for w in tab_w[0, k])
        along = lambda x, dim, sg: _roll(x, sg * s0, dim) * w0 + _roll(x, sg * s1, dim) * w1      # noqa: E731
        h, v, i, d = (t[..., k, :, :, :] for t in stacks)
        outs[0].append(along(h, -1, 1))
        outs[1].append(along(v, -2, 1))
        outs[2].append(along(along(i, -1, 1), -2, -1))           # hci4d.py:971-975: the opposite sign along H
        outs[3].append(along(along(d, -1, 1), -2, 1))
    return [torch.stack(o, -4) for o in outs]


def fuse_f64(means, logvars, grid, idx=None):
    """ensamble.py:78-101: (mean, logvar, posterior) of (S, B, H, W) members; idx: the arg-min member per pixel (B, H, W),
    taken from logvars (the lowest index on a tie, as torch.min returns on the CPU) when None"""
    S = means.shape[0]
    if idx is None:
        idx = torch.min(logvars, 0)[1]
    idx = idx.unsqueeze(0)
    mean, logvar = means.gather(0, idx)[0], logvars.gather(0, idx)[0]
    g = grid.to(means.dtype).view(1, S, 1, 1)
    posterior = 0
    for j in range(S):
        b = torch.exp(logvars[j]).unsqueeze(1)
        posterior = posterior + 1.0 / (2.0 * b) * torch.exp(-torch.abs(g - means[j].unsqueeze(1)) / b)
    return mean, logvar, posterior / float(S)


def grid_of(disp=DISP):
    n = len(np.arange(*disp))
    return torch.from_numpy(np.linspace(disp[0], disp[1], n)).float()        # ensamble.py:91: float64 linspace into float32


def ensamble_f64(model, stacks, disp=DISP):
    means, logvars = [], []
    for sd in np.arange(*disp):
        out = model(*shift_f64(stacks, float(sd)))
        means.append(out['mean'] + float(sd))
        logvars.append(out['logvar'])
    means, logvars = torch.stack(means), torch.stack(logvars)
    mean, logvar, posterior = fuse_f64(means, logvars, grid_of(disp))
    return {'mean': mean, 'logvar': logvar, 'means': means, 'logvars': logvars, 'posterior': posterior}


# ------------------------------------------------------------------------------------------------ kernel references
def reduce_bwd_f64(means, logvars, grid, g_mean, g_logvar, g_post):
    """float64 autograd of fuse_f64 on float32 inputs (numpy or torch), the arg-min index taken from those inputs (strict <,
    lowest index).  Any of the three incoming gradients may be None.  Returns (g_means, g_logvars) float64."""
    m = torch.as_tensor(means).double().requires_grad_(True)
    lv = torch.as_tensor(logvars).double().requires_grad_(True)
    idx = torch.as_tensor(np.argmin(np.asarray(logvars), axis=0))             # (numpy: the first minimum)
    mean, logvar, post = fuse_f64(m, lv, torch.as_tensor(grid), idx)
    loss = 0
    for out, g in ((mean, g_mean), (logvar, g_logvar), (post, g_post)):
        if g is not None:
            loss = loss + (out * torch.as_tensor(g).double()).sum()
    loss.backward()
    return tuple(torch.zeros_like(t) if t.grad is None else t.grad for t in (m, lv))      # (mean alone never reaches logvars)


def shift_one_f64(x, kind, tab_s, tab_w):
    """one stack (views, 3, H, W) sheared for the members of a table: (n, views, 3, H, W); kind as mmlf_shift_pack's"""
    outs = []
    for s in range(tab_s.shape[0]):
        vs = []
        for k in range(x.shape[0]):
            (s0, s1), (w0, w1) = (int(t) for t in tab_s[s, k]), (float(t) for t in tab_w[s, k])
            along = lambda t, dim, sg: _roll(t, sg * s0, dim) * w0 + _roll(t, sg * s1, dim) * w1      # noqa: E731
            v = x[k]
            if kind != 1:
                v = along(v, -1, 1)
            if kind != 0:
                v = along(v, -2, -1 if kind == 2 else 1)
            vs.append(v)
        outs.append(torch.stack(vs))
    return torch.stack(outs)


def unshift_f64(g, kind, tab_s, tab_w):
    """g (n, views, 3, H, W) float32 -> (the float64 autograd adjoint of shift_one_f64 summed over the members, the same
    adjoint of |g| under |w|: sum |w g| over the terms of each element), both (views, 3, H, W)"""
    res = []
    for gg, ww in ((torch.as_tensor(g).double(), tab_w), (torch.as_tensor(g).double().abs(), np.abs(tab_w))):
        x = torch.zeros(gg.shape[1:], dtype=torch.float64, requires_grad=True)
        (shift_one_f64(x, kind, tab_s, ww) * gg).sum().backward()
        res.append(x.grad)
    return res


# ------------------------------------------------------------------------------------------------ end-to-end cases
def build(state, device='cpu', dtype=torch.float32, kw=KW):
    from mmlf_amd.feed_forward import FeedForward
    m = FeedForward(**kw)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    m = m.to(device)
    return (m.to(dtype) if dtype != torch.float32 else m).eval()


def case_inputs(frame, seed):
    B, H, W = frame
    return [torch.from_numpy(s) for s in synth.synth_inputs(B, H, seed=seed, ps_w=W)[0]]


def loss_weights(frame, seed, S=len(np.arange(*DISP))):
    """the random weights of the loss: one tensor per output, float32 values held in float64"""
    B, H, W = frame
    rs = np.random.RandomState(1000 + seed)
    shapes = {'mean': (B, H, W), 'logvar': (B, H, W), 'posterior': (B, S, H, W), 'means': (S, B, H, W), 'logvars': (S, B, H, W)}
    return {k: torch.from_numpy(rs.uniform(-1, 1, s).astype(np.float32)) for k, s in shapes.items()}


def loss_of(out, weights, keys=('mean', 'logvar', 'posterior')):
    return sum((out[k] * weights[k].to(out[k].device, out[k].dtype)).sum() for k in keys)


def gap_mask(logvars, tau=TAU):
    """pixels (B, H, W) where the two lowest logvar members are closer than tau: the arg-min may differ between two
    arithmetic paths there"""
    two = torch.sort(logvars.detach().double(), 0)[0][:2]
    return (two[1] - two[0]) < tau


@functools.lru_cache(maxsize=None)
def reference(frame, seed, masked=False, keys=('mean', 'logvar', 'posterior')):
    """float64 run of ensamble_f64 for a case: dict with the state, the weights (masked: those of mean and logvar zeroed at
    gap_mask pixels), the outputs, `scale` (the power of two that lifts every stack's max |gradient| to GRAD_FLOOR), the four
    stacks' gradients and every parameter gradient of loss * scale, the mask and the smallest gap."""
    state = synth.synth_state(synth.param_spec(**KW), seed=seed)
    m = build(state, dtype=torch.float64)
    xs = [s.double().requires_grad_(True) for s in case_inputs(frame, seed)]
    out = ensamble_f64(m, xs)
    weights = loss_weights(frame, seed)
    mask = gap_mask(out['logvars'])
    if masked:
        weights = dict(weights, mean=weights['mean'] * ~mask, logvar=weights['logvar'] * ~mask)
    loss_of(out, weights, keys).backward()
    smallest = min(float(x.grad.abs().max()) for x in xs)
    assert smallest > 0
    scale = 2.0 ** max(0, math.ceil(math.log2(GRAD_FLOOR / smallest)))
    two = torch.sort(out['logvars'].detach(), 0)[0][:2]
    return {'state': state, 'weights': weights, 'out': {k: v.detach() for k, v in out.items()}, 'scale': scale,
            'dx': [x.grad * scale for x in xs], 'dp': {n: p.grad * scale for n, p in m.named_parameters()},
            'mask': mask, 'gap': float((two[1] - two[0]).min()), 'keys': keys}


def run_module(ens, stacks, weights, scale, keys=('mean', 'logvar', 'posterior'), want=(True,) * 4):
    """one forward and backward of loss * scale through an Ensamble module; (outputs, the four input gradients)"""
    xs = [s.clone().requires_grad_(w) for s, w in zip(stacks, want)]
    out = ens(*xs)
    (loss_of(out, weights, keys) * scale).backward()
    return out, [x.grad for x in xs]
