"""Ensamble: drop-in for reference mmlf/model/ensamble.py:9-118 (the ESE method).

A 70-member shift ensemble with shared weights: for every disparity offset in
``np.arange(disp_min, disp_max, disp_step)`` the four view stacks are sheared by that offset
(``Shift``, reference mmlf/data/hci4d.py:894-990), the UPR model predicts (mean, logvar), and the
members are fused per pixel (arg-min logvar) plus a Laplace-mixture posterior.

On CUDA tensors: one HIP kernel shears all members at once (``mmlf_shift_views``), the members run
through the model as ONE batch when the model is in eval mode (eval-mode BatchNorm is a per-channel
affine map, so batching members is exact), and one kernel does the fusion (``mmlf_ensamble_reduce``).
On CPU tensors the same arithmetic runs in torch ops, member by member.

Differentiable as the reference's torch code is: the fusion is an autograd node over the members' means and
logvars (backward ``mmlf_ese_reduce_bwd``), and under autograd the members of the UPR model in eval mode are one node over the
four stacks and the model's parameters that keeps nothing per member and runs the members again in backward
(``mmlf_ese_unshift_sum`` takes the stacks' gradients out of the trunk's grid layout).
"""
import math
import os

import numpy as np
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import call, call_ese, check, ptr
from .feed_forward import laplacian


# MMLF_ESE_FUSED=0: the members go through mmlf_shift_views and the module's own forward (A/B of the fused member path)
FUSED_MEMBERS = os.environ.get('MMLF_ESE_FUSED', '1') != '0'


def shift_table(disps, views):
    """(shift0, shift1, 1-alpha, alpha) per (member, view), exactly as hci4d.py:934-938."""
    half = int(views / 2)
    tab_s = np.zeros((len(disps), views, 2), np.int32)
    tab_w = np.zeros((len(disps), views, 2), np.float32)
    for s, disp in enumerate(disps):
        for k in range(views):
            alpha, s0 = math.modf(float(disp) * (k - half))
            alpha = abs(alpha)
            s1 = s0 + math.copysign(1.0, s0)
            tab_s[s, k] = (int(s0), int(s1))
            tab_w[s, k] = (1.0 - alpha, alpha)
    return tab_s, tab_w


def _roll(x, s, dim):
    # cat([x[-s:], x[:-s]]) with Python slice clamping: |s| >= size leaves x unchanged
    return x if abs(s) >= x.shape[dim] else torch.roll(x, s, dim)


def shift_views_torch(stacks, disp):
    """hci4d.Shift on torch tensors (..., views, 3, H, W); returns new tensors (CPU path)."""
    h, v, i, d = [t.clone() for t in stacks]
    views = h.shape[-4]
    tab_s, tab_w = shift_table([disp], views)
    for k in range(views):
        (s0, s1), (w0, w1) = tab_s[0, k], tab_w[0, k]
        for t in (h, i, d):
            x = t[..., k, :, :, :]
            t[..., k, :, :, :] = _roll(x, int(s0), -1) * float(w0) + _roll(x, int(s1), -1) * float(w1)
    for k in range(views):
        (s0, s1), (w0, w1) = tab_s[0, k], tab_w[0, k]
        for t, sign in ((v, 1), (i, -1), (d, 1)):
            x = t[..., k, :, :, :]
            t[..., k, :, :, :] = _roll(x, sign * int(s0), -2) * float(w0) + _roll(x, sign * int(s1), -2) * float(w1)
    return h, v, i, d


def _fused_model(model, inner, views, c):
    """whether the members of this model can go through mmlf_shift_pack and the trunk on packed inputs: the UPR model itself
    (not a wrapper; not with the DPP head, whose mean is the arg-max one), native, on its own number of RGB views"""
    return bool(FUSED_MEMBERS and model is inner and getattr(inner, '_native_ok', False) and getattr(inner, 'uncert', False)
                and not getattr(inner, 'discrete', False) and views == inner.views and c == 3)


def _fused_members(model, inner, views, c):
    """whether the members take the fused path of _members_hip: a _fused_model in evaluation, outside autograd"""
    return bool(_fused_model(model, inner, views, c) and not inner.training and not torch.is_grad_enabled())


def _shear_pack(inner, src, tab_s, tab_w, s0, n, dev):
    """members [s0, s0 + n) of one batch item, sheared straight into the trunk's input layout: (Geometry, cs, four grid
    tensors).  src: the item's four contiguous (views, 3, H, W) stacks."""
    from . import engine
    views, c, hh, ww = src[0].shape
    geo = engine.Geometry(n, hh, ww, inner._trunk.ksize)
    cs = engine.cs_of(views * c)
    xs = geo.bufs([cs] * 4, dev)
    for kind, (t, x) in enumerate(zip(src, xs)):
        call('mmlf_shift_pack', ptr(t), kind, ptr(x), cs, ptr(tab_s[s0:s0 + n]), ptr(tab_w[s0:s0 + n]),
             n, views, hh, ww, ptr(x.absmax), _lib.stream_ptr())
    return geo, cs, xs


class _ReduceFn(torch.autograd.Function):
    """mean, logvar, posterior of the ensemble (ensamble.py:78-101) as a differentiable function of the members' means and
    logvars: forward = mmlf_ensamble_reduce, backward = mmlf_ese_reduce_bwd.  An output nobody
    differentiates arrives as None in backward and goes to the kernel as NULL."""

    @staticmethod
    def forward(ctx, means, logvars, grid):
        S, b, hh, ww = means.shape
        mean = torch.empty((b, hh, ww), dtype=torch.float32, device=means.device)
        logvar = torch.empty_like(mean)
        posterior = torch.empty((b, S, hh, ww), dtype=torch.float32, device=means.device)
        call('mmlf_ensamble_reduce', ptr(means), ptr(logvars), ptr(grid), ptr(mean), ptr(logvar),
             ptr(posterior), S, b, hh, ww, _lib.stream_ptr())
        ctx.save_for_backward(means, logvars, grid)
        ctx.set_materialize_grads(False)
        return mean, logvar, posterior

    @staticmethod
    @once_differentiable
    def backward(ctx, g_mean, g_logvar, g_post):
        if g_mean is None and g_logvar is None and g_post is None:
            return None, None, None
        means, logvars, grid = ctx.saved_tensors
        S, b, hh, ww = means.shape
        dev = means.device
        gs = []
        for name, g, shape in (('mean', g_mean, (b, hh, ww)), ('logvar', g_logvar, (b, hh, ww)), ('posterior', g_post, (b, S, hh, ww))):
            if g is not None:
                check(g, f'Ensamble: gradient of {name}', dev, shape=shape, contiguous=False)
                g = g.contiguous()
            gs.append(g)
        g_means, g_logvars = torch.empty_like(means), torch.empty_like(logvars)
        with torch.cuda.device(dev):
            call_ese('mmlf_ese_reduce_bwd', ptr(means), ptr(logvars), ptr(grid), ptr(gs[0]), ptr(gs[1]), ptr(gs[2]),
                     ptr(g_means), ptr(g_logvars), S, b, hh, ww, _lib.stream_ptr())
        return g_means, g_logvars, None


class _MembersFn(torch.autograd.Function):
    """(means, logvars) of every member as ONE autograd node over the four view stacks and the inner model's parameters
    (DESIGN.md 4.18).  Nothing per member is kept: forward runs the fused member path and saves the inputs and the shift
    tables; backward shears and runs the members again, batch item by batch item and in the forward's chunks of
    `member_budget_bytes`, each chunk under a tape (Trunk.forward(save=True)) that its Trunk.backward uses up, and takes the
    stacks' gradients from the grid layout with mmlf_ese_unshift_sum.  The parameter gradients of all chunks accumulate in
    one flat buffer, as in _TrunkFn.
    The values forward returns are those of the kind of pass backward runs again, so that the ReLU masks backward sees are
    the forward's: with a trainable parameter BatchNorm stays a pass of its own, with every parameter frozen it is folded
    into conv2 and the values are the bits of the no_grad forward."""

    @staticmethod
    def forward(ctx, ens, h, v, i, d, *params):
        inner = ens.model
        names = inner._param_names
        ctx.ens = ens
        ctx.trainable = [n for n, need in zip(names, ctx.needs_input_grad[5:]) if need]
        ctx.want_x = tuple(bool(w) for w in ctx.needs_input_grad[1:5])
        dev, views = h.device, h.shape[1]
        tab_s, tab_w = shift_table(ens.members(), views)
        tab_s, tab_w = torch.from_numpy(tab_s).to(dev), torch.from_numpy(tab_w).to(dev)
        ctx.save_for_backward(h, v, i, d, tab_s, tab_w, *params)
        ctx.set_materialize_grads(False)
        with torch.no_grad(), torch.cuda.device(dev):
            return _MembersFn._run(ctx, (h, v, i, d), tab_s, tab_w, params, None)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_means, g_logvars):
        n_in = 5 + len(ctx.ens.model._param_names)
        if g_means is None and g_logvars is None:
            return (None,) * n_in
        # (a second backward through the same forward fails here, on the released tensors, ahead of any launch)
        h, v, i, d, tab_s, tab_w, *params = ctx.saved_tensors
        S, b, hh, ww = len(ctx.ens.members()), h.shape[0], h.shape[3], h.shape[4]
        gouts = []
        for name, g in (('means', g_means), ('logvars', g_logvars)):
            if g is None:
                g = torch.zeros((S, b, hh, ww), dtype=torch.float32, device=h.device)
            check(g, f'Ensamble: gradient of {name}', h.device, shape=(S, b, hh, ww), contiguous=False)
            gouts.append(g)
        with torch.cuda.device(h.device):
            dstacks, grads = _MembersFn._run(ctx, (h, v, i, d), tab_s, tab_w, params, gouts)
        return (None, *dstacks, *grads)

    @staticmethod
    def _run(ctx, stacks, tab_s, tab_w, params, gouts):
        """gouts None: the forward pass, returns (means, logvars); else the backward pass for the gradients
        gouts = (g_means, g_logvars), returns (the four stacks' gradients, the parameters' gradients; None where unwanted)"""
        ens, trainable, want_x = ctx.ens, ctx.trainable, ctx.want_x
        inner = ens.model
        trunk, names = inner._trunk, inner._param_names
        b, views, c, hh, ww = stacks[0].shape
        dev = stacks[0].device
        disps = ens.members()
        S = len(disps)
        _lib.load()
        p = inner._tensor_dict()                        # buffers; the parameters as the node received them
        p.update(zip(names, (t.detach() for t in params)))
        trunk.check_params(p, dev)                      # the trunk's own check, ahead of the first shear launch
        frozen = not trainable
        chunk = ens._chunk(inner, S, hh, ww, taped=True)     # (the forward's chunks are the backward's)
        kw = dict(input_grads=want_x, frozen=frozen, trainable=trainable)
        if gouts is None:
            # the pass backward will run again keeps BatchNorm unfolded where the plan says so: only a forward under a tape
            # runs that form, and its tape is dropped at once
            save = trunk.batchnorm and not trunk.plan(() if frozen else trainable, want_x, False).fold
            offs = torch.from_numpy(disps.astype(np.float32)).to(dev)
            means = torch.empty((S, b, hh, ww), dtype=torch.float32, device=dev)
            logvars = torch.empty_like(means)
        else:
            dstacks = [torch.zeros(t.shape, dtype=torch.float32, device=dev) if w else None for t, w in zip(stacks, want_x)]
            grads, by_name = None, {}
            if trainable:
                sizes = [p[n].numel() for n in trainable]
                flat = torch.zeros(sum(sizes), dtype=torch.float32, device=dev)
                grads, o = {}, 0
                for n, sz in zip(trainable, sizes):
                    grads[n] = by_name[n] = flat[o:o + sz].view_as(p[n])
                    o += sz
            per_launch = max(1, _lib.ESE_MAX_TAB // views)
        for bi in range(b):
            src = [t[bi].contiguous() for t in stacks]
            for s0 in range(0, S, chunk):
                n = min(chunk, S - s0)
                geo, cs, xs = _shear_pack(inner, src, tab_s, tab_w, s0, n, dev)
                if gouts is None:
                    out, tape = trunk.forward(p, None, False, save, packed=(geo, xs), **(kw if save else {}))
                    del xs, tape
                    means[s0:s0 + n, bi] = out[:, 0] + offs[s0:s0 + n].view(-1, 1, 1)
                    logvars[s0:s0 + n, bi] = out[:, 1]
                    continue
                out, tape = trunk.forward(p, None, False, True, packed=(geo, xs), **kw)
                del xs, out
                gout = torch.stack((gouts[0][s0:s0 + n, bi], gouts[1][s0:s0 + n, bi]), 1)
                got = trunk.backward(p, tape, gout, grads, input_grads=want_x, packed_grads=True)
                del tape
                for kind, (entry, dst) in enumerate(zip(got, dstacks)):
                    if entry is None:
                        continue
                    gx, gcs = entry
                    for m0 in range(0, n, per_launch):
                        m = min(per_launch, n - m0)
                        call_ese('mmlf_ese_unshift_sum', ptr(gx[m0 * geo.G * gcs:]), gcs, kind, ptr(tab_s[s0 + m0:s0 + m0 + m]),
                                 ptr(tab_w[s0 + m0:s0 + m0 + m]), m, views, hh, ww, ptr(dst[bi]), _lib.stream_ptr())
                del got
        if gouts is None:
            return means, logvars
        return dstacks, [by_name.get(n) for n in names]


class Ensamble(nn.Module):
    def __init__(self, model, val_disp_min, val_disp_max, val_disp_step, **kwarg):
        super().__init__()
        self.disp_min, self.disp_max, self.disp_step = val_disp_min, val_disp_max, val_disp_step
        assert self.disp_min < self.disp_max
        assert self.disp_step > 0.0
        self.model = model
        self.member_budget_bytes = 24e9     # per activation buffer when members are batched; per tape under autograd (_chunk)

    def members(self):
        return np.arange(self.disp_min, self.disp_max, self.disp_step)

    def forward(self, h_views, v_views, i_views=None, d_views=None):
        if i_views is None or d_views is None:
            # The reference's signature has the same defaults (ensamble.py:40), but its own loop cannot run without the
            # diagonal stacks: it hands Shift a 2-tuple (ensamble.py:63-64) and Shift reads data[2] and data[3]
            # unconditionally (hci4d.py:927-928) -- IndexError before the first member.  Same exception type here.
            raise IndexError('Ensamble: i_views and d_views are required (the reference\'s Shift indexes data[2] and '
                             'data[3] for a two-stack ensemble too, hci4d.py:927-928: list index out of range)')
        disps = self.members()
        S = len(disps)
        if h_views.is_cuda:
            means, logvars = self._members_hip(h_views, v_views, i_views, d_views, disps)
        else:
            means, logvars = [], []
            for sd in disps:
                out = self.model(*shift_views_torch((h_views, v_views, i_views, d_views), float(sd)))
                means.append(out['mean'] + float(sd))
                logvars.append(out['logvar'])
            means, logvars = torch.stack(means), torch.stack(logvars)
        b, hh, ww = means.shape[1:]
        grid = torch.from_numpy(np.linspace(self.disp_min, self.disp_max, S)).float().to(means.device)
        if means.is_cuda:
            means, logvars = means.contiguous(), logvars.contiguous()
            mean, logvar, posterior = _ReduceFn.apply(means, logvars, grid)
        else:
            idx = torch.min(logvars, 0)[1].unsqueeze(0)
            mean, logvar = means.gather(0, idx)[0], logvars.gather(0, idx)[0]
            g = grid.view(1, -1, 1, 1).expand(b, S, hh, ww)
            posterior = torch.zeros((b, S, hh, ww))
            for k in range(S):
                posterior += laplacian(g, means[k], torch.exp(logvars[k]))
            posterior /= float(S)
        return {'mean': mean, 'logvar': logvar, 'means': means, 'logvars': logvars, 'posterior': posterior}

    def _chunk(self, inner, S, hh, ww, taped=False):
        """members of one trunk pass: all of them in evaluation (eval-mode BatchNorm is a per-channel map, so batching is
        exact), as far as `member_budget_bytes` allows -- per activation buffer on the paths that keep one layer at a time;
        taped (the differentiable member node, whose passes keep every layer of the chunk for their backward): for the three
        buffers of every block together, so that the same setting bounds the node's peak"""
        per_member = (hh + 2) * (ww + 2) * 4 * max(getattr(inner, 'chs', 70), 8) * 4
        if taped:
            from .engine import cs_of
            per_member = (hh + 2) * (ww + 2) * 4 * sum(3 * cs_of(site.spec.cout) for site in inner._trunk.sites)
        chunk = S if not inner.training else 1
        return int(max(1, min(chunk, self.member_budget_bytes // per_member)))

    def _members_hip(self, h, v, i, d, disps):
        b, views, c, hh, ww = h.shape
        S = len(disps)
        dev = h.device
        for name, t in (('h_views', h), ('v_views', v), ('i_views', i), ('d_views', d)):
            # raw pointers go to the shift kernels (any strides: each batch item is made contiguous below)
            check(t, f'Ensamble: {name}', dev, shape=h.shape, contiguous=False)
        model = self.model
        inner = model.module if hasattr(model, 'module') else model
        # Under autograd the members of the UPR model in evaluation are ONE node over the stacks and the parameters, which keeps
        # nothing per member and runs the members again in backward (_MembersFn).  Everything else -- train
        # mode, a DataParallel wrapper, another head, a model that is not native -- goes through the code below as ever, and
        # is differentiable where the module's own forward is.
        if torch.is_grad_enabled() and _fused_model(model, inner, views, c) and not inner.training:
            td = inner._tensor_dict()
            params = [td[n] for n in inner._param_names]
            if any(t.requires_grad for t in (h, v, i, d, *params)):
                return _MembersFn.apply(self, h, v, i, d, *params)
        tab_s, tab_w = shift_table(disps, views)
        tab_s, tab_w = torch.from_numpy(tab_s).to(dev), torch.from_numpy(tab_w).to(dev)
        chunk = self._chunk(inner, S, hh, ww)
        offs = torch.from_numpy(disps.astype(np.float32)).to(dev)
        means = torch.empty((S, b, hh, ww), dtype=torch.float32, device=dev)
        logvars = torch.empty_like(means)
        # Fused member path (round 6): the shear writes the trunk's own input layout (mmlf_shift_pack: no (n, views, 3, H, W)
        # intermediate, no pack pass) and the members' UPR `posterior` -- 108 planes per member that ensamble.py:66-76 never
        # reads -- is not formed.  Same bits as the path below (tests/test_ensamble.py).  For the uncertainty model itself, in
        # evaluation, outside autograd; anything else (a DataParallel wrapper, another head) takes the module's own forward.
        fused = _fused_members(model, inner, views, c)
        if fused:
            inner._trunk.check_params(inner._tensor_dict(), dev)       # the trunk's own check, ahead of the first shear launch
        for bi in range(b):
            src = [t[bi].contiguous() for t in (h, v, i, d)]
            for s0 in range(0, S, chunk):
                n = min(chunk, S - s0)
                if fused:
                    _lib.load()
                    with torch.cuda.device(dev):
                        geo, cs, xs = _shear_pack(inner, src, tab_s, tab_w, s0, n, dev)
                        out, _ = inner._trunk.forward(inner._tensor_dict(), None, False, False, packed=(geo, xs))
                        del xs
                    means[s0:s0 + n, bi] = out[:, 0] + offs[s0:s0 + n].view(-1, 1, 1)
                    logvars[s0:s0 + n, bi] = out[:, 1]
                    continue
                outs = [torch.empty((n, views, c, hh, ww), dtype=torch.float32, device=dev) for _ in range(4)]
                call('mmlf_shift_views', *[ptr(t) for t in src], *[ptr(t) for t in outs],
                     ptr(tab_s[s0:s0 + n]), ptr(tab_w[s0:s0 + n]), n, views, hh, ww, _lib.stream_ptr())
                out = model(*outs)
                means[s0:s0 + n, bi] = out['mean'] + offs[s0:s0 + n].view(-1, 1, 1)
                logvars[s0:s0 + n, bi] = out['logvar']
        return means, logvars
