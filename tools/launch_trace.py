"""What the host code of the trunk (mmlf_amd/engine.py) does, as one JSON file: for a set of tiny configurations, every
call through the C ABI with its arguments, the `on_done` keys of Trunk.backward in call order, sha256 of the output, of
every gradient and of every buffer, and the allocator's peak.  Two trees whose files are equal issue the same launches
with the same arguments and compute the same bits: the oracle of a refactor of the host code.

    python tools/launch_trace.py OUT.json          (in each tree; then compare the files, or `--diff A.json B.json`)
    python tools/launch_trace.py --dry OUT.json    (no GPU: the host code alone, see below)

--dry: nothing is launched.  engine.call records the call and returns (the host-only mmlf_audit_* entries still run), the
stream pointer is 0, the tensors live on the CPU and the side-stream weight gradient is off; result hashes and the allocator
peak are left out.  The library loads without a GPU (its CU count falls back to 256).  Off CUDA the engine packs every filter
per layer (there is no one-launch prepack), so a dry file compares two TREES on one machine and never against a GPU file.

Uses only FeedForward, mmlf_amd.synth, engine.call and _lib.stream_ptr (which it wraps) and the trainable= / input_grads= /
frozen= keywords of Trunk.forward and Trunk.backward, so it runs unchanged in older trees that have them.
"""
import ctypes
import hashlib
import itertools
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmlf_amd import _lib, engine, synth                    # noqa: E402
from mmlf_amd.feed_forward import FeedForward               # noqa: E402

DEV = 'cuda:0'
B, H, W = 2, 7, 5
KW = dict(model_in_blocks=2, model_out_blocks=3, model_views=3, model_cross=False, model_unet=False,
          model_batchnorm_momentum=0.1, val_disp_min=-3.5, val_disp_max=3.5)
HEADS = {1: {}, 2: {'model_uncert': True}, 36: {'model_discrete': True}}          # BASE, UPR, DPP (4 x 3 views x 3)
NETS = {'k2bn': dict(model_ksize=2, model_no_batchnorm=False), 'k2nobn': dict(model_ksize=2, model_no_batchnorm=True),
        'k3bn': dict(model_ksize=3, model_no_batchnorm=False)}
PASSES = {'train_saved': (True, True), 'eval_folded': (False, False), 'eval_saved': (False, True),
          'train_nograd': (True, False)}                                             # name: (train, save)

# which parameters stay trainable (run(trainable=...)); 'none': forward(frozen=True) and backward(grads=None)
TRAINABLE = {'all': lambda n: True, 'out_net': lambda n: n.startswith('out_net.'), 'head': lambda n: n.startswith('out_net.2.'),
             'bias_bn': lambda n: not n.endswith(('.0.weight', '.2.weight')), 'hv0': lambda n: n.startswith('in_net_hv.0.'),
             'none': None}
ALL_X, H_ONLY = (True,) * 4, (True, False, False, False)

DRY = False
TRACE = []
_real_call = engine.call


def _arg(a, ctype):
    if isinstance(a, ctypes.Array):
        return ['a', [(('p' if v else 0) if a._type_ is ctypes.c_void_p else v) for v in a]]
    if ctype is ctypes.c_void_p:
        return 'p' if a else 0
    if a is None:
        return 0
    assert isinstance(a, (int, float)), (a, ctype)
    return a


def _traced_call(name, *args):
    types = _lib.SIGNATURES[name][1]
    assert len(types) == len(args), name
    TRACE.append([name, [_arg(a, t) for a, t in zip(args, types)]])
    if not DRY or name.startswith('mmlf_audit_'):
        _real_call(name, *args)


engine.call = _traced_call            # (engine binds `call` by name at import)


def go_dry():
    """--dry: from here on nothing is launched and nothing needs a device"""
    global DRY, DEV
    DRY, DEV = True, 'cpu'
    _lib.stream_ptr = lambda: 0
    if not torch.cuda.is_available():
        torch.cuda.current_stream = lambda device=None: None      # (older trees ask for it at the top of Trunk.backward)


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def model_of(net, chs, oc):
    kw = dict(KW, model_chs=chs, model_uncert=False, model_discrete=False, **NETS[net])
    kw.update(HEADS[oc])
    model = FeedForward(**kw)
    state = synth.formula_state([(k, v.shape) for k, v in model.state_dict().items()], seed=5)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    assert model._native_ok and model.out_chs == oc
    return model.to(DEV)


def run(net, chs, oc, pas, mode='f16x3', overlap=True, packed=False, extents=False, frame=(B, H, W), trainable=None,
        input_grads=None):
    """trainable: a key of TRAINABLE (None: the passes' default, every parameter and no keyword); input_grads: four bools, or
    a pair of such tuples (what forward is told, what backward is asked for)"""
    B, H, W = frame
    train, save = PASSES[pas]
    engine.CONV_MODE, engine.OVERLAP_WGRAD, engine.CHECK_EXTENTS = mode, overlap and not DRY, extents
    engine.EXTENT_CHECKS = 0
    model = model_of(net, chs, oc)
    dev = torch.device(DEV)
    stacks = [torch.from_numpy(s).to(dev) for s in synth.synth_inputs(B, H, views=3, seed=3, ps_w=W)[0]]
    gout = torch.from_numpy(np.random.RandomState(17).uniform(-1, 1, (B, oc, H, W)).astype(np.float32)).to(dev)
    p = {n: t.detach() for n, t in model._tensor_dict().items()}
    if not DRY:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
    del TRACE[:]
    done = []
    kw_f, kw_b, names, dstacks = {}, {}, model._param_names, []
    if input_grads is not None:
        fwd_x, bwd_x = input_grads if len(input_grads) == 2 else (input_grads, input_grads)
        kw_f['input_grads'], kw_b['input_grads'] = fwd_x, bwd_x
    if trainable == 'none':
        kw_f['frozen'], names = True, None
    elif trainable is not None:
        names = [n for n in model._param_names if TRAINABLE[trainable](n)]
        kw_f['trainable'] = names
    with torch.no_grad():
        if packed:        # inputs already in the grid layout, as the Ensamble hands them over
            geo = engine.Geometry(B, H, W, model._trunk.ksize)
            cs = engine.cs_of(9)
            xs = geo.bufs([cs] * 4, dev)
            for t, x in zip(stacks, xs):
                engine.call('mmlf_pack_nchw', t.data_ptr(), 9, x.data_ptr(), cs, B, H, W, x.absmax.data_ptr(),
                            _lib.stream_ptr())
            out, tape = model._trunk.forward(p, None, train, save, packed=(geo, xs), **kw_f)
        else:
            out, tape = model._trunk.forward(p, stacks, train, save, **kw_f)
        grads = {}
        if save:
            grads = {n: torch.zeros_like(p[n]) for n in names} if names is not None else None
            dstacks = model._trunk.backward(p, tape, gout, grads, on_done=done.append, **kw_b) or []
    res = {'trace': [list(t) for t in TRACE], 'on_done': done}
    if not DRY:
        torch.cuda.synchronize()
        res['peak_bytes'] = torch.cuda.max_memory_allocated()
        res['sha256'] = dict({'out': sha(out)}, **{f'grad/{n}': sha(g) for n, g in (grads or {}).items()},
                             **{f'buffer/{n}': sha(t) for n, t in model.named_buffers()},
                             **{f'dstack/{k}': sha(t) for k, t in zip('hvid', dstacks) if t is not None})
    if extents:
        res['extent_checks'] = engine.EXTENT_CHECKS
    return res


def configurations():
    for net, chs, oc, pas in itertools.product(NETS, (6, 32), HEADS, PASSES):
        for mode in (('f16x3', 'bf16x6', 'f32') if net != 'k3bn' else ('f16x3',)):
            # the side-stream weight gradient exists for wide 2x2 blocks in backward only
            for overlap in ((True, False) if chs == 32 and net != 'k3bn' and PASSES[pas][1] else (True,)):
                yield f'{net} chs={chs} oc={oc} {pas} {mode} overlap={int(overlap)}', (net, chs, oc, pas, mode, overlap)
    yield 'packed: k2bn chs=6 oc=2 eval_folded', ('k2bn', 6, 2, 'eval_folded', 'f16x3', True, True)
    for net, pas in (('k2bn', 'train_saved'), ('k2nobn', 'train_saved'), ('k3bn', 'train_saved'), ('k2bn', 'eval_folded')):
        yield f'extents: {net} chs=32 oc=2 {pas}', (net, 32, 2, pas, 'f16x3', True, False, True)
    # the default width (70: the 280-wide G = 18 launches, 80-column kernels over 4 and 9 chunks) and column blocks (96: 384 wide)
    for net, chs, oc, pas in itertools.product(('k2bn', 'k2nobn'), (70, 96), HEADS, PASSES):
        for mode in ('f16x3', 'bf16x6', 'f32'):
            for overlap in ((True, False) if PASSES[pas][1] else (True,)):
                yield f'{net} chs={chs} oc={oc} {pas} {mode} overlap={int(overlap)}', (net, chs, oc, pas, mode, overlap)
    # ... and a pitch of 128, where the sixteen-wave tile's window no longer fits: the register-streamed launches
    for net, pas in itertools.product(('k2bn', 'k2nobn'), ('train_saved', 'eval_folded')):
        yield f'pitch 128: {net} chs=70 oc=1 {pas}', (net, 70, 1, pas, 'f16x3', True, False, False, (1, 3, 126))
    # partial training and input gradients (Trunk.plan): every trainable set with no, all four and H's input gradient alone
    part = lambda net, chs, pas, mode, tr, want: (                                  # noqa: E731
        f'partial: {net} chs={chs} {pas} {mode} trainable={tr} input_grads={want}',
        (net, chs, 1, pas, mode, True, False, False, (B, H, W), tr, want))
    for net, chs, pas, tr in itertools.product(NETS, (6, 32), ('train_saved', 'eval_saved'), TRAINABLE):
        for want in (None, ALL_X, H_ONLY):
            yield part(net, chs, pas, 'f16x3', tr, want)
    for net in NETS:       # backward asks for less than forward recorded for; a partial set in the exact-f32 mode
        yield part(net, 32, 'train_saved', 'f16x3', 'out_net', (ALL_X, H_ONLY))
        yield part(net, 32, 'train_saved', 'f32', 'bias_bn', H_ONLY)


def diff(a, b):
    """prints what differs between two result files; exit status 1 if anything does"""
    ra, rb = json.load(open(a)), json.load(open(b))
    bad = 0
    for key in sorted(set(ra) | set(rb)):
        x, y = ra.get(key), rb.get(key)
        if x is None or y is None:
            print(f'{key}: only in {a if y is None else b}')
            bad += 1
            continue
        for field in sorted(set(x) | set(y)):
            if x.get(field) == y.get(field):
                continue
            bad += 1
            if field == 'trace':
                k = next((i for i, (u, v) in enumerate(zip(x[field], y[field])) if u != v), min(len(x[field]), len(y[field])))
                print(f'{key}: trace differs at call {k} of {len(x[field])} / {len(y[field])}:')
                print('   ', x[field][k] if k < len(x[field]) else None)
                print('   ', y[field][k] if k < len(y[field]) else None)
            elif field == 'sha256':
                print(f'{key}: tensors differ:', [n for n in x[field] if x[field][n] != y[field].get(n)])
            else:
                print(f'{key}: {field}: {x.get(field)} != {y.get(field)}')
    print(f'{len(ra)} / {len(rb)} configurations, {bad} differences')
    return 1 if bad else 0


def main():
    if sys.argv[1] == '--diff':
        sys.exit(diff(sys.argv[2], sys.argv[3]))
    path = sys.argv[-1]
    if sys.argv[1] == '--dry':
        go_dry()
    results = {}
    for key, args in configurations():
        assert key not in results, key
        results[key] = run(*args)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(results, f, indent=0, sort_keys=True)
    print(f'{len(results)} configurations, {sum(len(r["trace"]) for r in results.values())} calls -> {path}')


if __name__ == '__main__':
    main()
