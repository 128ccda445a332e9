"""The Ensamble's gradients on the GPU (reference mmlf/model/ensamble.py:40-118, which autograd
differentiates in the four view stacks and in the model's parameters).

  1. mmlf_ese_reduce_bwd against float64 autograd of the fusion on the same float32 inputs, the arg-min taken from them;
  2. mmlf_ese_unshift_sum against the float64 autograd adjoint of the shear on the same tables, to a bound the test computes
     from the data;
  3. the module end to end against the float64 restatement of tests/ese_grad_refs.py (conditioning and the masked share are
     asserted on the CPU, tests/test_ese_grad_cpu.py), weights frozen and trainable;
  4. the structure: what used to raise works, chunks, frozen launches, the paths that keep the module's own forward."""
import itertools

import numpy as np
import pytest
import torch

import ese_grad_refs as refs
from conftest import TINY_KW
from mmlf_amd import synth
from mmlf_amd.ensamble import Ensamble, shift_table

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


class _Spy:
    """records the entry points that go through _lib.call / _lib.call_ese from the engine and the modules"""

    def __init__(self, monkeypatch):
        from mmlf_amd import _lib, engine, ensamble, feed_forward
        self.names = []
        real_call, real_call_ese = _lib.call, _lib.call_ese

        def wrap(real):
            def call(name, *args):
                self.names.append(name)
                return real(name, *args)
            return call
        for mod in (_lib, engine, feed_forward, ensamble):
            monkeypatch.setattr(mod, 'call', wrap(real_call))
        for mod in (_lib, ensamble):
            monkeypatch.setattr(mod, 'call_ese', wrap(real_call_ese))


# ------------------------------------------------------------------------------------------------ 1: kernel (a)
def _reduce_bwd(means, logvars, grid, gs):
    from mmlf_amd import _lib
    dev = _dev()
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)        # noqa: E731
    m, lv, gr = t(means), t(logvars), t(grid)
    g = [t(a) for a in gs]
    S, B, H, W = means.shape
    out = [torch.full_like(m, float('nan')) for _ in range(2)]          # every element is written
    _lib.call_ese('mmlf_ese_reduce_bwd', _lib.ptr(m), _lib.ptr(lv), _lib.ptr(gr), *[_lib.ptr(a) for a in g],
                  _lib.ptr(out[0]), _lib.ptr(out[1]), S, B, H, W, _lib.stream_ptr())
    return out


def _check_reduce(tag, means, logvars, grid, gs):
    got = _reduce_bwd(means, logvars, grid, gs)
    want = refs.reduce_bwd_f64(means, logvars, grid, *gs)
    for name, g, w in zip(('g_means', 'g_logvars'), got, want):
        q = refs.ratio(g, w)
        print(f'{tag} {name}: max |gradient| {float(w.abs().max()):.3e}, error at {q:.3e} of the bar')
        assert q <= 1.0, (tag, name, q)
    return got


def _reduce_inputs(S, frame, seed):
    rs = np.random.RandomState(seed)
    B, H, W = frame
    means = rs.uniform(-1.2, 1.2, (S, B, H, W)).astype(np.float32)
    logvars = rs.uniform(-2, 1, (S, B, H, W)).astype(np.float32)
    grid = np.linspace(-1, 1, S).astype(np.float32)
    gs = [rs.uniform(-1, 1, shape).astype(np.float32) for shape in ((B, H, W), (B, H, W), (B, S, H, W))]
    return means, logvars, grid, gs


@pytest.mark.parametrize('frame', [(1, 1, 1), (2, 5, 7), (1, 3, 67)])          # (the last crosses a 64-thread block)
@pytest.mark.parametrize('S', [1, 4, 70])
def test_reduce_backward_against_float64(S, frame):
    means, logvars, grid, gs = _reduce_inputs(S, frame, S * 100 + frame[2])
    for keep in itertools.product((True, False), repeat=3):
        if any(keep):                                                  # the seven non-empty NULL combinations
            _check_reduce(f'S={S} {frame} {keep}', means, logvars, grid, [g if k else None for g, k in zip(gs, keep)])


def test_reduce_backward_gives_a_tie_to_the_lowest_index():
    means, logvars, grid, gs = _reduce_inputs(4, (2, 5, 7), 11)
    logvars[1, 0] = logvars[3, 0] = logvars.min() - 1.0                # members 1 and 3 tie for the minimum on image 0
    got = _check_reduce('tie', means, logvars, grid, [gs[0], gs[1], None])
    g_means, g_logvars = (g.cpu().numpy() for g in got)
    assert np.array_equal(g_means[1, 0], gs[0][0]) and np.array_equal(g_logvars[1, 0], gs[1][0])
    assert not g_means[3, 0].any() and not g_logvars[3, 0].any()


def test_reduce_backward_mean_on_a_grid_value_adds_nothing():
    means, logvars, grid, gs = _reduce_inputs(4, (2, 5, 7), 12)
    means[:] = grid[2]                                                 # every |grid_2 - m_j| is exactly 0
    gs[2][:, [0, 1, 3]] = 0                                            # ... and only that term carries a gradient
    got = _check_reduce('on the grid', means, logvars, grid, [None, None, gs[2]])
    assert not got[0].cpu().numpy().any()                              # sign(0) = 0: nothing reaches the means
    assert got[1].abs().max() > 0


# ------------------------------------------------------------------------------------------------ 2: kernel (b)
def _grid_layout(g, cs, fill):
    """(n, views, 3, H, W) -> the trunk's grid layout (n, H + 2, W + 2, cs) with `fill` in the border and the pad channels"""
    n, views, _, H, W = g.shape
    out = np.full((n, H + 2, W + 2, cs), fill, dtype=np.float32)
    out[:, 1:H + 1, 1:W + 1, :3 * views] = g.reshape(n, 3 * views, H, W).transpose(0, 2, 3, 1)
    return out


def _unshift(grid, cs, kind, tab_s, tab_w, views, H, W, out):
    from mmlf_amd import _lib
    dev = _dev()
    g, ts, tw = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (grid, tab_s, tab_w))
    _lib.call_ese('mmlf_ese_unshift_sum', _lib.ptr(g), cs, kind, _lib.ptr(ts), _lib.ptr(tw), tab_s.shape[0], views, H, W,
                  _lib.ptr(out), _lib.stream_ptr())
    return out


def _check_unshift(tag, members, views, H, W, seed):
    from mmlf_amd.engine import cs_of
    dev = _dev()
    cs = cs_of(3 * views)
    n = len(members)
    tab_s, tab_w = shift_table(members, views)
    for kind in range(4):
        g = np.random.RandomState(seed + kind).uniform(-1, 1, (n, views, 3, H, W)).astype(np.float32)
        want, mag = refs.unshift_f64(g, kind, tab_s, tab_w)
        # a float32 sum of at most 4 n products, each of at most three rounded factors, added to what `out` held
        bound = (4 * n + 4) * 2.0 ** -24 * mag
        zero = lambda: torch.zeros((views, 3, H, W), dtype=torch.float32, device=dev)        # noqa: E731
        once = _unshift(_grid_layout(g, cs, 0.0), cs, kind, tab_s, tab_w, views, H, W, zero())
        err = (once.double().cpu() - want).abs()
        print(f'{tag} kind {kind}: worst error at {float((err / bound).max()):.3f} of the bound')
        assert bool((err <= bound).all()), (tag, kind)
        # NaN in the border and the pad channels: never read
        nan = _unshift(_grid_layout(g, cs, np.nan), cs, kind, tab_s, tab_w, views, H, W, zero())
        assert torch.equal(nan, once), (tag, kind)
        # accumulation: two halves of the member list into one tensor
        h = n // 2
        two = zero()
        for sl in (slice(0, h), slice(h, n)):
            _unshift(_grid_layout(g[sl], cs, 0.0), cs, kind, tab_s[sl], tab_w[sl], views, H, W, two)
        assert bool(((two.double().cpu() - want).abs() <= bound).all()), (tag, kind)
        assert bool(((two.double().cpu() - once.double().cpu()).abs() <= bound).all()), (tag, kind)


@pytest.mark.parametrize('views', [9, 3])
@pytest.mark.parametrize('H,W', [(9, 13), (5, 29), (7, 130)])
def test_unshift_sum_against_the_float64_adjoint(H, W, views):
    _check_unshift(f'{views} views {H}x{W}', np.arange(-1, 1.5, 0.5), views, H, W, 7 * W + views)


def test_unshift_sum_with_shifts_past_the_frame():
    members = np.array([-3.5, -1.75, 0.0, 1.75])
    assert int(np.abs(shift_table(members, 9)[0]).max()) >= 13         # shifts of 14 and 15: the identity rule
    _check_unshift('clamped', members, 9, 9, 13, 5)


# ------------------------------------------------------------------------------------------------ 3: end to end
def _budget(m, frame, chunk):
    """the member_budget_bytes at which the differentiable member node takes `chunk` members per trunk pass"""
    from mmlf_amd.engine import cs_of
    tape = (frame[1] + 2) * (frame[2] + 2) * 4 * sum(3 * cs_of(site.spec.cout) for site in m._trunk.sites)
    return chunk * tape + 1


def _gpu_run(frame, seed, frozen, want=(True,) * 4, disp=refs.DISP, chunk=None):
    """one scaled forward + backward of the case's loss over all five outputs (mean and logvar masked) on the GPU; other
    members than the case's: fresh weights for their number, the case's scale"""
    ref = refs.reference(frame, seed, masked=True, keys=refs.ALL_KEYS)
    weights = ref['weights'] if disp == refs.DISP else refs.loss_weights(frame, seed, len(np.arange(*disp)))
    dev = _dev()
    m = refs.build(ref['state'], dev)
    assert m._native_ok and not m.training
    for p in m.parameters():
        p.requires_grad_(not frozen)
    ens = Ensamble(m, *disp)
    if chunk is not None:
        ens.member_budget_bytes = _budget(m, frame, chunk)
        assert ens._chunk(m, len(ens.members()), frame[1], frame[2], taped=True) == chunk
    stacks = [s.to(dev) for s in refs.case_inputs(frame, seed)]
    out, dx = refs.run_module(ens, stacks, weights, ref['scale'], ref['keys'] if disp == refs.DISP else ('means', 'logvars'), want)
    return m, ens, out, dx, ref


@pytest.mark.parametrize('frozen', [True, False])
@pytest.mark.parametrize('frame,seed', refs.GPU_CASES)
def test_gradients_against_float64(frame, seed, frozen):
    m, _, out, dx, ref = _gpu_run(frame, seed, frozen)
    tag = f'{frame} seed {seed} {"frozen" if frozen else "trainable"}'
    share = float(ref['mask'].double().mean())
    assert share <= refs.MASK_CAP, share
    # a kept pixel cannot change its member: the GPU logvars sit within the model tolerance of the float64 ones
    lv, lv64 = out['logvars'].detach().double().cpu(), ref['out']['logvars']
    excess = float(((lv - lv64).abs() - (refs.LOGVAR_ATOL + refs.LOGVAR_RTOL * lv64.abs())).max())
    print(f'{tag}: {share:.2%} masked; logvars at most {float((lv - lv64).abs().max()):.2e} from float64')
    assert excess <= 0, (tag, excess)
    keep = ~ref['mask']
    assert torch.equal(torch.min(lv, 0)[1][keep], torch.min(lv64, 0)[1][keep]), tag
    for k, g, r in zip('hvid', dx, ref['dx']):
        q = refs.ratio(g, r)
        print(f'{tag} d loss / d {k}_views: max |gradient| {float(r.abs().max()):.3e}, error at {q:.3e} of the bar')
        assert g.dtype == torch.float32 and g.shape == r.shape and q <= 1.0, (tag, k, q)
    for n, p in m.named_parameters():
        if frozen:
            assert p.grad is None, n
            continue
        q = refs.ratio(p.grad, ref['dp'][n])
        print(f'{tag} d loss / d {n}: max |gradient| {float(ref["dp"][n].abs().max()):.3e}, error at {q:.3e} of the bar')
        assert q <= 1.0, (tag, n, q)


# ------------------------------------------------------------------------------------------------ 4: structure
def _tiny(dev, seed=0, train=False, **kw):
    from mmlf_amd.feed_forward import FeedForward
    kw = dict(TINY_KW, **kw)
    m = FeedForward(**kw)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_state(synth.param_spec(**kw), seed).items()})
    return m.to(dev).train(train)


def test_posterior_backward_fills_the_stacks_gradient():
    """what the module could not do: mean / logvar / posterior had no grad_fn on CUDA tensors"""
    dev = _dev()
    ens = Ensamble(_tiny(dev, model_uncert=True), *refs.DISP)
    xs = [s.to(dev).requires_grad_(k == 0) for k, s in enumerate(refs.case_inputs((2, 9, 13), 0))]
    out = ens(*xs)
    assert all(out[k].grad_fn is not None for k in ('mean', 'logvar', 'posterior', 'means', 'logvars'))
    out['posterior'].sum().backward()
    assert xs[0].grad is not None and xs[0].grad.shape == xs[0].shape and float(xs[0].grad.abs().max()) > 0
    assert all(x.grad is None for x in xs[1:])
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in ens.model.parameters())


FIVE = (-1.0, 1.5, 0.5)


def test_chunks_of_three_and_two_members_equal_one_chunk_of_five():
    """the member node alone: the loss is over `means` and `logvars` (five members have no float64 case of their own, and the
    fusion node does not see the chunks)"""
    frame, seed = refs.GPU_CASES[0]
    runs = {}
    for chunk in (5, 3):
        m, ens, out, dx, _ = _gpu_run(frame, seed, False, disp=FIVE, chunk=chunk)
        runs[chunk] = (out, dx, {n: p.grad for n, p in m.named_parameters()})
    for a, b in zip(runs[5][1], runs[3][1]):
        assert refs.ratio(b, a.double().cpu()) <= 1.0
    for n, a in runs[5][2].items():
        assert refs.ratio(runs[3][2][n], a.double().cpu()) <= 1.0, n


def test_member_lists_longer_than_one_unshift_launch_are_split(monkeypatch):
    """mmlf_ese_unshift_sum holds n views <= MMLF_ESE_MAX_TAB table entries: with the limit at 18 the four members of a chunk
    go as two launches of two (the second from an offset into the gradient), accumulated into the same tensor"""
    from mmlf_amd import _lib
    monkeypatch.setattr(_lib, 'ESE_MAX_TAB', 18)
    frame, seed = refs.GPU_CASES[0]
    spy = _Spy(monkeypatch)
    _, _, _, dx, ref = _gpu_run(frame, seed, True)
    assert spy.names.count('mmlf_ese_unshift_sum') == 2 * 4 * frame[0]
    for k, g, r in zip('hvid', dx, ref['dx']):
        assert refs.ratio(g, r) <= 1.0, k


def _peak_of_one_step(m, disp, chunk, frame):
    """allocator peak, above what is allocated before the step, of one forward + backward through the Ensamble"""
    dev = _dev()
    ens = Ensamble(m, *disp)
    ens.member_budget_bytes = _budget(m, frame, chunk)
    peaks = []
    for _ in range(2):                                 # (the first step allocates the trunk's persistent workspace)
        m.zero_grad(set_to_none=True)
        xs = [s.to(dev).requires_grad_(True) for s in refs.case_inputs(frame, 0)]
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = ens(*xs)
        (out['mean'].sum() + out['logvar'].sum() + out['posterior'].sum()).backward()
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - base)
        del out, xs
    return peaks[-1]


def test_peak_memory_does_not_grow_with_the_members_beyond_one_chunk():
    """eight members against four in chunks of two: the peak may grow by the tensors that have a plane per member -- means,
    logvars, posterior, their gradients and the copies autograd holds of them, sixteen planes per member at the very most --
    and by nothing of the trunk's; eight members in ONE chunk tape four times as much"""
    frame = (1, 32, 32)
    m = _tiny(_dev(), model_uncert=True)
    four = _peak_of_one_step(m, (-1.0, 1.0, 0.5), 2, frame)
    eight = _peak_of_one_step(m, (-1.0, 1.0, 0.25), 2, frame)
    whole = _peak_of_one_step(m, (-1.0, 1.0, 0.25), 8, frame)
    planes = 16 * 4 * frame[0] * frame[1] * frame[2] * 4
    print(f'peak above the inputs: 4 members {four} B, 8 members {eight} B (allowed growth {planes} B), 8 in one chunk {whole} B')
    assert eight <= four + planes + 64 * 1024, (four, eight)
    assert whole > 2 * eight, (eight, whole)


def test_parameter_gradients_do_not_depend_on_the_stacks_asking():
    frame, seed = refs.GPU_CASES[0]
    m0, _, out0, dx0, _ = _gpu_run(frame, seed, False, want=(False,) * 4)
    m1, _, out1, dx1, _ = _gpu_run(frame, seed, False)
    assert dx0 == [None] * 4 and all(g is not None for g in dx1)
    for k in out0:
        assert torch.equal(out0[k], out1[k]), k
    for (n, p), (_, q) in zip(m0.named_parameters(), m1.named_parameters()):
        assert torch.equal(p.grad, q.grad), n


def test_frozen_net_runs_the_inference_launches_and_no_weight_gradient(monkeypatch):
    frame, seed = refs.GPU_CASES[0]
    spy = _Spy(monkeypatch)
    m, ens, out, dx, _ = _gpu_run(frame, seed, True)
    names = list(spy.names)
    assert all(g is not None for g in dx) and all(p.grad is None for p in m.parameters())
    assert not [n for n in names if 'wgrad' in n], names
    assert not [n for n in names if n.startswith(('mmlf_bn_apply_relu', 'mmlf_bn_bwd', 'mmlf_bn_stats_'))], names
    # one unpack per trunk pass (its output; one chunk per batch item, forward and again in backward): the stacks' gradients
    # stay in the grid layout
    assert names.count('mmlf_unpack_nchw') == 2 * frame[0] and names.count('mmlf_shift_pack') == 2 * 4 * frame[0]
    assert names.count('mmlf_ese_unshift_sum') == 4 * frame[0] and names.count('mmlf_ese_reduce_bwd') == 1
    assert 'mmlf_shift_views' not in names
    with torch.no_grad():
        plain = ens(*[s.to(_dev()) for s in refs.case_inputs(frame, seed)])
    for k, v in out.items():
        assert torch.equal(v.detach(), plain[k]), k


@pytest.mark.parametrize('path', ['train', 'dataparallel', 'dpp'])
def test_other_models_keep_the_modules_own_forward(path, monkeypatch):
    dev = _dev()
    m = _tiny(dev, train=path == 'train', **({'model_discrete': True} if path == 'dpp' else {'model_uncert': True}))
    model = torch.nn.DataParallel(m, device_ids=[0]) if path == 'dataparallel' else m
    spy = _Spy(monkeypatch)
    ens = Ensamble(model, *refs.DISP)
    xs = [s.to(dev).requires_grad_(True) for s in refs.case_inputs((2, 9, 13), 0)]
    out = ens(*xs)
    assert 'mmlf_shift_views' in spy.names and 'mmlf_shift_pack' not in spy.names
    assert all(out[k].grad_fn is not None for k in ('mean', 'logvar', 'posterior'))
    (out['mean'].sum() + out['logvar'].sum() + out['posterior'].sum()).backward()
    assert 'mmlf_ese_reduce_bwd' in spy.names and 'mmlf_ese_unshift_sum' not in spy.names
    # the members of this path are sheared by a raw mmlf_shift_views launch, as ever: the gradient goes through the
    # module's own forward to the parameters and stops short of the stacks
    assert all(x.grad is None for x in xs)
    grads = [p.grad for p in m.parameters()]
    assert all(g is not None for g in grads)
    if path != 'dpp':                  # (the DPP head's logvar is a log of a variance that may be 0: feed_forward._HeadDppFn)
        assert all(bool(torch.isfinite(g).all()) for g in grads) and max(float(g.abs().max()) for g in grads) > 0


def test_second_backward_raises_and_launches_nothing(monkeypatch):
    dev = _dev()
    ens = Ensamble(_tiny(dev, model_uncert=True), *refs.DISP)
    xs = [s.to(dev).requires_grad_(True) for s in refs.case_inputs((2, 9, 13), 0)]
    out = ens(*xs)
    loss = out['means'].sum() + out['posterior'].sum()
    loss.backward()
    spy = _Spy(monkeypatch)
    with pytest.raises(RuntimeError, match='second time'):
        loss.backward()
    assert spy.names == []
