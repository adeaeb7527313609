"""Per-block gradient parity of the fused autograd blocks (lcasr_amd.functional) against float64.  TEST INFRASTRUCTURE.

A case (tests/block_cases.py) names its float tensors, a `fused` closure over the product's functional blocks and a `plain` closure
over the restatements of tests/block_refs.py.  check_block runs

  * the plain formula in float64                                  - the truth,
  * the plain formula under torch.autocast('cpu', bfloat16)       - the yardstick (it never touches the code under test),
  * the fused block (HIP kernels, or tests/kernel_refs.py through conftest's `emulated_ops`),

and asserts for every output and every differentiable input t, with relative L2 errors against the truth,

      E_fused[t] <= max(2 * E_ac[t], 2^-8).

Factor 2: two bf16 evaluations that round at different points are independent realisations of the same noise; a missing term or
a wrong scale moves a tensor by far more.  Floor 2^-8: the two bf16 roundings every block applies and autocast may not (its bf16
operand and its bf16 output gradient).  A tensor whose float64 norm is below 1e-9 of the block's gradient rms is analytically
zero (the depthwise-conv bias in front of a training BatchRenorm); it must have rms <= 1e-3 x the rms of all the block's float64
gradients (the floor convention of common_model.rel_l2_errors).  A gradient that is None on one side only fails.

The inputs of a case must be conditioned so that every bound is <= CAP = 2.5e-2 (E_ac <= 1.25e-2): asserted, as a property of
the inputs.  A case whose inputs cannot meet it at test size carries its own cap, recorded next to the case.
"""
from __future__ import annotations

import contextlib

import torch

FACTOR, FLOOR, CAP = 2.0, 2.0 ** -8, 2.5e-2
ZERO_REL, ZERO_RMS = 1e-9, 1e-3
F32, F64 = torch.float32, torch.float64


class Case:
    """name; tensors {name: f32 CPU tensor | None}; params / streams: the differentiable names (parameters take direct gradients,
    streams are activations); fused(Fn, t) and plain(t) -> (tuple of outputs, dict of extra results compared like outputs);
    dy: one f32 CPU tensor (or None: output unused) per output; cap: the bound's cap for this case."""

    def __init__(self, name, block, tensors, params, streams, fused, plain, dy, cap=CAP):
        self.name, self.block, self.tensors, self.params, self.streams = name, block, tensors, list(params), list(streams)
        self.fused, self.plain, self.dy, self.cap = fused, plain, tuple(dy), cap
        self.nondirect = set()                      # parameters the block sees through a non-leaf stand-in: autograd accumulates them

    @property
    def diff(self):
        return self.streams + self.params

    def __repr__(self):
        return self.name


class Result:
    def __init__(self, outs, grads, extras):
        self.outs, self.grads, self.extras = outs, grads, extras          # CPU float64 tensors (a grad may be None)


def _cpu64(t):
    return None if t is None else t.detach().to('cpu', F64)


def _leaves(case, dtype, device):
    t = {}
    for k, v in case.tensors.items():
        if v is None:
            t[k] = None
            continue
        w = v.detach().to(device=device, dtype=dtype if v.is_floating_point() else v.dtype).clone()
        t[k] = w.requires_grad_(True) if k in case.diff else w
    return t


def _loss_backward(outs, dys):
    loss = None
    for y, dy in zip(outs, dys):
        if dy is None:
            continue
        dy = dy.to(y.device)
        if dy.shape != y.shape:
            raise ValueError(f'dy {tuple(dy.shape)} does not fit output {tuple(y.shape)}')
        term = (y.to(dy.dtype) * dy).sum()
        loss = term if loss is None else loss + term
    loss.backward()


def _collect(case, t, outs, extras):
    return Result([_cpu64(y) for y in outs], {k: _cpu64(t[k].grad) for k in case.diff}, {k: _cpu64(torch.as_tensor(v)) for k, v in extras.items()})


def run_plain(case, autocast: bool) -> Result:
    dtype = F32 if autocast else F64
    t = _leaves(case, dtype, 'cpu')
    ctx = torch.autocast('cpu', dtype=torch.bfloat16) if autocast else contextlib.nullcontext()
    with ctx:
        outs, extras = case.plain(t)
    _loss_backward(outs, [None if d is None else d.to(F32 if autocast else F64) for d in case.dy])
    return _collect(case, t, outs, extras)


def run_fused(case, Fn, device='cpu', direct=False, dys=None, backward=None):
    """The fused block with p.grad starting as None (returned gradients), or - direct - with set_direct_grad(True) and every
    parameter's p.grad pre-filled (random, non-zero, contiguous): the Result then holds p.grad - pre-fill, and the second value
    returned lists the parameters the grad-ready hook fired for.  backward(outs): another way to start the backward."""
    Fn.clear_weight_cache()
    Fn._twins.clear()
    t = _leaves(case, F32, device)
    fired, before = [], {}
    if direct:
        g = torch.Generator().manual_seed(97)
        for k in case.params:
            if t[k] is not None:
                before[k] = (0.1 * torch.randn(t[k].shape, generator=g) + 0.05).to(device)
                t[k].grad = before[k].clone()
        names = {id(t[k]): k for k in case.params if t[k] is not None}
        Fn.set_grad_ready_hook(lambda p: fired.append(names.get(id(p), '?')))
        Fn.set_direct_grad(True)
    try:
        outs, extras = case.fused(Fn, t)
        if backward is not None:
            backward(outs)
        else:
            _loss_backward(outs, case.dy if dys is None else dys)
        if device != 'cpu':
            torch.cuda.synchronize()
    finally:
        if direct:
            Fn.set_direct_grad(False)
            Fn.set_grad_ready_hook(None)
    res = _collect(case, t, outs, extras)
    if direct:
        for k, b in before.items():                              # a parameter nobody wrote to still holds its pre-fill: no gradient
            untouched = k not in fired and torch.equal(t[k].grad, b)
            res.grads[k] = None if untouched else res.grads[k] - _cpu64(b)
    Fn._twins.clear()
    return (res, fired) if direct else res


def _rel(a, ref):
    return float((a - ref).norm()) / float(ref.norm())


def grad_rms(truth: Result) -> float:
    gs = [g for g in truth.grads.values() if g is not None]
    return (sum(float(g.pow(2).sum()) for g in gs) / max(sum(g.numel() for g in gs), 1)) ** 0.5


def is_zero_grad(truth: Result, k: str) -> bool:
    g = truth.grads[k]
    return g is not None and float(g.norm()) < ZERO_REL * grad_rms(truth) * g.numel() ** 0.5


def assess(case, truth: Result, ac: Result, fused: Result):
    """-> (report line, failures, rows): rows = [(tensor, E_fused, E_ac)]."""
    fails, rows = [], []
    rms = grad_rms(truth)

    def one(name, tr, a, f):
        if tr is None or f is None:
            if (tr is None) != (f is None):
                fails.append(f'{name}: gradient is None on one side only (float64 {"None" if tr is None else "tensor"}, fused {"None" if f is None else "tensor"})')
            return
        if tuple(f.shape) != tuple(tr.shape):
            fails.append(f'{name}: shape {tuple(f.shape)} against {tuple(tr.shape)}')
            return
        if not bool(torch.isfinite(f).all()):
            fails.append(f'{name}: not finite')
            return
        if name in truth.grads and is_zero_grad(truth, name):
            r = float(f.pow(2).mean()) ** 0.5
            rows.append((name + '(zero)', r / rms, 0.0))
            if r > ZERO_RMS * rms:
                fails.append(f'{name}: analytically zero, rms {r:.3e} > {ZERO_RMS} x {rms:.3e}')
            return
        if float(tr.norm()) == 0.0:
            if float(f.norm()) != 0.0: fails.append(f'{name}: float64 is exactly zero, fused is not')
            return
        ef, ea = _rel(f, tr), _rel(a, tr)
        rows.append((name, ef, ea))
        bound = max(FACTOR * ea, FLOOR)
        if bound > case.cap:
            fails.append(f'{name}: the inputs give a bound of {bound:.3e} > cap {case.cap:.3e} (E_ac {ea:.3e}): condition the inputs')
        if ef > bound:
            fails.append(f'{name}: E_fused {ef:.3e} > max(2 x {ea:.3e}, 2^-8)')

    for i, (tr, a, f) in enumerate(zip(truth.outs, ac.outs, fused.outs)):
        one(f'y{i}', tr, a, f)
    for k in truth.extras:
        one('buf.' + k, truth.extras[k], ac.extras[k], fused.extras[k])
    for k in case.diff:
        one(k, truth.grads[k], ac.grads[k], fused.grads[k])
    line = f'[block {case.block}] {case.name}: ' + ', '.join(f'{n} {ef:.2e}/{ea:.2e}={ef / ea if ea else float("nan"):.2f}' for n, ef, ea in rows)
    return line, fails, rows


_plain_cache: dict = {}


def plain_results(case):
    """(truth, yardstick) of a case, computed once and shared by every test that needs them."""
    if case.name not in _plain_cache:
        _plain_cache[case.name] = (run_plain(case, False), run_plain(case, True))
    return _plain_cache[case.name]


def check_result(case, fused: Result, tag=''):
    truth, ac = plain_results(case)
    line, fails, rows = assess(case, truth, ac, fused)
    print(line + (f' ({tag})' if tag else ''))
    assert not fails, f'{case.name} {tag}: ' + '; '.join(fails)
    return rows


def check_block(case, Fn, device='cpu'):
    """Mode (a): returned gradients, p.grad starting as None."""
    res = run_fused(case, Fn, device)
    check_result(case, res, 'returned')
    return res


def check_block_direct(case, Fn, device='cpu'):
    """Mode (b): direct accumulation into pre-filled p.grad; the hook fires exactly once per parameter written."""
    truth, _ = plain_results(case)
    res, fired = run_fused(case, Fn, device, direct=True)
    check_result(case, res, 'direct')
    want = sorted(k for k in case.params if truth.grads[k] is not None and k not in case.nondirect)
    assert sorted(fired) == want, (case.name, sorted(fired), want)
    return res


def same_results(a: Result, b: Result, what, exact=(), tol=1e-5, skip=()):
    """b against a: names in `exact` (or all of them when exact is True) torch.equal, the others within tol relative L2."""
    pairs = [(f'y{i}', x, y) for i, (x, y) in enumerate(zip(a.outs, b.outs))] + [(k, a.grads[k], b.grads[k]) for k in a.grads]
    for name, x, y in pairs:
        if name in skip:
            continue
        assert (x is None) == (y is None), (what, name)
        if x is None:
            continue
        if exact is True or name in exact:
            assert torch.equal(x, y), (what, name, float((x - y).abs().max()))
        else:
            n = float(x.norm())
            assert float((x - y).norm()) <= tol * n + 1e-30, (what, name, float((x - y).norm()) / max(n, 1e-30))


# ---- the further gradient modes ------------------------------------------------------------------------------------------------
def _with_dy(case, dy, suffix):
    c = Case(case.name + suffix, case.block, case.tensors, case.params, case.streams, case.fused, case.plain, dy, case.cap)
    c.nondirect = case.nondirect
    return c


def check_noncontiguous_dy(case, Fn, device='cpu'):
    """Mode (d), one dy per used output (case.dy; None: output unused): output gradients of stride 0 (sum of y.sum() over the used
    outputs, backward - what nll.sum().backward() hands head_ctc) and of transposed strides
    (dy.transpose(-1, -2).contiguous().transpose(-1, -2), in the output's dtype) give what contiguous tensors of the same values give
    - within 1e-5 relative L2 (f32 sums of another order at most; the blocks start with dy.contiguous()) - and meet the block's
    bound against float64.  A 1-D output (head_ctc's nll) has no transposed form - .t() changes nothing there - and runs stride 0 only."""
    used = [i for i, d in enumerate(case.dy) if d is not None]
    ones = _with_dy(case, [None if d is None else torch.ones_like(d) for d in case.dy], '-ones')
    ones.cap = float('inf')                     # this dy is set by the mode, not conditioned: the bound holds, the cap on it does not apply
    seen = []

    def start(grads):
        def go(outs):
            for i in used:
                outs[i].register_hook(lambda g: seen.append(g.is_contiguous()))
            if grads is None:
                sum(outs[i].sum() for i in used).backward()
            else:
                torch.autograd.backward([outs[i] for i in used], [grads[i].to(outs[i].device, outs[i].dtype).transpose(-1, -2).contiguous().transpose(-1, -2)
                                                                  for i in used])
        return go

    base1 = run_fused(ones, Fn, device)
    got1 = run_fused(ones, Fn, device, backward=start(None))
    assert seen == [False] * len(used), seen
    same_results(base1, got1, case.name + ' stride-0 dy')
    check_result(ones, got1, 'stride-0 dy')
    if all(case.dy[i].dim() >= 2 for i in used):
        base = run_fused(case, Fn, device)
        got = run_fused(case, Fn, device, backward=start(case.dy))
        assert seen == [False] * (2 * len(used)), seen
        same_results(base, got, case.name + ' transposed dy')
        check_result(case, got, 'transposed dy')


def check_twin_on_off(case, Fn, device, monkeypatch, colsum_biases):
    """A chain with and without the parked twins: dx and every weight gradient torch.equal; the bias gradients that take the
    parked column sums (`colsum_biases`) within 1e-5 relative, since the fixed-order column sums differ from colsum_'s."""
    on = run_fused(case, Fn, device)
    taken = []
    orig = Fn._take_twin
    monkeypatch.setattr(Fn, '_take_twin', lambda dy: (lambda r: (taken.append(r[1] is not None), r)[1])(orig(dy)))
    run_fused(case, Fn, device)
    assert sum(taken) >= len(colsum_biases), (taken, 'the chain did not hand its gradients over through parked twins')
    monkeypatch.setattr(Fn, '_take_twin', orig)
    park = Fn._park_twin
    monkeypatch.setattr(Fn, '_park_twin', lambda dx, dx16, colsum: None)
    off = run_fused(case, Fn, device)
    monkeypatch.setattr(Fn, '_park_twin', park)
    names = [f'y{i}' for i in range(len(on.outs))] + [k for k in on.grads if k not in colsum_biases]
    same_results(on, off, case.name + ' twin on/off', exact=names, tol=1e-5)
    return on, off


def check_stale_twin(case, Fn, device, monkeypatch):
    """ff -> ff from an ff case's tensors.  The first block's backward receives the dx the second one parked a twin of; a hook
    doubles that dx IN PLACE before the first block runs.  The version counter moved, so _take_twin must cast afresh: the first
    block's gradients are those of a run whose hook returns a new tensor 2 * dx (which no twin can match)."""
    calls = []
    orig = Fn._take_twin

    def spy(dy):
        e = Fn._twins.get(dy.data_ptr())
        r = orig(dy)
        calls.append(dict(parked=e is not None, parked_version=None if e is None else e[1], version=dy._version, twin=r[1] is not None))
        return r

    def run(hook):
        Fn.clear_weight_cache(); Fn._twins.clear(); calls.clear()
        t = _leaves(case, F32, device)
        args = [t[k] for k in ('nw', 'nb', 'w1', 'w2', 'b1', 'b2')]
        mid = Fn.ff_block(t['x'], *args, 0.5, 'layer_norm', 1e-5, 0, True)
        y = Fn.ff_block(mid, *args, 0.5, 'layer_norm', 1e-5, 0, True)
        if hook is not None: mid.register_hook(hook)
        y.backward(case.dy[0].to(device))
        return Result([_cpu64(y)], {k: _cpu64(t[k].grad) for k in case.diff}, {}), [dict(c) for c in calls]

    monkeypatch.setattr(Fn, '_take_twin', spy)
    _, plain_calls = run(None)
    assert plain_calls[1]['parked'] and plain_calls[1]['twin'] and plain_calls[1]['version'] == plain_calls[1]['parked_version'], plain_calls
    stale, stale_calls = run(lambda g: (g.mul_(2.0), None)[1])
    c = stale_calls[1]
    assert c['parked'] and c['version'] != c['parked_version'] and not c['twin'], stale_calls       # same memory, newer version: cast afresh
    fresh, fresh_calls = run(lambda g: g * 2.0)
    assert not fresh_calls[1]['parked'] and not fresh_calls[1]['twin'], fresh_calls
    same_results(fresh, stale, case.name + ' stale twin', tol=1e-5)
    Fn._twins.clear()
