"""Componentwise parity of the HIP kernels against float64: an error budget for EVERY element (or a row-local bound for every
row), instead of one number per tensor.  TEST INFRASTRUCTURE, plain importable module (no fixtures, no pytest hooks).

Why: `kernel_test_utils.close` divides the largest error by the largest magnitude of the WHOLE tensor and `block_parity.assess`
is a relative L2 over the whole tensor.  With inputs of one scale an error confined to small elements (a quiet sample's rows, a
cancelled sum, a bias beside a large product), a half-ulp bias (a truncating bf16 store) or a dropped small term passes both.

Truth: kernel_test_utils.ref(name, ..., prec=float64) on the exact bf16 / f32 values the kernel reads.  Where kernel_refs rounds to
bf16 by itself (the saved pre-activation of gemm, gemm_qkv_rotary, gemm_softmax_bwd, attn_fwd, attn_bwd) the truth is the same
formula restated here in float64 without the rounding.  The float64 reference's own error is budgeted where it is not negligible
(_ref_err_x, _ref_err_dgelu: the cancellation in kernel_refs' tanh form of GELU); nothing else is added to a budget.

Metrics
  check_elements   |out - truth| <= budget + ulp_store(|truth| + budget) / 2   for every element.  The budget bounds the error
                   of the f32 value the kernel holds before its store; the second term is the store's round-to-nearest.
  check_rounding   bf16 outputs, over the elements whose budget is <= ulp / 16 (the store rounding dominates there):
                   mean of sign(truth) (out - truth) / ulp within +-0.05, on at least 1e4 elements.  Round-to-nearest-even leaves
                   a residue uniform on [-1/2, 1/2] ulp: mean 0, standard deviation 0.29 / sqrt(n) <= 0.003; the budget adds
                   at most 1/16 ulp of noise to an element, of either sign.  Truncation leaves a residue uniform on [-1, 0]: mean
                   -0.5.  +-0.05 is 17 standard deviations from the first and 0.45 ulp from the second: derived, not fitted.
  check_slices     ops without a closed budget (attention, the norm / softmax backwards): per slice (a row, a column)
                   e = |out - truth|_2 / |truth|_2 <= max(FACTOR e_yardstick, FLOOR) with block_parity's FACTOR = 2, FLOOR = 2^-8
                   and the yardstick kernel_refs in f32 (it never touches the code under test).  A slice whose float64 norm is
                   exactly zero must be exactly zero in the output.

Budgets (u = 2^-23, the relative spacing bound of f32; first-order propagation in float64, class V below)
  accumulation     S = sum_k |a||b| in f64, E_acc = (K + splits) u S.  bf16 x bf16 products are exact in f32; a sum of K terms
                   in ANY order with at most one ulp of relative error per partial sum (round-to-nearest is half of one, a
                   truncating accumulator one) is off by at most (K - 1) u S to first order; each split-K slab is stored and added.
  epilogue         resid + alpha act(acc + bias [, aux]) restated operation by operation from csrc/gemm_tile.h
                   (epi_math_store_at) and csrc/common.h (sigmoidf_, geluf_, gelu_both, dgeluf_, dsiluf_) on V values: every f32
                   operation adds u x the magnitude of its result's operands, v_exp_f32 and v_rcp_f32 one ulp each, the rounded
                   exponent argument |argument| u through d 2^t / dt = ln2 2^t, an f32 constant half an ulp of itself.  An
                   incoming error is carried with the derivative of the operation (|act'| E_pre falls out of this).  A result
                   below the smallest normal may be flushed to zero: every operation also admits 2^-126 absolute.
  reductions       L u sum|x| with L the longest chain of additions, stated next to each case from the kernel's loop.
  cast             budget zero: only the store rounding remains.

Graded inputs (`graded`): normals rounded to bf16; row i of A scaled by 2^((7 i mod 25) - 12), row j of B by 2^((5 j mod 13) - 6);
on every third row of A the second half of K is the negative of the first except the last element, which is halved, and B's
halves are equal, so those true sums are a 2K-th of S and less.  Bias, residual and aux are graded the same way along their axes.
Magnitudes stay within 2^+-40.

Scaling exactness (`check_scaling`): for epilogues without bias, residual or nonlinearity and alpha a power of two,
gemm(D_r A, B D_c) == D_r gemm(A, B) D_c bit for bit with D_r, D_c the power-of-two gradings: every element's arithmetic scales
exactly, so any difference means data crossed between rows or columns.
"""
from __future__ import annotations

import math

import torch

import kernel_refs as R
from block_parity import FACTOR, FLOOR
from kernel_test_utils import BF, F32, F64, ref

U = 2.0 ** -23
TINY = 2.0 ** -126
MANT = {BF: 7, F32: 23}
LOG2E, LN2 = 1.4426950408889634, math.log(2.0)
ROUNDING_MAX_K = 136        # check_rounding needs budget <= ulp / 16 < 2^-11 |truth|: E_acc >= (K + 1) u |truth| leaves none from K = 2^12 on, too few past a few hundred


def _c64(t):
    return t.detach().to('cpu', F64)


def _cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------------ the metrics
def ulp(x, dtype):
    """Spacing of bf16 (2^(floor(log2|x|) - 7)) or f32 (... - 23) at |x|, with |x| floored at the smallest normal."""
    x = torch.as_tensor(x, dtype=F64).abs()
    x = torch.where(torch.isfinite(x), x, torch.full_like(x, TINY)).clamp_min(TINY)
    _, e = torch.frexp(x)                                           # x = m 2^e, m in [1/2, 1): floor(log2 x) = e - 1
    return torch.ldexp(torch.ones_like(x), e - 1 - MANT[dtype])


def _where(ratio):
    i = int(torch.argmax(ratio))
    idx = []
    for s in reversed(ratio.shape):
        idx.append(i % s); i //= s
    return tuple(reversed(idx))


def check_elements(out, truth, budget, store_dtype, name):
    """Every element within budget + half a store ulp; returns the worst err / bound.  Non-finite truths must be met exactly."""
    o, t = _c64(out), _c64(truth)
    assert o.shape == t.shape, f'{name}: shape {tuple(o.shape)} vs {tuple(t.shape)}'
    b = torch.as_tensor(budget, dtype=F64).expand(t.shape)
    fin = torch.isfinite(t)
    assert torch.equal(o[~fin], t[~fin]), f'{name}: non-finite values differ'
    assert bool(torch.isfinite(o[fin]).all()), f'{name}: non-finite output'
    assert bool(torch.isfinite(b[fin]).all()) and bool((b[fin] >= 0).all()), f'{name}: the budget itself is not finite'
    bound = b + 0.5 * ulp(t.abs() + b, store_dtype)
    z = torch.zeros_like(t)
    ratio = torch.where(fin, (torch.where(fin, o, z) - torch.where(fin, t, z)).abs() / bound, z)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if worst > 1.0:
        at = _where(ratio)
        raise AssertionError(f'{name}: element {at} out {float(o[at])!r} truth {float(t[at])!r} err/bound {worst:.3g}; '
                             f'{float((ratio > 1).double().mean()):.3%} of the elements over the bound')
    return worst


def check_rounding(out, truth, budget, name):
    """Signed rounding statistic of a bf16 output (see the module docstring); returns it."""
    o, t = _c64(out), _c64(truth)
    b = torch.as_tensor(budget, dtype=F64).expand(t.shape)
    un = ulp(t, BF)
    sel = torch.isfinite(t) & (t.abs() >= TINY) & (b <= un / 16)
    n = int(sel.sum())
    assert n >= 10 ** 4, f'{name}: only {n} elements whose budget is <= ulp / 16'
    stat = float((torch.sign(t) * (o - t) / un)[sel].mean())
    assert abs(stat) <= 0.05, f'{name}: signed rounding statistic {stat:+.4f} over {n} elements (RNE 0, truncation -0.5)'
    return stat


def check_slices(out, truth, yardstick, axis_spec, name, terms=None):
    """axis_spec: the dimensions that make up ONE slice (the norms run over them); every other index names a slice.
    terms (optional, same shape as truth): the magnitude of the summands of every element.  A slice can be exactly zero in float64
    because nothing contributes to it (padding: terms are zero too, and the output must be exactly zero) or because its summands
    cancel exactly (a query row that sees ONE key: P = 1, dS = dP - delta = 0, dq = 0).  The second kind is roundoff of those
    summands in any f32 evaluation, the yardstick included (measured on the CPU: up to 0.25 where the summands are 2^20), so
    it is held to the same rule with the norm of the summands in the place of the norm of their sum."""
    o, t, y = _c64(out), _c64(truth), _c64(yardstick)
    assert o.shape == t.shape == y.shape, f'{name}: shapes {tuple(o.shape)} {tuple(t.shape)} {tuple(y.shape)}'
    assert bool(torch.isfinite(o).all()), f'{name}: non-finite output'
    d = tuple(axis_spec)
    nt = t.pow(2).sum(d).sqrt()
    zero = nt == 0
    if terms is not None:
        ns = _c64(terms).pow(2).sum(d).sqrt()
        nt = torch.where(zero, ns, nt)                              # cancelled slices: relative to their summands
        zero = nt == 0
    bad = zero & (o.abs().amax(d) != 0) if d else zero & (o.abs() != 0)
    assert not bool(bad.any()), f'{name}: slice {_where(bad.double())} is exactly zero in float64 and not zero in the output'
    safe = torch.where(zero, torch.ones_like(nt), nt)
    e = (o - t).pow(2).sum(d).sqrt() / safe
    ey = (y - t).pow(2).sum(d).sqrt() / safe
    ratio = torch.where(zero, torch.zeros_like(e), e / torch.clamp_min(FACTOR * ey, FLOOR))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if worst > 1.0:
        at = _where(ratio)
        raise AssertionError(f'{name}: slice {at} rel L2 {float(e[at]):.3e} vs yardstick {float(ey[at]):.3e}: err/bound {worst:.3g}; '
                             f'{float((ratio > 1).double().mean()):.3%} of the slices over the bound')
    return worst


def report(name, **figs):
    """One line per case in the style of block_parity's report."""
    print(f'[componentwise] {name}: ' + ' '.join(f'{k}={v:.3g}' for k, v in figs.items()))


# ------------------------------------------------------------------------------------------- first-order error propagation in f64
class V:
    """A float64 value and a bound on the absolute error of the f32 quantity the kernel holds for it."""

    def __init__(self, val, err=None):
        self.val = torch.as_tensor(val, dtype=F64)
        self.err = torch.zeros_like(self.val) if err is None else torch.as_tensor(err, dtype=F64)

    @staticmethod
    def of(x):
        return x if isinstance(x, V) else V(x)

    @staticmethod
    def const(c):                                                   # an f32 literal of the kernel: half an ulp from the real number
        return V(torch.tensor(float(c), dtype=F64), torch.tensor(abs(float(c)) * U / 2, dtype=F64))

    def __add__(self, o):
        o = V.of(o)
        return V(self.val + o.val, self.err + o.err + U * (self.val.abs() + o.val.abs()) + TINY)

    def __sub__(self, o):
        o = V.of(o)
        return V(self.val - o.val, self.err + o.err + U * (self.val.abs() + o.val.abs()) + TINY)

    def __mul__(self, o):
        o = V.of(o)
        p = self.val * o.val
        return V(p, self.val.abs() * o.err + o.val.abs() * self.err + U * p.abs() + TINY)

    def scaled(self, c):                                            # times an exactly representable scalar (alpha, 1 / d is NOT one)
        return self * V(torch.tensor(float(c), dtype=F64))

    def exp2(self):                                                 # v_exp_f32: one ulp; +inf is exact (common.h)
        r = torch.exp2(self.val)
        e = torch.where(torch.isinf(r), torch.zeros_like(r), r * (LN2 * self.err + U) + TINY)
        return V(r, e)

    def rcp(self, ulps=1):                                          # v_rcp_f32: one ulp; rcp(inf) = 0 exactly
        r = 1.0 / self.val
        inf = torch.isinf(self.val)
        rel = torch.where(inf, torch.zeros_like(r), self.err / self.val.abs())
        return V(r, torch.where(inf, torch.zeros_like(r), r.abs() * (rel + ulps * U) + TINY))

    def sqrt(self, ulps=2):
        r = torch.sqrt(self.val)
        return V(r, 0.5 * self.err / r.clamp_min(TINY) + ulps * U * r + TINY)

    def rsqrt(self, ulps=2):
        r = torch.rsqrt(self.val)
        return V(r, r * (0.5 * self.err / self.val + ulps * U) + TINY)

    def log2(self):                                                 # v_log_f32: one ulp of the result
        r = torch.log2(self.val)
        return V(r, self.err / (self.val * LN2) + U * r.abs() + TINY)

    def sum(self, dim, chain, keepdim=False):
        """Sum along `dim` by a tree whose longest chain of additions is `chain`."""
        return V(self.val.sum(dim, keepdim=keepdim), self.err.sum(dim, keepdim=keepdim) + chain * U * self.val.abs().sum(dim, keepdim=keepdim) + TINY)


def v_sigmoid(x):                                                   # common.h sigmoidf_: rcp(1 + exp2(-log2e x))
    return (V(1.0) + (V.const(-LOG2E) * x).exp2()).rcp()


def v_gelu_both(x):                                                 # common.h gelu_both (geluf_ is its first half)
    c2 = V.const(2 * 0.7978845608028654)
    x2 = x * x
    z = x * (V(1.0) + V.const(0.044715) * x2)
    s = (V(1.0) + (V.const(-2 * 0.7978845608028654 * LOG2E) * z).exp2()).rcp()
    g = x * s
    dg = s + g * (V(1.0) - s) * c2 * (V(1.0) + V.const(3 * 0.044715) * x2)
    return g, dg


def v_dgelu(x):                                                     # common.h dgeluf_
    c2 = V.const(2 * 0.7978845608028654)
    x2 = x * x
    z = x * (V(1.0) + V.const(0.044715) * x2)
    s = (V(1.0) + (V.const(-2 * 0.7978845608028654 * LOG2E) * z).exp2()).rcp()
    return s + x * s * (V(1.0) - s) * c2 * (V(1.0) + V.const(3 * 0.044715) * x2)


def v_dsilu(x):                                                     # common.h dsiluf_
    s = v_sigmoid(x)
    return s * (V(1.0) + x * (V(1.0) - s))


def v_epilogue(v, bias=None, resid=None, aux=None, act='none', alpha=1.0):
    """gemm_tile.h epi_math_store_at on V values: returns (the value stored to C, the value stored to pre or None)."""
    pre = None
    if bias is not None: v = v + V(_c64(bias))
    if act == 'gelu_dsave': v, pre = v_gelu_both(v)
    else: pre = v
    if act == 'mulaux': v = v * V(_c64(aux))
    elif act == 'gelu': v = v_gelu_both(v)[0]
    elif act == 'silu': v = v * v_sigmoid(v)
    elif act == 'dgelu': v = v * v_dgelu(V(_c64(aux)))
    elif act == 'dsilu': v = v * v_dsilu(V(_c64(aux)))
    if alpha != 1.0 or resid is not None:
        v = v.scaled(alpha)
        if resid is not None: v = v + V(_c64(resid))
    return v, pre


# ------------------------------------------------------------------------------------------------------------------ graded inputs
def scale_rows(n):
    return torch.ldexp(torch.ones(n, dtype=F64), (7 * torch.arange(n)) % 25 - 12)


def scale_cols(n):
    return torch.ldexp(torch.ones(n, dtype=F64), (5 * torch.arange(n)) % 13 - 6)


def graded(M, N, K, layout='nt', seed=0, unit=False):
    """The operands of a graded product, in the memory layout of `layout`; unit: the same values before the row scalings."""
    g = torch.Generator().manual_seed(seed + M + N + K)
    A = torch.randn(M, K, generator=g).to(BF).double()
    B = torch.randn(N, K, generator=g).to(BF).double()
    h = K // 2
    A[::3, h:2 * h] = -A[::3, :h]
    A[::3, 2 * h - 1] *= 0.5
    B[:, h:2 * h] = B[:, :h]
    if not unit:
        A = A * scale_rows(M)[:, None]; B = B * scale_cols(N)[:, None]
    A, B = A.to(BF), B.to(BF)
    if layout == 'nt': return A, B
    if layout == 'nn': return A, B.t().contiguous()
    return A.t().contiguous(), B.t().contiguous()


def graded_vec(N, seed=2):
    g = torch.Generator().manual_seed(seed + N)
    return (torch.randn(N, generator=g).double() * scale_cols(N)).float()


def graded_mat(M, N, dtype=F32, seed=3):
    g = torch.Generator().manual_seed(seed + M + N)
    return (torch.randn(M, N, generator=g).to(dtype).double() * scale_rows(M)[:, None] * scale_cols(N)[None, :]).to(dtype)


def logical(a, b, layout):
    """(M, K) and (N, K) float64 views of the operands."""
    a, b = _c64(a), _c64(b)
    if layout == 'nt': return a, b
    if layout == 'nn': return a, b.t()
    return a.t(), b.t()


# ---------------------------------------------------------------------------------------------------------------------- the GEMM
def _ref_err_x(x):
    """The float64 reference's own error where kernel_refs cancels: 0.5 x (1 + tanh(.)) and x (1 - sigmoid(x)) lose 2^-53 of 1
    times |x| while the function is not saturated (|x| < 64 with room; past that both sides are exactly 0 or x)."""
    return 2.0 ** -50 * x.abs().clamp_max(64.0)


def _ref_err_dgelu(x):
    """Likewise kernel_refs._dgelu: 0.5 (1 + t) + 0.5 x (1 - t^2) k (1 + 0.134 x^2), unsaturated for |x| < 8."""
    m = x.abs().clamp_max(8.0)
    return 2.0 ** -50 * (1 + m + 0.134 * m ** 3)


def gemm_expect(a, b, layout='nt', bias=None, resid=None, aux=None, act='none', alpha=1.0, out_dtype=BF, save_pre=False, split_k=1,
                accum=None):
    """[(truth, budget, store dtype)] for the output, then for the saved pre-activation / gelu' if the call returns one.
    accum (its value BEFORE the call): C += alpha A B, the residual form of the same epilogue."""
    A, B = logical(a, b, layout)
    K = A.shape[1]
    acc = V(A @ B.t(), (K + split_k) * U * (A.abs() @ B.abs().t()))
    if accum is not None: resid, out_dtype = accum.reshape(acc.val.shape), F32
    v, pre = v_epilogue(acc, bias, resid, aux, act, alpha)
    kw = dict(bias=bias, resid=resid, aux=aux, act=act, alpha=alpha, out_dtype=out_dtype)
    truth = ref('gemm', a, b, layout, **kw)
    x = ref('gemm', a, b, layout, bias=bias, out_dtype=F32)                         # acc + bias, unrounded
    e_out, e_pre = v.err, pre.err
    if act in ('gelu', 'gelu_dsave'): e_out = e_out + abs(alpha) * _ref_err_x(x)
    elif act == 'dgelu': e_out = e_out + (alpha * x).abs() * _ref_err_dgelu(_c64(aux))
    elif act == 'dsilu': e_out = e_out + (alpha * x).abs() * _ref_err_x(_c64(aux))
    res = [(truth, e_out, out_dtype)]
    if save_pre or act == 'gelu_dsave':
        if act == 'gelu_dsave':
            e_pre, x = e_pre + _ref_err_dgelu(x), R._dgelu(x)
        res.append((x, e_pre, BF))
    return res


def check_gemm(gemm, dev, a, b, layout, name, rounding=True, **kw):
    """Run `gemm` (the op or its stand-in) and check every output; returns {figure: value} for the report."""
    exp = gemm_expect(a, b, layout, **kw)
    kd = {k: (dev(v.clone()) if k == 'accum' else dev(v)) for k, v in kw.items()}
    out = gemm(dev(a), dev(b), layout, **kd)
    outs = out if isinstance(out, tuple) else (out,)
    assert len(outs) == len(exp), f'{name}: {len(outs)} outputs, {len(exp)} expected'
    figs = {}
    for i, (o, (t, bud, sd)) in enumerate(zip(outs, exp)):
        tag = ('out', 'pre')[i]
        assert o.dtype == sd, f'{name} {tag}: dtype {o.dtype}'
        figs[tag] = check_elements(o, t, bud, sd, f'{name} {tag}')
        if sd == BF and rounding:
            figs[tag + '_rnd'] = check_rounding(o, t, bud, f'{name} {tag}')
    report(name, **figs)
    return figs, outs


def check_scaling(gemm, dev, M, N, K, layout, name, seed=0, **kw):
    a, b = graded(M, N, K, layout, seed)
    a0, b0 = graded(M, N, K, layout, seed, unit=True)
    out, out0 = gemm(dev(a), dev(b), layout, **kw), gemm(dev(a0), dev(b0), layout, **kw)
    want = _c64(out0) * scale_rows(M)[:, None] * scale_cols(N)[None, :]
    same = _c64(out) == want
    assert bool(same.all()), f'{name}: {int((~same).sum())} elements differ from the scaled unit product, first at {_where((~same).double())}'


EPILOGUES = [dict(bias=True), dict(bias=True, act='gelu', save_pre=True), dict(bias=True, act='gelu_dsave', save_pre=True),
             dict(aux=True, act='mulaux', alpha=0.5), dict(act='silu'), dict(aux=True, act='dgelu', alpha=0.5), dict(aux=True, act='dsilu'),
             dict(bias=True, resid=True, alpha=0.5, out_dtype=F32), dict(resid=True, out_dtype=F32)]      # test_gemm_epilogues' list


def epilogue_inputs(kw, M, N):
    kw = dict(kw)
    if kw.get('bias'): kw['bias'] = graded_vec(N)
    if kw.get('resid'): kw['resid'] = graded_mat(M, N, F32, 3)
    if kw.get('aux'): kw['aux'] = graded_mat(M, N, BF, 4)
    return kw


# ------------------------------------------------------------------------------------------------------ qkv rotary, softmax backward
def qkv_rotary_expect(x, w, bias, cos, sin, N, H, D, two_pass=False):
    """kernel_refs.gemm_qkv_rotary restated on V values (it rounds to bf16 by itself): the rotation is two products and a sum.
    two_pass: the shape is not taken by the 256-row kernel's rotary epilogue, and sconf_gemm_qkv_rotary (csrc/gemm.hip, its last
    three statements: sconf_gemm_bf16 into C, then sconf_rotary_inplace on C) stores the product as bf16 before it rotates:
    q and k carry half a bf16 ulp more into the rotation (the v block is not rotated: the store is its only rounding)."""
    A, B = _c64(x), _c64(w)
    K = A.shape[1]
    y = V(A @ B.t(), (K + 1) * U * (A.abs() @ B.abs().t()))
    if bias is not None: y = y + V(_c64(bias))
    if two_pass:
        e = y.err + 0.5 * ulp(y.val.abs() + y.err, BF)
        e.view(A.shape[0], 3, -1)[:, 2] = y.err.view(A.shape[0], 3, -1)[:, 2]
        y = V(y.val, e)
    M = A.shape[0]
    val, err = y.val.view(M // N, N, 3, H, D).clone(), y.err.view(M // N, N, 3, H, D).clone()
    c, s = V(_c64(cos).view(1, N, 1, D // 2)), V(_c64(sin).view(1, N, 1, D // 2))
    for wch in (0, 1):
        p = V(val[:, :, wch, :, :D // 2].clone(), err[:, :, wch, :, :D // 2].clone())
        q = V(val[:, :, wch, :, D // 2:].clone(), err[:, :, wch, :, D // 2:].clone())
        lo, hi = p * c - q * s, q * c + p * s
        val[:, :, wch, :, :D // 2], err[:, :, wch, :, :D // 2] = lo.val, lo.err
        val[:, :, wch, :, D // 2:], err[:, :, wch, :, D // 2:] = hi.val, hi.err
    return val.view(M, 3 * H * D), err.view(M, 3 * H * D)


def softmax_bwd_gemm_expect(dy, wt, probs, delta):
    """dl = p (dp - delta): truth in f64, budget |p| (E_dp + u (|dp| + |delta|))."""
    A, B = _c64(dy), _c64(wt)
    dp = A @ B.t()
    E = (A.shape[1] + 1) * U * (A.abs() @ B.abs().t())
    p, dl = _c64(probs), _c64(delta)[:, None]
    return p * (dp - dl), p.abs() * (E + U * (dp.abs() + dl.abs()))


# ------------------------------------------------------------------------------------------------------------------- reductions
def rowdot_expect(a, b, bias):
    """rowdot_kernel: a lane adds 8 products per load and loads every 512 columns, wave_sum adds 6 levels:
    L = 8 ceil(d / 512) + 6 (22 at d = 776)."""
    d = a.shape[-1]
    y = V(_c64(b)) - V(_c64(bias)) if bias is not None else V(_c64(b))
    s = (V(_c64(a)) * y).sum(-1, 8 * _cdiv(d, 512) + 6)
    return ref('rowdot', a, b, bias), s.err


def colsum_geometry(M, N):
    """colsum_geo of csrc/elementwise.hip: column blocks of 256, rb row blocks of rpb rows each."""
    cb = _cdiv(N, 256)
    rb = max(1, min(_cdiv(M, 64), 2048 // cb))
    rpb = _cdiv(M, rb)
    return cb, _cdiv(M, rpb), rpb


def colsum_chain(M, N):
    """colsum_kernel: a thread adds every fourth row of its row block (ceil(rpb / 4) additions), then the four row lanes' sums
    (3); with more than one row block the same kernel adds the rb partial rows the same way (ceil(rb / 4) + 3).
    M, N = 1234, 72: rb = 20, rpb = 62, L = 16 + 3 + 5 + 3 = 27."""
    _, rb, rpb = colsum_geometry(M, N)
    return _cdiv(rpb, 4) + 3 + (_cdiv(rb, 4) + 3 if rb > 1 else 0)


def colsum_expect(x, out0, alpha):
    """L u sum|x| with L = colsum_chain, then alpha v + out."""
    xv = V(_c64(x).reshape(-1, x.shape[-1]))
    s = xv.sum(0, colsum_chain(*xv.val.shape)).scaled(alpha) + V(_c64(out0))
    return ref('colsum_', x, out0.clone(), alpha), s.err


def sumsq_chain(n):
    """sumsq_kernel of csrc/optim.hip on min(ceil(n / 1024), 2048) workgroups of 256 threads: a thread adds four squares and
    their sum to its accumulator per pass (4 additions; ceil(n / (4 * 256 * workgroups)) passes), block_sum adds 6 wave levels
    and the 4 waves; the workgroups' sums are added in float64.  n = 70040: 69 workgroups, one pass, L = 4 + 10 = 14."""
    blocks = min(_cdiv(n, 1024), 2048)
    return 4 * _cdiv(n, 1024 * blocks) + 10


def sumsq_expect(g, out0):
    """L u sum g^2 with L = sumsq_chain, each square one rounding; out is float64 and takes the sum without a further f32 rounding."""
    gv = V(_c64(g).reshape(-1))
    s = (gv * gv).sum(0, sumsq_chain(gv.val.numel()))
    return _c64(out0) + (_c64(g) ** 2).sum(), s.err


# ---------------------------------------------------------------------------------------------------------------------- softmax
def softmax_expect(x, log, out_dtype):
    """softmax_fwd_kernel: v - max (exact inputs), __expf = exp2(v log2e), the row sum by 4 additions per thread and pass of 1024 columns, 6 wave
    levels and 4 waves (L = 4 ceil(C / 1024) + 10), inv = 1 / s (two ulps), ls = log2(s) ln2."""
    xv = _c64(x)
    C = xv.shape[-1]
    v = V(xv) - V(xv.amax(-1, keepdim=True))
    e = (v * V.const(LOG2E)).exp2()
    s = e.sum(-1, 4 * _cdiv(C, 1024) + 10, keepdim=True)
    y = v - s.log2() * V.const(LN2) if log else e * s.rcp(2)
    return ref('softmax_fwd', x, log, out_dtype), y.err


# ------------------------------------------------------------------------------------------------------------------------- norms
def norm_expect(x, w, b, mode, eps):
    """norm_fwd_kernel: a lane adds 4 values per pass of 256 columns, wave_sum 6 levels (L = 4 ceil(d / 256) + 6) for the sum and for the sum of squares;
    mean = s / d, rstd = rsqrt(q / d + eps) (rms_norm: 1 / (sqrt(q / d) + eps)), y = (v - mean) rstd w + b.
    Returns ((y, E_y), (mean, E_mean), (rstd, E_rstd)) with float64 truths."""
    xv = V(_c64(x))
    d = xv.val.shape[-1]
    L = 4 * _cdiv(d, 256) + 6
    inv_d = V.const(1.0 / d)
    if mode == 'layer_norm':
        mean = xv.sum(-1, L, keepdim=True) * inv_d
        t = xv - mean
        rstd = ((t * t).sum(-1, L, keepdim=True) * inv_d + V(eps)).rsqrt()
    else:
        mean = V(torch.zeros_like(xv.val[..., :1]))
        t = xv
        q = (t * t).sum(-1, L, keepdim=True) * inv_d
        rstd = (q.sqrt() + V(eps)).rcp(2) if mode == 'rms_norm' else (q + V(eps)).rsqrt()
    y = t * rstd * V(_c64(w))
    if mode == 'layer_norm' and b is not None: y = y + V(_c64(b))
    ty, tm, tr = ref('norm_fwd', x, w, b, mode, eps, F32)
    return (ty, y.err), (tm, mean.err.reshape(-1)), (tr, rstd.err.reshape(-1))


# --------------------------------------------------------------------------------------------------------------------- attention
def attention_inputs(B, N, H, D, seed=0):
    """q, k unit normals; v and dout scaled by 2^e per (sample, head), e from -10 (the LAST sample, the shortest in every case of
    the tests) to 10, so that the shortest sample is also the quietest."""
    def rn(s):
        g = torch.Generator().manual_seed(seed + s + B + N + H + D)
        return torch.randn(B, N, H, D, generator=g)
    e = torch.linspace(10, -10, B * H).round().view(B, 1, H, 1)
    sc = torch.ldexp(torch.ones(B, 1, H, 1), e.to(torch.int32))
    return rn(0).to(BF), rn(1).to(BF), (rn(2) * sc).to(BF), (rn(3) * sc).to(BF)


# ------------------------------------------------------------------------------- the cases, shared by the CPU and the GPU tests
# Each runner takes the op namespace (lcasr_amd.hip.ops, or kernel_refs as the f32 stand-in) and the function that moves a
# tensor to where that namespace computes.
def rot_tables(N, D):
    inv = 1.0 / (1500000 ** (torch.arange(0, D, 2).float() / D))
    f = torch.arange(N).float()[:, None] * inv[None]
    return torch.cos(f).contiguous(), torch.sin(f).contiguous()


def run_qkv_rotary(ops, dev, Bn, N, H, K, epilogue=None):
    """epilogue: None (the stand-in: one rounding), True / False: the 256-row kernel's rotary epilogue must / must not take the shape."""
    D = 128
    x, w = graded(Bn * N, 3 * H * D, K, 'nt', seed=11)
    cos, sin = rot_tables(N, D)
    out = ops.gemm_qkv_rotary(dev(x), dev(w), None, dev(cos), dev(sin), N, H, D)
    if epilogue is not None:                                        # which path ran: the two-launch one equals its parts bit for bit
        two = ops.rotary_inplace_(ops.gemm(dev(x), dev(w), 'nt'), dev(cos), dev(sin), Bn, N, H, D)
        assert torch.equal(out, two) != epilogue, 'rotary epilogue taken' if not epilogue else 'rotary epilogue NOT taken'
    truth, bud = qkv_rotary_expect(x, w, None, cos, sin, N, H, D, two_pass=epilogue is False)
    name = f'gemm_qkv_rotary {(Bn, N, H, K)}' + {None: '', True: ' epilogue', False: ' two launches'}[epilogue]
    figs = dict(out=check_elements(out, truth, bud, BF, name))
    if K <= ROUNDING_MAX_K and epilogue is not False: figs['rnd'] = check_rounding(out, truth, bud, name)
    report(name, **figs)
    return figs


def softmax_bwd_gemm_inputs(M, V_, K):
    g = torch.Generator().manual_seed(M + V_ + K)
    probs = torch.softmax(torch.randn(M, V_, generator=g) * 2.0 * scale_rows(M)[:, None].float().clamp(2.0 ** -3, 2.0 ** 2), -1).to(BF)
    dy, wt = graded(M, V_, K, 'nt', seed=13)
    dp = dy.double() @ wt.double().t()
    delta = (probs.double() * dp).sum(-1).float().contiguous()
    return dy, wt, probs, delta


def run_gemm_softmax_bwd(ops, dev, M, V_, K):
    dy, wt, probs, delta = softmax_bwd_gemm_inputs(M, V_, K)
    out = ops.gemm_softmax_bwd(dev(dy), dev(wt), dev(probs), dev(delta))
    truth, bud = softmax_bwd_gemm_expect(dy, wt, probs, delta)
    name = f'gemm_softmax_bwd {(M, V_, K)}'
    figs = dict(out=check_elements(out, truth, bud, BF, name))
    report(name, **figs)
    return figs


def run_reductions(ops, dev):
    figs = {}
    M, d = 1029, 776
    a, b, bias = graded_mat(M, d, BF, 5), graded_mat(M, d, BF, 6), graded_vec(d, 7)
    for bs in (None, bias):
        t, bud = rowdot_expect(a, b, bs)
        figs[f'rowdot{"" if bs is None else "_bias"}'] = check_elements(ops.rowdot(dev(a), dev(b), dev(bs)), t, bud, F32, 'rowdot')
    for dt in (BF, F32):
        x, out0 = graded_mat(1234, 72, dt, 8), graded_vec(72, 9)
        t, bud = colsum_expect(x, out0, 0.5)
        figs[f'colsum_{dt}'.replace('torch.', '')] = check_elements(ops.colsum_(dev(x), dev(out0.clone()), 0.5), t, bud, F32, f'colsum_ {dt}')
    g = graded_mat(515, 136, F32, 10)
    out0 = torch.ones((), dtype=F64)
    t, bud = sumsq_expect(g, out0)
    got = ops.sumsq_(dev(g), dev(out0.clone()))
    blocks = min(_cdiv(g.numel(), 1024), 2048)                      # their float64 sums are added one after the other
    figs['sumsq'] = float(((_c64(got) - t).abs() / (bud + (blocks + 1) * 2.0 ** -53 * t.abs())).max())
    assert figs['sumsq'] <= 1.0, f'sumsq_: err/bound {figs["sumsq"]:.3g}'
    report('reductions', **figs)
    return figs


def cast_input():
    """Graded normals, then values ON bf16 ties (odd and even neighbours), just beside them, +-0 and +-inf."""
    x = graded_mat(515, 136, F32, 12).reshape(-1)
    base = torch.tensor([1.0, 1.0078125, -3.0, 2.0 ** -20, 2.0 ** 30 * 1.5], dtype=F64)       # bf16 values
    half = ulp(base, BF) / 2
    ties = torch.cat([base + half, base - half, base + half * (1 + 2.0 ** -15), base + half * (1 - 2.0 ** -15)]).float()
    special = torch.tensor([0.0, -0.0, float('inf'), float('-inf')])
    return torch.cat([x, ties, special])


def run_cast(ops, dev):
    x = cast_input()
    got = ops.cast(dev(x), BF)
    figs = dict(to_bf16=check_elements(got, x.double(), 0.0, BF, 'cast f32->bf16'), rnd=check_rounding(got, x.double(), 0.0, 'cast f32->bf16'))
    assert torch.equal(got.cpu().view(torch.int16), x.to(BF).view(torch.int16)), 'cast f32->bf16: bits (ties to even, signed zeros)'
    back = ops.cast(dev(x.to(BF)), F32)
    assert torch.equal(back.cpu().view(torch.int32), x.to(BF).float().view(torch.int32)), 'cast bf16->f32 is exact'
    report('cast', **figs)
    return figs


def softmax_input(C, dtype):
    M = 37
    g = torch.Generator().manual_seed(C)
    sc = torch.tensor([0.25, 1.0, 3.0, 8.0])[torch.arange(M) % 4][:, None]
    sh = torch.tensor([-80.0, 0.0, 80.0])[torch.arange(M) % 3][:, None]
    return (torch.randn(M, C, generator=g) * sc + sh).to(dtype)


def run_softmax_fwd(ops, dev, C):
    figs = {}
    for log, xd, yd in ((False, BF, BF), (True, F32, F32), (False, F32, F32)):
        x = softmax_input(C, xd)
        t, bud = softmax_expect(x, log, yd)
        name = f'softmax_fwd C={C} log={log} {xd}->{yd}'
        if not log:
            assert float(t.min()) < 2.0 ** -60 and bool((bud <= 2.0 ** -9 * t + TINY * 64).all()), 'probabilities are budgeted relative to themselves'
        figs[f'{"log" if log else "p"}_{"bf16" if yd == BF else "f32"}'] = check_elements(ops.softmax_fwd(dev(x), log, yd), t, bud, yd, name)
    report(f'softmax_fwd C={C}', **figs)
    return figs


def norm_inputs(M, d, xd):
    x = graded_mat(M, d, xd, 14)
    return x, graded_vec(d, 15), graded_vec(d, 16)


def run_norm_fwd(ops, dev, mode, d, M=515):
    eps = 1e-8 if mode == 'rms_norm' else 1e-5
    figs = {}
    for xd, yd in ((F32, BF), (F32, F32), (BF, BF)):
        x, w, b = norm_inputs(M, d, xd)
        if mode != 'layer_norm': b = None
        (ty, ey), (tm, em), (tr, er) = norm_expect(x, w, b, mode, eps)
        y, mean, rstd = ops.norm_fwd(dev(x), dev(w), dev(b), mode, eps, yd)
        tag = f'{"bf16" if xd == BF else "f32"}_{"bf16" if yd == BF else "f32"}'
        name = f'norm_fwd {mode} d={d} {tag}'
        figs['y_' + tag] = check_elements(y, ty, ey, yd, name + ' y')
        if mode == 'layer_norm': figs['mean_' + tag] = check_elements(mean, tm, em, F32, name + ' mean')
        figs['rstd_' + tag] = check_elements(rstd, tr, er, F32, name + ' rstd')
    report(f'norm_fwd {mode} d={d}', **figs)
    return figs


ATTN_CASES = [  # B, N, H, D, lengths, window, SCONF_ATTN_WIDE=0 (the 4-wave kernels)
    (3, 192, 2, 32, [192, 100, 7], (-1, -1), False), (2, 260, 2, 128, [260, 131], (-1, -1), False),
    (2, 256, 2, 128, [256, 77], (64, 0), False), (2, 256, 2, 128, [256, 77], (64, 0), True),
    (3, 192, 2, 64, [192, 100, 7], (-1, -1), False), (2, 260, 2, 256, [260, 131], (-1, -1), False),   # head_dim 64, 256: test_head_dims_gpu
]


def attn_fwd_restated(q, k, v, lengths, window, prec, as_kernel):
    """kernel_refs.attn_fwd restated so that its roundings can be chosen.  prec = float64, as_kernel = False: the truth, with NO
    rounding at all (kernel_refs rounds o to bf16 by itself, and a per-row L2 error against a rounded truth is a count of
    elements that flipped to the neighbouring bf16 value: a discontinuous, heavy-tailed statistic on rows of 32 - 256 elements).
    prec = float32, as_kernel = True: the yardstick, with the kernels' rounding points - P = exp(s - reference) is packed to bf16
    for the PV MFMA (csrc/attention.hip pack8: `pf[kt][..] = pack8(s[kt], ..)`, `plo = pack8(sb, 0)`), the row sum l stays f32
    and divides at the end, o is stored as bf16."""
    B, N, H, D = q.shape
    q, k, v = q.to(prec), k.to(prec), v.to(prec)
    s = torch.einsum('bihd,bjhd->bhij', q, k) * D ** -0.5
    s = s.masked_fill(~R._attn_mask(B, N, lengths, window, q.device)[:, None], float('-inf'))
    m = s.amax(-1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    p = torch.exp(s - m)
    l = p.sum(-1)
    pv = p.to(BF).to(prec) if as_kernel else p
    o = torch.einsum('bhij,bjhd->bihd', pv, v) / l.permute(0, 2, 1)[..., None]
    lse = m.squeeze(-1) + torch.log(l)
    qpad = torch.arange(N)[None, :] >= lengths[:, None]
    o = torch.nan_to_num(o, nan=0.0).masked_fill(qpad[:, :, None, None], 0.0).contiguous()
    return (o.to(BF) if as_kernel else o), lse.masked_fill(qpad[:, None, :], float('inf')).contiguous()


def attn_bwd_restated(q, k, v, o, dout, lse, lengths, window, prec, as_kernel):
    """kernel_refs.attn_bwd restated likewise.  as_kernel: P = exp(s - lse) and dS = P (dP - delta) are packed to bf16 for the dV
    and the dQ / dK MFMAs (csrc/attention.hip: `pb0 = pack8(s, 0) ... db0 = pack8(dp, 0)` in the dK/dV kernels, `d0 = pack8(dp, 0)`
    in the dQ kernels), delta = rowsum(dO O) comes from the bf16 O handed in (delta_from_frags), the gradients are stored as bf16.
    The truth takes the unrounded float64 o and lse of attn_fwd_restated."""
    B, N, H, D = q.shape
    sc = D ** -0.5
    q, k, v, o, g, lse = q.to(prec), k.to(prec), v.to(prec), o.to(prec), dout.to(prec), lse.to(prec)
    s = torch.einsum('bihd,bjhd->bhij', q, k) * sc
    s = s.masked_fill(~R._attn_mask(B, N, lengths, window, q.device)[:, None], float('-inf'))
    p = torch.nan_to_num(torch.exp(s - lse[..., None]), nan=0.0, posinf=0.0)
    g = g.masked_fill((torch.arange(N)[None, :] >= lengths[:, None])[:, :, None, None], 0.0)
    delta = (g * o).sum(-1).permute(0, 2, 1)[..., None]
    ds = p * (torch.einsum('bihd,bjhd->bhij', g, v) - delta)
    pb, dsb = (p.to(BF).to(prec), ds.to(BF).to(prec)) if as_kernel else (p, ds)
    dv = torch.einsum('bhij,bihd->bjhd', pb, g)
    dq = torch.einsum('bhij,bjhd->bihd', dsb, k) * sc
    dk = torch.einsum('bhij,bihd->bjhd', dsb, q) * sc
    if as_kernel: return tuple(t.contiguous().to(BF) for t in (dq, dk, dv))
    dq_terms = torch.einsum('bhij,bjhd->bihd', p * (torch.einsum('bihd,bjhd->bhij', g, v).abs() + delta.abs()), k.abs()) * sc
    return dq.contiguous(), dk.contiguous(), dv.contiguous(), dq_terms


def run_attention(ops, dev, case, spoil=None):
    """Forward: o per (b, n, h) row against the unrounded float64 restatement, with the f32 restatement that rounds where the
    kernels do as the yardstick; lse absolute 2e-3 on valid rows.
    Backward: dq, dk, dv per row.  attn_bwd READS o and lse: delta = rowsum(dO o) comes from the bf16 o it is handed
    (csrc/attention.hip delta_from_frags).  So the kernel, the yardstick and the float64 truth are all evaluated on the same
    inputs (q, k, v, o, dout, lse) with o, lse the yardstick forward's bf16 o and f32 lse - the exact values the kernel reads,
    made without the code under test.  (With a truth whose delta comes from the exact o, the bf16 store of o is an error of
    1 - 5 % in dk rows made of one or two cancelling dS values - the last keys under window (64, 0) - and it differs between
    two realisations of that store by more than FACTOR: MI355X, key row (0, 254, 0) 4.86e-2 against the yardstick's 1.61e-2;
    on the CPU the yardstick alone moves between 0.65e-2 and 1.61e-2 there when o is rounded from slightly different values.
    The kernels on their own forward's o and lse are held by test_kernels_gpu.py::test_attention_fwd_bwd.)
    spoil(o) -> o: a planted defect on the forward output (the CPU self-test)."""
    B, N, H, D, lens, win, _ = case
    q, k, v, do = attention_inputs(B, N, H, D)
    ln = torch.tensor(lens, dtype=torch.int32)
    o64, lse64 = attn_fwd_restated(q, k, v, ln, win, F64, False)
    oy, lsey = attn_fwd_restated(q, k, v, ln, win, F32, True)
    for a_, b_ in zip(ref('attn_fwd', q, k, v, ln, win), (o64, lse64)):      # the restated truth IS kernel_refs' before its bf16 store
        fin = torch.isfinite(b_)
        assert torch.equal(torch.isfinite(a_.double()), fin) and bool(((a_.double() - b_)[fin].abs() <= 2.0 ** -8 * b_[fin].abs() + 1e-12).all())
    o, lse = ops.attn_fwd(dev(q), dev(k), dev(v), dev(ln), win)
    if spoil is not None: o = spoil(o)
    name = f'attention {case}'
    figs = dict(o=check_slices(o, o64, oy, (3,), name + ' o'))
    m = torch.isfinite(lse64)
    assert torch.equal(torch.isfinite(_c64(lse)), m), name + ' lse: rows without a key'
    assert float((_c64(lse)[m] - lse64[m]).abs().max()) < 2e-3, name + ' lse'
    for a_, b_ in zip(ref('attn_bwd', q, k, v, o64, do, lse64, ln, win), attn_bwd_restated(q, k, v, o64, do, lse64, ln, win, F64, False)):
        assert bool(((a_.double() - b_).abs() <= 2.0 ** -8 * b_.abs() + 1e-12).all()), 'restated backward against kernel_refs'
    dq64, dk64, dv64, dq_terms = attn_bwd_restated(q, k, v, oy, do, lsey, ln, win, F64, False)
    dqy, dky, dvy = attn_bwd_restated(q, k, v, oy, do, lsey, ln, win, F32, True)
    got = ops.attn_bwd(dev(q), dev(k), dev(v), dev(oy), dev(do), dev(lsey), dev(ln), win)
    for n_, g_, t_, y_ in zip(('dq', 'dk', 'dv'), got, (dq64, dk64, dv64), (dqy, dky, dvy)):
        figs[n_] = check_slices(g_, t_, y_, (3,), f'{name} {n_}', terms=dq_terms if n_ == 'dq' else None)
    report(name, **figs)
    return figs


def run_norm_bwd(ops, dev, mode, d, M=515):
    """dx per row, dweight / dbias per column (axis_spec (): every column is its own slice)."""
    eps = 1e-8 if mode == 'rms_norm' else 1e-5
    x, w, b = norm_inputs(M, d, F32)
    dy, dres = graded_mat(M, d, BF, 17), graded_mat(M, d, F32, 18)
    has_b = mode == 'layer_norm'
    _, m64, r64 = ref('norm_fwd', x, w, b if has_b else None, mode, eps, F32)
    _, my, ry = R.norm_fwd(x, w, b if has_b else None, mode, eps, F32)
    z64 = lambda: torch.zeros(d, dtype=F64)
    dw64, db64 = z64(), z64()
    dx64 = ref('norm_bwd', dy, x, w, m64, r64, mode, eps, dres, F32, dw64, db64 if has_b else None)
    dwy, dby = torch.zeros(d), torch.zeros(d)
    dxy = R.norm_bwd(dy, x, w, my, ry, mode, eps, dres, F32, dwy, dby if has_b else None)
    dw, db = dev(torch.zeros(d)), dev(torch.zeros(d))
    _, mean, rstd = ops.norm_fwd(dev(x), dev(w), dev(b) if has_b else None, mode, eps, F32)
    dx = ops.norm_bwd(dev(dy), dev(x), dev(w), mean, rstd, mode, eps, dev(dres), F32, dw, db if has_b else None)
    name = f'norm_bwd {mode} d={d}'
    figs = dict(dx=check_slices(dx, dx64, dxy, (1,), name + ' dx'), dw=check_slices(dw, dw64, dwy, (), name + ' dweight'))
    if has_b: figs['db'] = check_slices(db, db64, dby, (), name + ' dbias')
    report(name, **figs)
    return figs


def run_softmax_bwd(ops, dev, C, log):
    """dx per row, the fused column sums per column."""
    xd = F32 if log else BF
    y = R.softmax_fwd(softmax_input(C, F32) * 0.125, log, xd)
    dy = graded_mat(y.shape[0], C, xd, 19)
    cs64, csy, cs = torch.zeros(C, dtype=F64), torch.zeros(C), dev(torch.zeros(C))
    t = ref('softmax_bwd', y, dy, log, BF, colsum_into=cs64)
    yd = R.softmax_bwd(y, dy, log, BF, colsum_into=csy)
    got = ops.softmax_bwd(dev(y), dev(dy), log, BF, colsum_into=cs)
    name = f'softmax_bwd C={C} log={log}'
    figs = dict(dx=check_slices(got, t, yd, (1,), name + ' dx'), colsum=check_slices(cs, cs64, csy, (), name + ' column sums'))
    report(name, **figs)
    return figs


def run_norm2_bwd(ops, dev, d, M=515):
    """The two-LayerNorm backward: dx per row, the four parameter gradients per column."""
    x, w1, b1 = norm_inputs(M, d, F32)
    w2, b2 = graded_vec(d, 21), graded_vec(d, 22)
    dh2, dres = graded_mat(M, d, BF, 17), graded_mat(M, d, F32, 18)
    st64 = ref('norm2_fwd', x, w1, b1, w2, b2, 1e-5, 1e-5)[2]
    sty = R.norm2_fwd(x, w1, b1, w2, b2, 1e-5, 1e-5)[2]
    g64, gy, gg = [torch.zeros(d, dtype=F64) for _ in range(4)], [torch.zeros(d) for _ in range(4)], [dev(torch.zeros(d)) for _ in range(4)]
    dx64 = ref('norm2_bwd', dh2, x, w1, b1, w2, b2, st64, dres, *g64)
    dxy = R.norm2_bwd(dh2, x, w1, b1, w2, b2, sty, dres, *gy)
    st = ops.norm2_fwd(dev(x), dev(w1), dev(b1), dev(w2), dev(b2), 1e-5, 1e-5)[2]
    dx = ops.norm2_bwd(dev(dh2), dev(x), dev(w1), dev(b1), dev(w2), dev(b2), st, dev(dres), *gg)
    name = f'norm2_bwd d={d}'
    figs = dict(dx=check_slices(dx, dx64, dxy, (1,), name + ' dx'))
    for n_, a_, t_, y_ in zip(('dw1', 'db1', 'dw2', 'db2'), gg, g64, gy):
        figs[n_] = check_slices(a_, t_, y_, (), f'{name} {n_}')
    report(name, **figs)
    return figs
