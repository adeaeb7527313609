"""Inputs and high-precision references of the launch-geometry parity tests (test_kernel_geometry_gpu.py), shared with the CPU
self-check of those references (test_kernel_geometry_refs.py).  TEST INFRASTRUCTURE, plain importable module.

Every `*_inputs` function returns the CPU tensors one case feeds the kernel (already rounded to the dtypes the kernel reads) and every
`*_ref` function restates the op on them with tests/kernel_refs.py evaluated in a chosen precision (kernel_test_utils.ref): float64
is the reference of the GPU tests, float32 the reference-only error the self-check measures against it."""
import os
import sys

import torch

import kernel_refs as R
from kernel_test_utils import BF, F32, TOL_BF16, TOL_F32, ref, ref_precision, rnd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEFAULT_CUS = 256                                    # MI355X; the GPU tests read the real count from sconf_num_cus()
NORM_WAVES = 8                                       # NBW of csrc/norm.hip: waves per workgroup of the persistent backward kernels


def eps_of(mode):
    return 1e-8 if mode == 'rms_norm' else 1e-5


def rows_for_trips(nw):
    """Rows that give every wave of a persistent kernel with nw row-walking waves 3 trips, the last one ragged (44 % of it live)."""
    return 2 * nw + (7 * nw) // 16 + 3


def norm_bwd_waves(d, cus=DEFAULT_CUS):
    """Row-walking waves of sconf_norm_bwd once its grid is capped at one workgroup per CU (norm.hip launch_bwd: rows wider than
    1024 take a pair of waves each)."""
    return cus * NORM_WAVES // (2 if d > 1024 else 1)


def row_slices(M, nw, rows=40):
    """Row blocks for the bit-identity checks: the first pass, the middle of the second pass, the ragged end of the last one."""
    return [(0, rows), (nw + nw // 2 - rows // 2, nw + nw // 2 + rows // 2), (M - rows + 3, M)]


# ---------------------------------------------------------------------------------------------------------------- norms
def norm_inputs(mode, d, M, xd, gd):
    x = rnd(M, d, dtype=xd, scale=2.0) + 0.5
    w = rnd(d, dtype=F32, seed=1) * 0.1 + 1.0
    b = rnd(d, dtype=F32, seed=2) * 0.1 if mode == 'layer_norm' else None
    return dict(x=x.to(xd), w=w, b=b, dy=rnd(M, d, dtype=gd, seed=3), dres=rnd(M, d, dtype=F32, seed=4))


def norm_ref(inp, mode, prec, with_dres=True):
    d = inp['x'].shape[-1]
    y, _, rstd = ref('norm_fwd', inp['x'], inp['w'], inp['b'], mode, eps_of(mode), F32, prec=prec)
    dw, db = torch.zeros(d, dtype=prec), (torch.zeros(d, dtype=prec) if inp['b'] is not None else None)
    dx = ref('norm_bwd', inp['dy'], inp['x'], inp['w'], None, None, mode, eps_of(mode), inp['dres'] if with_dres else None, F32, dw, db, prec=prec)
    out = dict(y=y, rstd=rstd, dx=dx, dw=dw)
    if db is not None: out['db'] = db
    return out


NORM_TOL = dict(y=TOL_F32, rstd=TOL_F32, dx=5e-3, dw=5e-3, db=5e-3)


def norm2_inputs(d, M):
    x = rnd(M, d, dtype=F32, scale=2.0) + 0.5
    return dict(x=x, w1=rnd(d, dtype=F32, seed=1) * 0.1 + 1.0, b1=rnd(d, dtype=F32, seed=2) * 0.1, w2=rnd(d, dtype=F32, seed=5) * 0.1 + 1.0,
                b2=rnd(d, dtype=F32, seed=6) * 0.1, dh2=rnd(M, d, dtype=BF, seed=3), dres=rnd(M, d, dtype=F32, seed=4))


def norm2_ref(inp, twice, prec, with_dres=True):
    d = inp['x'].shape[-1]
    p = [inp[k] for k in ('w1', 'b1', 'w2', 'b2')]
    y1, h2, st = ref('norm2_fwd', inp['x'], *p, 1e-5, 1e-5, twice, prec=prec)
    g = [torch.zeros(d, dtype=prec) for _ in range(4)]
    dx = ref('norm2_bwd', inp['dh2'], inp['x'], *p, st, inp['dres'] if with_dres else None, *g, prec=prec)
    return dict(y1=y1, h2=h2, dx=dx, dw1=g[0], db1=g[1], dw2=g[2], db2=g[3])


NORM2_TOL = dict(y1=TOL_F32, h2=TOL_BF16, dx=5e-3, dw1=5e-3, db1=5e-3, dw2=5e-3, db2=5e-3)


# -------------------------------------------------------------------------------------------------------------- softmax
def softmax_inputs(M, C, xd, gd):
    return dict(x=rnd(M, C, dtype=F32, scale=3.0).to(xd), dy=rnd(M, C, dtype=gd, seed=5))


def softmax_ref(inp, log, prec):
    """y in `prec`; the backward is taken at the y the kernel is given (the f32-reference's output rounded to the kernel's type)."""
    y = ref('softmax_fwd', inp['x'], log, F32, prec=prec)
    return dict(y=y, dx=ref('softmax_bwd', inp['y_in'], inp['dy'], log, F32, prec=prec))


# ---------------------------------------------------------------------------------------------------------- conv module
CONV_KSIZES = [3, 5, 7]
CONV_WIDTHS = [100, 260, 516]
CONV_TALL = [(4, 8250, 256, 16), (4, 16500, 256, 32), (4, 11000, 768, 64)]     # B, N, d, frames per time tile the shape reaches


def tall_tile_lengths(B, N, tn):
    """Sample ends within ksize / 2 frames of a time-tile edge: a full sample, 3 frames past an edge, 2 before one, on one."""
    assert B == 4
    return [N, tn * (N // tn // 2) + 3, tn * (N // tn // 3) - 2, tn * (N // tn - 5)]


def convmod_inputs(B, N, d, ks, lens):
    """g: the pointwise_conv1 output; h_in / coef: the forward's own outputs (f32 reference, h rounded to bf16 as stored) that the
    backward reads - inputs of the backward case, the same for the kernel and for both reference precisions."""
    g = rnd(B * N, 2 * d)
    w = rnd(d, ks, dtype=F32, seed=1) * 0.3
    bias = rnd(d, dtype=F32, seed=2) * 0.1
    ln = torch.tensor(lens, dtype=torch.int32) if lens is not None else None
    bw, bb = rnd(d, dtype=F32, seed=3) * 0.1 + 1, rnd(d, dtype=F32, seed=4) * 0.1
    h_in, stats = R.glu_dwconv_fwd(g, ln, w, bias, B, N)
    rm, rs = rnd(d, dtype=F32, seed=5) * 0.1, rnd(d, dtype=F32, seed=6).abs() * 0.2 + 0.8
    coef = {t: R.brn_finalize(stats, B * N, rm.clone(), rs.clone(), torch.tensor(0, dtype=torch.int64), bw, bb, t) for t in (True, False)}
    return dict(g=g, w=w, bias=bias, ln=ln, bw=bw, bb=bb, h_in=h_in, coef=coef, dy=rnd(B * N, d, seed=7), B=B, N=N, d=d, ks=ks)


def convmod_ref(inp, prec, trainings=(True,)):
    B, N, d, ks = inp['B'], inp['N'], inp['d'], inp['ks']
    h, stats = ref('glu_dwconv_fwd', inp['g'], inp['ln'], inp['w'], inp['bias'], B, N, prec=prec)
    out = dict(h=h, stats=stats)
    for t in trainings:
        gs = [torch.zeros(d, ks, dtype=prec), torch.zeros(d, dtype=prec), torch.zeros(d, dtype=prec), torch.zeros(d, dtype=prec)]
        dg, cs = ref('convmod_bwd', inp['dy'], inp['h_in'], inp['g'], inp['ln'], inp['w'], inp['bw'], inp['coef'][t], B, N, t, 1e-3, *gs,
                     colsum=True, prec=prec)
        out.update({f'dg{int(t)}': dg, f'cs{int(t)}': cs, f'ddw{int(t)}': gs[0], f'dbdw{int(t)}': gs[1], f'dbrn_w{int(t)}': gs[2],
                    f'dbrn_b{int(t)}': gs[3]})
    return out


def convmod_tols(out):
    """name -> (tolerance, floor), the tolerances of test_convmod_fwd_bwd.  The dw-conv bias gradient is analytically ~0 in training
    mode (BatchRenorm removes the mean): it is compared on the scale of the dw-conv weight gradient, as there."""
    tol = dict(h=(TOL_BF16, 0.0), stats=(5e-3, 0.0))
    for t in (0, 1):
        if f'dg{t}' not in out: continue
        tol[f'dg{t}'] = (2e-2, 0.0)
        tol[f'cs{t}'] = (1e-2, float(out[f'cs{t}'].abs().max()))
        for nm in ('ddw', 'dbdw', 'dbrn_w', 'dbrn_b'):
            tol[f'{nm}{t}'] = (1e-2, float(out[f'ddw{t}'].abs().max()) if nm == 'dbdw' else 0.0)
    return tol


# ------------------------------------------------------------------------------------------------------------------- CTC
# B N = 67584 frames (past the gather's 65536-workgroup cap) in SHORT sequences: torch's float32 CTC, the reference-only error the
# self-check measures, drifts with the sequence length (8.5e-4 of the gradient's maximum at N = 256, 7.4e-5 at N = 32).
CTC_SHAPE = (2112, 32, 128, 6)                       # B, N, C, S


def ctc_inputs(B, N, C, S):
    g = torch.Generator().manual_seed(N + B)
    lg = torch.randn(B, N, C, generator=g) * 2.0
    tg = torch.randint(0, C - 1, (B, S), generator=g, dtype=torch.int32)
    tg[0, 1] = tg[0, 0]                                              # a repeated label (needs the blank in between)
    il = torch.randint(2 * S + 1, N + 1, (B,), generator=g, dtype=torch.int32)
    tl = torch.randint(1, S + 1, (B,), generator=g, dtype=torch.int32)
    il[0] = N; tl[0] = S; tl[3] = 0                                  # a full sample, an empty target
    il[-8:] = N                                                      # the rows behind the gather's grid cap are live frames
    go = torch.rand(B, generator=g) + 0.5
    lp = torch.log_softmax(lg.double(), -1).float()                  # the log-probabilities the log-prob form of the operator reads
    return dict(lg=lg, lp=lp, tg=tg, il=il, tl=tl, go=go, blank=C - 1)


def ctc_ref(inp, prec):
    a = (inp['tg'], inp['il'], inp['tl'])
    nll, _ = ref('ctc_fwd', inp['lp'], *a, inp['blank'], prec=prec)
    grad = ref('ctc_bwd', inp['lp'], None, nll, *a, inp['go'], inp['blank'], prec=prec)
    nll_l, _ = ref('ctc_fwd_logits', inp['lg'], *a, inp['blank'], prec=prec)
    with ref_precision(prec):                                        # d(logits) without the reference's rounding to bf16
        lg = inp['lg'].detach().clone().to(prec).requires_grad_(True)
        n_ = torch.nn.functional.ctc_loss(torch.log_softmax(lg, -1).transpose(0, 1), inp['tg'].long(), inp['il'].long(), inp['tl'].long(),
                                          blank=inp['blank'], reduction='none', zero_infinity=False)
        n_.backward(inp['go'].to(prec))
    return dict(nll=nll, grad=grad, nll_logits=nll_l, dlogits=lg.grad)


# -------------------------------------------------------------------------------------------------------------- attention
ATTN_SETTINGS = {  # name -> (B, lengths, window)
    'full': (1, None, (-1, -1)),
    'window': (1, None, (128, 128)),
    'left_ragged': (2, [1777, 40], (256, 0)),
}


def rotary(N, D):
    from oracle.sconformer_ref import rotary_tables
    cos, sin = rotary_tables(N, D, 1.5e6)
    return cos[:, :D // 2].contiguous().float(), sin[:, :D // 2].contiguous().float()


def attn_inputs(B, N, H, D, lens):
    return dict(q=rnd(B, N, H, D), k=rnd(B, N, H, D, seed=1), v=rnd(B, N, H, D, seed=2), do=rnd(B, N, H, D, seed=3),
                ln=torch.tensor(lens, dtype=torch.int32) if lens is not None else None, rot=rotary(N, D))


def attn_ref(inp, win, scale, prec):
    q, k, v, ln = inp['q'], inp['k'], inp['v'], inp['ln']
    o, lse = ref('attn_fwd', q, k, v, ln, win, scale, prec=prec)
    dq, dk, dv = ref('attn_bwd', q, k, v, o, inp['do'], lse, ln, win, scale, prec=prec)
    dqr, dkr, _ = ref('attn_bwd', q, k, v, o, inp['do'], lse, ln, win, scale, rot=inp['rot'], prec=prec)
    return dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv, dq_rot=dqr, dk_rot=dkr)


ATTN_TOL = dict(o=TOL_BF16, dq=2e-2, dk=2e-2, dv=2e-2, dq_rot=2e-2, dk_rot=2e-2)


# ---------------------------------------------------------------------------------------------------------------- MADGRAD
MADGRAD_CAP = 4096 * 1024                            # elements per trip of madgrad_kernel at its grid cap (optim.hip sconf_madgrad_step)
MADGRAD_N = int(2.5 * MADGRAD_CAP) + 3               # the n % 4 tail falls in the third trip
MADGRAD_HYPER = dict(lr=3e-3, momentum=0.9, eps=1e-6)
MADGRAD_STEPS = [  # per step: weight decay, gradient scale, max_norm, whether one gradient element is +inf
    dict(wd=0.1, gs=0.125, max_norm=0.8, inf=False),     # the norm (~400) is above max_norm: clipped
    dict(wd=0.1, gs=0.125, max_norm=1e4, inf=False),     # below max_norm: the clip factor is 1
    dict(wd=0.0, gs=1.0, max_norm=0.0, inf=False),       # no clipping at all, no weight decay
    dict(wd=0.1, gs=0.125, max_norm=0.8, inf=True),      # skipped
    dict(wd=0.1, gs=0.125, max_norm=0.8, inf=False),     # applies with the k the skipped step left alone
]


def madgrad_inputs(n=MADGRAD_N):
    p = rnd(n, dtype=F32)
    gs = [rnd(n, dtype=F32, seed=10 + i) for i in range(len(MADGRAD_STEPS))]
    for g, st in zip(gs, MADGRAD_STEPS):
        if st['inf']: g[n // 2 + 1] = float('inf')
    return dict(p=p, g=gs)


def madgrad_ref(inp, prec):
    """State after every step: (p, grad_sum_sq, s, x0, k) with kernel_refs.madgrad_step_ (the semantics of lcasr/optim/madgrad.py
    plus the global-norm clip and the skipped non-finite step) evaluated in `prec`."""
    n = inp['p'].numel()
    p = inp['p'].to(prec).clone(); gss = torch.zeros(n, dtype=prec); s = torch.zeros(n, dtype=prec); x0 = torch.zeros(n, dtype=prec)
    k, out = 0, []
    h = MADGRAD_HYPER
    with ref_precision(prec):
        for g, st in zip(inp['g'], MADGRAD_STEPS):
            sq = float((g.double() ** 2).sum())
            R.madgrad_step_(p, g.to(prec), gss, s, x0, None, sq, st['max_norm'], st['gs'], h['lr'], h['momentum'], h['eps'], st['wd'], k)
            if not st['inf']: k += 1
            out.append(dict(p=p.clone(), gss=gss.clone(), s=s.clone(), x0=x0.clone(), k=k))
    return out


# ------------------------------------------------------------------------------------------- elementwise, grid-stride loops
# Each entry point below caps its grid and walks the rest with a grid-stride loop; the cases are sized at >= 2.5 x the elements
# one trip of the capped grid covers, plus a remainder that is not a multiple of a workgroup's chunk.
CAST_N = int(2.5 * 4096 * 256 * 8) + 5               # elementwise.hip sconf_cast: 4096 workgroups x 256 threads x 8 elements
AFFINE_M, AFFINE_D = int(2.5 * 8192 * 256) + 3, 8    # convmod.hip sconf_affine_silu_fwd: 8192 x 256 threads, 8 elements (= one row) each
MASK_B, MASK_N, MASK_D = 5, 8192 * 256 // 2 + 3, 4   # elementwise.hip sconf_mask_rows: 8192 x 256 threads, 4 elements (= one row) each
ROT_B, ROT_N, ROT_H, ROT_D = 5, 16384 * 256 // 4 + 3, 1, 16   # sconf_rotary_inplace: 16384 x 256 threads, one (row, q|k) each: 2.5 x 2 M rows
ROWDOT_M, ROWDOT_D = int(2.5 * 65536 * 4) + 3, 8     # elementwise.hip sconf_rowdot: 65536 workgroups x 4 rows
OVL_W, OVL_n, OVL_STRIDE, OVL_C = 3, 4300003, 3100000, 4      # infer.hip sconf_overlap_*: 16384 x 256 threads, 4 columns each: span 10.5 M rows
SILU_T_ROWS, SILU_T_F8, SILU_T_C = int(2.5 * 8192) + 3, 10, 8  # subsample.hip sconf_sub_silu_transpose: 8192 workgroups, a row each


def affine_inputs(M=AFFINE_M, d=AFFINE_D):
    return dict(h=rnd(M, d), coef=torch.cat([rnd(4, d, dtype=F32, seed=1), rnd(1, d, dtype=F32, seed=2) * 0.2 + 1.0, rnd(1, d, dtype=F32, seed=3) * 0.1]))


def rotary_inputs(B=ROT_B, N=ROT_N, H=ROT_H, D=ROT_D):
    g = torch.Generator().manual_seed(N)
    ang = torch.rand(N, D // 2, generator=g) * 6.283
    return dict(qkv=rnd(B * N, 3 * H * D), cos=torch.cos(ang), sin=torch.sin(ang), B=B, N=N, H=H, D=D)


def rowdot_inputs(M=ROWDOT_M, d=ROWDOT_D):
    return dict(a=rnd(M, d), b=rnd(M, d, seed=1), bias=rnd(d, dtype=F32, seed=2))


def silu_t_inputs(rows=SILU_T_ROWS, F8=SILU_T_F8, C=SILU_T_C):
    return dict(pre=rnd(rows, F8, C, seed=6), ds=rnd(rows, C * F8, seed=7))

