"""Case table of the write-footprint tests (tests/footprint.py): for every entry point of include/sconf.h that launches work, the
regions it reads and writes, the argument list, and the kernel_refs function that restates it.  TEST INFRASTRUCTURE, plain module.

CASES maps a case id to (family, entry point, builder); builder(lib) lays the arena out and returns a footprint.Case.  Builders need
the library only for its host-side queries (workspace sizes, kernel routing), so they also run where there is no GPU.  Shapes are the
smallest at which the indexing can still go wrong, not workload shapes.  Workspaces are carved at EXACTLY the size the query or the
header formula gives, with a guard right behind."""
import ctypes
import math

import torch

import attn_maps_refs
import dyneval_refs
import eval_refs
import geometry_cases as G
import kernel_refs as R
from footprint import ACC, Arena, Case, IN, INOUT, OUT, SCRATCH
from kernel_test_utils import BF, F32, F64, TOL_BF16, TOL_F32, ref, rnd

I32, I64 = torch.int32, torch.int64
ACT = {'none': 0, 'gelu': 1, 'silu': 2, 'dgelu': 3, 'dsilu': 4, 'gelu_dsave': 5, 'mulaux': 6}
LAYOUT = {'nt': 0, 'nn': 1, 'tn': 2}
NORM_MODE = {'layer_norm': 0, 'rms_norm': 1, 'rms_norm_apex': 2}
DT = {F32: 0, BF: 1}

NO_LAUNCH = {'sconf_gemm_num_splits'}          # returns a value, launches nothing
CASES = {}


def case(family, entry, id, *args, **kw):
    def deco(fn):
        assert id not in CASES, id
        CASES[id] = (family, entry, lambda lib: fn(lib, id, *args, **kw))
        return fn
    return deco


def build(id, lib):
    return CASES[id][2](lib)


def ids_of(family):
    return [i for i, (f, _, _) in CASES.items() if f == family]


def put(a, name, t, cls=IN, **kw):
    """A region holding tensor t (IN / ACC / INOUT content)."""
    return a.take(name, tuple(t.shape), t.dtype, cls, init=t.contiguous(), **kw)


def distinct(*least, step=8):
    """One leading dimension per entry of `least`: multiples of `step`, each larger than its row length, no two equal."""
    used, out = set(), []
    for n in least:
        ld = (n // step + 1) * step
        while ld in used: ld += step
        used.add(ld); out.append(ld)
    assert len(set(out)) == len(out) and all(l > n for l, n in zip(out, least))
    return out


def ints(*v):
    return torch.tensor(v, dtype=I32)


def lens_i32(v):
    return None if v is None else torch.tensor(v, dtype=I32)


# ====================================================================================================================== GEMM
EPILOGUES = {  # name: (bias, resid, aux, pre, act, alpha, out_f32)
    'plain': (0, 0, 0, 0, 'none', 1.0, 0),
    'bias_resid_alpha_f32': (1, 1, 0, 0, 'none', 0.5, 1),
    'resid_f32': (0, 1, 0, 0, 'none', 1.0, 1),
    'gelu_dsave': (0, 0, 0, 1, 'gelu_dsave', 1.0, 0),
    'dgelu': (0, 0, 1, 0, 'dgelu', 1.0, 0),
    'bias_save_pre': (1, 0, 0, 1, 'none', 1.0, 0),
    'mulaux': (0, 0, 1, 0, 'mulaux', 1.0, 0),
    'bias_resid_pre_f32': (1, 1, 0, 1, 'none', 1.0, 1),
}


def gemm_case(lib, id, layout, M, N, K, epi, want, split_k=1, accum=False):
    """sconf_gemm_bf16 with six pairwise different leading dimensions; want: the kernel sconf_gemm_variant must report."""
    has_bias, has_resid, has_aux, has_pre, act, alpha, out_f32 = EPILOGUES[epi]
    ar, ac = (K, M) if layout == 'tn' else (M, K)
    br, bc = (N, K) if layout == 'nt' else (K, N)
    lda, ldb, ldc, ldr, ldaux, ldpre = distinct(ac, bc, N, N, N, N)
    if accum: ldr = ldc                                               # in-place accumulation: resid IS C
    lds = [lda, ldb, ldc, ldaux, ldpre] + ([] if accum else [ldr])
    assert len(set(lds)) == len(lds), f'{id}: leading dimensions not pairwise different: {lds}'
    assert ldc % (8 if layout == 'nt' else 4) == 0
    a = Arena()
    A = put(a, 'A', rnd(ar, ac, seed=1) * 0.5, ld=lda)
    B = put(a, 'B', rnd(br, bc, seed=2) * 0.5, ld=ldb)
    splits = lib.sconf_gemm_num_splits(K, split_k) if split_k > 1 else 1
    cdt = F32 if out_f32 or split_k > 1 else BF
    if splits > 1:
        C = a.take('C', (splits, M, N), F32, OUT, strides=(M * ldc, ldc, 1))
    elif accum:
        C = put(a, 'C', rnd(M, N, dtype=F32, seed=3), ACC, ld=ldc, order='fixed')
    else:
        C = a.take('C', (M, N), cdt, OUT, ld=ldc)
    bias = put(a, 'bias', rnd(N, dtype=F32, seed=4)) if has_bias else None
    resid = C if accum else (put(a, 'resid', rnd(M, N, dtype=F32, seed=5), ld=ldr) if has_resid else None)
    aux = put(a, 'aux', rnd(M, N, seed=6), ld=ldaux) if has_aux else None
    pre = a.take('pre', (M, N), BF, OUT, ld=ldpre) if has_pre else None
    got = lib.sconf_gemm_variant(LAYOUT[layout], M, N, K, lda, ldb, split_k, ACT[act], int(resid is not None), int(pre is not None))
    assert got == want, f'{id}: sconf_gemm_variant reports {got}, the case is meant for {want}'
    args = [LAYOUT[layout], A, B, C, M, N, K, lda, ldb, ldc, bias, resid, ldr, aux, ldaux, pre, ldpre, float(alpha), ACT[act],
            int(cdt == F32), split_k]

    def restate(v):
        if splits > 1:
            kps = -(-(-(-K // 64)) // split_k) * 64
            sl = lambda t, s, kdim: t.narrow(kdim, s * kps, min(kps, K - s * kps))
            ka, kb = (0 if layout == 'tn' else 1), (1 if layout == 'nt' else 0)
            return {'C': torch.stack([ref('gemm', sl(v['A'], s, ka), sl(v['B'], s, kb), layout, out_dtype=F32) for s in range(splits)])}
        if accum:
            return {'C': ref('gemm', v['A'], v['B'], layout, alpha=alpha, accum=v['C'].clone())}
        out = ref('gemm', v['A'], v['B'], layout, v.get('bias'), v.get('resid'), v.get('aux'), act, alpha, cdt, save_pre=bool(has_pre))
        return {'C': out[0], 'pre': out[1]} if has_pre else {'C': out}
    staging = 'lds-dma' if K % 64 == 0 else 'register'
    return Case(id, 'sconf_gemm_bf16', a, args, 'gemm', restate, variant=f'{got} ({staging} staging, {splits} split(s))')


_E128 = ('plain', 'bias_resid_alpha_f32', 'gelu_dsave', 'dgelu', 'bias_save_pre', 'mulaux')
for _lay, _N in (('nt', 144), ('nn', 136), ('tn', 136)):
    for _i, _e in enumerate(_E128):
        for _K in (72, 128):
            if _lay != 'nt' and (_i + (_K == 128)) % 2: continue         # NN / TN: every epilogue once, K alternating
            case('gemm128', 'sconf_gemm_bf16', f'gemm128-{_lay}-{_e}-K{_K}', _lay, 200, _N, _K, _e, 0)(gemm_case)
for _lay, _N in (('nt', 144), ('tn', 136)):
    case('gemm128', 'sconf_gemm_bf16', f'gemm128-{_lay}-splitk3-K2560', _lay, 200, _N, 2560, 'plain', 0, split_k=3)(gemm_case)
    case('gemm128', 'sconf_gemm_bf16', f'gemm128-{_lay}-accum-K128', _lay, 200, _N, 128, 'resid_f32', 0, accum=True)(gemm_case)


@case('gemm128', 'sconf_splitk_reduce', 'splitk_reduce-overwrite', 0)
@case('gemm128', 'sconf_splitk_reduce', 'splitk_reduce-accumulate', 1)
def splitk_reduce_case(lib, id, accumulate):
    splits, n = 3, 4 * 1031
    a = Arena()
    slab = put(a, 'slab', rnd(splits, n, dtype=F32, seed=1))
    out = put(a, 'out', rnd(n, dtype=F32, seed=2), ACC, order='fixed') if accumulate else a.take('out', n, F32, OUT)
    restate = lambda v: {'out': v['slab'].double().sum(0) + (v['out'].double() if accumulate else 0)}
    return Case(id, 'sconf_splitk_reduce', a, [slab, out, splits, n, accumulate], 'gemm (split_k: the sum over the slabs)', restate)


def _smallest_m(lib, layout, N, K, want, act=0, resid=0, pre=0, split_k=1):
    for M in range(256, 65536 + 1, 256):
        lda, ldb = distinct(M if layout == 'tn' else K, K if layout == 'nt' else N)
        if lib.sconf_gemm_variant(LAYOUT[layout], M, N, K, lda, ldb, split_k, act, resid, pre) == want: return M
    raise AssertionError(f'no M up to 65536 routes ({layout}, N={N}, K={K}) to kernel {want}')


def gemm256_case(lib, id, N, K, epi, want):
    has_bias, has_resid, has_aux, has_pre, act, alpha, out_f32 = EPILOGUES[epi]
    M = _smallest_m(lib, 'nt', N, K, want, ACT[act], has_resid, has_pre)
    return gemm_case(lib, id, 'nt', M, N, K, epi, want)


for _N, _want in ((1024, 1), (3072, 2)):
    for _i, _e in enumerate(('plain', 'resid_f32', 'gelu_dsave', 'mulaux', 'bias_resid_pre_f32')):
        case('gemm256', 'sconf_gemm_bf16', f'gemm256-v{_want}-{_e}-K{(64, 192)[_i % 2]}', _N, (64, 192)[_i % 2], _e, _want)(gemm256_case)


@case('gemm256', 'sconf_gemm_bf16', 'gemm256-v3-tn-splitk')
def gemm256_tn_case(lib, id):
    M = N = 768
    for split in range(2, 65):
        K = 64 * 32 if split <= 32 else 64 * split
        lda, ldb = distinct(M, N)
        if lib.sconf_gemm_variant(2, M, N, K, lda, ldb, split, 0, 0, 0) == 3:
            return gemm_case(lib, id, 'tn', M, N, K, 'plain', 3, split_k=split)
    raise AssertionError('no split up to 64 routes the (768, 768) TN problem to the 256-row kernel')


@case('gemm256', 'sconf_gemm_softmax_bwd', 'gemm_softmax_bwd')
def gemm_softmax_bwd_case(lib, id):
    V, K = 1024, 64
    for M in range(256, 65536 + 1, 256):
        if lib.sconf_gemm_variant(0, M, V, K, *distinct(K, K), 1, 7, 0, 0) == 1: break
    else:
        raise AssertionError('no M routes sconf_gemm_softmax_bwd to the 256-wide kernel')
    lddy, ldw, ldp = distinct(K, K, V)
    a = Arena()
    dy = put(a, 'dy', rnd(M, K, seed=1) * 0.5, ld=lddy)
    wt = put(a, 'Wt', rnd(V, K, seed=2) * 0.5, ld=ldw)
    probs = put(a, 'probs', torch.softmax(rnd(M, V, dtype=F32, seed=3) * 2, -1).to(BF), ld=ldp)
    delta = put(a, 'delta', rnd(M, dtype=F32, seed=4) * 0.1)
    dl = a.take('dl', (M, V), BF, OUT)
    colslab = a.take('colslab', (2 * M // 256, V), F32, OUT, tol=2e-3)

    def restate(v):
        d = ref('gemm_softmax_bwd', v['dy'], v['Wt'], v['probs'], v['delta'])          # rounded to bf16, as stored
        # sconf.h defines the slab through its column sums (the two wave-row lines of a 256-row panel add up to the panel's sums)
        return {'dl': d, 'colslab': (d.double().view(M // 256, 256, V).sum(1), lambda t: t.double().view(M // 256, 2, V).sum(1))}
    return Case(id, 'sconf_gemm_softmax_bwd', a, [dy, wt, probs, delta, dl, colslab, M, V, K, lddy, ldw, ldp], 'gemm_softmax_bwd', restate,
                variant='1 (256 wide)')


def qkv_rotary_case(lib, id, Bn, N, H, K, bias, fused):
    from oracle.sconformer_ref import rotary_tables
    D, M = 128, Bn * N
    lda, ldb = distinct(K, K)
    routed = lib.sconf_gemm_variant(0, M, 3 * H * D, K, lda, ldb, 1, 0, 0, 0) in (1, 2)
    assert routed == fused, f'{id}: the shape {"does not reach" if fused else "reaches"} the 256-row kernels'
    cos, sin = rotary_tables(N, D, 1.5e6)
    a = Arena()
    x = put(a, 'x', rnd(M, K, seed=1), ld=lda)
    w = put(a, 'w', rnd(3 * H * D, K, seed=2) * 0.1, ld=ldb)
    b = put(a, 'bias', rnd(3 * H * D, dtype=F32, seed=3)) if bias else None
    c = put(a, 'cos', cos[:, :D // 2].contiguous()); s = put(a, 'sin', sin[:, :D // 2].contiguous())
    out = a.take('C', (M, 3 * H * D), BF, OUT, tol=TOL_BF16 if fused else 1.6e-2)   # the fallback rounds to bf16 twice (test_gemm_qkv_rotary)
    restate = lambda v: {'C': ref('gemm_qkv_rotary', v['x'], v['w'], v.get('bias'), v['cos'], v['sin'], N, H, D)}
    return Case(id, 'sconf_gemm_qkv_rotary', a, [x, w, out, M, K, H, D, lda, ldb, b, c, s, N], 'gemm_qkv_rotary', restate,
                variant='rotary epilogue' if fused else 'gemm + rotary_inplace')


case('gemm256', 'sconf_gemm_qkv_rotary', 'qkv_rotary-fused', 32, 256, 6, 768, True, True)(qkv_rotary_case)
case('gemm256', 'sconf_gemm_qkv_rotary', 'qkv_rotary-fallback', 1, 64, 4, 64, False, False)(qkv_rotary_case)


@case('gemm256', 'sconf_rowdot', 'rowdot')
def rowdot_case(lib, id):
    M, d = 301, 72
    lda, ldb = distinct(d, d)
    a = Arena()
    x = put(a, 'a', rnd(M, d, seed=1), ld=lda); y = put(a, 'b', rnd(M, d, seed=2), ld=ldb)
    bias = put(a, 'bias', rnd(d, dtype=F32, seed=3)); out = a.take('out', M, F32, OUT)
    return Case(id, 'sconf_rowdot', a, [x, y, bias, out, M, d, lda, ldb], 'rowdot', lambda v: {'out': ref('rowdot', v['a'], v['b'], v['bias'])})


# ====================================================================================================================== norms
def norm_fwd_case(lib, id, mode, d, M, xd, yd):
    inp = G.norm_inputs(mode, d, M, xd, F32)
    a = Arena()
    x = put(a, 'x', inp['x']); w = put(a, 'w', inp['w']); b = put(a, 'b', inp['b']) if inp['b'] is not None else None
    y = a.take('y', (M, d), yd, OUT); mean = a.take('mean', M, F32, OUT); rstd = a.take('rstd', M, F32, OUT)

    def restate(v):
        yr, mr, rr = ref('norm_fwd', v['x'], v['w'], v.get('b'), mode, G.eps_of(mode), yd)
        return {'y': yr, 'mean': mr, 'rstd': rr}
    return Case(id, 'sconf_norm_fwd', a, [NORM_MODE[mode], x, DT[xd], w, b, y, DT[yd], mean, rstd, M, d, G.eps_of(mode)], 'norm_fwd', restate)


def norm_bwd_case(lib, id, mode, d, M, xd, gd, dxd, dres, twin, null_ws):
    inp = G.norm_inputs(mode, d, M, xd, gd)
    _, mean_, rstd_ = R.norm_fwd(inp['x'], inp['w'], inp['b'], mode, G.eps_of(mode), F32)
    a = Arena()
    dy = put(a, 'dy', inp['dy']); x = put(a, 'x', inp['x']); w = put(a, 'w', inp['w'])
    mean = put(a, 'mean', mean_.contiguous()); rstd = put(a, 'rstd', rstd_.contiguous())
    dr = put(a, 'dres', inp['dres']) if dres else None
    dx = a.take('dx', (M, d), dxd, OUT, tol=5e-3)
    order = 'atomic' if null_ws else 'fixed'                       # sconf.h: the workspace fixes the order, NULL = f32 atomics
    dw = put(a, 'dw', rnd(d, dtype=F32, seed=7), ACC, order=order, tol=5e-3)
    db = put(a, 'db', rnd(d, dtype=F32, seed=8), ACC, order=order, tol=5e-3) if mode == 'layer_norm' else None
    nws = 0 if null_ws else int(lib.sconf_norm_bwd_workspace(M, d))
    ws = a.take('workspace', nws, F32, SCRATCH) if nws else None
    assert not twin or (dxd == F32 and ws is not None)
    dx16 = a.take('dx_bf16', (M, d), BF, OUT) if twin else None
    cs = a.take('dx_colsum', d, F32, OUT, tol=2e-3) if twin else None

    def restate(v):
        gw, gb = v['dw'].double(), (v['db'].double() if db is not None else None)
        r = ref('norm_bwd', v['dy'], v['x'], v['w'], None, None, mode, G.eps_of(mode), v.get('dres'), dxd, gw, gb, twin=twin)
        out = {'dx': r[0] if twin else r, 'dw': gw}
        if gb is not None: out['db'] = gb
        if twin: out.update(dx_bf16=r[1], dx_colsum=r[2])
        return out
    args = [NORM_MODE[mode], dy, DT[gd], x, DT[xd], w, mean, rstd, dr, dx, DT[dxd], dw, db, ws, nws, dx16, cs, M, d, G.eps_of(mode)]
    return Case(id, 'sconf_norm_bwd', a, args, 'norm_bwd', restate, variant='fixed order' if nws else 'atomics')


_MODES = ('layer_norm', 'rms_norm', 'rms_norm_apex')
for _j, _d in enumerate((4, 68, 772, 1028, 2048)):
    for _i, _m in enumerate(_MODES):
        _xd, _yd = ((BF, F32), (F32, BF), (F32, F32), (BF, BF))[(_i + _j) % 4]
        case('norm', 'sconf_norm_fwd', f'norm_fwd-{_m}-d{_d}-M37', _m, _d, 37, _xd, _yd)(norm_fwd_case)
        _k = (_i + _j) % 3                                          # 0: dres, 1: the bf16 twin, 2: NULL workspace (atomics)
        case('norm', 'sconf_norm_bwd', f'norm_bwd-{_m}-d{_d}-M37-{("dres", "twin", "nullws")[_k]}', _m, _d, 37, _xd,
             BF if _k == 0 else F32, BF if _k == 0 and _xd == BF else F32, _k != 2, _k == 1, _k == 2)(norm_bwd_case)
for _d in (68, 2048):
    _M = G.rows_for_trips(G.norm_bwd_waves(_d))
    case('norm', 'sconf_norm_fwd', f'norm_fwd-layer_norm-d{_d}-trips', 'layer_norm', _d, _M, BF, BF)(norm_fwd_case)
    case('norm', 'sconf_norm_bwd', f'norm_bwd-layer_norm-d{_d}-trips', 'layer_norm', _d, _M, BF, BF, F32, True, True, False)(norm_bwd_case)


def norm2_fwd_case(lib, id, d, M, twice):
    inp = G.norm2_inputs(d, M)
    a = Arena()
    p = [put(a, k, inp[k]) for k in ('x', 'w1', 'b1', 'w2', 'b2')]
    y1 = a.take('y1', (M, d), F32, OUT); h2 = a.take('h2', (M, d), BF, OUT)
    st = [a.take(n, M, F32, OUT, tol=1e-5) for n in ('mean1', 'rstd1', 'mean2', 'rstd2')]
    # mean3 / rstd3 are unused with twice = 0 (sconf.h): IN regions, so a write into them is a confinement failure
    st += [a.take(n, M, F32, OUT, tol=1e-5) if twice else put(a, n, rnd(M, dtype=F32, seed=9)) for n in ('mean3', 'rstd3')]

    def restate(v):
        y1r, h2r, s = ref('norm2_fwd', v['x'], v['w1'], v['b1'], v['w2'], v['b2'], 1e-5, 1e-5, bool(twice))
        return dict(zip(['y1', 'h2', 'mean1', 'rstd1', 'mean2', 'rstd2', 'mean3', 'rstd3'], [y1r, h2r] + list(s)))
    return Case(id, 'sconf_norm2_fwd', a, p + [y1, h2] + st + [twice, M, d, 1e-5, 1e-5], 'norm2_fwd', restate)


def norm2_bwd_case(lib, id, d, M, twice, dres, twin):
    inp = G.norm2_inputs(d, M)
    _, _, stats = R.norm2_fwd(*[inp[k] for k in ('x', 'w1', 'b1', 'w2', 'b2')], 1e-5, 1e-5, bool(twice))
    a = Arena()
    dh2 = put(a, 'dh2', inp['dh2'])
    p = [put(a, k, inp[k]) for k in ('x', 'w1', 'b1', 'w2', 'b2')]
    names = ('mean1', 'rstd1', 'mean2', 'rstd2', 'mean3', 'rstd3')
    st = [put(a, n, (stats[i] if i < len(stats) else rnd(M, dtype=F32, seed=9)).contiguous()) for i, n in enumerate(names)]
    dr = put(a, 'dres', inp['dres']) if dres else None
    dx = a.take('dx', (M, d), F32, OUT, tol=5e-3)
    g = [put(a, n, rnd(d, dtype=F32, seed=10 + i), ACC, order='fixed', tol=5e-3) for i, n in enumerate(('dw1', 'db1', 'dw2', 'db2'))]
    nws = int(lib.sconf_norm2_bwd_workspace(M, d))
    ws = a.take('workspace', nws, F32, SCRATCH)
    dx16 = a.take('dx_bf16', (M, d), BF, OUT) if twin else None
    cs = a.take('dx_colsum', d, F32, OUT, tol=2e-3) if twin else None

    def restate(v):
        gr = [v[n].double() for n in ('dw1', 'db1', 'dw2', 'db2')]
        s = tuple(v[n] for n in names[:6 if twice else 4])
        r = ref('norm2_bwd', v['dh2'], v['x'], v['w1'], v['b1'], v['w2'], v['b2'], s, v.get('dres'), *gr, twin=twin)
        out = dict(zip(('dw1', 'db1', 'dw2', 'db2'), gr), dx=r[0] if twin else r)
        if twin: out.update(dx_bf16=r[1], dx_colsum=r[2])
        return out
    args = [dh2] + p + st + [twice, dr, dx] + g + [ws, nws, dx16, cs, M, d]
    return Case(id, 'sconf_norm2_bwd', a, args, 'norm2_bwd', restate)


for _i, _d in enumerate((4, 260, 768)):
    for _tw in (0, 1):
        case('norm', 'sconf_norm2_fwd', f'norm2_fwd-d{_d}-twice{_tw}', _d, 37, _tw)(norm2_fwd_case)
        case('norm', 'sconf_norm2_bwd', f'norm2_bwd-d{_d}-twice{_tw}', _d, 37, _tw, (_i + _tw) % 2 == 0, (_i + _tw) % 2 == 1)(norm2_bwd_case)
case('norm', 'sconf_norm2_bwd', 'norm2_bwd-d260-trips', 260, G.rows_for_trips(G.norm_bwd_waves(260)), 0, True, True)(norm2_bwd_case)


# ============================================================================================ softmax, colsum, mask, cast, rotary
def softmax_fwd_case(lib, id, log, M, C, xd, yd):
    a = Arena()
    x = put(a, 'x', rnd(M, C, dtype=xd, scale=3.0)); y = a.take('y', (M, C), yd, OUT)
    return Case(id, 'sconf_softmax_fwd', a, [log, x, DT[xd], y, DT[yd], M, C], 'softmax_fwd',
                lambda v: {'y': ref('softmax_fwd', v['x'], bool(log), yd)})


def softmax_bwd_case(lib, id, log, M, C, yd, colsum):
    y0 = R.softmax_fwd(rnd(M, C, dtype=F32, scale=3.0), bool(log), yd)
    a = Arena()
    y = put(a, 'y', y0); dy = put(a, 'dy', rnd(M, C, dtype=yd, seed=5)); dx = a.take('dx', (M, C), BF, OUT)
    cs = put(a, 'colsum_out', rnd(C, dtype=F32, seed=6), ACC, order='fixed', tol=2e-3) if colsum else None   # per-slab sums, then sconf_colsum
    nws = int(lib.sconf_softmax_bwd_workspace(M, C)) if colsum else 0
    ws = a.take('workspace', nws, F32, SCRATCH) if colsum else None

    def restate(v):
        out = {'dx': ref('softmax_bwd', v['y'], v['dy'], bool(log), BF)}
        if colsum:                                            # the sums of the bf16-ROUNDED dx, as test_softmax compares them
            out['colsum_out'] = v['colsum_out'].double() + R.softmax_bwd(v['y'], v['dy'], bool(log), BF).double().sum(0)
        return out
    return Case(id, 'sconf_softmax_bwd', a, [log, y, DT[yd], dy, DT[yd], dx, DT[BF], cs, ws, M, C], 'softmax_bwd', restate)


for _C in (132, 8192):
    for _M in (37, 5000):
        case('rows', 'sconf_softmax_fwd', f'softmax_fwd-C{_C}-M{_M}', int(_M == 37), _M, _C, F32 if _M == 37 else BF, F32 if _M == 37 else BF)(softmax_fwd_case)
        for _cs in (0, 1):
            case('rows', 'sconf_softmax_bwd', f'softmax_bwd-C{_C}-M{_M}-colsum{_cs}', int(_M == 37), _M, _C, F32 if _M == 37 else BF, _cs)(softmax_bwd_case)


def colsum_case(lib, id, M, N, xd, want_ws):
    ld, = distinct(N, step=4)
    nws = int(lib.sconf_colsum_workspace(M, N))
    assert bool(nws) == want_ws, f'{id}: sconf_colsum_workspace({M}, {N}) = {nws}'
    a = Arena()
    x = put(a, 'x', rnd(M, N, dtype=xd, seed=1), ld=ld)
    out = put(a, 'out', rnd(N, dtype=F32, seed=2), ACC, order='fixed', tol=2e-3)
    ws = a.take('workspace', nws, torch.uint8, SCRATCH) if nws else None
    return Case(id, 'sconf_colsum', a, [x, DT[xd], out, M, N, ld, 0.5, ws, nws], 'colsum_',
                lambda v: {'out': ref('colsum_', v['x'], v['out'].double(), 0.5)}, variant='row blocks' if nws else 'one row block')


case('rows', 'sconf_colsum', 'colsum-small-nows', 37, 72, BF, False)(colsum_case)
case('rows', 'sconf_colsum', 'colsum-rowblocks-ws', 20000, 68, F32, True)(colsum_case)


@case('rows', 'sconf_mask_rows', 'mask_rows-bf16', BF)
@case('rows', 'sconf_mask_rows', 'mask_rows-f32', F32)
def mask_rows_case(lib, id, dt):
    B, N, d = 3, 17, 68
    a = Arena()
    x = put(a, 'x', rnd(B * N, d, dtype=dt), INOUT); ln = put(a, 'lengths', ints(N, 5, 0))
    return Case(id, 'sconf_mask_rows', a, [x, DT[dt], ln, B, N, d], 'mask_rows_', lambda v: {'x': R.mask_rows_(v['x'].clone(), v['lengths'], B, N)})


@case('rows', 'sconf_cast', 'cast-f32-bf16', F32, BF)
@case('rows', 'sconf_cast', 'cast-bf16-f32', BF, F32)
def cast_case(lib, id, sd, dd):
    n = 4099
    a = Arena()
    src = put(a, 'src', rnd(n, dtype=sd)); dst = a.take('dst', n, dd, OUT, tol=0.0)
    return Case(id, 'sconf_cast', a, [src, DT[sd], dst, DT[dd], n], 'cast', lambda v: {'dst': v['src'].to(dd)})


@case('rows', 'sconf_cast_transpose', 'cast_transpose')
def cast_transpose_case(lib, id):
    Rr, Cc = 100, 36
    a = Arena()
    src = put(a, 'src', rnd(Rr, Cc, dtype=F32)); dst = a.take('dst', (Cc, Rr), BF, OUT, tol=0.0)
    return Case(id, 'sconf_cast_transpose', a, [src, dst, Rr, Cc], 'cast_transpose', lambda v: {'dst': R.cast_transpose(v['src'])})


@case('rows', 'sconf_cast_shadows', 'cast_shadows')
def cast_shadows_case(lib, id):
    """Three entries: a regrouped one with both shadows, one with only dst, one with only dstT."""
    shapes = [(-96, 40), (33, 65), (31, 36)]
    a = Arena()
    src = [put(a, f'src{i}', rnd(abs(r), c, dtype=F32, seed=i)) for i, (r, c) in enumerate(shapes)]
    dst = [a.take('dst0', (96, 40), BF, OUT, tol=0.0), a.take('dst1', (33, 65), BF, OUT, tol=0.0), None]
    dstT = [a.take('dstT0', (40, 96), BF, OUT, tol=0.0), None, a.take('dstT2', (36, 31), BF, OUT, tol=0.0)]
    tile0, firsts = 0, []
    for r, c in shapes:
        firsts.append(tile0); tile0 += ((abs(r) + 31) // 32) * ((c + 31) // 32)

    def table(addr):
        rows = [[addr(src[i]), addr(dst[i]) if dst[i] else 0, addr(dstT[i]) if dstT[i] else 0, r, c, firsts[i]] for i, (r, c) in enumerate(shapes)]
        return torch.tensor(rows + [[0, 0, 0, 0, 0, tile0]], dtype=I64)
    tab = a.take('table', (len(shapes) + 1, 6), I64, IN, init=table)

    def restate(v):
        w0 = v['src0'].view(32, 3, 40).permute(1, 0, 2).reshape(96, 40)
        return {'dst0': w0.to(BF), 'dstT0': w0.t().to(BF), 'dst1': v['src1'].to(BF), 'dstT2': v['src2'].t().to(BF)}
    return Case(id, 'sconf_cast_shadows', a, [tab, len(shapes), tile0], 'cast_shadows', restate,
                indirect=[r.name for r in src + dst + dstT if r is not None])


def _rot_tables(N, D):
    from oracle.sconformer_ref import rotary_tables
    cos, sin = rotary_tables(N, D, 1.5e6)
    return cos[:, :D // 2].contiguous(), sin[:, :D // 2].contiguous()


@case('rows', 'sconf_rotary_qkv', 'rotary_qkv-fwd', 0, True)
@case('rows', 'sconf_rotary_qkv', 'rotary_qkv-fwd-norotary', 0, False)
@case('rows', 'sconf_rotary_qkv', 'rotary_qkv-bwd', 1, True)
def rotary_qkv_case(lib, id, bwd, use):
    B, N, H, D = 2, 50, 2, 32
    cos_, sin_ = _rot_tables(N, D)
    a = Arena()
    cos = put(a, 'cos', cos_) if use else None; sin = put(a, 'sin', sin_) if use else None
    if not bwd:
        qkv = put(a, 'qkv', rnd(B * N, H * D * 3))
        q, k, v = (a.take(n, (B, N, H, D), BF, OUT) for n in 'qkv')
        restate = lambda t: dict(zip('qkv', ref('rotary_qkv_fwd', t['qkv'], t.get('cos'), t.get('sin'), B, N, H, D)))
    else:
        qkv = a.take('qkv', (B * N, H * D * 3), BF, OUT)              # bwd != 0: dqkv is written to `qkv`, every element
        q, k, v = (put(a, n, rnd(B, N, H, D, seed=i)) for i, n in enumerate('qkv'))
        restate = lambda t: {'qkv': ref('rotary_qkv_bwd', t['q'], t['k'], t['v'], t.get('cos'), t.get('sin'), B, N, H, D)}
    return Case(id, 'sconf_rotary_qkv', a, [bwd, qkv, cos, sin, q, k, v, B, N, H, D, int(use)], 'rotary_qkv_bwd' if bwd else 'rotary_qkv_fwd', restate)


@case('rows', 'sconf_rotary_inplace', 'rotary_inplace')
def rotary_inplace_case(lib, id):
    """q and k blocks in place; the v block of every token is a guard (stride gap between the q | k runs)."""
    B, N, H, D = 2, 50, 2, 32
    cos_, sin_ = _rot_tables(N, D)
    a = Arena()
    qk = put(a, 'qk', rnd(B * N, 2 * H * D), INOUT, ld=3 * H * D)
    cos = put(a, 'cos', cos_); sin = put(a, 'sin', sin_)

    def restate(t):
        full = torch.zeros(B * N, 3 * H * D, dtype=BF)
        full[:, :2 * H * D] = t['qk']
        return {'qk': ref('rotary_inplace_', full.double(), t['cos'], t['sin'], B, N, H, D, prec=F64)[:, :2 * H * D]}
    return Case(id, 'sconf_rotary_inplace', a, [qk, cos, sin, B, N, H, D], 'rotary_inplace_', restate)


# ====================================================================================================================== attention
ATTN_SHAPES = {  # name: (B, N, H, D, lengths, window, waves)
    'd128-n333-ragged': (2, 333, 3, 128, [333, 131], (-1, -1), 8),
    'd128-n200': (2, 200, 2, 128, None, (-1, -1), 4),
    'd32-n300-win16': (2, 300, 2, 32, None, (16, 16), 4),
    'd64-n257-win24_8': (1, 257, 2, 64, None, (24, 8), 4),
    'd256-n257-win24_8': (1, 257, 2, 256, None, (24, 8), 4),
}


def _attn_views(a, names, B, N, H, D, cls_of, init_of):
    """One region per operand, each with its own token and batch stride: multiples of 8, no two equal; padding = guards."""
    ts = distinct(*[H * D] * len(names))
    bs = distinct(*[N * t for t in ts])
    regs, triples = {}, {}
    for n, t, b in zip(names, ts, bs):
        st = (b, t, D, 1)
        init = init_of(n)
        regs[n] = a.take(n, (B, N, H, D), BF, cls_of(n), strides=st, init=init, tol=2e-2 if n in ('dq', 'dk', 'dv') else None,
                         produced=(cls_of(n) == IN and init is None))
        triples[n] = (ctypes.c_int64 * 3)(b, t, D)
    flat = [x for n in names for x in triples[n]]
    assert all(x % 8 == 0 for x in flat) and len({tuple(triples[n]) for n in names}) == len(names)
    assert len(set(ts)) == len(ts) and len(set(bs)) == len(bs), 'attention stride triples must differ'
    return regs, triples


def attn_case(lib, id, shape, bwd, rot=False):
    B, N, H, D, lens, win, waves = ATTN_SHAPES[shape]
    names = ['q', 'k', 'v', 'o'] + (['dout', 'dq', 'dk', 'dv'] if bwd else [])
    a = Arena()
    seeds = {'q': 0, 'k': 1, 'v': 2, 'dout': 3}
    cls_of = lambda n: OUT if n in ('dq', 'dk', 'dv') or (n == 'o' and not bwd) else IN
    init_of = lambda n: rnd(B, N, H, D, seed=seeds[n]) if n in seeds else None
    regs, st = _attn_views(a, names, B, N, H, D, cls_of, init_of)
    got = lib.sconf_attn_waves(D, N, max(s[1] for s in st.values()))
    assert got == waves, f'{id}: sconf_attn_waves reports {got}, the case is meant for the {waves}-wave kernels'
    ln = put(a, 'lengths', lens_i32(lens)) if lens else None
    lse = a.take('lse', (B, H, N), F32, IN if bwd else OUT, produced=bwd)
    sc = D ** -0.5
    fwd_args = [regs['q'], regs['k'], regs['v'], regs['o'], lse, ln, B, N, H, D, st['q'], st['k'], st['v'], st['o'], win[0], win[1], sc]
    if not bwd:
        restate = lambda v: dict(zip(('o', 'lse'), ref('attn_fwd', v['q'], v['k'], v['v'], v.get('lengths'), win)))
        return Case(id, 'sconf_attn_fwd', a, fwd_args, 'attn_fwd', restate, variant=f'{got}-wave')
    delta = a.take('delta', 2 * B * H * N, F32, SCRATCH)
    cos = sin = None
    if rot:
        c_, s_ = _rot_tables(N, D)
        cos, sin = put(a, 'rot_cos', c_), put(a, 'rot_sin', s_)
    args = [regs[n] for n in ('q', 'k', 'v', 'o', 'dout')] + [lse, delta, regs['dq'], regs['dk'], regs['dv'], ln, B, N, H, D] + \
           [st[n] for n in ('q', 'k', 'v', 'o', 'dout', 'dq', 'dk', 'dv')] + [win[0], win[1], sc, cos, sin]

    def restate(v):
        r = ref('attn_bwd', v['q'], v['k'], v['v'], None, v['dout'], None, v.get('lengths'), win, rot=(v['rot_cos'], v['rot_sin']) if rot else None)
        return dict(zip(('dq', 'dk', 'dv'), r))
    return Case(id, 'sconf_attn_bwd', a, args, 'attn_bwd', restate, before=[('sconf_attn_fwd', fwd_args)], variant=f'{got}-wave')


for _s in ATTN_SHAPES:
    case('attention', 'sconf_attn_fwd', f'attn_fwd-{_s}', _s, False)(attn_case)
    case('attention', 'sconf_attn_bwd', f'attn_bwd-{_s}', _s, True)(attn_case)
case('attention', 'sconf_attn_bwd', 'attn_bwd-d128-n333-ragged-rot', 'd128-n333-ragged', True, rot=True)(attn_case)
case('attention', 'sconf_attn_bwd', 'attn_bwd-d32-n300-win16-rot', 'd32-n300-win16', True, rot=True)(attn_case)


def attn_maps_case(lib, id, entry, B, N, H, D, lens, win, out_dt=F32):
    a = Arena()
    names = ['q', 'k', 'v', 'o']
    seeds = {'q': 0, 'k': 1, 'v': 2}
    profile = entry == 'sconf_attn_offset_profile'
    if not profile: names = ['q', 'k']
    regs, st = _attn_views(a, names, B, N, H, D, lambda n: SCRATCH if n == 'o' else IN, lambda n: rnd(B, N, H, D, seed=seeds[n]) if n in seeds else None)
    ln = put(a, 'lengths', lens_i32(lens)) if lens else None
    sc = D ** -0.5
    if not profile:
        out = a.take('out', (B, H, N, N), out_dt, OUT, tol=1e-4 if out_dt == F32 else 1e-4 + 2.0 ** -8)
        args = [regs['q'], regs['k'], out, DT[out_dt], ln, B, N, H, D, st['q'], st['k'], win[0], win[1], sc]
        return Case(id, entry, a, args, 'attn_maps_refs.scores_f64', lambda v: {'out': attn_maps_refs.scores_f64(v['q'], v['k'], v.get('lengths'), win)})
    lse = a.take('lse', (B, H, N), F32, IN, produced=True)
    fwd_args = [regs['q'], regs['k'], regs['v'], regs['o'], lse, ln, B, N, H, D, st['q'], st['k'], st['v'], st['o'], win[0], win[1], sc]
    prof = a.take('prof', (B, H, 2 * N - 1), F32, OUT, tol=4e-3)
    nws = int(lib.sconf_attn_offset_profile_workspace(B, N, H, win[0], win[1]))
    ws = a.take('workspace', nws, torch.uint8, SCRATCH)
    args = [regs['q'], regs['k'], lse, prof, ln, B, N, H, D, st['q'], st['k'], win[0], win[1], sc, ws, nws]
    return Case(id, entry, a, args, 'attn_maps_refs.exact_profile_f64', lambda v: {'prof': attn_maps_refs.exact_profile_f64(v['q'], v['k'], v.get('lengths'), win)},
                before=[('sconf_attn_fwd', fwd_args)])


# shapes of test_attn_maps_gpu.py's cases: ragged without a window, a two-sided window over two key tiles, one sample without lengths
case('attention', 'sconf_attn_scores', 'attn_scores-f32', 'sconf_attn_scores', 2, 200, 2, 32, [200, 131], (-1, -1), F32)(attn_maps_case)
case('attention', 'sconf_attn_scores', 'attn_scores-bf16-win', 'sconf_attn_scores', 2, 300, 2, 128, [300, 64], (24, 8), BF)(attn_maps_case)
case('attention', 'sconf_attn_offset_profile', 'attn_offset_profile', 'sconf_attn_offset_profile', 1, 125, 2, 64, None, (-1, -1))(attn_maps_case)
case('attention', 'sconf_attn_offset_profile', 'attn_offset_profile-win', 'sconf_attn_offset_profile', 2, 300, 2, 128, [300, 64], (24, 8))(attn_maps_case)


# ====================================================================================================================== conv module
CONV_SHAPES = {'b3n77d256': (3, 77, 256, [77, 30, 1]), 'b2n37d100': (2, 37, 100, None), 'b2n37d104': (2, 37, 104, None)}


def _conv_inputs(shape, ks):
    B, N, d, lens = CONV_SHAPES[shape]
    g = rnd(B * N, 2 * d)
    w = rnd(d, ks, dtype=F32, seed=1) * 0.3
    bias = rnd(d, dtype=F32, seed=2) * 0.1
    return B, N, d, lens_i32(lens), g, w, bias


def glu_dwconv_case(lib, id, shape, ks):
    B, N, d, lens, g_, w_, b_ = _conv_inputs(shape, ks)
    a = Arena()
    g = put(a, 'g', g_); ln = put(a, 'lengths', lens) if lens is not None else None
    w = put(a, 'w', w_); bias = put(a, 'bias', b_)
    h = a.take('h', (B * N, d), BF, OUT)
    stats = put(a, 'stats', torch.ones(2, d, dtype=F64), ACC, order='fixed', tol=5e-3)      # pre-zeroed by the op layer: the kernel adds
    nws = int(lib.sconf_glu_dwconv_fwd_workspace(B, N, d))
    ws = a.take('workspace', nws, torch.uint8, SCRATCH)

    def restate(v):
        hr, st = ref('glu_dwconv_fwd', v['g'], v.get('lengths'), v['w'], v['bias'], B, N)
        return {'h': hr, 'stats': st + v['stats']}
    return Case(id, 'sconf_glu_dwconv_fwd', a, [g, ln, w, bias, h, stats, ws, nws, B, N, d, ks], 'glu_dwconv_fwd', restate,
                variant=f'{lib.sconf_convmod_tile_frames(B, N, d)} frames per tile')


def _brn_inputs(d):
    return (rnd(d, dtype=F32, seed=3) * 0.1 + 1, rnd(d, dtype=F32, seed=4) * 0.1, rnd(d, dtype=F32, seed=5) * 0.1,
            rnd(d, dtype=F32, seed=6).abs() * 0.2 + 0.8)


def brn_finalize_case(lib, id, shape, training):
    B, N, d, lens, g_, w_, b_ = _conv_inputs(shape, 9)
    _, stats_ = R.glu_dwconv_fwd(g_, lens, w_, b_, B, N)
    bw, bb, rm, rs = _brn_inputs(d)
    a = Arena()
    stats = put(a, 'stats', stats_.contiguous())
    cls = INOUT if training else IN
    rmean = put(a, 'running_mean', rm, cls, tol=1e-5); rstd = put(a, 'running_std', rs, cls, tol=1e-5)
    nbt = put(a, 'num_batches_tracked', torch.tensor([30000], dtype=I64), cls)
    w = put(a, 'weight', bw); b = put(a, 'bias', bb)
    coef = a.take('coef', (6, d), F32, OUT, tol=1e-4)

    def restate(v):
        m, s, n = v['running_mean'].double(), v['running_std'].double(), v['num_batches_tracked'].clone()
        out = {'coef': ref('brn_finalize', v['stats'], B * N, m, s, n, v['weight'], v['bias'], bool(training))}
        if training: out.update(running_mean=m, running_std=s, num_batches_tracked=n)
        return out
    return Case(id, 'sconf_brn_finalize', a, [stats, B * N, rmean, rstd, nbt, w, b, coef, d, training, 1e-3, 0.01], 'brn_finalize', restate)


def _coef(shape, training):
    B, N, d, lens, g_, w_, b_ = _conv_inputs(shape, 9)
    h_, stats_ = R.glu_dwconv_fwd(g_, lens, w_, b_, B, N)
    bw, bb, rm, rs = _brn_inputs(d)
    return h_, R.brn_finalize(stats_, B * N, rm.clone(), rs.clone(), torch.tensor(30000), bw, bb, bool(training))


def affine_silu_case(lib, id, shape):
    B, N, d, *_ = CONV_SHAPES[shape]
    h_, coef_ = _coef(shape, 1)
    a = Arena()
    h = put(a, 'h', h_); coef = put(a, 'coef', coef_); y = a.take('y', (B * N, d), BF, OUT)
    return Case(id, 'sconf_affine_silu_fwd', a, [h, coef, y, B * N, d], 'affine_silu_fwd', lambda v: {'y': ref('affine_silu_fwd', v['h'], v['coef'])})


def convmod_bwd_case(lib, id, shape, ks, training, colsum):
    B, N, d, lens, g_, w_, b_ = _conv_inputs(shape, ks)
    h_, stats_ = R.glu_dwconv_fwd(g_, lens, w_, b_, B, N)
    bw, bb, rm, rs = _brn_inputs(d)
    coef_ = R.brn_finalize(stats_, B * N, rm.clone(), rs.clone(), torch.tensor(30000), bw, bb, bool(training))
    a = Arena()
    dy = put(a, 'dy', rnd(B * N, d, seed=7)); h = put(a, 'h', h_); g = put(a, 'g', g_)
    ln = put(a, 'lengths', lens) if lens is not None else None
    w = put(a, 'w', w_); brn_w = put(a, 'brn_weight', bw); coef = put(a, 'coef', coef_)
    red = put(a, 'red', torch.zeros(2, d, dtype=F64), ACC, order='fixed')                     # PRE-ZEROED scratch the kernel sums into
    bcoef = a.take('bcoef', (3, d), F32, OUT)
    dg = a.take('dg', (B * N, 2 * d), BF, OUT, tol=2e-2)
    dw = put(a, 'dw', rnd(ks, d, dtype=F32, seed=8), ACC, order='fixed', tol=1e-2)            # [k][d], as the kernel accumulates the taps
    dbias = put(a, 'dbias', rnd(d, dtype=F32, seed=9), ACC, order='fixed', tol=1e-2)
    dbw = put(a, 'dbrn_weight', rnd(d, dtype=F32, seed=10), ACC, order='fixed', tol=1e-2)     # one add per channel from the fixed-order red
    dbb = put(a, 'dbrn_bias', rnd(d, dtype=F32, seed=11), ACC, order='fixed', tol=1e-2)
    cs = put(a, 'dg_colsum', rnd(2 * d, dtype=F32, seed=12), ACC, order='fixed', tol=1e-2) if colsum else None
    nws = int(lib.sconf_convmod_bwd_workspace(B, N, d, ks, colsum))
    ws = a.take('workspace', nws, torch.uint8, SCRATCH)

    def restate(v):
        gw, gb, gbw, gbb = torch.zeros(d, ks, dtype=F64), v['dbias'].double(), v['dbrn_weight'].double(), v['dbrn_bias'].double()
        r = ref('convmod_bwd', v['dy'], v['h'], v['g'], v.get('lengths'), v['w'], v['brn_weight'], v['coef'], B, N, bool(training), 1e-3,
                gw, gb, gbw, gbb, colsum=bool(colsum))
        out = {'dg': r[0] if colsum else r, 'dw': v['dw'].double() + gw.t(), 'dbias': gb, 'dbrn_weight': gbw, 'dbrn_bias': gbb}
        # bcoef rows k0, k1, k2 of dh = k0 dz - k1 - xhat0 k2 (kernel_refs.convmod_bwd's A, A S1 / M and k2)
        mean, s_, _, _, A, Bc = v['coef'].double()
        hf = v['h'].double()
        dz = v['dy'].double() * R._dsilu(hf * A + Bc)
        S1, S2, M = dz.sum(0), (dz * (hf - mean) / s_).sum(0), B * N
        sigma = s_ - 1e-3
        zero = torch.zeros_like(A)
        out['bcoef'] = torch.stack([A, A * S1 / M, torch.where(sigma > 0, A * (s_ / sigma) * S2 / M, zero)] if training else [A, zero, zero])
        if colsum: out['dg_colsum'] = v['dg_colsum'].double() + r[1]
        return out
    args = [dy, h, g, ln, w, brn_w, coef, red, bcoef, dg, dw, dbias, dbw, dbb, cs, ws, nws, B, N, d, ks, training, 1e-3]
    return Case(id, 'sconf_convmod_bwd', a, args, 'convmod_bwd', restate, unvalued=['red'],
                variant=f'{lib.sconf_convmod_tile_frames(B, N, d)} frames per tile')


for _i, _s in enumerate(('b3n77d256', 'b2n37d100')):
    for _ks in (3, 9):
        case('convmod', 'sconf_glu_dwconv_fwd', f'glu_dwconv_fwd-{_s}-k{_ks}', _s, _ks)(glu_dwconv_case)
        for _tr in (0, 1):
            case('convmod', 'sconf_convmod_bwd', f'convmod_bwd-{_s}-k{_ks}-train{_tr}-colsum{(_tr + _i + _ks // 9) % 2}', _s, _ks, _tr, (_tr + _i + _ks // 9) % 2)(convmod_bwd_case)
    for _tr in (0, 1):
        case('convmod', 'sconf_brn_finalize', f'brn_finalize-{_s}-train{_tr}', _s, _tr)(brn_finalize_case)
    # sconf_affine_silu_fwd refuses d % 8 != 0 on the host: its ragged width is 104
    case('convmod', 'sconf_affine_silu_fwd', f'affine_silu_fwd-{(_s, "b2n37d104")[_i]}', (_s, 'b2n37d104')[_i])(affine_silu_case)


# ====================================================================================================================== subsampler
SUB_SHAPES = {'b1t131c512': (1, 80, 131, 512), 'b2t77c96': (2, 80, 77, 96), 'b1t70c576': (1, 80, 70, 576), 'b2f24t37c64': (2, 24, 37, 64)}
_half = R._half


def _sub_w(C):
    return (rnd(C, 9, dtype=F32, seed=1) * 0.3, rnd(C, dtype=F32, seed=2) * 0.1, rnd(C, 9, dtype=F32, seed=3) * 0.3, rnd(C, dtype=F32, seed=4) * 0.1)


def sub_conv0_case(lib, id, shape, xd, bwd):
    B, F, T, C = SUB_SHAPES[shape]
    w0, b0, _, _ = _sub_w(C)
    a = Arena()
    x = put(a, 'x', rnd(B, F, T, dtype=xd))
    if not bwd:
        w = put(a, 'w', w0); b = put(a, 'bias', b0); y = a.take('y', (B, _half(T), _half(F), C), BF, OUT)
        return Case(id, 'sconf_sub_conv0_fwd', a, [x, DT[xd], w, b, y, B, F, T, C], 'sub_conv0_fwd', lambda v: {'y': ref('sub_conv0_fwd', v['x'], v['w'], v['bias'])})
    dpre = put(a, 'dpre0', rnd(B, _half(T), _half(F), C, seed=5))
    dw = put(a, 'dw', rnd(C, 9, dtype=F32, seed=6), ACC, order='atomic', tol=5e-3); db = put(a, 'dbias', rnd(C, dtype=F32, seed=7), ACC, order='atomic', tol=5e-3)

    def restate(v):
        gw, gb = v['dw'].double(), v['dbias'].double()
        ref('sub_conv0_bwd_', v['dpre0'], v['x'], gw, gb)
        return {'dw': gw, 'dbias': gb}
    return Case(id, 'sconf_sub_conv0_bwd', a, [dpre, x, DT[xd], dw, db, B, F, T, C], 'sub_conv0_bwd_', restate)


def sub_dwconv_case(lib, id, shape, bwd, colsum=0):
    B, F, T, C = SUB_SHAPES[shape]
    Ti, Fi = _half(T), _half(F)
    _, _, wd, bd = _sub_w(C)
    a = Arena()
    x = put(a, 'pre_in', rnd(B, Ti, Fi, C, seed=5)); w = put(a, 'w', wd)
    if not bwd:
        b = put(a, 'bias', bd); y = a.take('y', (B, _half(Ti), _half(Fi), C), BF, OUT)
        return Case(id, 'sconf_sub_dwconv_fwd', a, [x, w, b, y, B, Ti, Fi, C], 'sub_dwconv_fwd', lambda v: {'y': ref('sub_dwconv_fwd', v['pre_in'], v['w'], v['bias'])})
    dout = put(a, 'dout', rnd(B, _half(Ti), _half(Fi), C, seed=6))
    dpre = a.take('dpre_in', (B, Ti, Fi, C), BF, OUT)
    dw = put(a, 'dw', rnd(C, 9, dtype=F32, seed=7), ACC, order='fixed', tol=5e-3); db = put(a, 'dbias', rnd(C, dtype=F32, seed=8), ACC, order='fixed', tol=5e-3)
    cs = put(a, 'dpre_colsum', rnd(C, dtype=F32, seed=9), ACC, order='atomic', tol=2e-3) if colsum else None
    nws = int(lib.sconf_sub_dwconv_bwd_workspace(B, Ti, Fi, C, colsum))
    ws = a.take('workspace', nws, torch.uint8, SCRATCH)

    def restate(v):
        gw, gb = v['dw'].double(), v['dbias'].double()
        out = {'dpre_in': ref('sub_dwconv_bwd', v['dout'], v['w'], v['pre_in'], gw, gb), 'dw': gw, 'dbias': gb}
        if colsum: out['dpre_colsum'] = v['dpre_colsum'].double() + out['dpre_in'].double().reshape(-1, C).sum(0)
        return out
    return Case(id, 'sconf_sub_dwconv_bwd', a, [dout, w, x, dpre, dw, db, cs, ws, nws, B, Ti, Fi, C], 'sub_dwconv_bwd', restate)


def sub_stage01_case(lib, id, shape, xd, bwd, mfma):
    """mfma: SCONF_SUB_MFMA as the GPU test sets it; the routing is asserted from sconf_sub_stage01_slabs under that setting.  The VALU
    kernels keep the mel and the taps in f32 (their backward the stage-0 activations too): kernel_refs restates them with valu=True,
    without the bf16 operand roundings of the MFMA kernels (at (F,T) = (24,37) the two restatements are 6.1e-3 of max|dw0| apart)."""
    B, F, T, C = SUB_SHAPES[shape]
    w0_, b0_, wd_, bd_ = _sub_w(C)
    slabs = lib.sconf_sub_stage01_slabs(F, C, bwd)
    if shape == 'b1t70c576' and mfma: assert slabs > 1, f'{id}: {slabs} channel slab(s), the case is meant for several'   # 576 = 256 + 256 + 64
    a = Arena()
    x = put(a, 'x', rnd(B, F, T, dtype=xd)); w0 = put(a, 'w0', w0_); b0 = put(a, 'b0', b0_); wd = put(a, 'wd', wd_)
    T4, F4 = _half(_half(T)), _half(_half(F))
    if not bwd:
        bd = put(a, 'bd', bd_); d1 = a.take('d1', (B, T4, F4, C), BF, OUT)
        restate = lambda v: {'d1': ref('sub_stage01_fwd', v['x'], v['w0'], v['b0'], v['wd'], v['bd'], valu=not mfma)}
        return Case(id, 'sconf_sub_stage01_fwd', a, [x, DT[xd], w0, b0, wd, bd, d1, B, F, T, C], 'sub_stage01_fwd', restate,
                    variant=f'{slabs} slab(s), SCONF_SUB_MFMA={int(mfma)}')
    dd1 = put(a, 'dd1', rnd(B, T4, F4, C, seed=5))
    nws = int(lib.sconf_sub_stage01_bwd_workspace(B, F, T, C))
    order = 'fixed' if nws else 'atomic'                               # sconf.h: the MFMA backward sums through the workspace, the VALU one atomically
    g = [put(a, n, rnd(*s, dtype=F32, seed=6 + i), ACC, order=order, tol=5e-3) for i, (n, s) in enumerate((('dw0', (C, 9)), ('db0', (C,)), ('dwd', (C, 9)), ('dbd', (C,))))]
    ws = a.take('workspace', nws, torch.uint8, SCRATCH) if nws else None

    def restate(v):
        gr = [v[n].double() for n in ('dw0', 'db0', 'dwd', 'dbd')]
        ref('sub_stage01_bwd_', v['dd1'], v['x'], v['w0'], v['b0'], v['wd'], *gr, valu=not mfma)
        return dict(zip(('dw0', 'db0', 'dwd', 'dbd'), gr))
    assert bool(nws) == bool(slabs), f'{id}: workspace {nws} B with {slabs} MFMA slab(s)'
    return Case(id, 'sconf_sub_stage01_bwd', a, [dd1, x, DT[xd], w0, b0, wd] + g + [ws, nws, B, F, T, C], 'sub_stage01_bwd_', restate,
                variant=f'{slabs} slab(s), workspace {nws} B, SCONF_SUB_MFMA={int(mfma)}')


def sub_silu_transpose_case(lib, id, bwd):
    Rr, F8, C = 14, 10, 96
    a = Arena()
    pre = put(a, 'pre', rnd(Rr, F8, C, seed=6))
    ds = put(a, 'ds', rnd(Rr, C * F8, seed=7)) if bwd else None
    out = a.take('out', (Rr, F8, C) if bwd else (Rr, C * F8), BF, OUT)
    return Case(id, 'sconf_sub_silu_transpose', a, [bwd, pre, ds, out, Rr, F8, C], 'sub_silu_transpose',
                lambda v: {'out': ref('sub_silu_transpose', v['pre'], v.get('ds'))})


MFMA_OFF = set()                                                       # case ids the GPU test runs under SCONF_SUB_MFMA=0
for _i, _s in enumerate(SUB_SHAPES):
    _xd = (F32, BF)[_i % 2]
    case('subsample', 'sconf_sub_conv0_fwd', f'sub_conv0_fwd-{_s}', _s, _xd, 0)(sub_conv0_case)
    case('subsample', 'sconf_sub_conv0_bwd', f'sub_conv0_bwd-{_s}', _s, _xd, 1)(sub_conv0_case)
    case('subsample', 'sconf_sub_dwconv_fwd', f'sub_dwconv_fwd-{_s}', _s, 0)(sub_dwconv_case)
    case('subsample', 'sconf_sub_dwconv_bwd', f'sub_dwconv_bwd-{_s}-colsum{_i % 2}', _s, 1, _i % 2)(sub_dwconv_case)
    for _mf in (1, 0):
        if not _mf and _s == 'b1t70c576': continue                      # the two-slab shape is about the MFMA kernels
        _sfx = '' if _mf else '-valu'
        case('subsample', 'sconf_sub_stage01_fwd', f'sub_stage01_fwd-{_s}{_sfx}', _s, (_xd, BF if _xd == F32 else F32)[1 - _mf], 0, _mf)(sub_stage01_case)
        case('subsample', 'sconf_sub_stage01_bwd', f'sub_stage01_bwd-{_s}{_sfx}', _s, (_xd, BF if _xd == F32 else F32)[1 - _mf], 1, _mf)(sub_stage01_case)
        if not _mf: MFMA_OFF |= {f'sub_stage01_fwd-{_s}-valu', f'sub_stage01_bwd-{_s}-valu'}
case('subsample', 'sconf_sub_silu_transpose', 'sub_silu_transpose-fwd', 0)(sub_silu_transpose_case)
case('subsample', 'sconf_sub_silu_transpose', 'sub_silu_transpose-bwd', 1)(sub_silu_transpose_case)


# ====================================================================================================================== CTC
def _ctc_inputs(B, N, C, S, logits):
    g = torch.Generator().manual_seed(N + C)
    x = torch.randn(B, N, C, generator=g) * (2.0 if logits else 1.0)
    if not logits: x = torch.log_softmax(x, -1)
    tg = torch.randint(0, C - 1, (B, S), generator=g, dtype=I32)
    tg[0, 1] = tg[0, 0]
    il = torch.full((B,), N, dtype=I32); tl = torch.full((B,), S, dtype=I32)
    il[1] = N - 17; tl[1] = max(1, S // 3); il[-1] = max(2 * S + 1, N // 2)
    return x, tg, il, tl


def _lattice_unspecified(B, N, L, il, tl):
    """sconf.h: alpha / beta at frames >= input_lengths[b] or states >= 2 * target_lengths[b] + 1, and the offsets of those frames,
    are unspecified."""
    t = torch.arange(N)[None, :, None] >= il[:, None, None].long()
    s = torch.arange(L)[None, None, :] >= (2 * tl[:, None, None].long() + 1)
    lat = (t | s).expand(B, N, L).clone()
    offs = torch.cat([(torch.arange(N)[None, :] >= il[:, None].long()).reshape(-1)] * 2 + [torch.zeros(B, dtype=torch.bool)])
    return lat, offs


def ctc_case(lib, id, B, N, C, S, logits, bwd, colsum=0):
    x_, tg_, il_, tl_ = _ctc_inputs(B, N, C, S, logits)
    L = 2 * S + 1
    blank = C - 1
    lat_u, offs_u = _lattice_unspecified(B, N, L, il_, tl_)
    a = Arena()
    x = put(a, 'x', x_); tg = put(a, 'targets', tg_); il = put(a, 'input_lengths', il_); tl = put(a, 'target_lengths', tl_)
    cls = IN if bwd else OUT
    kw = dict(produced=True) if bwd else {}
    lse = a.take('lse', (B, N), F32, cls, **kw) if logits else None
    lpg = a.take('lpg', (B, N, L), F32, cls, **kw)                      # the emission gather fills every frame and state
    alpha, beta = (a.take(n, (B, N, L), F32, cls, unspecified=None if bwd else lat_u, **kw) for n in ('alpha', 'beta'))
    offs = a.take('offs', 2 * B * N + B, F64, cls, unspecified=None if bwd else offs_u, **kw)
    nll = a.take('nll', B, F32, cls, tol=1e-4, **kw)
    fwd_args = [x, tg, il, tl] + ([lse] if logits else []) + [lpg, alpha, beta, offs, nll, B, N, C, S, blank]
    fwd = 'sconf_ctc_fwd_logits' if logits else 'sconf_ctc_fwd'
    if not bwd:
        def restate(v):
            out = {'nll': ref('ctc_fwd_logits' if logits else 'ctc_fwd', v['x'], v['targets'], v['input_lengths'], v['target_lengths'], blank)[0]}
            # the emission gather: lpg[b,t,s] = log-prob of state s's label (blank at even s), 0 outside the sample's frames and states
            x64 = v['x'].double()
            live_t = torch.arange(N)[None, :] < v['input_lengths'][:, None].long()
            if logits:
                lse64 = torch.logsumexp(x64, -1)
                out['lse'] = lse64 * live_t
                x64 = x64 - lse64[..., None]
            lab = torch.full((B, L), blank, dtype=torch.long)
            lab[:, 1::2] = v['targets'].long()
            live_s = torch.arange(L)[None, :] < (2 * v['target_lengths'][:, None].long() + 1)
            out['lpg'] = torch.gather(x64, 2, lab[:, None, :].expand(B, N, L)) * (live_t[:, :, None] & live_s[:, None, :])
            return out
        return Case(id, fwd, a, fwd_args, 'ctc_fwd_logits' if logits else 'ctc_fwd', restate, unvalued=['alpha', 'beta', 'offs'])
    go = put(a, 'grad_out', torch.tensor([1.0, 0.5, 2.0][:B]))
    if not logits:
        grad = a.take('grad', (B, N, C), F32, OUT, tol=2e-4, order='atomic')     # sconf.h: label occupancies are summed with atomics
        args = [x, lpg, alpha, beta, offs, nll, tg, il, tl, go, grad, B, N, C, S, blank]
        restate = lambda v: {'grad': ref('ctc_bwd', v['x'], None, None, v['targets'], v['input_lengths'], v['target_lengths'], v['grad_out'], blank)}
        return Case(id, 'sconf_ctc_bwd', a, args, 'ctc_bwd', restate, before=[(fwd, fwd_args)])
    dl = a.take('dlogits', (B, N, C), BF, OUT, tol=1.5e-2, order='atomic')
    cs = put(a, 'colsum_out', rnd(C, dtype=F32, seed=3), ACC, order='atomic', tol=1e-2) if colsum else None
    nws = int(lib.sconf_ctc_bwd_logits_workspace(B * N, C)) if colsum else 0
    ws = a.take('workspace', nws, F32, SCRATCH) if colsum else None
    args = [x, lse, lpg, alpha, beta, offs, nll, tg, il, tl, go, dl, cs, ws, B, N, C, S, blank]

    def restate(v):
        acc = v['colsum_out'].double() if colsum else None
        out = {'dlogits': ref('ctc_bwd_logits', v['x'], None, None, v['targets'], v['input_lengths'], v['target_lengths'], v['grad_out'], blank, colsum_into=acc)}
        if colsum: out['colsum_out'] = acc
        return out
    return Case(id, 'sconf_ctc_bwd_logits', a, args, 'ctc_bwd_logits', restate, before=[(fwd, fwd_args)])


for _n, _sh in (('b3n125s31', (3, 125, 128, 31)), ('b2n700s300-long', (2, 700, 128, 300))):
    case('ctc', 'sconf_ctc_fwd', f'ctc_fwd-{_n}', *_sh, False, False)(ctc_case)
    case('ctc', 'sconf_ctc_bwd', f'ctc_bwd-{_n}', *_sh, False, True)(ctc_case)
case('ctc', 'sconf_ctc_fwd_logits', 'ctc_fwd_logits-b3n64s10', 3, 64, 32, 10, True, False)(ctc_case)
for _cs in (0, 1):
    case('ctc', 'sconf_ctc_bwd_logits', f'ctc_bwd_logits-b3n64s10-colsum{_cs}', 3, 64, 32, 10, True, True, _cs)(ctc_case)


# ====================================================================================================== evaluation and augmentation
@case('eval', 'sconf_overlap_add_exp', 'overlap_add_exp-windows', False)
@case('eval', 'sconf_overlap_add_exp', 'overlap_add_exp-second-w1', True)
def overlap_add_case(lib, id, second):
    """second: the ragged last window as a W = 1 call into the acc / count the first call left."""
    C, n, W, stride, N, pos0 = 128, 29, 5, 21, 200, 7
    g = torch.Generator().manual_seed(3)
    lp = torch.log_softmax(torch.randn(W, n, C, generator=g), -1)
    lp2 = torch.log_softmax(torch.randn(1, 13, C, generator=g), -1)
    acc0, cnt0 = rnd(N, C, dtype=F32, seed=1).abs(), torch.ones(N)
    a = Arena()
    acc = put(a, 'acc', acc0, ACC, order='atomic', tol=1e-5); cnt = put(a, 'count', cnt0, ACC, order='atomic', tol=0.0)
    first = [put(a, 'logp', lp), W, n, C, stride, pos0, acc, cnt, N]
    if not second:
        def restate(v):
            ac, c = v['acc'].double(), v['count'].double()
            R.overlap_add_exp_(v['logp'].double(), ac, c, pos0, stride)
            return {'acc': ac, 'count': c}
        return Case(id, 'sconf_overlap_add_exp', a, first, 'overlap_add_exp_', restate)
    p2 = pos0 + (W - 1) * stride + n - 4

    def restate2(v):                                                   # acc / count as the first call left them, plus the one window
        ac, c = v['acc'].double(), v['count'].double()
        R.overlap_add_exp_(v['logp2'].double(), ac, c, p2, 13)
        return {'acc': ac, 'count': c}
    return Case(id, 'sconf_overlap_add_exp', a, [put(a, 'logp2', lp2), 1, 13, C, 13, p2, acc, cnt, N], 'overlap_add_exp_', restate2,
                before=[('sconf_overlap_add_exp', first)])


@case('eval', 'sconf_overlap_finalize', 'overlap_finalize')
def overlap_finalize_case(lib, id):
    N, C, rows = 93, 128, 90
    a = Arena()
    acc = put(a, 'acc', rnd(N, C, dtype=F32, seed=1).abs() + 0.1); cnt = put(a, 'count', torch.randint(1, 4, (N,), generator=torch.Generator().manual_seed(0)).float())
    out = a.take('out', (rows, C), F32, OUT, tol=1e-5)
    return Case(id, 'sconf_overlap_finalize', a, [acc, cnt, out, rows, C], 'overlap_finalize', lambda v: {'out': ref('overlap_finalize', v['acc'], v['count'], rows)})


@case('eval', 'sconf_argmax_rows', 'argmax_rows')
def argmax_case(lib, id):
    M, C = 301, 132
    x_ = rnd(M, C, dtype=F32); x_[5, 100] = x_[5, 30] = 9.0; x_[6] = 0.0
    a = Arena()
    x = put(a, 'x', x_); idx = a.take('idx', M, I32, OUT, tol=0.0)
    return Case(id, 'sconf_argmax_rows', a, [x, M, C, idx], 'argmax_rows', lambda v: {'idx': R.argmax_rows(v['x'])})


@case('eval', 'sconf_copy_row_spans', 'copy_row_spans')
def copy_row_spans_case(lib, id):
    """Rows of dst outside every span keep their content: INOUT, the restatement starts from the initial dst."""
    W, n, C, N = 3, 20, 36, 50
    spans_ = torch.tensor([[2, 10, 0], [0, 7, 15], [5, 15, 30]], dtype=I32)
    a = Arena()
    src = put(a, 'src', rnd(W, n, C, dtype=F32)); spans = put(a, 'spans', spans_); dst = put(a, 'dst', rnd(N, C, dtype=F32, seed=1), INOUT, tol=0.0)

    def restate(v):
        d = v['dst'].clone(); eval_refs.copy_row_spans_(v['src'], v['spans'], d)
        return {'dst': d}
    return Case(id, 'sconf_copy_row_spans', a, [src, W, n, C, spans, dst, N], 'eval_refs.copy_row_spans_', restate)


@case('eval', 'sconf_edit_counts', 'edit_counts-short-nows', False)
@case('eval', 'sconf_edit_counts', 'edit_counts-long-ref-ws', True)
def edit_counts_case(lib, id, long_ref):
    import numpy as np
    rng = np.random.default_rng(5)
    if long_ref:
        n = lib.sconf_edit_pass_cols() + 37
        pairs = [eval_refs.random_pair(rng, 23, n, 50), eval_refs.random_pair(rng, 5, 9, 50)]
    else:
        pairs = [eval_refs.random_pair(rng, 17, 21, 30), eval_refs.random_pair(rng, 0, 4, 30), eval_refs.random_pair(rng, 40, 33, 30)]
    hyp_, ho_ = eval_refs.ragged([h for h, _ in pairs]); ref_, ro_ = eval_refs.ragged([r for _, r in pairs])
    P = len(pairs)
    nws = int(lib.sconf_edit_counts_workspace(P, max(len(h) for h, _ in pairs), max(len(r) for _, r in pairs)))
    assert bool(nws) == long_ref
    a = Arena()
    hyp = put(a, 'hyp', hyp_); ho = put(a, 'hyp_off', ho_); rf = put(a, 'ref', ref_); ro = put(a, 'ref_off', ro_)
    out = a.take('out', (P, 4), I64, OUT, tol=0.0)
    ws = a.take('workspace', nws, torch.uint8, SCRATCH) if nws else None
    return Case(id, 'sconf_edit_counts', a, [hyp, ho, rf, ro, P, out, ws, nws], 'eval_refs.edit_counts',
                lambda v: {'out': eval_refs.edit_counts(v['hyp'], v['hyp_off'], v['ref'], v['ref_off'])})


@case('eval', 'sconf_spec_mask', 'spec_mask-broadcast', 0)
@case('eval', 'sconf_spec_mask', 'spec_mask-batch-stride', 1)
def spec_mask_case(lib, id, batched):
    B, F, T = 3, 24, 101
    a = Arena()
    bstride = F * T + 12 if batched else 0                               # a batch stride of its own: the gap is a guard
    src_ = rnd(B if batched else 1, F, T, dtype=F32)
    src = a.take('src', tuple(src_.shape), F32, IN, strides=(bstride or F * T, T, 1), init=src_)
    dst = a.take('dst', (B, F, T), F32, OUT, tol=0.0)
    t_iv = put(a, 't_iv', torch.tensor([[[3, 9], [50, 50]], [[0, 4], [90, 101]], [[7, 7], [20, 33]]], dtype=I32))
    f_iv = put(a, 'f_iv', torch.tensor([[[2, 5]], [[0, 0]], [[20, 24]]], dtype=I32))
    mv = put(a, 'mask_value', torch.tensor([0.25]))
    restate = lambda v: {'dst': dyneval_refs.spec_mask(v['src'], v['t_iv'], v['f_iv'], v['mask_value'].reshape(()), B)}
    return Case(id, 'sconf_spec_mask', a, [src, bstride, dst, B, F, T, t_iv, 2, f_iv, 1, mv], 'dyneval_refs.spec_mask', restate)


@case('eval', 'sconf_mean_f32', 'mean_f32', False)
@case('eval', 'sconf_mean_f32', 'mean_f32-lengths', True)
def mean_case(lib, id, with_len):
    B, Rr, T = 3, 7, 211
    a = Arena()
    x = put(a, 'x', rnd(B, Rr, T, dtype=F32) + 0.5)
    ln = put(a, 'lengths', ints(211, 100, 1)) if with_len else None
    out = a.take('out', 1, F32, OUT, tol=1e-5)
    nws = int(lib.sconf_mean_f32_workspace(B * Rr * T))
    ws = a.take('workspace', nws, torch.uint8, SCRATCH)
    return Case(id, 'sconf_mean_f32', a, [x, B, Rr, T, ln, out, ws, nws], 'dyneval_refs.mean_f32',
                lambda v: {'out': dyneval_refs.mean_f32(v['x'], v.get('lengths')).reshape(1)})


@case('eval', 'sconf_ctc_collapse', 'ctc_collapse')
def ctc_collapse_case(lib, id):
    B, N, C, cap = 3, 61, 20, 61
    x_ = rnd(B, N, C, dtype=F32)
    ln_ = ints(61, 30, 0)
    a = Arena()
    x = put(a, 'x', x_); ln = put(a, 'lengths', ln_)
    idx = a.take('idx', B * N, I32, OUT, tol=0.0)                      # every frame's arg-max, behind the lengths too
    tg = a.take('targets', (B, cap), I32, OUT, tol=0.0); tl = a.take('target_lengths', B, I32, OUT, tol=0.0)

    def restate(v):
        t, l = dyneval_refs.ctc_collapse(v['x'], v['lengths'], C - 1, cap)
        return {'targets': t, 'target_lengths': l, 'idx': torch.argmax(v['x'], -1).reshape(-1).to(I32)}
    return Case(id, 'sconf_ctc_collapse', a, [x, B, N, C, ln, C - 1, idx, tg, cap, tl], 'dyneval_refs.ctc_collapse', restate)


# ====================================================================================================================== optimiser
# sconf_sumsq_workspace(n) is 8 bytes per workgroup for every n > 0: the smallest n with a workspace is 1, and no NULL form exists
@case('optim', 'sconf_sumsq', 'sumsq-n1', 1)
@case('optim', 'sconf_sumsq', 'sumsq-n4099', 4099)
@case('optim', 'sconf_sumsq', 'sumsq-n300001', 300001)
def sumsq_case(lib, id, n):
    nws = int(lib.sconf_sumsq_workspace(n))
    assert nws > 0
    a = Arena()
    g = put(a, 'g', rnd(n, dtype=F32)); out = put(a, 'out', torch.tensor([3.0], dtype=F64), ACC, order='fixed', tol=1e-5)
    ws = a.take('workspace', nws, torch.uint8, SCRATCH)
    return Case(id, 'sconf_sumsq', a, [g, n, out, ws, nws], 'sumsq_', lambda v: {'out': ref('sumsq_', v['g'], v['out'].clone())},
                variant=f'{nws // 8} workgroup sum(s)')


@case('optim', 'sconf_madgrad_step', 'madgrad_step-k0-shadow', 0, True, False)
@case('optim', 'sconf_madgrad_step', 'madgrad_step-kdev3-noshadow', 3, False, True)
@case('optim', 'sconf_madgrad_step', 'madgrad_step-k2-shadow-wd', 2, True, False)
def madgrad_case(lib, id, k, shadow, kdev):
    n = 4 * 1031                                                         # a multiple of 4 and of nothing larger
    a = Arena()
    p = put(a, 'p', rnd(n, dtype=F32, seed=1), INOUT, tol=1e-5); g = put(a, 'g', rnd(n, dtype=F32, seed=2))
    gss = put(a, 'grad_sum_sq', rnd(n, dtype=F32, seed=3).abs() if k else torch.zeros(n), INOUT, tol=1e-5)
    s = put(a, 's', rnd(n, dtype=F32, seed=4) * 0.1 if k else torch.zeros(n), INOUT, tol=1e-5)
    x0 = put(a, 'x0', rnd(n, dtype=F32, seed=5), IN) if k else a.take('x0', n, F32, OUT, tol=0.0)   # k == 0: the kernel creates x0 := p
    sh = a.take('bf16_shadow', n, BF, OUT) if shadow else None
    sq = put(a, 'sumsq', (rnd(n, dtype=F32, seed=2).double() ** 2).sum().reshape(1))
    kd = put(a, 'k_dev', torch.tensor([k], dtype=I64)) if kdev else None
    hp = dict(max_norm=0.8, grad_scale=1.0, lr=3e-3, momentum=0.9, eps=1e-6, wd=1e-2 if k == 2 else 0.0)

    def restate(v):
        pp, gg, ss = v['p'].double(), v['grad_sum_sq'].double(), v['s'].double()
        xx = v['x0'].double() if k else torch.zeros(n, dtype=F64)
        shd = torch.zeros(n, dtype=BF) if shadow else None
        R.madgrad_step_(pp, v['g'].double(), gg, ss, xx, shd, v['sumsq'], hp['max_norm'], hp['grad_scale'], hp['lr'], hp['momentum'], hp['eps'], hp['wd'], k)
        out = {'p': pp, 'grad_sum_sq': gg, 's': ss}
        if not k: out['x0'] = xx
        if shadow: out['bf16_shadow'] = shd
        return out
    args = [p, g, gss, s, x0, sh, n, sq, hp['max_norm'], hp['grad_scale'], hp['lr'], hp['momentum'], hp['eps'], hp['wd'], 0 if kdev else k, kd]
    return Case(id, 'sconf_madgrad_step', a, args, 'madgrad_step_', restate)


@case('optim', 'sconf_madgrad_advance', 'madgrad_advance')
def madgrad_advance_case(lib, id):
    a = Arena()
    k = put(a, 'k_dev', torch.tensor([6], dtype=I64), INOUT, tol=0.0); sq = put(a, 'sumsq', torch.tensor([2.5], dtype=F64))
    return Case(id, 'sconf_madgrad_advance', a, [k, sq, 1.0], 'madgrad_advance_', lambda v: {'k_dev': v['k_dev'] + 1})


FAMILIES = ('gemm128', 'gemm256', 'norm', 'rows', 'attention', 'convmod', 'subsample', 'ctc', 'eval', 'optim')
assert {f for f, _, _ in CASES.values()} == set(FAMILIES)
