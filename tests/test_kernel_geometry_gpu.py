"""GPU parity tests at the sizes where the launch geometry of the hot-path kernels changes: grid caps followed by grid-stride loops,
persistent waves that walk several rows, several rows per workgroup of the fixed-order column-sum slabs, the taller time tiles of the
conv module.  test_kernels_gpu.py compares every entry point with a reference below those thresholds; training runs above them.

Every case (1) ASSERTS that it reached the branch it is for, reading the choice from the library's own queries where one exists
(workspace sizes, sconf_convmod_tile_frames, sconf_num_cus) and otherwise sizing itself at >= 2.5 x the capped grid's reach (the source
line is named next to the size in geometry_cases.py), and prints the geometry on one `[geometry]` line; (2) checks
  * row-independent outputs BIT FOR BIT, row block by row block, against a small call over a slice of the same rows (first pass, middle
    of a later pass, ragged end) that takes the one-trip branch: same arithmetic per row, so any difference is an indexing fault.
    Three of them get an equal or stronger exact check instead: cast and mask_rows are exact operations, so the WHOLE output must
    equal torch's bit for bit (cast also against slice calls); softmax / fused-CTC dx with the column sums (several rows per workgroup)
    must equal, over ALL rows, the same call without them (one row per workgroup).  The rows of sconf_overlap_add_exp that two
    windows cover are sums of two terms, compared with the float64 restatement; its other rows and sconf_overlap_finalize bit for bit;
  * reductions and everything else against the float64 restatement of the op (tests/kernel_refs.py evaluated in float64 on the CPU)
    with the tolerances test_kernels_gpu.py uses for that op.
test_kernel_geometry_refs.py checks those references against their float32 form without a GPU."""
import pytest
import torch

import geometry_cases as G
import kernel_refs as R
from kernel_test_utils import BF, F32, F64, TOL_BF16, TOL_F32, close, dev, ref, rnd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import lcasr_amd.hip.ops as o
    o._lib.load()
    return o


def lib_():
    from lcasr_amd.hip import _lib
    return _lib.load()


def cdiv(a, b):
    return -(-a // b)


def geometry(what, **kw):
    print(f'[geometry] {what}: ' + ', '.join(f'{k}={v}' for k, v in kw.items()))


def same_bits(a, b, name):
    assert a.shape == b.shape and a.dtype == b.dtype, name
    assert torch.equal(a, b), f'{name}: {int((a != b).sum())} of {a.numel()} elements differ, max |diff| {float((a.float() - b.float()).abs().max()):.3e}'


def check(out, refs, tols, what):
    for k, t in tols.items():
        if out.get(k) is not None:
            tol, floor = t if isinstance(t, tuple) else (t, 0.0)
            close(out[k], refs[k], tol=tol, floor=floor, name=f'{what} {k}')


# ---------------------------------------------------------------------------------------------------------------- norms
@pytest.mark.parametrize('mode', ['layer_norm', 'rms_norm', 'rms_norm_apex'])
@pytest.mark.parametrize('d', [768, 1028, 2048])
def test_norm_bwd_several_rows_per_wave(ops, mode, d):
    """sconf_norm_bwd with its grid capped at one workgroup per CU: every wave walks 3 rows (row-ahead loads, for d > 1024 the
    double-buffered exchange of the two half-row sums and the clamped dead trip of the ragged end), and norm_bwd_reduce_kernel adds
    more than 48 workgroups' slabs (its 4-way unrolled loop)."""
    lib = lib_()
    cus = lib.sconf_num_cus()
    cs_ = 2 if d > 1024 else 1                                        # waves per row (norm.hip launch_bwd: CS)
    nw = G.norm_bwd_waves(d, cus)
    M = G.rows_for_trips(nw)
    grid = lib.sconf_norm_bwd_workspace(M, d) // (3 * d)
    assert grid == cus and grid * G.NORM_WAVES // cs_ == nw, 'grid not capped at one workgroup per CU'
    trips = cdiv(M, nw)
    assert trips >= 3 and M % nw != 0 and grid > 48
    geometry(f'norm_bwd {mode} d={d}', M=M, workgroups=grid, waves_per_row=cs_, trips=trips, last_trip_rows=M % nw)
    eps = G.eps_of(mode)
    for xd, gd, od in ((F32, BF, F32), (BF, F32, BF)):
        inp = G.norm_inputs(mode, d, M, xd, gd)
        want = G.norm_ref(inp, mode, F64)
        x, w, b, dy, dres = (dev(inp[k]) for k in ('x', 'w', 'b', 'dy', 'dres'))
        _, mean, rstd = ops.norm_fwd(x, w, b, mode, eps, BF)
        zeros = lambda: (torch.zeros(d).cuda(), torch.zeros(d).cuda() if b is not None else None)
        dw, db = zeros()
        got = ops.norm_bwd(dy, x, w, mean, rstd, mode, eps, dres, od, dw, db, twin=True)
        dx = got[0] if od == F32 else got
        check(dict(dx=dx, dw=dw, db=db), want, dict(dx=5e-3, dw=5e-3, db=5e-3), f'norm_bwd {mode} d={d} {xd}')
        if od == F32:                                                 # twin outputs: the bf16 copy and its column sums
            same_bits(got[1], dx.to(BF), 'dx16')
            close(got[2], got[1].double().sum(0).cpu(), tol=2e-3, name='twin column sums')
        dw0, db0 = zeros()                                            # dres = None
        dx0 = ops.norm_bwd(dy, x, w, mean, rstd, mode, eps, None, od, dw0, db0)
        close(dx0, G.norm_ref(inp, mode, F64, with_dres=False)['dx'], tol=5e-3, name='norm_bwd dx without dres')
        same_bits(dw0, dw, 'dw does not depend on dres')
        for a, e in G.row_slices(M, nw):                              # row blocks against the one-trip branch
            assert lib.sconf_norm_bwd_workspace(e - a, d) // (3 * d) * G.NORM_WAVES // cs_ >= e - a, 'slice does not take the one-trip branch'
            dws, dbs = zeros()
            small = ops.norm_bwd(dy[a:e], x[a:e], w, mean[a:e], rstd[a:e], mode, eps, dres[a:e], od, dws, dbs, twin=True)
            if od == F32:
                same_bits(small[0], dx[a:e], f'dx rows {a}:{e}'); same_bits(small[1], got[1][a:e], f'dx16 rows {a}:{e}')
            else:
                same_bits(small, dx[a:e], f'dx rows {a}:{e}')
            same_bits(ops.norm_bwd(dy[a:e], x[a:e], w, mean[a:e], rstd[a:e], mode, eps, None, od, dws, dbs), dx0[a:e], f'dx (no dres) rows {a}:{e}')


@pytest.mark.parametrize('twice', [False, True])
@pytest.mark.parametrize('d', [260, 768])
def test_norm2_bwd_several_rows_per_wave(ops, d, twice):
    """sconf_norm2_bwd with its grid capped: 3 rows per wave, ragged last trip (row-ahead loads in the two-norm form)."""
    lib = lib_()
    cus = lib.sconf_num_cus()
    nw = cus * G.NORM_WAVES
    M = G.rows_for_trips(nw)
    grid = lib.sconf_norm2_bwd_workspace(M, d) // (5 * d)
    assert grid == cus, 'grid not capped at one workgroup per CU'
    trips = cdiv(M, nw)
    assert trips >= 3 and M % nw != 0 and grid > 48
    geometry(f'norm2_bwd d={d} twice={twice}', M=M, workgroups=grid, trips=trips, last_trip_rows=M % nw)
    inp = G.norm2_inputs(d, M)
    want = G.norm2_ref(inp, twice, F64)
    x, w1, b1, w2, b2, dh2, dres = (dev(inp[k]) for k in ('x', 'w1', 'b1', 'w2', 'b2', 'dh2', 'dres'))
    y1, h2, st = ops.norm2_fwd(x, w1, b1, w2, b2, 1e-5, 1e-5, twice)
    check(dict(y1=y1, h2=h2), want, dict(y1=TOL_F32, h2=TOL_BF16), 'norm2_fwd')
    zeros = lambda: [torch.zeros(d).cuda() for _ in range(4)]
    for with_dres in (True, False):
        r = dres if with_dres else None
        g = zeros()
        dx, dx16, cs = ops.norm2_bwd(dh2, x, w1, b1, w2, b2, st, r, *g, twin=True)
        w_ = want if with_dres else G.norm2_ref(inp, twice, F64, with_dres=False)
        check(dict(dx=dx, dw1=g[0], db1=g[1], dw2=g[2], db2=g[3]), w_, {k: 5e-3 for k in ('dx', 'dw1', 'db1', 'dw2', 'db2')}, f'norm2_bwd dres={with_dres}')
        same_bits(dx16, dx.to(BF), 'dx16')
        close(cs, dx16.double().sum(0).cpu(), tol=2e-3, name='twin column sums')
        same_bits(ops.norm2_bwd(dh2, x, w1, b1, w2, b2, st, r, *zeros()), dx, 'dx without the twin')
        for a, e in G.row_slices(M, nw):
            assert lib.sconf_norm2_bwd_workspace(e - a, d) // (5 * d) * G.NORM_WAVES >= e - a
            small = ops.norm2_bwd(dh2[a:e], x[a:e], w1, b1, w2, b2, tuple(s[a:e] for s in st), None if r is None else r[a:e], *zeros(), twin=True)
            same_bits(small[0], dx[a:e], f'dx rows {a}:{e}'); same_bits(small[1], dx16[a:e], f'dx16 rows {a}:{e}')


@pytest.mark.parametrize('mode', ['layer_norm', 'rms_norm', 'rms_norm_apex'])
@pytest.mark.parametrize('d', [4, 68, 260, 772, 1028])
def test_norm_widths(ops, mode, d):
    """Widths the header promises (d % 4 == 0, d <= 2048) around the kernels' column steps: one live lane (4), a partly filled first
    256-column iteration (68), just over one and three iterations (260, 772), just over the two-wave split of the backward (1028: the
    upper-half wave has one live lane)."""
    M, eps = 37, G.eps_of(mode)
    geometry(f'norm {mode} d={d}', M=M, column_iterations=cdiv(d, 256), live_lanes_of_last=cdiv(d - (cdiv(d, 256) - 1) * 256, 4))
    for xd, yd in ((F32, BF), (F32, F32), (BF, BF)):
        inp = G.norm_inputs(mode, d, M, xd, yd)
        want = G.norm_ref(inp, mode, F64)
        x, w, b, dy, dres = (dev(inp[k]) for k in ('x', 'w', 'b', 'dy', 'dres'))
        y, mean, rstd = ops.norm_fwd(x, w, b, mode, eps, yd)
        close(y, want['y'], name=f'norm_fwd {mode} d={d} {xd}->{yd}'); close(rstd, want['rstd'], name='rstd')
        dw, db = torch.zeros(d).cuda(), (torch.zeros(d).cuda() if b is not None else None)
        dx, dx16, cs = ops.norm_bwd(dy, x, w, mean, rstd, mode, eps, dres, F32, dw, db, twin=True)
        check(dict(dx=dx, dw=dw, db=db), want, dict(dx=5e-3, dw=5e-3, db=5e-3), f'norm_bwd {mode} d={d}')
        same_bits(dx16, dx.to(BF), 'dx16')
        close(cs, dx16.double().sum(0).cpu(), tol=2e-3, name='twin column sums')


@pytest.mark.parametrize('d', [4, 68, 260, 772])
def test_norm2_widths_and_rejection(ops, d):
    """The fused pair of LayerNorms at the widths of test_norm_widths inside its documented domain (include/sconf.h: d <= 768), forward
    and backward, both forms; d = 772 is outside it and must be rejected with a message, not computed."""
    M = 37
    geometry(f'norm2 d={d}', M=M, column_iterations=cdiv(d, 256), live_lanes_of_last=cdiv(d - (cdiv(d, 256) - 1) * 256, 4), rejected=d > 768)
    inp = G.norm2_inputs(d, M)
    for twice in (False, True):
        x, w1, b1, w2, b2, dh2, dres = (dev(inp[k]) for k in ('x', 'w1', 'b1', 'w2', 'b2', 'dh2', 'dres'))
        if d > 768:
            with pytest.raises(RuntimeError, match='768'):
                ops.norm2_fwd(x, w1, b1, w2, b2, 1e-5, 1e-5, twice)
            continue
        want = G.norm2_ref(inp, twice, F64)
        y1, h2, st = ops.norm2_fwd(x, w1, b1, w2, b2, 1e-5, 1e-5, twice)
        g = [torch.zeros(d).cuda() for _ in range(4)]
        dx = ops.norm2_bwd(dh2, x, w1, b1, w2, b2, st, dres, *g)
        check(dict(y1=y1, h2=h2, dx=dx, dw1=g[0], db1=g[1], dw2=g[2], db2=g[3]), want, G.NORM2_TOL, f'norm2 d={d} twice={twice}')


# -------------------------------------------------------------------------------------------------------------- softmax
@pytest.mark.parametrize('C,M', [(132, 37), (8192, 37), (132, 2 * 2048 + 77)])
def test_softmax_widths_and_rows_per_workgroup(ops, C, M):
    """C = 132: one thread past the first wave's columns; C = 8192: every register iteration full (the header's limit).  M = 4173 with
    the column sums: 3 rows per workgroup (more rows than slabs), ragged last workgroup."""
    lib = lib_()
    ws = lib.sconf_softmax_bwd_workspace(M, C)
    saturated = ws == lib.sconf_softmax_bwd_workspace(4 * M, C)       # the slab count stops growing once rows per workgroup > 1
    assert saturated == (M > 2048), 'rows per workgroup of the fused column sums'
    slabs = min(M, 2048)
    geometry(f'softmax C={C}', M=M, register_iterations=cdiv(C, 1024), rows_per_workgroup=cdiv(M, slabs), workgroups=cdiv(M, cdiv(M, slabs)))
    for log, xd, yd in ((False, BF, BF), (True, F32, F32), (False, F32, F32)):
        inp = G.softmax_inputs(M, C, xd, yd)
        inp['y_in'] = R.softmax_fwd(inp['x'], log, yd)
        want = G.softmax_ref(inp, log, F64)
        y = ops.softmax_fwd(dev(inp['x']), log, yd)
        if log: assert float((y.double().cpu() - want['y']).abs().max()) < 2e-3, 'log_softmax abs err'
        else: close(y, want['y'], name=f'softmax C={C}')
        dx = ops.softmax_bwd(dev(inp['y_in']), dev(inp['dy']), log, BF)
        close(dx, want['dx'], name=f'softmax_bwd log={log} C={C}')
        cs = torch.ones(C).cuda()
        dx2 = ops.softmax_bwd(dev(inp['y_in']), dev(inp['dy']), log, BF, colsum_into=cs)
        same_bits(dx2, dx, 'dx with the column sums (several rows per workgroup) vs without (one)')
        close(cs, 1.0 + dx.double().sum(0).cpu(), tol=2e-3, name='softmax_bwd column sums')


# ---------------------------------------------------------------------------------------------------------- conv module
def _conv_geometry(lib, B, N, d, what):
    tn, rpt = lib.sconf_convmod_tile_frames(B, N, d), lib.sconf_convmod_bwd_rows_per_thread(B, N, d)
    cpb = min(64, d // 4); spbk = 256 // cpb
    gx = lib.sconf_glu_dwconv_fwd_workspace(B, N, d) // (16 * d)
    assert gx == cdiv(B * cdiv(N, tn), spbk), 'tile height and the forward grid disagree'
    geometry(what, B=B, N=N, d=d, TN=tn, rows_per_thread=rpt, grid_x=gx, grid_y=cdiv(d // 4, cpb), channel_groups_per_workgroup=cpb, slabs_per_workgroup=spbk)
    return tn, rpt


def _conv_case(ops, B, N, d, ks, lens, trainings):
    inp = G.convmod_inputs(B, N, d, ks, lens)
    want = G.convmod_ref(inp, F64, trainings)
    g, w, bias, ln, bw, dy, h_in = (dev(inp[k]) for k in ('g', 'w', 'bias', 'ln', 'bw', 'dy', 'h_in'))
    h, stats = ops.glu_dwconv_fwd(g, ln, w, bias, B, N)
    got = dict(h=h, stats=stats)
    for t in trainings:
        gg = [torch.zeros(d, ks).cuda(), torch.zeros(d).cuda(), torch.zeros(d).cuda(), torch.zeros(d).cuda()]
        dg, cs = ops.convmod_bwd(dy, h_in, g, ln, w, bw, dev(inp['coef'][t]), B, N, t, 1e-3, *gg, colsum=True)
        got.update({f'dg{int(t)}': dg, f'cs{int(t)}': cs, f'ddw{int(t)}': gg[0], f'dbdw{int(t)}': gg[1], f'dbrn_w{int(t)}': gg[2], f'dbrn_b{int(t)}': gg[3]})
        if ln is not None:                                            # frames behind a sample's length get no gradient
            pad = (torch.arange(N)[None, :] >= inp['ln'][:, None]).reshape(-1)
            assert float(dg.float().cpu()[pad].abs().max() if bool(pad.any()) else 0.0) == 0.0
    check(got, want, G.convmod_tols(want), f'convmod B={B} N={N} d={d} k={ks}')


@pytest.mark.parametrize('ks', G.CONV_KSIZES)
def test_convmod_kernel_sizes(ops, ks):
    """The 3-, 5- and 7-tap instantiations of the two sliding-window kernels."""
    B, N, d = 2, 100, 64
    assert _conv_geometry(lib_(), B, N, d, f'convmod ksize={ks}')[0] == 8
    _conv_case(ops, B, N, d, ks, [100, 37], (True, False))


@pytest.mark.parametrize('d', G.CONV_WIDTHS)
def test_convmod_channel_blocks(ops, d):
    """d / 4 = 25 does not divide the 256 threads of a workgroup (6 idle threads); 65 and 129 leave one channel group for a last,
    almost empty channel block.  Ragged lengths: a full sample, one that ends inside a time tile, an empty one."""
    B, N = 3, 50
    assert _conv_geometry(lib_(), B, N, d, f'convmod d={d}')[0] == 8
    _conv_case(ops, B, N, d, 9, [50, 13, 0], (True, False))


@pytest.mark.parametrize('B,N,d,tn', G.CONV_TALL)
def test_convmod_tall_time_tiles(ops, B, N, d, tn):
    """TN = 16, 32 and 64 (the tile training runs with) and the matching rows-per-thread steps of the statistics pass; in every case four
    samples: a full one and ends 3 frames past a tile edge, 2 before one and on one (within ksize / 2 of it)."""
    tn_, rpt = _conv_geometry(lib_(), B, N, d, f'convmod TN={tn}')
    assert tn_ == tn and rpt == tn
    _conv_case(ops, B, N, d, 9, G.tall_tile_lengths(B, N, tn), (True,))


# ------------------------------------------------------------------------------------------------------------------- CTC
def test_ctc_grid_cap_of_the_gather_and_rows_per_workgroup_of_the_fused_backward(ops):
    """B N = 67584 frames: the emission gather's grid is capped at 65536 workgroups (a second trip for the rest), and the fused
    gradient kernel with column sums walks several rows per workgroup.  Both operator forms, ragged batch, C = 128."""
    lib = lib_()
    B, N, C, S = G.CTC_SHAPE
    rows, slabs = B * N, 12 * lib.sconf_num_cus()
    assert rows > CAP_CTC_GATHER
    assert rows > slabs and lib.sconf_ctc_bwd_logits_workspace(rows, C) == lib.sconf_ctc_bwd_logits_workspace(2 * rows, C)
    geometry('ctc', frames=rows, gather_trips=cdiv(rows, CAP_CTC_GATHER), bwd_rows_per_workgroup=cdiv(rows, slabs), bwd_workgroups=cdiv(rows, cdiv(rows, slabs)))
    inp = G.ctc_inputs(B, N, C, S)
    want = G.ctc_ref(inp, F64)
    lg, lp, tg, il, tl, go = (dev(inp[k]) for k in ('lg', 'lp', 'tg', 'il', 'tl', 'go'))
    nll, ws = ops.ctc_fwd(lp, tg, il, tl, C - 1)
    assert float(((nll.double().cpu() - want['nll']) / want['nll']).abs().max()) < 1e-5
    grad = ops.ctc_bwd(lp, ws, nll, tg, il, tl, go, C - 1)
    close(grad, want['grad'], name='ctc grad', tol=2e-4)
    nll2, ws2 = ops.ctc_fwd_logits(lg, tg, il, tl, C - 1)
    assert float(((nll2.double().cpu() - want['nll_logits']) / want['nll_logits']).abs().max()) < 1e-5
    cs = torch.zeros(C, device='cuda')
    dl = ops.ctc_bwd_logits(lg, ws2, nll2, tg, il, tl, go, C - 1, colsum_into=cs)
    close(dl, want['dlogits'], name='fused CTC gradient', tol=1.5e-2, floor=1e-3)
    same_bits(ops.ctc_bwd_logits(lg, ws2, nll2, tg, il, tl, go, C - 1), dl, 'd(logits) with the column sums (several rows per workgroup) vs without (one)')
    close(cs, dl.double().sum((0, 1)).cpu(), name='fused CTC column sums', tol=2e-3, floor=1e-2)
    close(cs, want['dlogits'].to(BF).double().sum((0, 1)), name='fused CTC column sums vs reference', tol=1e-2, floor=1e-2)
    pad = (torch.arange(N)[None, :] >= inp['il'][:, None])
    assert float(dl.float().cpu()[pad].abs().max()) == 0.0 and float(grad.cpu()[pad].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------- elementwise, grid-stride loops
# Grid caps of the entry points below (workgroups; no query exposes them, so each case is sized at >= 2.5 x the capped grid's reach
# and names the launcher, file and function, under long-context-asr_amd/csrc/):
CAP_CAST = 4096            # elementwise.hip: sconf_cast, 256 threads x 8 elements
CAP_AFFINE = 8192          # convmod.hip:     sconf_affine_silu_fwd, 256 threads x 8 elements
CAP_MASK = 8192            # elementwise.hip: sconf_mask_rows, 256 threads x 4 elements
CAP_ROT_INPLACE = 16384    # elementwise.hip: sconf_rotary_inplace, 256 threads, one (row, q|k, head, 8 pairs) each
CAP_ROT_QKV = 8192         # elementwise.hip: sconf_rotary_qkv, 256 threads, one (row, head, 8 pairs) each
CAP_ROWDOT = 65536         # elementwise.hip: sconf_rowdot, 4 rows (one per wave)
CAP_OVERLAP = 16384        # infer.hip:       sconf_overlap_add_exp / sconf_overlap_finalize, 256 threads x 4 columns
CAP_SILU_T = 8192          # subsample.hip:   sconf_sub_silu_transpose, one row per workgroup
CAP_SUMSQ = 2048           # optim.hip:       sconf_sumsq, 256 threads x 4 elements
CAP_MADGRAD = 4096         # optim.hip:       sconf_madgrad_step, 256 threads x 4 elements
CAP_CTC_GATHER = 65536     # ctc.hip:         ctc_fwd_impl launching ctc_gather_kernel, one frame per workgroup


def _blocks(n, reach, rows=4096):
    """Row blocks in the first trip, the middle of the second and the ragged end of the last (reach = rows one trip covers)."""
    assert n >= 2.5 * reach and n % 256 != 0
    return [(0, rows), (reach + reach // 2, reach + reach // 2 + rows), (n - rows + 3, n)]


def test_cast_grid_stride(ops):
    n = G.CAST_N
    reach = CAP_CAST * 256 * 8
    geometry('cast', n=n, trips=cdiv(n, reach), tail=n % 8)
    assert n >= 2.5 * reach and n % 8 != 0
    x = rnd(n, dtype=F32)
    xd, xb = dev(x), dev(x.to(BF))
    y16, y32 = ops.cast(xd, BF), ops.cast(xb, F32)
    same_bits(y16.cpu(), x.to(BF), 'f32 -> bf16 (whole tensor against torch: the cast is exact)')
    same_bits(y32.cpu(), x.to(BF).float(), 'bf16 -> f32')
    for a, e in _blocks(n, reach):
        a -= a % 8
        same_bits(ops.cast(xd[a:e].clone(), BF), y16[a:e], f'f32 -> bf16 [{a}:{e}]'); same_bits(ops.cast(xb[a:e].clone(), F32), y32[a:e], f'bf16 -> f32 [{a}:{e}]')


def test_affine_silu_grid_stride(ops):
    M, d = G.AFFINE_M, G.AFFINE_D
    reach = CAP_AFFINE * 256 * 8 // d
    geometry('affine_silu', M=M, d=d, trips=cdiv(M, reach))
    inp = G.affine_inputs()
    h, coef = dev(inp['h']), dev(inp['coef'])
    y = ops.affine_silu_fwd(h, coef)
    for a, e in _blocks(M, reach):
        same_bits(ops.affine_silu_fwd(h[a:e].contiguous(), coef), y[a:e], f'rows {a}:{e}')
        close(y[a:e], ref('affine_silu_fwd', inp['h'][a:e], inp['coef']), name=f'affine_silu rows {a}:{e}')


def test_mask_rows_grid_stride(ops):
    B, N, d = G.MASK_B, G.MASK_N, G.MASK_D
    """An exact operation: the whole output against kernel_refs, bit for bit (lengths: full, short, empty, mid, one short of full)."""
    geometry('mask_rows', rows=B * N, d=d, trips=cdiv(B * N * (d // 4), CAP_MASK * 256))
    assert B * N * (d // 4) >= 2.5 * CAP_MASK * 256 and (B * N) % 256 != 0
    y = rnd(B * N, d)
    ln = torch.tensor([N, 5, 0, N // 2 + 1, N - 1], dtype=torch.int32)
    same_bits(ops.mask_rows_(dev(y.clone()), dev(ln), B, N).cpu(), R.mask_rows_(y.clone(), ln, B, N), 'mask_rows')


def test_rotary_grid_stride(ops):
    """sconf_rotary_inplace (16384 workgroups) and sconf_rotary_qkv in both directions (8192): 2.5 trips each."""
    inp = G.rotary_inputs()
    B, N, H, D = inp['B'], inp['N'], inp['H'], inp['D']
    M = B * N
    geometry('rotary', rows=M, H=H, D=D, inplace_trips=cdiv(M * 2 * H * (D // 16), CAP_ROT_INPLACE * 256), qkv_trips=cdiv(M * H * (D // 16), CAP_ROT_QKV * 256))
    reach = CAP_ROT_QKV * 256 // (H * (D // 16))                      # rows per trip: the same for both kernels at H = 1
    assert CAP_ROT_INPLACE * 256 // (2 * H * (D // 16)) == reach
    qkv, cos, sin = dev(inp['qkv']), dev(inp['cos']), dev(inp['sin'])
    rot = ops.rotary_inplace_(qkv.clone(), cos, sin, B, N, H, D)
    q, k, v = ops.rotary_qkv_fwd(qkv, cos, sin, B, N, H, D)
    back = ops.rotary_qkv_bwd(q, k, v, cos, sin, B, N, H, D)
    blocks = []
    for a, e in _blocks(M, reach):                                    # each block inside ONE sequence (small call: B = 1, N = its rows)
        if a % N + (e - a) > N: a, e = (a // N + 1) * N, (a // N + 1) * N + (e - a)
        blocks.append((a, e))
    assert blocks[1][0] // reach == 1 and blocks[2][1] == M
    for a, e in blocks:
        n0, n1 = a % N, a % N + (e - a)
        cs_, sn_ = cos[n0:n1].contiguous(), sin[n0:n1].contiguous()
        same_bits(ops.rotary_inplace_(qkv[a:e].clone(), cs_, sn_, 1, e - a, H, D), rot[a:e], f'in-place rows {a}:{e}')
        qs, ks_, vs = ops.rotary_qkv_fwd(qkv[a:e].contiguous(), cs_, sn_, 1, e - a, H, D)
        same_bits(qs.view(-1), q.view(M, -1)[a:e].reshape(-1), f'q rows {a}:{e}'); same_bits(ks_.view(-1), k.view(M, -1)[a:e].reshape(-1), f'k rows {a}:{e}')
        same_bits(vs.view(-1), v.view(M, -1)[a:e].reshape(-1), f'v rows {a}:{e}')
        same_bits(ops.rotary_qkv_bwd(qs, ks_, vs, cs_, sn_, 1, e - a, H, D), back[a:e], f'transpose rows {a}:{e}')
        c, s = inp['cos'][n0:n1], inp['sin'][n0:n1]
        qr, kr, vr = ref('rotary_qkv_fwd', inp['qkv'][a:e], c, s, 1, e - a, H, D)
        close(qs, qr, name='q'); close(ks_, kr, name='k'); assert torch.equal(vs.cpu(), vr)
        close(ops.rotary_qkv_bwd(qs, ks_, vs, cs_, sn_, 1, e - a, H, D), ref('rotary_qkv_bwd', qs.cpu(), ks_.cpu(), vs.cpu(), c, s, 1, e - a, H, D), name='transpose')
        want = ref('rotary_inplace_', inp['qkv'][a:e].clone(), c, s, 1, e - a, H, D)
        close(rot[a:e], want, name='in-place')


def test_rowdot_grid_stride(ops):
    M, d = G.ROWDOT_M, G.ROWDOT_D
    reach = CAP_ROWDOT * 4
    geometry('rowdot', M=M, d=d, trips=cdiv(M, reach))
    inp = G.rowdot_inputs()
    a_, b_, bias = dev(inp['a']), dev(inp['b']), dev(inp['bias'])
    out = ops.rowdot(a_, b_, bias)
    for a, e in _blocks(M, reach):
        same_bits(ops.rowdot(a_[a:e], b_[a:e], bias), out[a:e], f'rows {a}:{e}')
    want = ref('rowdot', inp['a'], inp['b'], inp['bias'])
    assert float((out.double().cpu() - want).abs().max()) <= 1e-4 * float(want.abs().max()) + 1e-5, 'rowdot vs the same sum in f64'


def test_overlap_average_grid_stride(ops):
    """sconf_overlap_add_exp / sconf_overlap_finalize at 2.5 trips of their capped grids.  Rows one window covers (acc = 0 + exp(logp)) and
    all of finalize are row-independent: bit for bit against one-trip calls (W = 1) over row blocks of the first trip, the second and
    the ragged end of the third.  Rows two windows cover are sums: against the float64 restatement (tolerance of
    test_overlap_average_and_argmax)."""
    W, n, stride, C = G.OVL_W, G.OVL_n, G.OVL_STRIDE, G.OVL_C
    pos0 = 5
    span = (W - 1) * stride + n
    N = pos0 + span + 2
    reach = CAP_OVERLAP * 256 // (C // 4)                             # rows per trip
    geometry('overlap', rows=span, C=C, add_trips=cdiv(span, reach), finalize_trips=cdiv(span, reach), rows_under_two_windows=(W - 1) * (n - stride))
    assert span >= 2.5 * reach and span % 256 != 0 and stride < n < 2 * stride
    g = torch.Generator().manual_seed(3)
    lp = torch.log_softmax(torch.randn(W, n, C, generator=g), -1)
    acc, cnt = torch.zeros(N, C, dtype=F64), torch.zeros(N, dtype=F64)
    R.overlap_add_exp_(lp.double(), acc, cnt, pos0, stride)
    lpd = dev(lp)
    a, c = torch.zeros(N, C, device='cuda'), torch.zeros(N, device='cuda')
    ops.overlap_add_exp_(lpd, a, c, pos0, stride)
    assert torch.equal(c.cpu().double(), cnt)
    assert torch.allclose(a.cpu().double(), acc, rtol=1e-5, atol=1e-7)
    got = ops.overlap_finalize(a[pos0:].contiguous(), c[pos0:].contiguous(), span)
    assert torch.allclose(got.cpu().double(), R.overlap_finalize(acc[pos0:], cnt[pos0:], span), rtol=1e-5, atol=1e-6)
    rows = 4096
    # rows (relative to pos0) that only window w covers: [0, stride) of w = 0, [n, 2 stride) of w = 1, [stride + n, span) of w = 2
    blocks = [(0, 0), (1, n + (2 * stride - n) // 2), (2, span - rows + 3)]
    for (w, r0), trip in zip(blocks, (0, 1, 2)):
        r1 = min(r0 + rows, span)
        assert r0 // reach == trip and (r1 - 1) // reach == trip and w * stride <= r0 and r1 <= w * stride + n
        assert (w == 0 or r0 >= (w - 1) * stride + n) and (w == W - 1 or r1 <= (w + 1) * stride), 'block lies under one window only'
        sa, sc = torch.zeros(r1 - r0, C, device='cuda'), torch.zeros(r1 - r0, device='cuda')
        ops.overlap_add_exp_(lpd[w:w + 1, r0 - w * stride:r1 - w * stride].contiguous(), sa, sc, 0, r1 - r0)
        same_bits(sa, a[pos0 + r0:pos0 + r1], f'acc rows {r0}:{r1} (window {w})'); same_bits(sc, c[pos0 + r0:pos0 + r1], f'count rows {r0}:{r1}')
    for r0, r1 in _blocks(span, reach):                               # finalize: any rows, those under two windows included
        same_bits(ops.overlap_finalize(a[pos0 + r0:pos0 + r1].contiguous(), c[pos0 + r0:pos0 + r1].contiguous(), r1 - r0), got[r0:r1], f'finalize rows {r0}:{r1}')


def test_sub_silu_transpose_grid_stride(ops):
    rows, F8, C = G.SILU_T_ROWS, G.SILU_T_F8, G.SILU_T_C
    geometry('sub_silu_transpose', rows=rows, trips=cdiv(rows, CAP_SILU_T))
    inp = G.silu_t_inputs()
    pre, ds = dev(inp['pre']), dev(inp['ds'])
    s, b = ops.sub_silu_transpose(pre), ops.sub_silu_transpose(pre, ds)
    for a, e in _blocks(rows, CAP_SILU_T, rows=64):
        same_bits(ops.sub_silu_transpose(pre[a:e].contiguous()), s[a:e], f'forward rows {a}:{e}')
        same_bits(ops.sub_silu_transpose(pre[a:e].contiguous(), ds[a:e].contiguous()), b[a:e], f'backward rows {a}:{e}')
    close(s, ref('sub_silu_transpose', inp['pre']), name='silu_transpose')
    close(b, ref('sub_silu_transpose', inp['pre'], inp['ds']), name='silu_transpose bwd')


# -------------------------------------------------------------------------------------------------------------- optimiser
def test_sumsq_grid_stride_fixed_order(ops):
    n = G.MADGRAD_N
    geometry('sumsq', n=n, trips=cdiv(n, CAP_SUMSQ * 1024), tail=n % 4)
    assert n >= 2.5 * CAP_SUMSQ * 1024 and n % 4 != 0
    g = rnd(n, dtype=F32, seed=10)
    out = [ops.sumsq_(dev(g), torch.zeros((), dtype=F64).cuda()) for _ in range(2)]
    want = float((g.double() ** 2).sum())
    assert abs(float(out[0]) - want) / want < 1e-5
    assert torch.equal(out[0], out[1]), 'the header promises a fixed summation order'


def test_madgrad_on_the_device(ops):
    """sconf_madgrad_step past its grid cap (2.5 trips, the n % 4 tail in the third) over five steps: weight decay, gradient scale, a
    norm above and below max_norm, max_norm = 0, one non-finite gradient (skipped: nothing moves, k stays), against
    kernel_refs.madgrad_step_ in float64 (tolerance 1e-5 as test_madgrad_matches_reference_fixture).  k from the host and from k_dev
    (advanced by sconf_madgrad_advance) must give the same bits; row blocks of the first two steps must equal small one-trip calls."""
    n, h = G.MADGRAD_N, G.MADGRAD_HYPER
    reach = CAP_MADGRAD * 1024
    assert reach == G.MADGRAD_CAP
    geometry('madgrad', n=n, trips=cdiv(n, reach), tail=n % 4, tail_trip=(n - n % 4) // reach)
    assert n >= 2.5 * reach and n % 4 == 3 and (n - n % 4) // reach >= 1
    inp = G.madgrad_inputs()
    want = G.madgrad_ref(inp, F64)
    new = lambda: dict(p=dev(inp['p']).clone(), gss=torch.zeros(n).cuda(), s=torch.zeros(n).cuda(), x0=torch.zeros(n).cuda(),
                       shadow=torch.zeros(n, dtype=BF).cuda())
    A, Bv = new(), new()                                              # k from the host / from the device
    names = ('p', 'gss', 's', 'x0', 'shadow')
    k_host, k_dev = 0, torch.zeros((), dtype=torch.int64).cuda()
    step = lambda S, g, sq, st, k: ops.madgrad_step_(S['p'], g, S['gss'], S['s'], S['x0'], S['shadow'], sq, st['max_norm'], st['gs'], h['lr'],
                                                     h['momentum'], h['eps'], st['wd'], k)
    for i, (gc, st) in enumerate(zip(inp['g'], G.MADGRAD_STEPS)):
        g = dev(gc)
        sq = ops.sumsq_(g, torch.zeros((), dtype=F64).cuda())
        before = {k: A[k].clone() for k in names}
        step(A, g, sq, st, k_host)
        step(Bv, g, sq, st, k_dev)
        ops.madgrad_advance_(k_dev, sq, st['gs'])
        if st['inf']:
            assert not torch.isfinite(sq)
            for k in names: same_bits(A[k], before[k], f'skipped step moved {k}')
        else:
            k_host += 1
        assert int(k_dev) == k_host == want[i]['k']
        for k in names: same_bits(Bv[k], A[k], f'step {i}: {k} with k from the device vs from the host')
        same_bits(A['shadow'], A['p'].to(BF), 'bf16 shadow')
        for k in ('p', 'gss', 's', 'x0'):
            close(A[k], want[i][k], tol=1e-5, name=f'madgrad step {i} {k}')
            close(A[k][-8:], want[i][k][-8:], tol=1e-5, name=f'madgrad step {i} {k} (tail)')
        if i < 2:
            kk = k_host - 1
            for a, e in _blocks(n, reach):
                a -= a % 4
                S = {k: before[k][a:e].clone() for k in names}
                step(S, g[a:e].clone(), sq, st, kk)
                for k in names: same_bits(S[k], A[k][a:e], f'step {i}: {k}[{a}:{e}]')


# -------------------------------------------------------------------------------------------------------------- attention
ATTN_CASES = [(D, s, True) for D in (32, 64, 128, 256) for s in G.ATTN_SETTINGS] + [(128, s, False) for s in G.ATTN_SETTINGS]


def _attn_case(ops, inp, win, scale, what):
    want = G.attn_ref(inp, win, scale, F64)
    q, k, v, do, ln = (dev(inp[x]) for x in ('q', 'k', 'v', 'do', 'ln'))
    o, lse = ops.attn_fwd(q, k, v, ln, win, scale)
    close(o, want['o'], name=f'{what} o')
    m = torch.isfinite(want['lse'])
    assert float((lse.double().cpu()[m] - want['lse'][m]).abs().max()) < 2e-3, 'lse'
    dq, dk, dv = ops.attn_bwd(q, k, v, o, do, lse, ln, win, scale)
    rq, rk, rv = ops.attn_bwd(q, k, v, o, do, lse, ln, win, scale, rot=(dev(inp['rot'][0]), dev(inp['rot'][1])))
    check(dict(dq=dq, dk=dk, dv=dv, dq_rot=rq, dk_rot=rk), want, G.ATTN_TOL, what)
    same_bits(rv, dv, 'dv does not depend on the rotary transpose')


@pytest.mark.parametrize('D,setting,wide', ATTN_CASES)
def test_attention_many_kv_tiles(ops, D, setting, wide, monkeypatch):
    """N = 2048: 16 (8-wave kernels: 8) query tiles and 32 key tiles of 64 per (batch, head); the windows and the ragged lengths
    (one below a key tile) leave most key tiles of a query tile out of bounds, so whole tiles are skipped far from the diagonal.
    Forward and backward, with and without the rotary transpose in the backward's epilogue; head_dim 128 through both kernel sets."""
    B, lens, win = G.ATTN_SETTINGS[setting]
    N, H = 2048, 2
    if wide: monkeypatch.delenv('SCONF_ATTN_WIDE', raising=False)
    else: monkeypatch.setenv('SCONF_ATTN_WIDE', '0')
    waves = lib_().sconf_attn_waves(D, N, H * D)                     # the kernel set the library takes for these (contiguous) views
    assert waves == (8 if wide and D == 128 else 4), 'case does not reach the kernel set it is for'
    # the tile counts below follow from the case's window and lengths (no query exposes which tiles a kernel skips)
    live = [cdiv(min(N, L), 64) for L in (lens or [N] * B)]
    per_q = 32 if win[0] < 0 else cdiv(win[0] + max(win[1], 0) + 128, 64) + 1
    geometry(f'attention D={D} {setting}', B=B, N=N, H=H, kernels=f'{waves}-wave', key_tiles=32, live_key_tiles=live,
             key_tiles_per_query_tile_at_most=min(32, per_q))
    _attn_case(ops, G.attn_inputs(B, N, H, D, lens), win, None, f'attention D={D} {setting}')


@pytest.mark.parametrize('D', [64, 128])
def test_attention_non_default_scale(ops, D):
    B, N, H = 2, 300, 2
    waves = lib_().sconf_attn_waves(D, N, H * D)
    assert waves == (8 if D == 128 else 4)
    geometry(f'attention D={D} scale', B=B, N=N, H=H, scale=0.05, kernels=f'{waves}-wave')
    _attn_case(ops, G.attn_inputs(B, N, H, D, [300, 131]), (-1, -1), 0.05, f'attention D={D} scale 0.05')
