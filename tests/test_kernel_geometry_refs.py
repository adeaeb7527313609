"""CPU self-check of the references test_kernel_geometry_gpu.py compares the kernels with: for every shape of that module the float64
restatement (tests/kernel_refs.py evaluated in float64) and the float32 form of the same functions must agree within the project's
tolerance for that op.  This checks the reference helpers (and the precision switch of kernel_test_utils.ref) without a GPU, and
shows that none of the larger shapes needs a tolerance wider than the one written in test_kernels_gpu.py: the reference-only error
printed per case is what a kernel with f32 accumulation can be expected to add by summation order alone."""
import pytest
import torch

import geometry_cases as G
import kernel_refs as R
from kernel_test_utils import BF, F32, F64, TOL_BF16, TOL_F32, ref, rel_err


def agree(lo, hi, tols, what):
    worst = {}
    for k, t in tols.items():
        if k not in hi or hi[k] is None: continue
        tol, floor = t if isinstance(t, tuple) else (t, 0.0)
        err = rel_err(lo[k], hi[k], floor)
        worst[k] = err
        assert err <= tol, f'{what} {k}: f32 vs f64 reference differ by {err:.3e} > {tol}'
    print(f'[reference-only error] {what}: ' + ', '.join(f'{k}={v:.1e}' for k, v in worst.items()))


def test_precision_switch_really_computes_in_float64():
    x = torch.tensor([[1.0, 1.0 + 2.0 ** -30, 3.0, 5.0]], dtype=F64)
    w = torch.ones(4)
    y64, _, _ = ref('norm_fwd', x, w, None, 'layer_norm', 0.0, F32, prec=F64)
    y32, _, _ = ref('norm_fwd', x, w, None, 'layer_norm', 0.0, F32, prec=F32)
    assert y64.dtype == F64 and y32.dtype == F32 and R.f32 == F32 and torch.get_default_dtype() == F32
    assert float(y64[0, 1] - y64[0, 0]) > 0 and float(y32[0, 1] - y32[0, 0]) == 0.0


@pytest.mark.parametrize('mode', ['layer_norm', 'rms_norm', 'rms_norm_apex'])
@pytest.mark.parametrize('d', [768, 1028, 2048])
def test_norm_bwd_rows(mode, d):
    M = G.rows_for_trips(G.norm_bwd_waves(d))
    for xd, gd in ((F32, BF), (BF, F32)):
        inp = G.norm_inputs(mode, d, M, xd, gd)
        agree(G.norm_ref(inp, mode, F32), G.norm_ref(inp, mode, F64), G.NORM_TOL, f'norm_bwd {mode} d={d} M={M}')


@pytest.mark.parametrize('twice', [False, True])
@pytest.mark.parametrize('d,M', [(260, None), (768, None), (4, 37), (68, 37), (260, 37), (772, 37)])
def test_norm2(d, M, twice):
    M = M or G.rows_for_trips(G.DEFAULT_CUS * G.NORM_WAVES)
    inp = G.norm2_inputs(d, M)
    agree(G.norm2_ref(inp, twice, F32), G.norm2_ref(inp, twice, F64), G.NORM2_TOL, f'norm2 d={d} M={M} twice={twice}')


@pytest.mark.parametrize('mode', ['layer_norm', 'rms_norm', 'rms_norm_apex'])
@pytest.mark.parametrize('d', [4, 68, 260, 772, 1028])
def test_norm_widths(mode, d):
    for xd, yd in ((F32, BF), (F32, F32), (BF, BF)):
        inp = G.norm_inputs(mode, d, 37, xd, yd)
        agree(G.norm_ref(inp, mode, F32), G.norm_ref(inp, mode, F64), G.NORM_TOL, f'norm {mode} d={d}')


@pytest.mark.parametrize('C,M', [(132, 37), (8192, 37), (132, 2 * 2048 + 77)])
def test_softmax(C, M):
    for log, xd, yd in ((False, BF, BF), (True, F32, F32), (False, F32, F32)):
        inp = G.softmax_inputs(M, C, xd, yd)
        inp['y_in'] = R.softmax_fwd(inp['x'], log, yd)
        lo, hi = G.softmax_ref(inp, log, F32), G.softmax_ref(inp, log, F64)
        if log: assert float((lo['y'].double() - hi['y']).abs().max()) < 2e-3
        agree(lo, hi, dict(dx=TOL_BF16) if log else dict(y=TOL_F32, dx=TOL_BF16), f'softmax C={C} M={M} log={log}')


CONV_SHAPES = ([(2, 100, 64, ks, [100, 37]) for ks in G.CONV_KSIZES] + [(3, 50, d, 9, [50, 13, 0]) for d in G.CONV_WIDTHS] +
               [(B, N, d, 9, G.tall_tile_lengths(B, N, tn)) for B, N, d, tn in G.CONV_TALL])


@pytest.mark.parametrize('B,N,d,ks,lens', CONV_SHAPES)
def test_convmod(B, N, d, ks, lens):
    inp = G.convmod_inputs(B, N, d, ks, lens)
    tr = (True, False) if N <= 100 else (True,)
    hi = G.convmod_ref(inp, F64, tr)
    agree(G.convmod_ref(inp, F32, tr), hi, G.convmod_tols(hi), f'convmod B={B} N={N} d={d} k={ks}')


def test_ctc():
    inp = G.ctc_inputs(*G.CTC_SHAPE)
    lo, hi = G.ctc_ref(inp, F32), G.ctc_ref(inp, F64)
    for k in ('nll', 'nll_logits'):
        assert float(((lo[k].double() - hi[k]) / hi[k]).abs().max()) < 1e-5, k
    agree(lo, hi, dict(grad=2e-4, dlogits=(1.5e-2, 1e-3)), f'ctc B, N, C, S = {G.CTC_SHAPE}')


@pytest.mark.parametrize('D', [32, 64, 128, 256])
@pytest.mark.parametrize('setting', list(G.ATTN_SETTINGS))
def test_attention(D, setting):
    B, lens, win = G.ATTN_SETTINGS[setting]
    inp = G.attn_inputs(B, 2048, 2, D, lens)
    lo, hi = G.attn_ref(inp, win, None, F32), G.attn_ref(inp, win, None, F64)
    m = torch.isfinite(hi['lse'])
    assert float((lo['lse'].double()[m] - hi['lse'][m]).abs().max()) < 2e-3
    agree(lo, hi, G.ATTN_TOL, f'attention D={D} {setting}')


@pytest.mark.parametrize('D', [64, 128])
def test_attention_scale(D):
    inp = G.attn_inputs(2, 300, 2, D, [300, 131])
    agree(G.attn_ref(inp, (-1, -1), 0.05, F32), G.attn_ref(inp, (-1, -1), 0.05, F64), G.ATTN_TOL, f'attention D={D} scale 0.05')


def test_madgrad_and_sumsq():
    inp = G.madgrad_inputs()
    lo, hi = G.madgrad_ref(inp, F32), G.madgrad_ref(inp, F64)
    assert [s['k'] for s in hi] == [1, 2, 3, 3, 4]
    for i, (a, b) in enumerate(zip(lo, hi)):
        agree(a, b, dict(p=1e-5, gss=1e-5, s=1e-5, x0=1e-5), f'madgrad n={G.MADGRAD_N} step {i}')
    assert torch.equal(hi[3]['p'], hi[2]['p']) and not torch.equal(hi[4]['p'], hi[3]['p'])
    g = inp['g'][0]
    assert abs(float((g * g).sum()) - float((g.double() ** 2).sum())) / float((g.double() ** 2).sum()) < 1e-5


def test_elementwise_rows():
    a = G.affine_inputs(M=4096)
    assert rel_err(ref('affine_silu_fwd', a['h'], a['coef'], prec=F32), ref('affine_silu_fwd', a['h'], a['coef'])) <= TOL_BF16
    r = G.rotary_inputs(B=1, N=4096)
    args = (r['cos'], r['sin'], 1, 4096, r['H'], r['D'])
    for lo, hi in zip(ref('rotary_qkv_fwd', r['qkv'], *args, prec=F32), ref('rotary_qkv_fwd', r['qkv'], *args)):
        assert rel_err(lo, hi) <= TOL_BF16
    assert rel_err(ref('rotary_inplace_', r['qkv'].clone(), *args, prec=F32), ref('rotary_inplace_', r['qkv'].clone(), *args)) <= TOL_BF16
    d = G.rowdot_inputs(M=4096)
    lo, hi = ref('rowdot', d['a'], d['b'], d['bias'], prec=F32), ref('rowdot', d['a'], d['b'], d['bias'])
    assert float((lo.double() - hi).abs().max()) <= 1e-4 * float(hi.abs().max()) + 1e-5
    s = G.silu_t_inputs(rows=64)
    assert rel_err(ref('sub_silu_transpose', s['pre'], prec=F32), ref('sub_silu_transpose', s['pre'])) <= TOL_BF16
    assert rel_err(ref('sub_silu_transpose', s['pre'], s['ds'], prec=F32), ref('sub_silu_transpose', s['pre'], s['ds'])) <= TOL_BF16
