"""Componentwise parity of the HIP kernels against float64 (tests/componentwise.py: budgets, metrics, graded inputs, cases).
Every value check here sees every element (check_elements, check_rounding) or every row / column (check_slices); the CPU file
test_componentwise.py shows that the references alone stay inside these bounds and that the planted defects do not.  Each test
prints its worst err / bound ratios; the MI355X figures are in DESIGN.md section 27."""
import pytest
import torch

import componentwise as C
from kernel_test_utils import BF, F32, dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import lcasr_amd.hip.ops as o
    o._lib.load()
    return o


def _variant(ops, layout, m, n, k, split=1, act='none', resid=False, pre=False):
    from lcasr_amd.hip import _lib
    return _lib.load().sconf_gemm_variant(ops.LAYOUT[layout], m, n, k, k if layout != 'tn' else m, k if layout == 'nt' else n, split,
                                          ops.ACT[act], int(resid), int(pre))


# ------------------------------------------------------------------------------------------------ the 128x128 GEMM kernel
@pytest.mark.parametrize('layout', ['nt', 'nn', 'tn'])
@pytest.mark.parametrize('M,N,K', [(200, 144, 72), (513, 256, 2400)])          # edge tiles in M and N; 1 and 37 K-tiles
def test_gemm_plain(ops, layout, M, N, K):
    if layout == 'tn': M = M // 8 * 8
    assert _variant(ops, layout, M, N, K) == 0, 'the shape must stay on the 128x128 kernel'
    a, b = C.graded(M, N, K, layout)
    for od in (BF, F32):
        C.check_gemm(ops.gemm, dev, a, b, layout, f'gemm {layout} {(M, N, K)} {od}', rounding=K <= C.ROUNDING_MAX_K, out_dtype=od)
        C.check_scaling(ops.gemm, dev, M, N, K, layout, f'scaling {layout} {(M, N, K)} {od}', out_dtype=od, alpha=0.5)


@pytest.mark.parametrize('layout', ['nt', 'nn'])
@pytest.mark.parametrize('kw', C.EPILOGUES, ids=lambda kw: '-'.join(f'{k}={v}' for k, v in kw.items()))
def test_gemm_epilogues(ops, layout, kw):
    M, N, K = 300, 192, 136
    a, b = C.graded(M, N, K, layout)
    C.check_gemm(ops.gemm, dev, a, b, layout, f'gemm {layout} {kw}', **C.epilogue_inputs(kw, M, N))


def test_gemm_split_k_and_accum(ops):
    K, M, N = 5000, 256, 136
    a, b = C.graded(M, N, K, 'tn')
    for sk in (2, 5, 16):
        C.check_gemm(ops.gemm, dev, a, b, 'tn', f'split_k {sk}', alpha=0.5, out_dtype=F32, split_k=sk)
        C.check_scaling(ops.gemm, dev, M, N, K, 'tn', f'scaling split_k {sk}', out_dtype=F32, alpha=0.5, split_k=sk)
    C.check_gemm(ops.gemm, dev, a, b, 'tn', 'accum', alpha=2.0, accum=C.graded_mat(M, N, F32, 20))


# ------------------------------------------------------------------------- the 256-row, 192-wide and TN kernels (gemm256.hip)
def _both(ops, monkeypatch, *args, **kw):
    monkeypatch.delenv('SCONF_GEMM_NO_256', raising=False)
    new = ops.gemm(*args, **kw)
    monkeypatch.setenv('SCONF_GEMM_NO_256', '1')
    old = ops.gemm(*args, **kw)
    monkeypatch.delenv('SCONF_GEMM_NO_256')
    return (new if isinstance(new, tuple) else (new,)), (old if isinstance(old, tuple) else (old,))


@pytest.mark.parametrize('N,K,variant', [(768, 256, 2), (1024, 192, 1)])
def test_gemm_256_row_kernels_nt(ops, N, K, variant, monkeypatch):
    """Graded inputs through the large-projection kernels: bit-identical to the 128x128 kernel for the plain, bias + residual,
    gelu_dsave and mulaux epilogues, and the plain output inside its float64 budget."""
    M = 16384
    monkeypatch.delenv('SCONF_GEMM_NO_256', raising=False)
    assert _variant(ops, 'nt', M, N, K) == variant, 'test shape does not route to the kernel it is meant to cover'
    a, b = C.graded(M, N, K, 'nt')
    ad, bd = dev(a), dev(b)
    bias, resid, aux = dev(C.graded_vec(N)), dev(C.graded_mat(M, N, F32, 3)), dev(C.graded_mat(M, N, BF, 4))
    for kw in (dict(), dict(bias=bias, resid=resid, alpha=0.5, out_dtype=F32), dict(bias=bias, act='gelu_dsave', save_pre=True),
               dict(aux=aux, act='mulaux', alpha=0.5)):
        assert _variant(ops, 'nt', M, N, K, act=kw.get('act', 'none'), resid='resid' in kw, pre=bool(kw.get('save_pre'))) == variant, \
            f'epilogue {list(kw)} does not route to the kernel it is meant to cover'
        new, old = _both(ops, monkeypatch, ad, bd, 'nt', **kw)
        for x, y in zip(new, old):
            assert torch.equal(x, y), (list(kw), int((x != y).sum()))
        if not kw:
            (t, bud, _), = C.gemm_expect(a, b, 'nt')
            C.report(f'gemm nt {(M, N, K)} variant {variant}', out=C.check_elements(new[0], t, bud, BF, f'gemm nt {(M, N, K)}'))


def test_gemm_256_row_kernel_tn_split_k(ops, monkeypatch):
    K, M, N, split = 8192, 3072, 768, 7
    monkeypatch.delenv('SCONF_GEMM_NO_256', raising=False)
    assert _variant(ops, 'tn', M, N, K, split=split) == 3
    a, b = C.graded(M, N, K, 'tn')
    new, old = _both(ops, monkeypatch, dev(a), dev(b), 'tn', out_dtype=F32, split_k=split, alpha=0.5)
    assert torch.equal(new[0], old[0])
    (t, bud, _), = C.gemm_expect(a, b, 'tn', out_dtype=F32, split_k=split, alpha=0.5)
    C.report(f'gemm tn {(M, N, K)} split {split}', out=C.check_elements(new[0], t, bud, F32, 'gemm tn split-K'))


@pytest.mark.parametrize('Bn,N,H,K,epilogue', [(2, 256, 2, 768, False), (1, 64, 4, 64, False), (32, 256, 6, 768, True)])
def test_gemm_qkv_rotary(ops, Bn, N, H, K, epilogue, monkeypatch):
    """The two small shapes run the GEMM and the in-place rotary (two bf16 stores, budgeted as such); the third is the smallest
    one of test_kernels_gpu.py that the 256-row kernel's rotary epilogue takes (one store)."""
    monkeypatch.delenv('SCONF_QKV_ROT_EPILOGUE_OFF', raising=False)
    C.run_qkv_rotary(ops, dev, Bn, N, H, K, epilogue)


def test_gemm_softmax_bwd(ops):
    M, V, K = 16384, 1024, 768
    assert ops.gemm_softmax_bwd_eligible(M, V, K)
    C.run_gemm_softmax_bwd(ops, dev, M, V, K)


# ------------------------------------------------------------------------------------------------ reductions, cast, softmax, norms
def test_reductions(ops):
    C.run_reductions(ops, dev)


def test_cast(ops):
    C.run_cast(ops, dev)


@pytest.mark.parametrize('C_', [128, 4096])
def test_softmax_fwd(ops, C_):
    C.run_softmax_fwd(ops, dev, C_)


@pytest.mark.parametrize('mode', ['layer_norm', 'rms_norm', 'rms_norm_apex'])
@pytest.mark.parametrize('d', [64, 768, 2048])
def test_norm_fwd(ops, mode, d):
    C.run_norm_fwd(ops, dev, mode, d)


# ------------------------------------------------------------------------------------------------ row-local: check_slices
@pytest.mark.parametrize('case', C.ATTN_CASES, ids=str)
def test_attention(ops, case, monkeypatch):
    """o per row from the kernels' forward; dq, dk, dv per row from the kernels' backward on the SAME (o, lse) that the yardstick
    and the float64 truth read (componentwise.run_attention says why: the backward takes delta from the bf16 o it is handed)."""
    if case[-1]: monkeypatch.setenv('SCONF_ATTN_WIDE', '0')
    else: monkeypatch.delenv('SCONF_ATTN_WIDE', raising=False)
    C.run_attention(ops, dev, case)


@pytest.mark.parametrize('mode', ['layer_norm', 'rms_norm', 'rms_norm_apex'])
@pytest.mark.parametrize('d', [64, 768, 2048])
def test_norm_bwd(ops, mode, d):
    C.run_norm_bwd(ops, dev, mode, d)


@pytest.mark.parametrize('d', [64, 768])
def test_norm2_bwd(ops, d):
    C.run_norm2_bwd(ops, dev, d)


@pytest.mark.parametrize('log', [False, True])
@pytest.mark.parametrize('C_', [128, 4096])
def test_softmax_bwd(ops, C_, log):
    C.run_softmax_bwd(ops, dev, C_, log)
