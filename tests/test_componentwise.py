"""The componentwise harness (tests/componentwise.py) checked on the CPU: kernel_refs in f32 stands in for the kernels.

1. Every case of test_componentwise_gpu.py (M reduced where the GPU shape is large) passes check_elements, check_rounding and
   check_slices with the stand-in: the condition on the inputs - the reference alone stays inside every bound.
2. Planted defects on the stand-in's output each FAIL the harness, and `close` at its standing tolerance PASSES (a), (b), (e) and
   (f): the gap this harness closes, written down as a test.

check_rounding needs elements whose budget is at most ulp / 16, which lies between 2^-12 |truth| and 2^-11 |truth|; E_acc >=
(K + 1) 2^-23 |truth|, so no element can qualify from K = 2^12 on, and since S = sum|a||b| is several times |truth| too few do from
a few hundred: the statistic is taken at the K = 72 / 136 / 64 shapes of the same kernels and stores (componentwise.ROUNDING_MAX_K)."""
import pytest
import torch

import componentwise as C
import kernel_refs as R
from kernel_test_utils import BF, F32, close


def same(t):
    return t


def _gelu_sig(x):
    """csrc/common.h geluf_: x sigmoid(2c(x + 0.044715 x^3)).  kernel_refs writes 0.5 x (1 + tanh(.)), which in f32 loses the
    negative tail to the cancellation in 1 + tanh (gelu(-6) = -0.0 instead of -1e-13): exact to 6e-8 |x|, as `close` asks, but not
    per element.  The kernels use the sigmoid form, so the stand-in for them does too; the float64 truth stays kernel_refs'."""
    return x * torch.sigmoid(2 * 0.7978845608028654 * (x + 0.044715 * x ** 3))


def _dgelu_sig(x):
    s = torch.sigmoid(2 * 0.7978845608028654 * (x + 0.044715 * x ** 3))
    return s + x * s * (1 - s) * (2 * 0.7978845608028654) * (1 + 3 * 0.044715 * x * x)


def standin_gemm(*a, **kw):
    old = R._gelu, R._dgelu
    R._gelu, R._dgelu = _gelu_sig, _dgelu_sig
    try:
        return R.gemm(*a, **kw)
    finally:
        R._gelu, R._dgelu = old


class AttentionStandIn:
    """kernel_refs.attn_fwd, and for the backward the f32 restatement that reads o and lse as the kernels do (kernel_refs.attn_bwd
    differentiates the exact forward and ignores both) - without the kernels' bf16 packing of P and dS, which the yardstick has."""
    attn_fwd = staticmethod(R.attn_fwd)

    @staticmethod
    def attn_bwd(q, k, v, o, dout, lse, lengths, window):
        return tuple(t.to(BF) for t in C.attn_bwd_restated(q, k, v, o, dout, lse, lengths, window, F32, False)[:3])


GEMM_SHAPES = [(200, 144, 72), (513, 256, 2400)]


def _m(layout, M):
    return M // 8 * 8 if layout == 'tn' else M


@pytest.mark.parametrize('layout', ['nt', 'nn', 'tn'])
@pytest.mark.parametrize('M,N,K', GEMM_SHAPES)
def test_gemm_plain(layout, M, N, K):
    M = _m(layout, M)
    a, b = C.graded(M, N, K, layout)
    for od in (BF, F32):
        C.check_gemm(R.gemm, same, a, b, layout, f'gemm {layout} {(M, N, K)} {od}', rounding=K <= C.ROUNDING_MAX_K, out_dtype=od)
        C.check_scaling(R.gemm, same, M, N, K, layout, f'scaling {layout} {od}', out_dtype=od, alpha=0.5)


@pytest.mark.parametrize('layout', ['nt', 'nn'])
@pytest.mark.parametrize('kw', C.EPILOGUES, ids=lambda kw: '-'.join(kw))
def test_gemm_epilogues(layout, kw):
    M, N, K = 300, 192, 136
    a, b = C.graded(M, N, K, layout)
    C.check_gemm(standin_gemm, same, a, b, layout, f'gemm {layout} {list(kw)}', **C.epilogue_inputs(kw, M, N))


def test_gemm_split_k_and_accum():
    K, M, N = 5000, 256, 136
    a, b = C.graded(M, N, K, 'tn')
    for sk in (2, 5, 16):
        C.check_gemm(R.gemm, same, a, b, 'tn', f'split_k {sk}', alpha=0.5, out_dtype=F32, split_k=sk)
    C.check_gemm(R.gemm, same, a, b, 'tn', 'accum', alpha=2.0, accum=C.graded_mat(M, N, F32, 20))


@pytest.mark.parametrize('M,N,K,layout', [(512, 768, 256, 'nt'), (512, 1024, 192, 'nt'), (512, 768, 1024, 'tn')])
def test_gemm_large_kernel_shapes_reduced(M, N, K, layout):
    a, b = C.graded(M, N, K, layout)
    C.check_gemm(R.gemm, same, a, b, layout, f'gemm {layout} {(M, N, K)}', rounding=False, out_dtype=F32 if layout == 'tn' else BF)


@pytest.mark.parametrize('Bn,N,H,K', [(2, 256, 2, 768), (1, 64, 4, 64)])
def test_qkv_rotary(Bn, N, H, K):
    C.run_qkv_rotary(R, same, Bn, N, H, K)


def test_gemm_softmax_bwd():
    C.run_gemm_softmax_bwd(R, same, 512, 1024, 768)


def test_reductions_and_cast():
    C.run_reductions(R, same)
    C.run_cast(R, same)


@pytest.mark.parametrize('C_', [128, 4096])
def test_softmax(C_):
    C.run_softmax_fwd(R, same, C_)
    for log in (False, True):
        C.run_softmax_bwd(R, same, C_, log)


@pytest.mark.parametrize('mode', ['layer_norm', 'rms_norm', 'rms_norm_apex'])
@pytest.mark.parametrize('d', [64, 768, 2048])
def test_norms(mode, d):
    C.run_norm_fwd(R, same, mode, d)
    C.run_norm_bwd(R, same, mode, d)


@pytest.mark.parametrize('case', C.ATTN_CASES[:3] + C.ATTN_CASES[4:], ids=str)
def test_attention(case):
    C.run_attention(AttentionStandIn, same, case)


# ------------------------------------------------------------------------------------------------------------ planted defects
def _truncate_bf16(x):
    """f32 -> bf16 by dropping the low 16 bits (round toward zero)."""
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF)


def _fails(fn, *a, **kw):
    with pytest.raises(AssertionError):
        fn(*a, **kw)


@pytest.mark.parametrize('M,N,K', GEMM_SHAPES)
def test_defect_a_truncating_bf16_store(M, N, K):
    a, b = C.graded(M, N, K, 'nt')
    (t, bud, _), = C.gemm_expect(a, b, 'nt')
    good, bad = R.gemm(a, b, 'nt'), _truncate_bf16(R.gemm(a, b, 'nt', out_dtype=F32))
    C.check_elements(good, t, bud, BF, 'rne')
    _fails(C.check_elements, bad, t, bud, BF, 'truncated')
    if K <= C.ROUNDING_MAX_K:
        assert abs(C.check_rounding(good, t, bud, 'rne')) < 0.01
        _fails(C.check_rounding, bad, t, bud, 'truncated')
    close(bad, t, name='the standing metric passes the truncating store')


def test_defect_b_bias_omitted_on_the_quiet_rows():
    M, N, K = 300, 192, 136
    a, b = C.graded(M, N, K, 'nt')
    bias = C.graded_vec(N)
    for od in (BF, F32):
        (t, bud, _), = C.gemm_expect(a, b, 'nt', bias=bias, out_dtype=od)
        bad = R.gemm(a, b, 'nt', bias=bias, out_dtype=od)
        quiet = C.scale_rows(M) <= 2.0 ** -6
        bad[quiet] = R.gemm(a, b, 'nt', out_dtype=od)[quiet]
        _fails(C.check_elements, bad, t, bud, od, 'bias dropped')
        close(bad, t, name='the standing metric passes the dropped bias')


def test_defect_c_rows_swapped():
    M, N, K = 200, 144, 72
    a, b = C.graded(M, N, K, 'nt')
    (t, bud, _), = C.gemm_expect(a, b, 'nt', out_dtype=F32)
    bad = R.gemm(a, b, 'nt', out_dtype=F32)
    bad[[128, 129]] = bad[[129, 128]]
    _fails(C.check_elements, bad, t, bud, F32, 'rows 128 and 129 swapped')


def test_defect_d_last_k_dropped_in_a_quiet_row_block():
    M, N, K = 513, 256, 2400
    a, b = C.graded(M, N, K, 'nt')
    (t, bud, _), = C.gemm_expect(a, b, 'nt', out_dtype=F32)
    bad = R.gemm(a, b, 'nt', out_dtype=F32)
    rows = torch.arange(192, 256)[C.scale_rows(M)[192:256] <= 2.0 ** -6]                 # the quiet rows >= 192 of row block 128..255
    bad[rows] = R.gemm(a[rows, :K - 8].contiguous(), b[:, :K - 8].contiguous(), 'nt', out_dtype=F32)
    _fails(C.check_elements, bad, t, bud, F32, 'last 8 k dropped')


def test_defect_e_relative_error_on_the_quiet_rows_of_an_f32_output():
    M, N, K = 200, 144, 72
    a, b = C.graded(M, N, K, 'nt')
    (t, bud, _), = C.gemm_expect(a, b, 'nt', out_dtype=F32)
    bad = R.gemm(a, b, 'nt', out_dtype=F32)
    quiet = C.scale_rows(M) <= 2.0 ** -6
    bad[quiet] *= 1 + 2.0 ** -12
    _fails(C.check_elements, bad, t, bud, F32, 'relative 2^-12')
    close(bad, t, name='the standing metric passes the relative error')


def test_defect_f_attention_rows_of_the_quietest_sample_scaled():
    case = C.ATTN_CASES[0]
    B, N, H, D, lens, win, _ = case
    q, k, v, _ = C.attention_inputs(B, N, H, D)

    def spoil(o):
        o = o.clone()
        o[B - 1] = (o[B - 1].float() * (1 + 2.0 ** -5)).to(BF)
        return o
    C.run_attention(AttentionStandIn, same, case)
    _fails(C.run_attention, AttentionStandIn, same, case, spoil=spoil)
    ln = torch.tensor(lens, dtype=torch.int32)
    good = R.attn_fwd(q, k, v, ln, win)[0]
    close(spoil(good), good, name='the standing metric passes the scaled rows')


def test_defect_in_the_attention_backward_of_the_quietest_sample():
    """The backward is checked on the yardstick forward's o and lse: a planted defect there must still fail."""
    case = C.ATTN_CASES[2]
    B = case[0]

    class Spoiled(AttentionStandIn):
        @staticmethod
        def attn_bwd(*a):
            dq, dk, dv = AttentionStandIn.attn_bwd(*a)
            dk = dk.clone()
            dk[B - 1] = (dk[B - 1].float() * (1 + 2.0 ** -5)).to(BF)
            return dq, dk, dv
    _fails(C.run_attention, Spoiled, same, case)
