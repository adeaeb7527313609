"""Per-block gradient parity of the fused autograd blocks on the GPU: lcasr_amd.functional over the HIP kernels against float64.

The cases (block_cases.py), the checker and the bound E_fused <= max(2 E_ac, 2^-8) (block_parity.py) are those of test_blocks.py, which
runs them over the emulated ops, anchors the restatements to the reference's captures and shows that the checker fails on a 5 % error
in any one tensor.  Gradient modes: (a) returned gradients, (b) direct accumulation into a pre-filled p.grad with the grad-ready
hook, (c) chains handing gradients over through parked bf16 twins (twin on / off, stale twin), (d) non-contiguous dy, (e) ff ckpt=1.
Each route a case is there for is asserted from the library's own queries: sc_delta_enabled, sub_stage01_slabs.

Measured on an MI355X (relative L2 against float64; maxima over the cases and tensors of a block; ratio = E_fused / E_ac):

  block            E_fused max   E_ac max    worst E_fused / E_ac (over tensors with E_ac >= 1e-4)
  norm             1.66e-03      1.24e-07    -     (f32 against f32; E_fused is the bf16-output case, below the 2^-8 floor)
  norm2            1.84e-03      1.50e-07    -     (as norm: h2 is bf16)
  ff               4.89e-03      4.73e-03    1.15  (nb, branch alone without biases)
  attn             7.12e-03      8.29e-03    0.96  (nb, rotary)
  conv             7.86e-03      1.47e-02    0.92  (nb, eval)
  selfcond         1.08e-02      1.09e-02    1.07  (nb, M 3072 V 4096: the sc_delta route)
  head             3.39e-03      4.27e-03    1.00  (x, return_logits)
  head_ctc         5.41e-03      6.35e-03    1.10  (w1, prenormed by norm2(twice))
  subsample        1.01e-02      1.03e-02    1.03  (b0, C 32)
  subsample4       5.84e-03      7.07e-03    1.07  (b0, C 32)
  chain-selfcond   1.15e-02      1.42e-02    1.17  (cv.brn_b, S64)
  chain-head_ctc   1.71e-02      2.33e-02    0.82  (at.nw)
Every tensor of every case lies between 0.3 and 1.2 times the yardstick; the factor 2 of the bound was never needed.
Caps set individually (block_cases.py, with the measured E_ac): conv in training (3.5e-2; E_ac of bpw1 and nb 1.07e-2 to 1.47e-2 here and
up to 1.75e-2 over other seeds) and the three chains (5e-2; E_ac up to 2.33e-2).  Every other case meets the common cap of 2.5e-2.
The chains have no tighter sensitivity than their cap allows: a tensor at E_ac 2.33e-2 has a bound of 4.66e-2, so an error of about
5 % is the smallest that is sure to fail there (test_blocks.py runs the 1.05 self-check on the S64 chains too).
Mode (d) runs every block: one dy per used output, stride 0 and transposed - norm with its f32 and its bf16 output, norm2 with dy on
y1 alone, on h2 alone and on both (the three branches of Norm2Fn.backward), head_ctc with the stride-0 dnll of nll.sum().backward(),
plain and behind norm2(twice) (its nll is 1-D: a transposed form does not exist, .t() changes nothing).
Routes: (M 512, V 1024, d 256) does NOT take the sc_delta backward (8 tiles of 256 x 256 against the 192 the kernel asks for), nor does
any M = 512 shape take the 256-row NT GEMM kernels; the sc_delta route is asserted and measured at (M 3072, V 4096, d 64).  So the S256
ff, attn and conv cases do not cover the 256-row NT kernels: of these cases only the two (M 3072, V 4096) self-conditioning ones do.
Found by these cases: conv_block with bpw1=None raised in its backward (it unpacked a pair that convmod_bwd returns only with column
sums); the case conv-...-bpw10 is its regression test.
"""
import pytest
import torch

import block_cases as C
import block_parity as P

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings('ignore::UserWarning')]


@pytest.fixture(scope='module')
def Fn():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import lcasr_amd.functional as F_
    import lcasr_amd.hip.ops as o
    o._lib.load()
    yield F_
    F_.clear_weight_cache()
    F_._twins.clear()


@pytest.mark.parametrize('case', C.ALL, ids=repr)
def test_block_returned_gradients(case, Fn):
    P.check_block(case, Fn, 'cuda')


@pytest.mark.parametrize('case', C.SMALL + C.CHAINS[:2] + C.BIG[3:4], ids=repr)
def test_block_direct_gradients(case, Fn):
    P.check_block_direct(case, Fn, 'cuda')
    assert not Fn._direct['on'] and Fn._direct['hook'] is None


def test_direct_gradients_reach_the_leaf_behind_a_non_leaf_weight(Fn):
    case = C.BY_NAME['selfcond-layer_norm-norm1-pre0-M231-d64-V129']
    res, fired = P.run_fused(case, Fn, 'cuda', direct=True)
    assert sorted(fired) == ['bre', 'nb', 'nw']
    assert all(res.grads[k] is not None and float(res.grads[k].norm()) > 0 for k in case.nondirect)
    P.check_result(case, res, 'direct, non-leaf wff')


@pytest.mark.parametrize('case', C.NONCONTIG, ids=repr)
def test_block_noncontiguous_dy(case, Fn):
    P.check_noncontiguous_dy(case, Fn, 'cuda')


def test_ff_checkpoint_recompute_is_bit_equal(Fn):
    a, b = P.run_fused(C.FF_CKPT[0], Fn, 'cuda'), P.run_fused(C.FF_CKPT[1], Fn, 'cuda')
    P.same_results(a, b, 'ff ckpt 0 / 1', exact=True)
    P.check_result(C.FF_CKPT[1], b, 'ckpt=1')


@pytest.mark.parametrize('case', C.CHAINS, ids=repr)
def test_chain_twin_on_off(case, Fn, monkeypatch):
    P.check_twin_on_off(case, Fn, 'cuda', monkeypatch, C.CHAIN_COLSUM_BIASES)


def test_stale_twin_is_not_taken(Fn, monkeypatch):
    P.check_stale_twin(C.SMALL_BY_BLOCK['ff'][0], Fn, 'cuda', monkeypatch)


def test_sc_delta_route_of_the_cases(Fn, monkeypatch):
    """The (M 3072, V 4096, d 64) cases take the sc_delta backward; (M 512, V 1024, d 256) and the tiny shapes do not (fewer than 3/4
    of a round of 256 x 256 tiles).  With SCONF_SC_DELTA=0 the same cases take the two-pass backward and meet the same bound."""
    monkeypatch.delenv('SCONF_SC_DELTA', raising=False)
    assert Fn.sc_delta_enabled(3072, 4096, 64)
    print(f'[route] sc_delta: (3072, 4096, 64) {Fn.sc_delta_enabled(3072, 4096, 64)}, (512, 1024, 256) {Fn.sc_delta_enabled(512, 1024, 256)}, '
          f'(231, 144, 64) {Fn.sc_delta_enabled(231, 144, 64)}')
    assert not Fn.sc_delta_enabled(512, 1024, 256) and not Fn.sc_delta_enabled(231, 144, 64)
    monkeypatch.setenv('SCONF_SC_DELTA', '0')
    assert not Fn.sc_delta_enabled(3072, 4096, 64)
    for case in C.SC_DELTA_OFF:
        P.check_result(case, P.run_fused(case, Fn, 'cuda'), 'SCONF_SC_DELTA=0')


def test_subsampler_routes_of_the_cases(Fn):
    """C 16 takes the VALU stage kernels and C 32 the MFMA ones, forward and backward (the cases themselves run in the tests above)."""
    from lcasr_amd.hip import ops
    seen = set()
    for case in C.SMALL:
        if case.block.startswith('subsample'):
            f, b = ops.sub_stage01_slabs(case.sub['F'], case.sub['C'], False), ops.sub_stage01_slabs(case.sub['F'], case.sub['C'], True)
            print(f'[route] {case.name}: stage-0/1 slabs forward {f}, backward {b}')
            assert (f == 0) == (b == 0) == (case.sub['C'] % 32 != 0), (case.name, f, b)
            seen.add((case.block, f != 0))
    assert seen == {('subsample', False), ('subsample', True), ('subsample4', False), ('subsample4', True)}


def test_attention_and_norm2_routes_of_the_cases(Fn):
    """S256 (D 128, N 256) takes the 8-wave attention kernels, S64 (D 32) the 4-wave ones; both widths take the fused norm pair."""
    from lcasr_amd.hip import _lib
    lib = _lib.load()
    for S, waves in ((C.S256, 8), (C.S64, 4)):
        got = int(lib.sconf_attn_waves(S['D'], S['N'], 3 * S['H'] * S['D']))
        print(f'[route] attention {S["tag"]}: {got} waves; norm2 {Fn.norm2_enabled(S["d"], "layer_norm", "layer_norm")}')
        assert got == waves and Fn.norm2_enabled(S['d'], 'layer_norm', 'layer_norm')
