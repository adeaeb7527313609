"""Write-footprint tests of every C-ABI entry point (include/sconf.h) on the device: tests/footprint.py runs each case of
tests/footprint_cases.py twice out of one guarded arena (0xFF fill, random fill) and checks confinement, completeness /
write-before-read, and the values against the float64 restatement.  One parametrised test per family; each case prints the entry
point, the kernel variant its routing query reported, the arena bytes and the guard bytes checked.

No case hands a kernel an undersized or misaligned buffer: the refusal paths are host-side and have their own tests."""
import pytest
import torch

import footprint as FP
import footprint_cases as FC

pytestmark = pytest.mark.gpu

SWITCHES = ('SCONF_SUB_MFMA', 'SCONF_GEMM_NO_256', 'SCONF_ATTN_WIDE', 'SCONF_QKV_ROT_EPILOGUE_OFF')


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import lcasr_amd.hip.ops as o
    o._lib.load()
    return o


def _check(ops, id, monkeypatch):
    for k in SWITCHES: monkeypatch.delenv(k, raising=False)
    if id in FC.MFMA_OFF: monkeypatch.setenv('SCONF_SUB_MFMA', '0')
    FP.run_on_device(FC.build(id, ops._lib.load()), ops._lib.PROTOTYPES)


@pytest.mark.parametrize('id', FC.ids_of('gemm128'))
def test_gemm_128x128_kernel(ops, id, monkeypatch):
    """Six pairwise different leading dimensions: a swapped ldr / ldaux / ldpre, or a split-K slab stride that is not M * ldc, writes
    into a guard."""
    _check(ops, id, monkeypatch)


@pytest.mark.parametrize('id', FC.ids_of('gemm256'))
def test_gemm_256_row_kernels(ops, id, monkeypatch):
    _check(ops, id, monkeypatch)


@pytest.mark.parametrize('id', FC.ids_of('norm'))
def test_norms(ops, id, monkeypatch):
    _check(ops, id, monkeypatch)


@pytest.mark.parametrize('id', FC.ids_of('rows'))
def test_softmax_colsum_mask_cast_rotary(ops, id, monkeypatch):
    _check(ops, id, monkeypatch)


@pytest.mark.parametrize('id', FC.ids_of('attention'))
def test_attention(ops, id, monkeypatch):
    """Every operand view has a token and a batch stride of its own; the padding between tokens and batches is guard."""
    _check(ops, id, monkeypatch)


@pytest.mark.parametrize('id', FC.ids_of('convmod'))
def test_conv_module(ops, id, monkeypatch):
    _check(ops, id, monkeypatch)


@pytest.mark.parametrize('id', FC.ids_of('subsample'))
def test_subsampler(ops, id, monkeypatch):
    _check(ops, id, monkeypatch)


@pytest.mark.parametrize('id', FC.ids_of('ctc'))
def test_ctc(ops, id, monkeypatch):
    _check(ops, id, monkeypatch)


@pytest.mark.parametrize('id', FC.ids_of('eval'))
def test_evaluation_and_augmentation(ops, id, monkeypatch):
    _check(ops, id, monkeypatch)


@pytest.mark.parametrize('id', FC.ids_of('optim'))
def test_optimiser(ops, id, monkeypatch):
    _check(ops, id, monkeypatch)

