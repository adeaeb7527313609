"""The K-tile stream of the 256-row GEMM kernels (gemm256.hip) after the per-item descriptors and the peeled tail: one buffer
descriptor per operand and WORK ITEM, K-tile steps in the scalar offset, a steady loop without validity tests for the K-tiles whose
prefetch stays inside the cursor's item and one general K-tile at every item crossing and past the stream's end.

In the manner of test_gemm_dma_gpu.py (whose helpers are used): every case asserts through sconf_gemm_variant which kernel the shape
reaches (1 = 256 wide, 2 = 192 wide, 3 = TN), then requires torch.equal against the same call under SCONF_GEMM_NO_256=1 (the
128x128 kernel, same K order per accumulator).  The cases are what the change newly puts at risk:
  short streams     fewer items than workgroups and one K-tile per item: the steady loop runs zero times, some workgroups have no item;
  tail entry        items = workgroups + 1 with 2 or 3 K-tiles each: one workgroup enters the tail straight after an item crossing;
  far corners       consecutive items of one workgroup more than 4 GiB apart in A, one K-tile each: every K-tile builds a descriptor;
  stray reads       operands as interior slices of NaN-filled parents: a read outside the operand that reaches an accumulator shows;
  far launches      a K-strided item whose k-range times ld passes 4 GiB at a K-tile that is no item boundary (per-K-tile rebase).
Item counts follow the device's CU count (the grid is min(items, CUs)).
"""
import pytest
import torch

from kernel_test_utils import BF
from test_gemm_dma_gpu import _both, _equal, _rand, _sliced, _variant, ops  # noqa: F401  (ops: the module's fixture)

pytestmark = pytest.mark.gpu


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _check(ops, monkeypatch, a, b, layout, variant, what, **kw):
    monkeypatch.delenv('SCONF_GEMM_NO_256', raising=False)
    assert _variant(ops, layout, a, b, split=kw.get('split_k', 1)) == variant, what
    new, old = _both(ops, monkeypatch, a, b, layout, **kw)
    _equal(new, old, what)
    assert not bool(torch.isnan(new[0]).any()), what
    return new[0]


def _floor_items():
    """an item count from the eligibility floor (3/4 of the CUs) up, below the CU count: a multiple of 4 for the tile grids below"""
    cus = _cus()
    n = -(-3 * cus // 16) * 4
    assert 3 * cus <= 4 * n and n < cus, (cus, n)
    return n


def test_short_streams_nt(ops, monkeypatch):
    """K = 64 and fewer items than workgroups (192 of 256 CUs): a stream is one K-tile, issued entirely by the prologue."""
    n = _floor_items()
    K = 64
    for (M, N, variant) in ((n // 4 * 256, 1024, 1), (n // 16 * 256, 3072, 2)):           # n items of 256x256 / of 256x192
        a, b = _rand(M, K, 61), _rand(N, K, 62)
        got = _check(ops, monkeypatch, a, b, 'nt', variant, ('short nt', M, N), out_f32=True)
        ref = a.float() @ b.float().t()
        assert float((got - ref).abs().max()) <= 1e-5 * float(ref.abs().max()) + 1e-6     # f32 sums of 64 products, as test_nt_short_k


@pytest.mark.parametrize('tiles', [1, 2])
def test_short_streams_tn(ops, monkeypatch, tiles):
    """TN with K-ranges of one K-tile (tiles = 1: K = 64; tiles = 2: K = 128 split in two) and fewer items than workgroups."""
    n = _floor_items()
    M, N, K = 4 * 256, n // (4 * tiles) * 256, 64 * tiles
    a, b = _rand(K, M, 63, scale=0.3), _rand(K, N, 64, scale=0.3)
    _check(ops, monkeypatch, a, b, 'tn', 3, ('short tn', tiles), split_k=tiles, out_f32=True)


@pytest.mark.parametrize('K', [128, 192])
@pytest.mark.parametrize('N,variant', [(256, 1), (192, 2)])
def test_tail_entry_nt(ops, monkeypatch, N, variant, K):
    """items = workgroups + 1 (one column of M tiles): workgroup 0 takes a second item, so at the crossing into it the cursor has
    one or two K-tiles left and the stream goes from the crossing K-tile straight into the tail; every other workgroup is in the
    tail from its first K-tile on."""
    M = (_cus() + 1) * 256
    a, b = _rand(M, K, 65 + K), _rand(N, K, 66 + K)
    _check(ops, monkeypatch, a, b, 'nt', variant, ('tail nt', N, K))


@pytest.mark.parametrize('tiles', [1, 2, 3])
def test_tail_entry_tn(ops, monkeypatch, tiles):
    """One 256x256 output tile, split_k = workgroups + 1, k-ranges of 1, 2 and 3 K-tiles."""
    splits = _cus() + 1
    K = splits * tiles * 64
    a, b = _rand(K, 256, 67 + tiles, scale=0.3), _rand(K, 256, 68 + tiles, scale=0.3)
    got = _check(ops, monkeypatch, a, b, 'tn', 3, ('tail tn', tiles), split_k=splits)
    ref = a.float().t() @ b.float()
    assert float((got - ref).abs().max()) <= 1e-4 * float(ref.abs().max())                  # as test_tn_uneven_last_split


LD_FAR = (1 << 19) + 64                       # the row stride of test_nt_rows_past_4_gib: 16 row tiles of it span 4 GiB + 512 KiB


def _far_rows(rows, cols, seed, scale=0.5):
    """(rows, cols) as a slice of an uninitialised buffer with row stride LD_FAR; only the slice is written"""
    buf = torch.empty(rows * LD_FAR, dtype=BF, device='cuda')
    v = buf.view(rows, LD_FAR)[:, 8:8 + cols]
    v.copy_(_rand(rows, cols, seed, scale))
    return v


@pytest.mark.parametrize('N,variant', [(512, 1), (384, 2)])
def test_nt_item_crossing_to_a_far_corner(ops, monkeypatch, N, variant):
    """Two column tiles and workgroups / 2 + 1 row tiles: items = workgroups + 2, and the second items of workgroups 0 and 1 lie 32
    places on in the item order, i.e. 16 row tiles = 4 GiB + 512 KiB further into A (4 row panels per patch).  K = 64: every K-tile
    of the stream is an item crossing that builds both descriptors."""
    cus = _cus()
    M, K = (cus // 2 + 1) * 256, 64
    a = _far_rows(M, K, 71)
    assert 16 * 256 * LD_FAR * 2 > (1 << 32)
    b = _rand(N, K, 72)
    got = _check(ops, monkeypatch, a, b, 'nt', variant, ('far corner nt', N), out_f32=True)
    ref = a.float() @ b.float().t()
    assert float((got - ref).abs().max()) <= 1e-5 * float(ref.abs().max()) + 1e-6
    del a
    torch.cuda.empty_cache()


def test_tn_item_crossing_to_a_far_corner(ops, monkeypatch):
    """One output tile, k-ranges of 2 K-tiles and a last one of 1 (uneven), split_k = workgroups + 1: the second item of workgroup 0
    starts 32 splits = 4096 k-rows = 4 GiB + 512 KiB further into A."""
    splits = _cus() + 1
    K = (splits - 1) * 128 + 64
    a = _far_rows(K, 256, 73, scale=0.3)
    assert 32 * 128 * LD_FAR * 2 > (1 << 32)
    b = _rand(K, 256, 74, scale=0.3)
    monkeypatch.delenv('SCONF_GEMM_NO_256', raising=False)
    assert ops._lib.load().sconf_gemm_num_splits(K, splits) == splits
    got = _check(ops, monkeypatch, a, b, 'tn', 3, 'far corner tn', split_k=splits)
    ref = a.float().t() @ b.float()
    assert float((got - ref).abs().max()) <= 1e-4 * float(ref.abs().max())
    del a
    torch.cuda.empty_cache()


@pytest.mark.parametrize('K', [64, 192])
@pytest.mark.parametrize('M,N,variant', [(12288, 1024, 1), (4096, 3072, 2)])
def test_no_stray_reads_nt(ops, monkeypatch, M, N, variant, K):
    """Both operands interior slices (ld > K, start 8 elements in) of NaN-filled parents, 1 and 3 K-tiles per item."""
    a, b = _sliced(_rand(M, K, 75), K + 64), _sliced(_rand(N, K, 76), K + 128)
    _check(ops, monkeypatch, a, b, 'nt', variant, ('stray nt', M, N, K), out_f32=True)


@pytest.mark.parametrize('tiles', [1, 3])
def test_no_stray_reads_tn(ops, monkeypatch, tiles):
    """TN: (K, 1024) and (K, 768) slices of NaN-filled parents, 64 k-ranges of 1 or 3 K-tiles: 768 items."""
    K = 64 * 64 * tiles
    a, b = _sliced(_rand(K, 1024, 77, scale=0.3), 1024 + 64), _sliced(_rand(K, 768, 78, scale=0.3), 768 + 128)
    _check(ops, monkeypatch, a, b, 'tn', 3, ('stray tn', tiles), split_k=64)


def test_tn_far_launch_rebases_inside_the_item(ops, monkeypatch):
    """The shape class of test_tn_k_range_past_4_gib with another ld and split: lda = 2^20 + 64 and two k-ranges of 33 K-tiles, each
    4.4 GB of A, so the 4 GiB line falls between K-tiles 31 and 32 of an item, not on an item boundary."""
    M = N = 4096; K = 66 * 64; lda = (1 << 20) + 64
    buf = torch.empty(K * lda, dtype=BF, device='cuda')
    a = buf.view(K, lda)[:, 8:8 + M]
    a.copy_(_rand(K, M, 79, scale=0.3))
    assert 33 * 64 * lda * 2 > (1 << 32) > 31 * 64 * lda * 2
    b = _rand(K, N, 80, scale=0.3)
    got = _check(ops, monkeypatch, a, b, 'tn', 3, 'tn far launch', split_k=2)
    ref = a.float().t() @ b.float()
    assert float((got - ref).abs().max()) <= 1e-4 * float(ref.abs().max())
    del a, buf
    torch.cuda.empty_cache()
