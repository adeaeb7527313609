"""The LDS-DMA prefetch of the 256-row GEMM kernels (gemm256.hip): one buffer descriptor per operand, rebased per work item and per
K-tile in scalar registers, one 32-bit offset per lane.  Every case runs the 256-row kernel and the same call under
SCONF_GEMM_NO_256=1 (the 128x128 kernel, same K order per accumulator) and requires torch.equal - the yardstick of the existing
256-row tests - after asserting through sconf_gemm_variant which kernel the shape reaches (1 = 256 wide, 2 = 192 wide, 3 = TN).

Routing note: with N = 3072 the tile-width rule takes the 192-wide tile (3072 = 16 x 192: 256 items at 192 x 9 cost units against
192 at 256 x 8), so the (4096, 3072) and (6400, 3072) shapes cover the 192-wide kernel; the same item counts on the 256-wide
kernel - 192, the eligibility floor, and 300, more items than workgroups - come from N = 1024 (not a multiple of 192) with
M = 12288 and M = 19200, and from the rotary entry point, which always takes the 256-wide tile.

The rotary case: under SCONF_GEMM_NO_256 the entry point runs GEMM + in-place rotary, which rounds to bf16 twice, so only the
unrotated v block can be bit-identical; the q / k blocks are held to the f32 reference with the bf16 tolerance of the parity
contract (test_kernels_gpu.py), as the existing rotary test does.
"""
import ctypes as C

import pytest
import torch

import kernel_refs as R
from kernel_test_utils import BF, F32, close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import lcasr_amd.hip.ops as o
    o._lib.load()
    return o


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _variant(ops, layout, a, b, split=1, act='none', resid=False, pre=False):
    if layout == 'nt': (M, K), N = a.shape, b.shape[0]
    else: (K, M), N = a.shape, b.shape[1]
    return ops._lib.load().sconf_gemm_variant(ops.LAYOUT[layout], M, N, K, a.stride(0), b.stride(0), split, ops.ACT[act], int(resid), int(pre))


def _gemm(ops, a, b, layout, bias=None, resid=None, aux=None, act='none', alpha=1.0, out_f32=False, save_pre=False, split_k=1, accum=None):
    """sconf_gemm_bf16 on row-strided views (ops.gemm takes contiguous operands only); split_k > 1: slabs + the fixed-order reduce."""
    assert a.stride(1) == 1 and b.stride(1) == 1
    if layout == 'nt': (M, K), N = a.shape, b.shape[0]
    else: (K, M), N = a.shape, b.shape[1]
    lib = ops._lib
    splits = lib.load().sconf_gemm_num_splits(K, int(split_k)) if split_k > 1 else 1
    out_f32 = out_f32 or splits > 1 or accum is not None
    c = torch.empty((splits, M, N) if splits > 1 else (M, N), dtype=F32 if out_f32 else BF, device='cuda')
    pre = torch.empty(M, N, dtype=BF, device='cuda') if save_pre else None
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib.call('sconf_gemm_bf16', ops.LAYOUT[layout], _ptr(a), _ptr(b), _ptr(c), M, N, K, a.stride(0), b.stride(0), N, _ptr(bias), _ptr(resid), N,
             _ptr(aux), N, _ptr(pre), N, float(alpha), ops.ACT[act], int(out_f32), int(split_k), stream)
    if splits > 1:
        out = accum.clone() if accum is not None else torch.empty(M, N, dtype=F32, device='cuda')
        lib.call('sconf_splitk_reduce', _ptr(c), _ptr(out), splits, M * N, int(accum is not None), stream)
        c = out
    return (c, pre) if save_pre else (c,)


def _both(ops, monkeypatch, *args, **kw):
    monkeypatch.delenv('SCONF_GEMM_NO_256', raising=False)
    new = _gemm(ops, *args, **kw)
    monkeypatch.setenv('SCONF_GEMM_NO_256', '1')
    old = _gemm(ops, *args, **kw)
    monkeypatch.delenv('SCONF_GEMM_NO_256')
    return new, old


def _equal(new, old, what):
    for x, y in zip(new, old):
        assert torch.equal(x, y), (what, float((x.float() - y.float()).abs().max()))


def _rand(rows, cols, seed, scale=0.5):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, cols, generator=g) * scale).to(BF).cuda()


def _sliced(t, ld, start=8):
    """the same values as a column slice of a wider buffer: row stride ld, base 16-byte aligned only"""
    buf = torch.full((t.shape[0], ld), float('nan'), dtype=BF, device='cuda')      # what lies around the slice must never be read into the product
    v = buf[:, start:start + t.shape[1]]
    v.copy_(t)
    assert v.data_ptr() % 32 == 16
    return v


# (M, N, variant): 192 items at N = 3072 (192-wide tile, see the module docstring) and the 256-wide counterpart
NT_SHAPES = [(4096, 3072, 2), (12288, 1024, 1)]


@pytest.mark.parametrize('K', [64, 128, 192])
@pytest.mark.parametrize('M,N,variant', NT_SHAPES)
@pytest.mark.parametrize('strided', [False, True])
def test_nt_short_k(ops, monkeypatch, M, N, variant, K, strided):
    """One, two and three K-tiles per item at the eligibility floor of 192 items (N = 3072: 256 items of the 192-wide tile): every K-tile of the
    prefetch stream crosses an item boundary or sits next to one, and an odd count flips the buffer parity between items.
    strided: lda = K + 64, ldb = K + 128, views that start 8 elements into their buffers."""
    a, b = _rand(M, K, K), _rand(N, K, K + 1)
    if strided: a, b = _sliced(a, K + 64), _sliced(b, K + 128)
    monkeypatch.delenv('SCONF_GEMM_NO_256', raising=False)
    assert _variant(ops, 'nt', a, b) == variant
    new, old = _both(ops, monkeypatch, a, b, 'nt', out_f32=True)
    _equal(new, old, ('nt', M, N, K, strided))
    ref = a.float() @ b.float().t()
    assert float((new[0] - ref).abs().max()) <= 1e-5 * float(ref.abs().max()) + 1e-6       # f32 sums of <= 192 products, as test_gemm_256_row_kernels_short_k


@pytest.mark.parametrize('M,N,variant', [(6400, 3072, 2), (19200, 1024, 1)])
def test_nt_more_items_than_workgroups(ops, monkeypatch, M, N, variant):
    """300 items (400 of the 192-wide tile) over 256 workgroups: some workgroups take two items, the others drain their stream early."""
    K = 192
    a, b = _rand(M, K, 7), _rand(N, K, 8)
    monkeypatch.delenv('SCONF_GEMM_NO_256', raising=False)
    assert _variant(ops, 'nt', a, b) == variant
    new, old = _both(ops, monkeypatch, a, b, 'nt')
    _equal(new, old, ('nt', M, N))


@pytest.mark.parametrize('K', [64, 192])
def test_nt_192_wide(ops, monkeypatch, K):
    M, N = 16384, 768
    a, b = _rand(M, K, 3 * K), _rand(N, K, 3 * K + 1)
    monkeypatch.delenv('SCONF_GEMM_NO_256', raising=False)
    assert _variant(ops, 'nt', a, b) == 2
    sa, sb = _sliced(a, K + 64), _sliced(b, K + 128)
    assert _variant(ops, 'nt', sa, sb) == 2
    for x, y, what in ((a, b, 'contiguous'), (sa, sb, 'sliced')):
        for kw in (dict(), dict(out_f32=True)):
            new, old = _both(ops, monkeypatch, x, y, 'nt', **kw)
            _equal(new, old, ('192-wide', K, what, kw))


@pytest.mark.parametrize('M,N,variant', [(12288, 1024, 1), (4096, 3072, 2)])
def test_nt_epilogue_kinds(ops, monkeypatch, M, N, variant):
    """The specialised epilogues read bias, residual and aux through compiler-visible loads behind the asm-issued DMA."""
    K = 192
    a, b = _rand(M, K, 11), _rand(N, K, 12, scale=0.2)
    g = torch.Generator().manual_seed(13)
    bias = torch.randn(N, generator=g).cuda(); resid = torch.randn(M, N, generator=g).cuda(); aux = torch.randn(M, N, generator=g).to(BF).cuda()
    monkeypatch.delenv('SCONF_GEMM_NO_256', raising=False)
    for kw in (dict(bias=bias), dict(resid=resid, out_f32=True), dict(bias=bias, resid=resid, alpha=0.5, out_f32=True),
               dict(bias=bias, act='gelu_dsave', save_pre=True), dict(act='gelu_dsave', save_pre=True), dict(aux=aux, act='mulaux', alpha=0.5)):
        assert _variant(ops, 'nt', a, b, act=kw.get('act', 'none'), resid='resid' in kw, pre=bool(kw.get('save_pre'))) == variant
        new, old = _both(ops, monkeypatch, a, b, 'nt', **kw)
        _equal(new, old, list(kw))


def test_nt_rotary_entry_point(ops, monkeypatch):
    """M = 4096, N = 3 x 8 x 128 = 3072, K = 192 through sconf_gemm_qkv_rotary: the 256-wide tile (192 items) with the rotary row
    permutation of the B images.  See the module docstring for the yardsticks."""
    import sys
    sys.path.insert(0, '.')
    from oracle.sconformer_ref import rotary_tables
    Bn, Nseq, H, D, K = 8, 512, 8, 128, 192
    M = Bn * Nseq
    cos, sin = rotary_tables(Nseq, D, 1.5e6)
    cos, sin = cos[:, :D // 2].contiguous().cuda(), sin[:, :D // 2].contiguous().cuda()
    x, w = _rand(M, K, 21), _rand(3 * H * D, K, 22, scale=0.1)
    bias = torch.randn(3 * H * D, generator=torch.Generator().manual_seed(23)).cuda()
    monkeypatch.delenv('SCONF_GEMM_NO_256', raising=False)
    for bi in (None, bias):
        got = ops.gemm_qkv_rotary(x, w, bi, cos, sin, Nseq, H, D)
        monkeypatch.setenv('SCONF_GEMM_NO_256', '1')
        two = ops.gemm_qkv_rotary(x, w, bi, cos, sin, Nseq, H, D)
        monkeypatch.delenv('SCONF_GEMM_NO_256')
        assert not torch.equal(got, two), 'rotary epilogue (256-wide kernel) NOT taken'
        v_cols = slice(2 * H * D, 3 * H * D)
        assert torch.equal(got[:, v_cols], two[:, v_cols])
        ref = R.gemm_qkv_rotary(x.cpu(), w.cpu(), None if bi is None else bi.cpu(), cos.cpu(), sin.cpu(), Nseq, H, D)
        close(got, ref, name='qkv + rotary epilogue vs f32 reference')


@pytest.mark.parametrize('sliced', [False, True])
def test_tn_uneven_last_split(ops, monkeypatch, sliced):
    """768 x 768 output, split_k = 28 over 900 K-tiles: 33 K-tiles per split, 9 in the last one; plain and accumulated."""
    M = N = 768; K = 900 * 64
    a, b = _rand(K, M, 31, scale=0.3), _rand(K, N, 32, scale=0.3)
    if sliced: a, b = _sliced(a, M + 64), _sliced(b, N + 128)
    monkeypatch.delenv('SCONF_GEMM_NO_256', raising=False)
    assert _variant(ops, 'tn', a, b, split=28) == 3
    new, old = _both(ops, monkeypatch, a, b, 'tn', split_k=28, alpha=0.5)
    _equal(new, old, ('tn', sliced))
    ref = 0.5 * (a.float().t() @ b.float())
    assert float((new[0] - ref).abs().max()) <= 1e-4 * float(ref.abs().max())                 # as test_gemm_256_row_kernel_tn_split_k
    acc = torch.randn(M, N, generator=torch.Generator().manual_seed(33)).cuda()
    new, old = _both(ops, monkeypatch, a, b, 'tn', split_k=28, alpha=0.5, accum=acc)
    _equal(new, old, ('tn accum', sliced))


@pytest.mark.parametrize('M', [4096, 8192])
def test_nt_rows_past_4_gib(ops, monkeypatch, M):
    """A (M, 128) as a slice of an uninitialised buffer with lda = 2^19 + 64 elements (only the slice is written), so the descriptor
    must be rebased per item.  M = 4096: a 4.3 GB buffer whose last row starts 524 416 bytes short of 2^32, so the
    offsets of this case stop just below 4 GiB.  M = 8192 (8.6 GB) puts the second half of the row tiles past 4 GiB."""
    N, K, lda = 3072, 128, (1 << 19) + 64
    buf = torch.empty(M * lda, dtype=BF, device='cuda')
    a = buf.view(M, lda)[:, 8:8 + K]
    a.copy_(_rand(M, K, 41))
    assert M * lda * 2 > (1 << 32) and (M < 8192 or (M // 2) * lda * 2 > (1 << 32))
    # 192-wide kernel (N = 3072), then the 256-wide one (N = 4096, not a multiple of 192)
    for n, variant in ((N, 2), (4096, 1)):
        b = _rand(n, K, 42 + n)
        monkeypatch.delenv('SCONF_GEMM_NO_256', raising=False)
        assert _variant(ops, 'nt', a, b) == variant
        new, old = _both(ops, monkeypatch, a, b, 'nt', out_f32=True)
        _equal(new, old, ('nt > 4 GiB', M, n))
        ref = a.float() @ b.float().t()
        assert float((new[0] - ref).abs().max()) <= 1e-5 * float(ref.abs().max()) + 1e-6


def test_tn_k_range_past_4_gib(ops, monkeypatch):
    """TN with A (K = 4224, M = 4096) as a slice of an uninitialised buffer with lda = 2^19 + 64: one work item's k-range times ld
    is 4.4 GB, so the descriptor must be rebased per K-tile (the shape class of config 5's weight gradients)."""
    M = N = 4096; K = 66 * 64; lda = (1 << 19) + 64
    buf = torch.empty(K * lda, dtype=BF, device='cuda')
    a = buf.view(K, lda)[:, 8:8 + M]
    a.copy_(_rand(K, M, 51, scale=0.3))
    assert (K - 1) * lda * 2 > (1 << 32)
    b = _rand(K, N, 52, scale=0.3)
    monkeypatch.delenv('SCONF_GEMM_NO_256', raising=False)
    assert _variant(ops, 'tn', a, b) == 3
    new, old = _both(ops, monkeypatch, a, b, 'tn', out_f32=True)
    _equal(new, old, 'tn > 4 GiB')
    ref = a.float().t() @ b.float()
    assert float((new[0] - ref).abs().max()) <= 1e-4 * float(ref.abs().max())
