"""GPU tests of the attention-map kernels (csrc/attn_maps.hip) through hip/ops.py, and of the two collectors on the model.

Kernel references are f64 torch on the same bf16 operands (tests/attn_maps_refs.py).  Bounds:
  scores   f32 output within 1e-4 * max|ref| (the bound test_kernels_gpu.py uses for f32 GEMM output); bf16 output within an added
           2^-8 * max|ref| (twice bf16's half-ulp); the -inf positions exactly those of the mask.
  profile  per entry |err| <= 4e-3 * ref + 1e-6 * live_rows against the profile of the exact f64 softmax: 4e-3 is twice the 2e-3
           the project allows on the forward's lse, which enters P once; each (b, h) total within 4e-3 of its live-row count;
           offsets outside the window exactly 0; two calls bit-equal.
Model: both collectors on the infer_tiny model against tests/golden/attn_maps_tiny.npz within twice the fixture's yardsticks (the
reference's own fp32-versus-bf16-autocast difference)."""
import functools

import pytest
import torch

import attn_maps_refs as R
from common_model import build_from_fixture
from conftest import load_golden

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
# (B, N, H, D, lengths, window): every head_dim; N not a multiple of the 32-row or the 256-key tile; ragged; one- and two-sided
# windows; two key tiles at N = 300 and 257; more than one band of 224 offsets wherever the window leaves more than 224
CASES = [(2, 200, 2, 32, [200, 131], (-1, -1)),
         (1, 125, 2, 64, None, (-1, -1)),
         (2, 300, 2, 128, [300, 64], (24, 8)),
         (1, 257, 1, 256, None, (-1, 40))]
PROFILE_CASES = [c + (1.0,) for c in CASES] + [CASES[0] + (4.0,)]          # the last one peaked: q scaled by 4


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import lcasr_amd.hip.ops as o
    o._lib.load()
    return o


@functools.lru_cache(maxsize=None)
def operands(B, N, H, D, lengths, qscale=1.0):
    """q, k, v as the blocks of one (B,N,3,H,D) bf16 buffer on the device, lengths as an int32 tensor, shared by the tests."""
    g = torch.Generator().manual_seed(B * 1000 + N + D)
    qkv = torch.randn(B, N, 3, H, D, generator=g)
    qkv[:, :, 0] *= qscale
    qkv = qkv.to(BF).cuda()
    ln = None if lengths is None else torch.tensor(lengths, dtype=torch.int32).cuda()
    return qkv, ln


@functools.lru_cache(maxsize=None)
def ref_scores(case):
    B, N, H, D, lengths, window = case
    qkv, ln = operands(B, N, H, D, None if lengths is None else tuple(lengths))
    return R.scores_f64(qkv[:, :, 0], qkv[:, :, 1], ln, window)


def _key(case):
    return case[:4] + (None if case[4] is None else tuple(case[4]),) + case[5:]


@pytest.mark.parametrize('case', CASES, ids=lambda c: f'B{c[0]}N{c[1]}H{c[2]}D{c[3]}w{c[5][0]}_{c[5][1]}')
def test_scores_against_f64(ops, case):
    B, N, H, D, lengths, window = _key(case)
    qkv, ln = operands(B, N, H, D, lengths)
    q, k = qkv[:, :, 0], qkv[:, :, 1]
    ref = ref_scores(_key(case))
    dead = torch.isinf(ref)
    top = float(ref[~dead].abs().max())
    for dtype, bound in ((torch.float32, 1e-4 * top), (BF, (1e-4 + 2.0 ** -8) * top)):
        got = ops.attn_scores(q, k, ln, window, out_dtype=dtype)
        assert got.shape == (B, H, N, N) and got.dtype == dtype
        assert torch.equal(got == float('-inf'), dead), 'the -inf positions are not those of the mask'
        err = float((got.double() - ref)[~dead].abs().max())
        print(f'scores {dtype} B{B} N{N} H{H} D{D}: max err {err:.3e}, bound {bound:.3e} (max|ref| {top:.3f})')
        assert err <= bound
        # the strided views of the qkv buffer against contiguous copies: bit for bit
        assert torch.equal(ops.attn_scores(q.contiguous(), k.contiguous(), ln, window, out_dtype=dtype), got)


@pytest.mark.parametrize('case', PROFILE_CASES, ids=lambda c: f'B{c[0]}N{c[1]}H{c[2]}D{c[3]}w{c[5][0]}_{c[5][1]}x{c[6]:g}')
def test_offset_profile_against_f64(ops, case):
    B, N, H, D, lengths, window, qscale = _key(case)
    qkv, ln = operands(B, N, H, D, lengths, qscale)
    q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    _, lse = ops.attn_fwd(q, k, v, ln, window)
    got = ops.attn_offset_profile(q, k, lse, ln, window)
    assert got.shape == (B, H, 2 * N - 1) and got.dtype == torch.float32
    assert torch.equal(ops.attn_offset_profile(q, k, lse, ln, window), got), 'two calls differ'
    ref = R.exact_profile_f64(q, k, ln, window)
    live = (ln.double() if ln is not None else torch.full((B,), float(N), dtype=torch.float64, device='cuda'))[:, None, None]
    err = (got.double() - ref).abs()
    slack = err - (4e-3 * ref + 1e-6 * live)
    tot = (got.double().sum(-1, keepdim=True) - live).abs()
    print(f'profile B{B} N{N} H{H} D{D} x{qscale:g}: max err {float(err.max()):.3e} at ref {float(ref.flatten()[err.argmax()]):.3e}, '
          f'worst slack {float(slack.max()):.3e}, peak {float(ref.max()):.3f}, total off by {float(tot.max()):.3e}')
    assert float(slack.max()) <= 0
    assert float(tot.max()) <= 4e-3
    d = torch.arange(-(N - 1), N, device='cuda')
    outside = torch.zeros_like(d, dtype=torch.bool)
    if window[0] >= 0: outside |= d < -window[0]
    if window[1] >= 0: outside |= d > window[1]
    assert (got[..., outside] == 0).all()
    # strided views against contiguous copies
    assert torch.equal(ops.attn_offset_profile(q.contiguous(), k.contiguous(), lse, ln, window), got)


def test_long_windowed_profile(ops):
    """The 10-hour evaluation mode in miniature: N = 70001 under a (64, 64) window - 137 query chunks of one 224-offset band, key
    tiles outside the band never visited - against a banded f64 reference."""
    B, N, H, D, window = 1, 70001, 1, 32, (64, 64)
    qkv, _ = operands(B, N, H, D, None)
    q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    _, lse = ops.attn_fwd(q, k, v, None, window)
    got = ops.attn_offset_profile(q, k, lse, None, window)
    ref = R.banded_profile_f64(q, k, window)[None]
    err = (got.double() - ref).abs()
    slack = err - (4e-3 * ref + 1e-6 * N)
    print(f'long windowed profile: max err {float(err.max()):.3e}, worst slack {float(slack.max()):.3e}, peak {float(ref.max()):.1f}, '
          f'total {float(got.double().sum()):.3f} of {N}')
    assert float(slack.max()) <= 0
    assert (got[..., :N - 1 - 64] == 0).all() and (got[..., N + 64:] == 0).all()
    assert torch.equal(ops.attn_offset_profile(q, k, lse, None, window), got)


def test_scores_64bit_indexing(ops):
    """H * N * N > 2^31 elements: sampled rows of a bf16 score matrix, the last row of the last head among them."""
    B, N, H, D = 1, 33000, 2, 32
    assert H * N * N > 2 ** 31
    qkv, _ = operands(B, N, H, D, None)
    q, k = qkv[:, :, 0], qkv[:, :, 1]
    got = ops.attn_scores(q, k, None, (-1, -1), out_dtype=BF)
    rows = [0, 31, 32, 16383, 32767, 32768, N - 2, N - 1]
    for h in range(H):
        ref = (q[0, rows, h].double() @ k[0, :, h].double().t()) * D ** -0.5
        err = float((got[0, h, rows].double() - ref).abs().max())
        top = float(ref.abs().max())
        assert err <= (1e-4 + 2.0 ** -8) * top, (h, err, top)
    del got


def _attn(m):
    return [l.attend.fn for l in m.layers]


def test_collectors_on_the_model_against_the_reference(ops):
    from lcasr_amd.components.attention import CollectAttentionOffsets, CollectAttentionProbs
    fx, gold = load_golden('infer_tiny'), load_golden('attn_maps_tiny')
    m = build_from_fixture(fx, 'cuda').eval()
    spec = torch.from_numpy(fx['spec'].copy())[:, :, :int(gold['frames'])].cuda()
    ragged, rl = torch.cat([spec, spec.flip(-1)], 0), torch.tensor([1000, 800]).cuda()
    with torch.no_grad():
        plain = m(spec, return_logits=True)['final_posteriors'].clone()
        plain_r = m(ragged, length=rl, return_logits=True)['final_posteriors'].clone()
    f32 = []
    hooks = [a.return_attention_module.register_forward_hook(lambda _m, _i, out: f32.append(out[1])) for a in _attn(m)]
    a, b = CollectAttentionProbs(_attn(m)), CollectAttentionOffsets(_attn(m))
    with torch.no_grad():
        seen = m(spec, return_logits=True)['final_posteriors']
    assert torch.equal(seen, plain)
    assert all(t.is_cuda and t.dtype == torch.float32 for t in f32)
    got, (prof, live) = a(), b()
    assert got.dtype == BF and tuple(got.shape) == tuple(gold['collector_shape'].tolist()) and live.tolist() == [125]
    want = torch.from_numpy(gold['scores'])
    for name, s in (('bf16 collector', got.float()), ('f32 hook', torch.stack(f32, 0).cpu())):
        d = (s - want).abs()
        print(f'[{name}] scores max|d| {float(d.max()):.5f} (yard {float(gold["yard.scores_max"]):.5f}) '
              f'mean|d| {float(d.mean()):.6f} (yard {float(gold["yard.scores_mean"]):.6f})')
        assert float(d.max()) <= 2 * float(gold['yard.scores_max'])
        assert float(d.mean()) <= 2 * float(gold['yard.scores_mean'])
    dp = (prof - torch.from_numpy(gold['profile'])).abs()
    print(f'profile max|d| {float(dp.max()):.5f} (yard {float(gold["yard.profile_max"]):.5f})')
    assert float(dp.max()) <= 2 * float(gold['yard.profile_max'])
    # the ragged batch, where the reference raises: padded rows and columns are -inf and contribute nothing
    f32.clear()
    with torch.no_grad():
        seen_r = m(ragged, length=rl, return_logits=True)['final_posteriors']
    assert torch.equal(seen_r, plain_r)
    s, (prof, live) = a().float(), b()
    assert live.tolist() == [125, 100] and tuple(s.shape) == (2, 2, 2, 125, 125) and tuple(prof.shape) == (2, 2, 2, 249)
    assert torch.isinf(s[:, 1, :, 100:, :]).all() and torch.isinf(s[:, 1, :, :, 100:]).all()
    assert torch.isfinite(s[:, 1, :, :100, :100]).all() and torch.isfinite(s[:, 0]).all()
    assert float((prof.sum(-1) - live[None, :, None]).abs().max()) <= 4e-3
    assert float(prof[:, 1, :, :24].abs().max()) == 0 and float(prof[:, 1, :, -24:].abs().max()) == 0
    for h in hooks: h.remove()
    a.remove(); b.remove()
    with torch.no_grad():
        assert torch.equal(m(spec, return_logits=True)['final_posteriors'], plain)
