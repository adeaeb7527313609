"""GPU tests of the attention kernels at head_dim 64 and 256 (the paper's 12 x 64 and 3 x 256 models): kernel parity against
tests/kernel_refs.py in the shapes of test_kernels_gpu.ATT_CASES, the overflow case of the forward, the two models from
seed against the reference fixtures h12_scalars / h3_scalars, a step at the full paper shape, and windowed inference."""
import numpy as np
import pytest
import torch

import kernel_refs as R
from common_model import rel_l2_errors, strided_like_fixture
from conftest import golden_cfg, load_golden
from test_head_dims import fixture_inputs

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
PAPER = dict(vocab_size=4095, n_layers=6, d_model=768, use_rotary=True, rotary_base_freq=1500000, decoder_norm=True,
             self_conditioning=True, default_norm='layer_norm', bias_in_ff=False, subsampling_conv_channels=256)


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import lcasr_amd.hip.ops as o
    o._lib.load()
    return o


def dev(t):
    return t.cuda() if isinstance(t, torch.Tensor) else t


def close(out, ref, tol=1.2e-2, name=''):
    assert out.shape == ref.shape, f'{name}: shape {tuple(out.shape)} vs {tuple(ref.shape)}'
    o, r = out.detach().float().cpu(), ref.detach().float().cpu()
    assert torch.isfinite(o).all(), f'{name}: non-finite output'
    scale = float(r.abs().max()) + 1e-12
    err = float((o - r).abs().max()) / scale
    assert err <= tol, f'{name}: max err {err:.3e} of max|ref|={scale:.3e} > {tol}'


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.randn(*shape, generator=g).to(BF)


def rot_tables(N, D):
    inv = 1.0 / (1500000 ** (torch.arange(0, D, 2).float() / D))
    f = torch.arange(N).float()[:, None] * inv[None]
    return torch.cos(f).contiguous(), torch.sin(f).contiguous()


def check_fwd_bwd(ops, q, k, v, ln, win, rot, tag):
    o, lse = ops.attn_fwd(dev(q), dev(k), dev(v), dev(ln), win)
    orf, lser = R.attn_fwd(q, k, v, ln, win)
    close(o, orf, name=f'{tag} o')
    m = torch.isfinite(lser)
    assert torch.equal(torch.isfinite(lse.cpu()), m), f'{tag} lse: dead rows'
    assert float(((lse.cpu()[m] - lser[m]).abs() / lser[m].abs().clamp_min(1.0)).max()) < 2e-3, f'{tag} lse'
    do = rnd(*q.shape, seed=3)
    rt = None if rot is None else (dev(rot[0]), dev(rot[1]))
    dq, dk, dv = ops.attn_bwd(dev(q), dev(k), dev(v), o, dev(do), lse, dev(ln), win, rot=rt)
    dqr, dkr, dvr = R.attn_bwd(q, k, v, orf, do, lser, ln, win, rot=rot)
    close(dq, dqr, 2e-2, f'{tag} dq'); close(dk, dkr, 2e-2, f'{tag} dk'); close(dv, dvr, 2e-2, f'{tag} dv')


HD_CASES = [  # B, N, H, lengths, window, rotary in the backward
    (1, 128, 1, None, (-1, -1), False), (2, 200, 2, None, (-1, -1), True), (2, 333, 3, None, (-1, -1), False),
    (3, 192, 2, [192, 100, 7], (-1, -1), True), (2, 260, 2, [260, 131], (-1, -1), False),
    (2, 300, 2, None, (16, 16), True), (1, 257, 2, None, (24, 8), False), (2, 256, 2, [256, 77], (64, 0), True),
]


@pytest.mark.parametrize('D', [64, 256])
@pytest.mark.parametrize('case', HD_CASES)
def test_attention_head_dims_fwd_bwd(ops, D, case):
    B, N, H, lens, win, rot = case
    q, k, v = rnd(B, N, H, D), rnd(B, N, H, D, seed=1), rnd(B, N, H, D, seed=2)
    ln = torch.tensor(lens, dtype=torch.int32) if lens else None
    check_fwd_bwd(ops, q, k, v, ln, win, rot_tables(N, D) if rot else None, f'D={D} {case}')


@pytest.mark.parametrize('D', [64, 256])
def test_attention_head_dims_strided_views(ops, D):
    """q, k, v as strided views of one packed (B, N, 3, H, D) buffer and dq, dk, dv written into the blocks of another - the
    model's layout - with the rotary transpose in the backward."""
    B, N, H = 2, 200, 3
    packed = rnd(B, N, 3, H, D)
    pd = dev(packed)
    o, lse = ops.attn_fwd(pd[:, :, 0], pd[:, :, 1], pd[:, :, 2], None)
    q, k, v = (packed[:, :, i].contiguous() for i in range(3))
    orf, lser = R.attn_fwd(q, k, v, None)
    close(o, orf, name=f'D={D} packed o')
    do = rnd(B, N, H, D, seed=3)
    cos, sin = rot_tables(N, D)
    g = torch.empty(B, N, 3, H, D, dtype=BF, device='cuda')
    ops.attn_bwd(pd[:, :, 0], pd[:, :, 1], pd[:, :, 2], o, dev(do), lse, None, rot=(dev(cos), dev(sin)),
                 out=(g[:, :, 0], g[:, :, 1], g[:, :, 2]))
    ref = R.attn_bwd(q, k, v, orf, do, lser, None, rot=(cos, sin))
    for i, name in enumerate(('dq', 'dk', 'dv')):
        close(g[:, :, i], ref[i], 2e-2, f'D={D} packed {name}')


@pytest.mark.parametrize('D', [64, 256])
@pytest.mark.parametrize('boost', [1.9, 30.0])
def test_attention_head_dims_planted_score(ops, D, boost):
    """test_attention_forward_fixed_reference_and_its_careful_redo at D = 64 / 256: one score far above the rest of its row
    (boost 30: ~1e4 in scaled units, beyond the f32 exponent from any earlier reference point) - finite and exact output."""
    B, N, H = 2, 640, 2
    q, k, v = rnd(B, N, H, D), rnd(B, N, H, D, seed=1), rnd(B, N, H, D, seed=2)
    q[0, 300, 0, :] = boost; k[0, 411, 0, :] = boost
    q[1, 77, 1, :] = -boost; k[1, 600, 1, :] = -boost
    o, lse = ops.attn_fwd(dev(q), dev(k), dev(v), None, (-1, -1))
    assert bool(torch.isfinite(o.float()).all()) and bool(torch.isfinite(lse).all())
    check_fwd_bwd(ops, q, k, v, None, (-1, -1), None, f'D={D} planted {boost}')


@pytest.mark.parametrize('case', ['h12_scalars', 'h3_scalars'])
def test_head_dim_config_from_seed(case):
    """exp_set_rot_12h / exp_set_rot_3h at B = 2, T = 2048 (N = 256), lengths [2048, 1531], from torch.manual_seed(12345) against
    the reference: the bounds of test_c2_config_from_seed (loss, log-prob slice, gradient norms, strided gradient samples)."""
    from lcasr_amd.losses import CTCLoss
    from lcasr_amd.models.sconformer_xl import SCConformerXL
    fx = load_golden(case)
    torch.manual_seed(12345)
    m = SCConformerXL(**golden_cfg(fx)).cuda().train()
    assert m.head_dim in (64, 256) and m.n_heads * m.head_dim == 768
    x, ln, tg, tl = fixture_inputs(fx)
    out = m(x.cuda(), length=ln.cuda())
    lp = out['final_posteriors']
    assert lp.shape == (2, 256, 4096)
    loss = CTCLoss(blank=4095, reduction='sum')(lp.transpose(0, 1), tg.cuda(), out['length'], tl.cuda())
    (loss / (2048 * 2) * 100).backward()
    torch.cuda.synchronize()
    rel = abs(float(loss) - float(fx['loss'])) / float(fx['loss'])
    d = (lp[:, ::17, ::97].float().cpu() - torch.from_numpy(fx['logp_slice'])).abs()
    print(f'[{case}] loss {float(loss):.3f} vs {float(fx["loss"]):.3f} (rel {rel:.2e}); log-prob slice max|d| {float(d.max()):.3f} mean {float(d.mean()):.4f}')
    assert torch.equal(out['length'].cpu(), torch.from_numpy(fx['out_length']))
    assert rel < 1e-3, (float(loss), float(fx['loss']))
    assert float(d.max()) < 0.35 and float(d.mean()) < 0.05
    ref = {k[6:]: float(fx[k]) for k in fx.files if k.startswith('gnorm.')}
    big = max(ref.values())
    for k, p in m.named_parameters():
        gn = float(p.grad.double().norm())
        if ref[k] > 0.01 * big:
            assert abs(gn - ref[k]) / ref[k] < 0.10, (k, gn, ref[k])
    cap, cap2 = int(fx['gs_cap']), int(fx['gs_cap2'])
    got = {k: strided_like_fixture(strided_like_fixture(p.grad.detach().float().cpu(), cap), cap2) for k, p in m.named_parameters()}
    errs = rel_l2_errors(got, {k[3:]: fx[k] for k in fx.files if k.startswith('gs.')})
    worst, med = max(errs.values()), float(np.median(list(errs.values())))
    print(f'[{case}] gradient rel-L2: median {med:.3f} worst {worst:.3f}')
    assert len(errs) == len(list(m.parameters()))
    assert worst < 0.15 and med < 0.065, sorted(errs.items(), key=lambda kv: -kv[1])[:5]


@pytest.mark.parametrize('n_heads,head_dim', [(12, 64), (3, 256)])
def test_head_dim_paper_shape_step(monkeypatch, n_heads, head_dim):
    """The paper shape (6L/768D, T = 16384 -> N = 2048, B = 1): finite loss and gradients; the first layer's attention output
    against kernel_refs on the q, k, v it was computed from."""
    import lcasr_amd.functional as Fn
    from lcasr_amd.losses import CTCLoss
    from lcasr_amd.models.sconformer_xl import SCConformerXL
    seen = []
    real = Fn.ops.attn_fwd

    def spy(q, k, v, lengths, window=(-1, -1), scale=None):
        o, lse = real(q, k, v, lengths, window, scale)
        if not seen: seen.append([t if t is None else t.detach().cpu() for t in (q, k, v, lengths, o, lse)] + [window])
        return o, lse
    monkeypatch.setattr(Fn.ops, 'attn_fwd', spy)
    torch.manual_seed(12345)
    m = SCConformerXL(n_heads=n_heads, head_dim=head_dim, **PAPER).cuda().train()
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, 80, 16384, generator=g).cuda()
    tg = torch.randint(0, 4095, (1, 512), generator=g).cuda()
    out = m(x)
    lp = out['final_posteriors']
    assert lp.shape == (1, 2048, 4096)
    loss = CTCLoss(blank=4095, reduction='sum')(lp.transpose(0, 1), tg, out['length'], torch.tensor([512]).cuda())
    (loss / 16384 * 100).backward()
    torch.cuda.synchronize()
    assert np.isfinite(float(loss)) and float(loss) > 0
    assert all(bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    assert float(sum(float(p.grad.double().pow(2).sum()) for p in m.parameters())) > 0
    q, k, v, ln, o, lse, win = seen[0]
    assert q.shape == (1, 2048, n_heads, head_dim)
    orf, lser = R.attn_fwd(q, k, v, ln, win)
    close(o, orf, name='layer-0 attention at N = 2048')
    assert float((lse - lser).abs().max()) < 2e-3


def test_fetch_logits_windowed_attention_12_heads():
    """Sliding-window inference (fetch_logits, batched windows) and greedy decoding on a 12 x 64 model with
    attention_window_size set: the HIP path against the same model with the kernel references on the CPU."""
    import lcasr_amd.functional as Fn
    from lcasr_amd.decoding.greedy import GreedyCTCDecoder
    from lcasr_amd.eval.utils import fetch_logits
    from lcasr_amd.models.sconformer_xl import SCConformerXL
    fx = load_golden('infer_tiny')
    cfg = dict(golden_cfg(fx), n_heads=12, head_dim=64, attention_window_size=24)
    torch.manual_seed(3)
    m = SCConformerXL(**cfg).eval()
    assert m.layers[0].attend.fn.left_window == 24
    sd = {k: v.clone() for k, v in m.state_dict().items()}

    class Tok:
        def vocab_size(self): return int(cfg['vocab_size'])

    class Args: config = {'audio_chunking': {'size': 512, 'overlap': 128}}

    spec = torch.from_numpy(fx['spec'])
    sl, ov = fx['cases'].tolist()[-1]
    gpu = fetch_logits(Args, m.cuda(), spec, sl, ov, Tok(), use_tqdm=False, batched=True, max_batch=3)
    mc = SCConformerXL(**cfg).eval()
    mc.load_state_dict(sd)
    Fn.clear_weight_cache()
    real_ops = Fn.ops
    try:
        Fn.ops = R
        cpu = fetch_logits(Args, mc, spec, sl, ov, Tok(), use_tqdm=False, batched=True, max_batch=3)
    finally:
        Fn.ops = real_ops
        Fn.clear_weight_cache()
    assert gpu.shape == cpu.shape
    d = np.abs(gpu - cpu)
    assert float(d.max()) < 0.3 and float(d.mean()) < 0.03, (float(d.max()), float(d.mean()))
    dec = GreedyCTCDecoder(tokenizer=None, blank_id=m.decoder.num_classes - 1)
    g2 = gpu.reshape(-1, gpu.shape[-1])
    ids = dec(torch.from_numpy(g2).cuda(), decode=False)
    am = g2.argmax(-1)
    want = [int(t) for i, t in enumerate(am) if t != m.decoder.num_classes - 1 and (i == 0 or t != am[i - 1])]
    assert ids == want
