"""GPU tests of the SpecAugment / dynamic-evaluation kernels (through lcasr_amd.hip.ops -> libsconf_hip.so) and of
dynamic_eval end to end on the HIP path, against tests/dyneval_refs.py and the reference's own run recorded in
tests/golden/dyneval_cases.npz.

Bounds: spec_mask, ctc_collapse, pseudo-labels and the restored state are exact; mean_f32 agrees with float64 to 1e-6
relative (f32 accumulation of <= 1e7 elements in a tree order) and is bit-identical from call to call; the dynamic_eval
numbers stay within 2x the reference's own fp32-vs-bf16-autocast noise on the same case (tests/dyneval_refs.py).

Measured on an MI355X (first run; the same for retokenize true and false; [reference's own autocast noise], bound = 2 x that):
    case        log-prob max     log-prob mean     prob max          per-step loss rel   parameter-change norm rel
    w256        0.262 [2.71]     0.0133 [0.104]    4.2e-5 [5.2e-4]   0.077  [0.77]       3.7e-6 [0.26]
    w256_e2     0.358 [5.14]     0.0213 [0.206]    4.6e-3 [1.1e-2]   0.096  [1.69]       4.6e-4 [0.49]
    single      0.659 [0.521]    0.0169 [0.0447]   3.8e-4 [8.1e-4]   6.3e-3 [7.2e-3]     3.0e-5 [1.6e-3]
    zero_mask   0.172 [1.98]     0.0115 [0.0934]   1.4e-5 [4.1e-4]   0.042  [0.67]       4.6e-3 [4.2e-2]
    no_mask     0.271 [0.425]    0.0110 [0.0437]   1.1e-5 [3.0e-4]   0.010  [1.07]       1.8e-2 [0.12]
Pseudo-labels equal the reference's in every window and epoch; epoch-2 summed loss < epoch-1 in w256_e2.  See DESIGN.md section 9."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import dyneval_refs as D
from common_model import build_from_fixture
from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import lcasr_amd.hip.ops as o
    o._lib.load()
    return o


def _intervals(B, n, size, g, kind):
    if kind == 'zero' or n == 0:
        return torch.zeros(B, n, 2, dtype=torch.int32)
    s = torch.randint(0, max(size - 1, 1), (B, n), generator=g)
    w = torch.randint(0, max(size // 3, 2), (B, n), generator=g)
    iv = torch.stack([s, torch.clamp(s + w, max=size)], -1).to(torch.int32)
    if kind == 'edges' and n >= 2:
        iv[:, 0] = torch.tensor([0, min(3, size)]); iv[:, 1] = torch.tensor([max(size - 2, 0), size])      # both ends of the axis
    if kind == 'touching' and n >= 2:
        iv[:, 1, 0] = iv[:, 0, 1]; iv[:, 1, 1] = torch.clamp(iv[:, 1, 0] + 5, max=size)                     # [a, b) then [b, b + 5)
    if kind == 'overlap' and n >= 2:
        iv[:, 1, 0] = torch.clamp(iv[:, 0, 0] + 1, max=size); iv[:, 1, 1] = torch.clamp(iv[:, 0, 1] + 4, max=size)
    return iv


@pytest.mark.parametrize('kind', ['random', 'zero', 'edges', 'touching', 'overlap'])
@pytest.mark.parametrize('broadcast', [False, True])
@pytest.mark.parametrize('B,F,T', [(3, 80, 256), (3, 80, 1001), (1, 80, 7), (2, 81, 4099)])
def test_spec_mask_equals_masked_fill(ops, B, F, T, broadcast, kind):
    g = torch.Generator().manual_seed(B * 7 + T)
    src = torch.randn(1 if broadcast else B, F, T, generator=g).cuda()
    t_iv, f_iv = _intervals(B, 2, T, g, kind).cuda(), _intervals(B, 3, F, g, kind).cuda()
    t_iv[-1] = 0; f_iv[-1] = 0                                   # the clean copy: a plain copy of the source
    mv = torch.tensor(0.12345, device='cuda')
    out = ops.spec_mask(src, t_iv, f_iv, mv, batch=B if broadcast else None)
    ref = D.spec_mask(src, t_iv, f_iv, mv, batch=B if broadcast else None)
    assert out.shape == (B, F, T) and torch.equal(out, ref)
    assert torch.equal(out[-1], src[0 if broadcast else -1])
    if kind != 'zero' and T > 7: assert int((out != src.expand(B, F, T)).sum()) > 0
    none = ops.spec_mask(src, t_iv[:, :0].contiguous(), f_iv[:, :0].contiguous(), mv, batch=B if broadcast else None)
    assert torch.equal(none, src.expand(B, F, T))


def test_spec_mask_over_2pow31_elements(ops):
    """B*F*T > 2^31 with a broadcast source: 64-bit offsets.  Rows are checked one at a time against the reference."""
    B, F, T = 75, 80, 360000
    assert B * F * T > 2 ** 31
    g = torch.Generator().manual_seed(3)
    src = torch.randn(1, F, T, generator=g).cuda()
    t_iv = _intervals(B, 2, T, g, 'random').cuda(); f_iv = _intervals(B, 3, F, g, 'random').cuda()
    mv = torch.tensor(-2.5, device='cuda')
    out = ops.spec_mask(src, t_iv, f_iv, mv, batch=B)
    for b in (0, 37, 44, 45, 74):                                # 45 * F * T is the first row past 2^31 elements
        assert torch.equal(out[b:b + 1], D.spec_mask(src, t_iv[b:b + 1], f_iv[b:b + 1], mv)), b


@pytest.mark.parametrize('shape', [(3, 80, 1001), (1, 80, 7), (2, 80, 16384), (10_000_000,), (4, 3, 5, 33)])
def test_mean_f32(ops, shape):
    g = torch.Generator().manual_seed(len(shape) + shape[-1])
    x = (torch.randn(*shape, generator=g) + 0.3).cuda()
    a, b = ops.mean_f32(x), ops.mean_f32(x)
    assert a.shape == () and a.dtype == torch.float32 and a.is_cuda
    assert torch.equal(a, b), 'not bit-identical from call to call'
    ref = float(x.double().mean())
    assert abs(float(a) - ref) <= 1e-6 * abs(ref), (float(a), ref)
    tail = x.reshape(-1)[1:]                                     # 4-byte aligned only
    ref = float(tail.double().mean())
    assert abs(float(ops.mean_f32(tail)) - ref) <= 1e-6 * abs(ref)
    if len(shape) >= 2:
        T = shape[-1]
        lengths = torch.tensor([max(1, T - 3 * i * max(T // 10, 1)) for i in range(shape[0])], dtype=torch.int32).clamp(1, T).cuda()
        a, b = ops.mean_f32(x, lengths), ops.mean_f32(x, lengths)
        ref = float(D.mean_f32(x, lengths).double())
        assert torch.equal(a, b) and abs(float(a) - ref) <= 1e-6 * abs(ref) + 1e-9, (float(a), ref)


def _collapse_case(ops, x, lengths, blank):
    tg, tl = ops.ctc_collapse(x, lengths, blank)
    B, N, _ = x.shape
    assert tg.shape == (B, N) and tg.dtype == torch.int32 and tl.dtype == torch.int32
    xc = x.cpu()
    for b in range(B):
        n = N if lengths is None else int(lengths[b])
        ids = D.greedy_ids(xc[b, :n], blank)
        assert int(tl[b]) == len(ids), (b, int(tl[b]), len(ids))
        assert tg[b, :len(ids)].tolist() == ids, b
        assert int(tg[b, len(ids):].abs().sum()) == 0, 'padding must be zero'
    return tg, tl


def test_ctc_collapse_equals_the_greedy_decoder(ops):
    from lcasr_amd.decoding.greedy import GreedyCTCDecoder
    fx = load_golden('infer_tiny')
    for k in sorted(f for f in fx.files if f.startswith('logits.')):
        x = torch.from_numpy(fx[k].copy()).cuda()
        tg, tl = _collapse_case(ops, x[None], None, 127)
        want = GreedyCTCDecoder(tokenizer=None, blank_id=127)(x, decode=False)
        assert tg[0, :int(tl[0])].tolist() == want == fx['greedy.' + k.split('.')[1]].tolist()
    # random (4, 2048, 4096): runs of repeated labels, blanks, exact ties (first index wins), ragged lengths
    g = torch.Generator().manual_seed(17)
    B, N, Cc, blank = 4, 2048, 4096, 4095
    lab = torch.randint(0, 6, (B, N), generator=g)
    lab = torch.where(torch.rand(B, N, generator=g) < 0.3, torch.full_like(lab, blank), lab * 700)
    x = torch.randn(B, N, Cc, generator=g)
    x.scatter_add_(2, lab[..., None], torch.full((B, N, 1), 12.0))
    x[1, 100:110] = 0.0                                            # all classes tie: index 0
    x[2, 500:520, 7] = 50.0; x[2, 500:520, 9] = 50.0               # two-way tie: the lower index
    lengths = torch.tensor([2048, 1999, 65, 0], dtype=torch.int32)
    _collapse_case(ops, x.cuda(), lengths.cuda(), blank)
    _collapse_case(ops, x.cuda(), None, blank)
    # all blank / all one token
    allb = torch.full((1, 300, 128), -5.0); allb[..., 127] = 0.0
    tg, tl = _collapse_case(ops, allb.cuda(), None, 127)
    assert int(tl[0]) == 0
    one = torch.full((1, 300, 128), -5.0); one[..., 42] = 0.0
    tg, tl = _collapse_case(ops, one.cuda(), None, 127)
    assert int(tl[0]) == 1 and int(tg[0, 0]) == 42


def test_ctc_collapse_too_small_a_buffer_is_reported_not_overrun(ops):
    B, N, Cc, S_cap, guard = 2, 256, 128, 10, 64
    x = torch.full((B, N, Cc), -5.0)
    x[0, torch.arange(N), torch.arange(N) % 100] = 0.0             # 256 distinct neighbours: 256 labels
    x[1, :, 3] = 0.0                                               # one label: fits
    x = x.cuda()
    buf = torch.full((B * S_cap + guard,), -77, dtype=torch.int32, device='cuda')
    idx = torch.empty(B * N, dtype=torch.int32, device='cuda'); tl = torch.empty(B, dtype=torch.int32, device='cuda')
    vp = lambda t: C.c_void_p(t.data_ptr())
    ops._lib.call('sconf_ctc_collapse', vp(x), B, N, Cc, None, 127, vp(idx), vp(buf), S_cap, vp(tl), ops._stream())
    assert tl.tolist() == [-1, 1]
    assert bool((buf[B * S_cap:] == -77).all()), 'wrote past the targets buffer'
    assert buf[:S_cap].tolist() == list(range(10)) and buf[S_cap:2 * S_cap].tolist() == [3] + [0] * 9
    assert idx[:N].tolist() == [i % 100 for i in range(N)]


@pytest.mark.parametrize('retokenize', [True, False])
@pytest.mark.parametrize('name', D.CASES)
def test_dynamic_eval_matches_the_reference_run(ops, monkeypatch, name, retokenize):
    fx = load_golden('dyneval_cases')
    model = D.fixture_model('cuda')
    rec = D.run_case(fx, name, model, monkeypatch, retokenize)
    D.compare(fx, name, rec)


def test_restore_after_an_exception_in_the_third_window(ops, monkeypatch):
    fx = load_golden('dyneval_cases')
    model = D.fixture_model('cuda')
    with pytest.raises(RuntimeError, match='injected failure'):
        D.run_case(fx, 'w256', model, monkeypatch, False, fail_at=2)


def test_all_blank_window_on_the_hip_path(ops, monkeypatch):
    import lcasr_amd.functional as Fn
    from lcasr_amd.eval.dynamic_eval import dynamic_eval
    model = D.fixture_model('cuda')
    with torch.no_grad():
        model.decoder.ff.bias[-1] += 50.0
    seen, real = [], Fn.ctc_nll

    def rec(lp, tg, il, tl, blank):
        out = real(lp, tg, il, tl, blank)
        seen.append((int(tl.max()), float(out.detach().sum()), float(-lp.detach()[..., blank].double().sum())))
        return out

    monkeypatch.setattr(Fn, 'ctc_nll', rec)
    for retok in (True, False):
        out = dynamic_eval(D.Args(), model, D.fixture_spec()[:, :, :256].cuda(), 256, 0, D.Tok(127), use_tqdm=False, retokenize=retok)
        assert out.shape == (32, 128) and np.isfinite(out).all()
    for S, nll, want in seen:
        assert S == 0 and abs(nll - want) <= 1e-4 * max(1.0, abs(want)), (S, nll, want)


def test_a_trainer_goes_on_training_after_dynamic_eval(ops):
    """A Trainer built BEFORE dynamic_eval takes the same next step as an identical one that never saw the call: the model's
    parameters are back in the Trainer's flat buffer, bit for bit, BatchRenorm statistics included (train mode)."""
    from lcasr_amd.eval.dynamic_eval import dynamic_eval
    from lcasr_amd.train import Trainer
    fx = load_golden('tiny_ln_ragged')
    x, ln = torch.from_numpy(fx['x']).cuda(), torch.from_numpy(fx['lengths']).cuda()
    tg, tl = torch.from_numpy(fx['targets']).cuda(), torch.from_numpy(fx['target_lengths']).cuda()
    losses, finals = [], []
    for adapt in (False, True):
        m = build_from_fixture(fx, 'cuda')
        tr = Trainer(m, lr=1e-3)
        first = float(tr.step(x, ln, tg, tl))
        if adapt:
            flat = tr.opt.flat[0].data.clone()
            out = dynamic_eval(D.Args(), m, D.fixture_spec().cuda(), 256, 64, D.Tok(127), use_tqdm=False, retokenize=False)
            assert np.isfinite(out).all() and torch.equal(flat, tr.opt.flat[0].data)
            fp = tr.opt.flat[0]
            assert all(p.data_ptr() == fp.data.data_ptr() + 4 * o and p.grad.data_ptr() == fp.grad.data_ptr() + 4 * o
                       for p, o in zip(fp.params, fp.offsets))
        losses.append((first, float(tr.step(x, ln, tg, tl)), float(tr.step(x, ln, tg, tl))))
        finals.append(tr.opt.flat[0].data.clone())
    assert losses[0] == losses[1], losses
    assert losses[0][2] != losses[0][1], 'the steps must move the model for this test to mean anything'
    assert torch.equal(finals[0], finals[1])


def test_benchmark_like_run_for_the_record(ops):
    """Config 3 (6L/768D/6H, vocabulary 4095) from seed, a 131072-frame recording in 16384-frame windows with 2048 overlap,
    retokenize=False: finite output, parameters restored.  The wall times are printed for DESIGN.md; no threshold - there is no
    parent-commit number to hold them against."""
    from lcasr_amd.eval.dynamic_eval import dynamic_eval
    from lcasr_amd.eval.utils import fetch_logits
    from lcasr_amd.models.sconformer_xl import SCConformerXL
    torch.manual_seed(0)
    model = SCConformerXL(vocab_size=4095, n_layers=6, d_model=768, n_heads=6, head_dim=128, subsampling_conv_channels=256, use_rotary=True,
                          rotary_base_freq=1500000, decoder_norm=True, self_conditioning=True, default_norm='layer_norm', bias_in_ff=False).cuda().eval()
    spec = torch.randn(1, 80, 131072, generator=torch.Generator().manual_seed(1)).cuda()
    before = [p.detach().clone() for p in model.parameters()]
    tok = D.Tok(4095)
    times = {}
    for what in ('dynamic_eval', 'dynamic_eval (2nd call)', 'fetch_logits', 'fetch_logits (2nd call)'):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        if what.startswith('dynamic'):
            out = dynamic_eval(D.Args(), model, spec, 16384, 2048, tok, use_tqdm=False, retokenize=False, return_numpy=False)
        else:
            ref = fetch_logits(D.Args(), model, spec, 16384, 2048, tok, use_tqdm=False, return_numpy=False)
        torch.cuda.synchronize(); times[what] = time.perf_counter() - t0
    print('[dynamic_eval record] 131072 frames, 16384/2048 windows, config 3: ' + ', '.join(f'{k} {v * 1e3:.1f} ms' for k, v in times.items()))
    assert out.shape == ref.shape and bool(torch.isfinite(out).all())
    assert all(torch.equal(p, q) for p, q in zip(model.parameters(), before))
