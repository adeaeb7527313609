"""CPU tests of SpecAugment, the dynamic-evaluation loop and Trainer(spec_augment=): host logic on the emulated op layer
(tests/kernel_refs.py + the references of the three new ops in tests/dyneval_refs.py), against the reference's own run
recorded in tests/golden/dyneval_cases.npz (tools/make_dynamic_eval_golden.py).

Bounds: see tests/dyneval_refs.py - labels and restored state exact, numbers within 2x the reference's own fp32-vs-autocast
noise on the same case.  Measured on the emulated path (it rounds like the HIP path), largest figure over the five cases against the bound of that case:
log-prob max 0.463 (single window; bound 2 x 0.521), per-step loss rel 8.9e-3 (single window; bound 2 x 7.2e-3), parameter-change
norm rel 4.5e-2 (no masks; bound 2 x 0.116).  See DESIGN.md section 9."""
import numpy as np
import pytest
import torch

import dyneval_refs as D
from common_model import build_from_fixture
from conftest import load_golden


@pytest.fixture
def emu(emulated_ops, monkeypatch):
    import lcasr_amd.optim as OPT
    D.attach(monkeypatch, emulated_ops)
    monkeypatch.setattr(OPT, 'ops', emulated_ops)
    return emulated_ops


def _law_ok(iv, size, mp):
    s, e = iv[..., 0], iv[..., 1]
    assert iv.dtype == torch.int32
    assert bool((s >= 0).all()) and bool((e <= size).all()) and bool((e >= s).all()), 'interval outside the axis'
    assert int((e - s).max()) <= mp, f'mask wider than {mp}'


@pytest.mark.parametrize('F,T', [(80, 256), (80, 1000), (80, 17)])
def test_draw_obeys_the_interval_law(F, T):
    from lcasr_amd.utils.augmentation import SpecAugment
    g = torch.Generator().manual_seed(F * 1000 + T)
    # the dynamic-evaluation default: time width from min_p
    aug = SpecAugment(n_time_masks=2, n_freq_masks=3, freq_mask_param=42, min_p=0.05)
    width = int(int(T * 0.05) / 2)
    assert aug.time_mask_width(T) == width
    seen_t, seen_f = 0, 0
    for _ in range(200):
        t_iv, f_iv = aug.draw((4, F, T), generator=g)
        assert t_iv.shape == (4, 2, 2) and f_iv.shape == (4, 3, 2)
        _law_ok(f_iv, F, 42)
        if width < 1:
            assert int(t_iv.abs().sum()) == 0                      # mask_param' < 1: nothing is masked
        else:
            _law_ok(t_iv, T, width)
        seen_t = max(seen_t, int((t_iv[..., 1] - t_iv[..., 0]).max())); seen_f = max(seen_f, int((f_iv[..., 1] - f_iv[..., 0]).max()))
    assert seen_f > 42 // 2 and (width < 2 or seen_t >= width // 2), 'the draws never come near the allowed width'
    assert len({tuple(r) for r in f_iv[:, 0].tolist()}) > 1, 'iid masks: the examples must differ'
    # max_p < 1 caps the width at int(size * p)
    capped = SpecAugment(n_time_masks=1, n_freq_masks=1, freq_mask_param=42, time_mask_param=100, max_p=0.1)
    for _ in range(100):
        t_iv, f_iv = capped.draw((3, F, T), generator=g)
        if int(T * 0.1) < 1: assert int(t_iv.abs().sum()) == 0
        else: _law_ok(t_iv, T, min(100, int(T * 0.1)))
        _law_ok(f_iv, F, min(42, int(F * 0.1)))
    # shared masks: iid_masks=False, or no batch axis
    shared = SpecAugment(n_time_masks=1, n_freq_masks=2, freq_mask_param=30, time_mask_param=10, iid_masks=False)
    t_iv, f_iv = shared.draw((5, F, T), generator=g)
    assert t_iv.shape == (5, 1, 2) and bool((t_iv == t_iv[:1]).all()) and bool((f_iv == f_iv[:1]).all())
    t_iv, f_iv = aug.draw((F, T), generator=g)
    assert t_iv.shape == (1, 2, 2) and f_iv.shape == (1, 3, 2)
    none = SpecAugment(n_time_masks=0, n_freq_masks=0, freq_mask_param=42)
    t_iv, f_iv = none.draw((2, F, T), generator=g)
    assert t_iv.shape == (2, 0, 2) and f_iv.shape == (2, 0, 2)


def test_constructor_asserts_like_the_reference():
    from lcasr_amd.utils.augmentation import SpecAugment
    with pytest.raises(AssertionError): SpecAugment(n_time_masks=2, n_freq_masks=0, freq_mask_param=1)
    with pytest.raises(AssertionError): SpecAugment(n_time_masks=0, n_freq_masks=0, freq_mask_param=1, min_p=1.5)
    with pytest.raises(AssertionError): SpecAugment(n_time_masks=0, n_freq_masks=0, freq_mask_param=1, max_p=-0.1)
    SpecAugment(n_time_masks=0, n_freq_masks=1, freq_mask_param=1, unknown_key=3)


def test_forward_is_the_masked_fill_sequence(emu):
    from lcasr_amd.utils.augmentation import SpecAugment
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 80, 200, generator=g) + 0.7
    lengths = torch.tensor([200, 150, 33])
    aug = SpecAugment(n_time_masks=2, n_freq_masks=3, freq_mask_param=42, min_p=0.2)
    for ln in (None, lengths):
        drawn = {}
        real = aug.draw
        aug.draw = lambda *a, **k: drawn.setdefault('iv', real(*a, **k))
        y = aug(x, ln, generator=torch.Generator().manual_seed(9))
        aug.draw = real
        t_iv, f_iv = drawn['iv']
        if ln is None: mean = x.double().mean()
        else: mean = torch.cat([x[b, :, :int(ln[b])].reshape(-1) for b in range(3)]).double().mean()
        ref = x.clone()
        for j in range(2):
            for b in range(3): ref[b, :, int(t_iv[b, j, 0]):int(t_iv[b, j, 1])] = float(mean)
        for j in range(3):
            for b in range(3): ref[b, int(f_iv[b, j, 0]):int(f_iv[b, j, 1]), :] = float(mean)
        assert y.shape == x.shape and int((y != x).sum()) > 0
        assert float((y - ref).abs().max()) < 1e-6
    z = SpecAugment(n_time_masks=1, n_freq_masks=1, freq_mask_param=20, time_mask_param=30, zero_masking=True)
    y = z(x, generator=torch.Generator().manual_seed(1))
    changed = y != x
    assert int(changed.sum()) > 0 and bool((y[changed] == 0).all())


@pytest.mark.parametrize('retokenize', [True, False])
@pytest.mark.parametrize('name', D.CASES)
def test_dynamic_eval_matches_the_reference_run(emu, monkeypatch, name, retokenize):
    fx = load_golden('dyneval_cases')
    model = D.fixture_model()
    rec = D.run_case(fx, name, model, monkeypatch, retokenize)
    D.compare(fx, name, rec)


def test_restore_after_an_exception_in_the_third_window(emu, monkeypatch):
    fx = load_golden('dyneval_cases')
    model = D.fixture_model()
    with pytest.raises(RuntimeError, match='injected failure'):
        D.run_case(fx, 'w256', model, monkeypatch, True, fail_at=2)          # run_case checks the restore in its `finally`


def test_signature_mirrors_the_reference():
    import inspect
    from lcasr_amd.eval.dynamic_eval import dynamic_eval, dynamic_eval_ctc_loss
    assert dynamic_eval is dynamic_eval_ctc_loss
    ps = inspect.signature(dynamic_eval).parameters
    assert list(ps)[:11] == ['args', 'model', 'spec', 'seq_len', 'overlap', 'tokenizer', 'use_tqdm', 'optim', 'num_negatives', 'lr_args', 'spec_augment_config']
    assert list(ps)[11:] == ['augmentation', 'retokenize', 'return_numpy']
    assert ps['num_negatives'].default == 2 and ps['lr_args'].default == {'lr': 8e-5} and ps['use_tqdm'].default is True
    assert ps['spec_augment_config'].default == {'n_time_masks': 2, 'n_freq_masks': 3, 'freq_mask_param': 42, 'time_mask_param': -1,
                                                 'min_p': 0.05, 'zero_masking': False}


def test_all_blank_window_gives_minus_sum_log_p_blank(emu, monkeypatch):
    """S = 0: the loss of a window whose clean copy decodes to nothing is -sum log p(blank) over the augmented rows / (N * rows),
    as torch gives for an empty target - on both label paths."""
    import lcasr_amd.functional as Fn
    from lcasr_amd.eval.dynamic_eval import dynamic_eval
    model = D.fixture_model()
    with torch.no_grad():
        model.decoder.ff.bias[-1] += 50.0                          # blank wins every frame
    spec = D.fixture_spec()[:, :, :256]
    seen = []
    real = Fn.ctc_nll

    def rec(lp, tg, il, tl, blank):
        out = real(lp, tg, il, tl, blank)
        seen.append((int(tl.max()), float(out.detach().sum()), float(-lp.detach()[..., blank].double().sum())))
        return out

    monkeypatch.setattr(Fn, 'ctc_nll', rec)
    for retok in (True, False):
        out = dynamic_eval(D.Args(), model, spec, 256, 0, D.Tok(127), use_tqdm=False, retokenize=retok)
        assert out.shape == (32, 128) and np.isfinite(out).all()
    assert len(seen) == 2
    for S, nll, want in seen:
        assert S == 0 and abs(nll - want) <= 1e-4 * max(1.0, abs(want))


def test_trainer_spec_augment(emu, monkeypatch):
    """spec_augment=None is today's step bit for bit; with a module the model is fed the masked batch."""
    from lcasr_amd.train import Trainer
    fx = load_golden('tiny_ln_ragged')
    x, ln = torch.from_numpy(fx['x']), torch.from_numpy(fx['lengths'])
    tg, tl = torch.from_numpy(fx['targets']), torch.from_numpy(fx['target_lengths'])

    def two_steps(**kw):
        m = build_from_fixture(fx)
        tr = Trainer(m, **kw)
        for _ in range(2): tr.step(x, ln, tg, tl)
        return [p.detach().clone() for p in m.parameters()]

    a, b = two_steps(fused_loss=False), two_steps(fused_loss=False, spec_augment=None)
    assert all(torch.equal(p, q) for p, q in zip(a, b))

    class Marker(torch.nn.Module):
        def forward(self, audio, lengths):
            assert lengths is ln
            return audio * 0 + 3.0

    m = build_from_fixture(fx)
    fed = []
    m.register_forward_pre_hook(lambda _m, args: fed.append(args[0].clone()))
    Trainer(m, fused_loss=False, spec_augment=Marker()).step(x, ln, tg, tl)
    assert len(fed) == 1 and bool((fed[0] == 3.0).all())
