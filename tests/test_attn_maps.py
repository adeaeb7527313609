"""CPU tests of the attention-map collectors (components/attention.py): CollectAttentionProbs and CollectAttentionOffsets on the
lcasr_amd model with emulated ops against what the reference itself produced (tests/golden/attn_maps_tiny.npz, written by
tools/make_attn_maps_golden.py), the observed path's output equality and refusals, the two host helpers, and the host side of the
new C ABI entry points.  The op layer is tests/attn_maps_refs.py::Ops (the two new references, kernel_refs for the rest).

Yardstick: the fixture stores the reference's own fp32-versus-bf16-autocast difference of every quantity; each figure here must
stay within twice that."""
import ctypes
import os

import pytest
import torch

import attn_maps_refs as R
from common_model import build_from_fixture
from conftest import load_golden


@pytest.fixture
def maps_ops(emulated_ops, monkeypatch):
    import lcasr_amd.functional as Fn
    ops = R.Ops()
    monkeypatch.setattr(Fn, 'ops', ops)
    return ops


def _tiny():
    fx, gold = load_golden('infer_tiny'), load_golden('attn_maps_tiny')
    m = build_from_fixture(fx).eval()
    spec = torch.from_numpy(fx['spec'].copy())[:, :, :int(gold['frames'])]
    return m, spec, gold


def _attn(m):
    return [l.attend.fn for l in m.layers]


def test_collect_attention_probs_against_the_reference(maps_ops, tmp_path):
    """On the parent the flag was stored and never read: the same collector returned nothing.  Here it returns the reference's
    (L,B,H,N,N) bf16 stack of scaled pre-softmax scores and writes the reference's file names."""
    from lcasr_amd.components.attention import CollectAttentionProbs
    m, spec, gold = _tiny()
    f32 = []
    hooks = [a.return_attention_module.register_forward_hook(lambda _m, _i, out: f32.append(out[1].float().cpu())) for a in _attn(m)]
    col = CollectAttentionProbs(_attn(m), save_path=str(tmp_path), save_prefix='run')
    assert all(a.return_attention_weights for a in _attn(m))
    with torch.no_grad():
        m(spec)
    assert len(col.collect()) == 2
    got = col()
    assert col.collect() == []
    want = torch.from_numpy(gold['scores'])
    assert tuple(got.shape) == tuple(gold['collector_shape'].tolist()) == (2, 1, 2, 125, 125)
    assert got.dtype == torch.bfloat16 and got.device.type == 'cpu'
    for name, s in (('bf16 collector', got.float()), ('f32 hook', torch.stack(f32, 0))):
        d = (s - want).abs()
        print(f'[{name}] scores max|d| {float(d.max()):.5f} (yard {float(gold["yard.scores_max"]):.5f}) '
              f'mean|d| {float(d.mean()):.6f} (yard {float(gold["yard.scores_mean"]):.6f})')
        assert float(d.max()) <= 2 * float(gold['yard.scores_max'])
        assert float(d.mean()) <= 2 * float(gold['yard.scores_mean'])
    assert sorted(os.listdir(tmp_path)) == ['run_0.pt', 'run_1.pt']
    assert torch.equal(torch.load(tmp_path / 'run_1.pt'), got[1])
    for h in hooks: h.remove()
    # discard=True keeps nothing; without a prefix the files are layer_{idx}.pt
    col.remove()
    d2 = tmp_path / 'plain'; d2.mkdir()
    col2 = CollectAttentionProbs(_attn(m), discard=True, save_path=str(d2))
    with torch.no_grad():
        m(spec)
    assert col2.collect() == [] and sorted(os.listdir(d2)) == ['layer_0.pt', 'layer_1.pt']


def test_collect_attention_offsets_against_the_reference(maps_ops):
    from lcasr_amd.components.attention import CollectAttentionOffsets, mass_within, mean_abs_offset
    m, spec, gold = _tiny()
    col = CollectAttentionOffsets(_attn(m))
    with torch.no_grad():
        m(spec)
    prof, live = col()
    want = torch.from_numpy(gold['profile'])
    assert tuple(prof.shape) == (2, 1, 2, 249) and prof.dtype == torch.float32 and live.tolist() == [125]
    d = (prof - want).abs()
    print(f'profile max|d| {float(d.max()):.5f} (yard {float(gold["yard.profile_max"]):.5f})')
    assert float(d.max()) <= 2 * float(gold['yard.profile_max'])
    assert float((prof.sum(-1) - 125).abs().max()) < 1e-3
    # the helpers on the model's profile: everything lies within N - 1, and a mean offset exists for every (layer, b, head)
    assert torch.allclose(mass_within(prof, live, 124), torch.ones(2, 1, 2), atol=1e-5)
    assert mean_abs_offset(prof, live).shape == (2, 1, 2) and float(mean_abs_offset(prof, live).min()) > 0
    with pytest.raises(RuntimeError, match='nothing collected'):
        col()


def test_observed_path_output_equals_the_plain_path(maps_ops):
    from lcasr_amd.components.attention import CollectAttentionOffsets, CollectAttentionProbs
    m, spec, _ = _tiny()
    ragged = torch.cat([spec, spec.flip(-1)], 0), torch.tensor([1000, 800])
    with torch.no_grad():
        plain = m(spec)['final_posteriors'].clone()
        plain_r = m(ragged[0], length=ragged[1])['final_posteriors'].clone()
    a, b = CollectAttentionProbs(_attn(m)), CollectAttentionOffsets(_attn(m))
    with torch.no_grad():
        seen = m(spec)['final_posteriors']
        assert torch.equal(seen, plain)
        a.clear(); b.clear()
        seen_r = m(ragged[0], length=ragged[1])['final_posteriors']
    assert torch.equal(seen_r, plain_r)
    # the ragged batch: padded rows and columns are -inf / contribute nothing
    s, (prof, live) = a().float(), b()
    assert live.tolist() == [125, 100] and tuple(s.shape) == (2, 2, 2, 125, 125)
    assert torch.isinf(s[:, 1, :, 100:, :]).all() and torch.isinf(s[:, 1, :, :, 100:]).all() and torch.isfinite(s[:, 1, :, :100, :100]).all()
    assert torch.isfinite(s[:, 0]).all()
    assert float((prof.sum(-1) - live[None, :, None]).abs().max()) < 1e-3
    assert float(prof[:, 1, :, :24].abs().max()) == 0 and float(prof[:, 1, :, -24:].abs().max()) == 0      # |delta| >= 101 has no live pair
    a.remove(); b.remove()
    assert not any(x.return_attention_weights or x.return_attention_offsets for x in _attn(m))
    with torch.no_grad():
        assert torch.equal(m(spec)['final_posteriors'], plain)


def test_flags_respect_the_current_window(maps_ops):
    from lcasr_amd.components.attention import CollectAttentionOffsets, CollectAttentionProbs
    m, spec, _ = _tiny()
    for x in _attn(m): x.left_window, x.right_window = 8, 3
    a, b = CollectAttentionProbs(_attn(m)), CollectAttentionOffsets(_attn(m))
    with torch.no_grad():
        m(spec)
    s, (prof, live) = a().float(), b()
    i, j = torch.arange(125)[:, None], torch.arange(125)[None, :]
    inside = (j >= i - 8) & (j <= i + 3)
    assert torch.isfinite(s[..., inside]).all() and torch.isinf(s[..., ~inside]).all()
    assert float(prof[..., :124 - 8].abs().max()) == 0 and float(prof[..., 124 + 4:].abs().max()) == 0
    assert float((prof.sum(-1) - 125).abs().max()) < 1e-3


@pytest.mark.parametrize('flag', ['return_attention_weights', 'return_attention_offsets'])
def test_observed_path_refuses_grad_and_training(maps_ops, flag):
    m, spec, _ = _tiny()
    setattr(m.layers[0].attend.fn, flag, True)
    with pytest.raises(RuntimeError, match=flag):
        m(spec)                                                    # eval mode, grad enabled
    m.train()
    with torch.no_grad(), pytest.raises(RuntimeError, match=flag):
        m(spec)                                                    # no grad, training mode
    m.eval()
    with torch.no_grad():
        m(spec)


def test_helpers_on_a_hand_made_profile():
    from lcasr_amd.components.attention import mass_within, mean_abs_offset
    # N = 4: offsets -3 .. 3.  Batch of 2 with 4 and 2 live rows, one head.
    prof = torch.tensor([[[0.0, 0.5, 0.5, 2.0, 1.0, 0.0, 0.0]], [[0.0, 0.0, 0.25, 1.5, 0.25, 0.0, 0.0]]])
    live = torch.tensor([4, 2])
    assert mass_within(prof, live, 0).tolist() == [[0.5], [0.75]]
    assert mass_within(prof, live, 1).tolist() == [[0.875], [1.0]]
    assert mass_within(prof, live, 3).tolist() == [[1.0], [1.0]]
    assert mean_abs_offset(prof, live).tolist() == [[(0.5 * 2 + 0.5 + 1.0) / 4], [0.25]]
    stacked = torch.stack([prof, prof], 0)                         # a leading layer axis
    assert mass_within(stacked, live, 1).shape == (2, 2, 1) and mean_abs_offset(stacked, live)[1].tolist() == [[0.625], [0.25]]


def test_references_agree_with_the_forward_reference():
    """attn_maps_refs against kernel_refs.attn_fwd: softmax of the scores reproduces its lse, the profile sums to the live rows,
    and the banded reference equals the dense one."""
    import kernel_refs
    g = torch.Generator().manual_seed(5)
    B, N, H, D = 2, 37, 2, 32
    q, k, v = (torch.randn(B, N, H, D, generator=g).bfloat16() for _ in range(3))
    lengths = torch.tensor([37, 20], dtype=torch.int32)
    for window in ((-1, -1), (5, 2)):
        _, lse = kernel_refs.attn_fwd(q, k, v, lengths, window)
        s = R.scores_f64(q, k, lengths, window)
        live = torch.arange(N)[None, :] < lengths[:, None]
        assert torch.isinf(s[~live[:, None, :].expand(B, H, N)]).all()
        assert torch.allclose(torch.logsumexp(s, -1)[live[:, None, :].expand(B, H, N)], lse.double()[live[:, None, :].expand(B, H, N)], atol=1e-5)
        prof = R.attn_offset_profile(q, k, lse, lengths, window)
        assert prof.shape == (B, H, 2 * N - 1) and torch.allclose(prof.sum(-1), lengths.float()[:, None].expand(B, H), atol=1e-4)
    _, lse = kernel_refs.attn_fwd(q[:1], k[:1], v[:1], None, (5, 2))
    dense = R.profile_f64(q[:1], k[:1], lse, None, (5, 2))[0]
    assert torch.allclose(R.banded_profile_f64(q[:1], k[:1], (5, 2), lse), dense, atol=1e-12)
    exact = R.exact_profile_f64(q[:1], k[:1], None, (5, 2))[0]
    assert torch.allclose(R.banded_profile_f64(q[:1], k[:1], (5, 2)), exact, atol=1e-12) and torch.allclose(exact, dense, atol=1e-4)


def test_host_side_validation_of_the_new_entry_points():
    from lcasr_amd.hip import _lib
    lib = _lib.load()
    assert lib.sconf_version() == 220
    st = (ctypes.c_int64 * 3)(64, 64, 32)
    one = ctypes.c_void_p(16)
    assert lib.sconf_attn_scores(one, one, one, 0, None, 1, 8, 2, 48, st, st, -1, -1, 1.0, None) != 0 and b'head_dim' in lib.sconf_last_error()
    assert lib.sconf_attn_scores(None, one, one, 0, None, 1, 8, 2, 32, st, st, -1, -1, 1.0, None) != 0 and b'null' in lib.sconf_last_error()
    assert lib.sconf_attn_scores(one, one, None, 0, None, 1, 8, 2, 32, st, st, -1, -1, 1.0, None) != 0 and b'null out' in lib.sconf_last_error()
    assert lib.sconf_attn_scores(one, one, one, 2, None, 1, 8, 2, 32, st, st, -1, -1, 1.0, None) != 0 and b'out_dtype' in lib.sconf_last_error()
    bad = (ctypes.c_int64 * 3)(64, 60, 32)
    assert lib.sconf_attn_scores(one, one, one, 0, None, 1, 8, 2, 32, bad, st, -1, -1, 1.0, None) != 0 and b'multiples of 8' in lib.sconf_last_error()
    assert lib.sconf_attn_scores(ctypes.c_void_p(8), one, one, 0, None, 1, 8, 2, 32, st, st, -1, -1, 1.0, None) != 0 and b'aligned' in lib.sconf_last_error()
    # workspace: one 224-float row per (b, h, 512-row chunk, band of 224 offsets); bounded by the window when there is one
    ws = lib.sconf_attn_offset_profile_workspace
    assert ws(1, 125, 2, -1, -1) == 2 * 1 * 2 * 224 * 4                      # 249 offsets: 2 bands
    assert ws(2, 16384, 16, -1, -1) == 32 * 32 * 147 * 224 * 4               # 32767 offsets: 147 bands, 32 chunks
    assert ws(1, 70001, 1, 64, 64) == 137 * 1 * 224 * 4                      # 129 offsets: one band whatever N is
    assert ws(1, 140002, 1, 64, 64) == 274 * 1 * 224 * 4 and ws(0, 8, 1, -1, -1) == -1
    need = ws(1, 8, 2, -1, -1)
    rc = lib.sconf_attn_offset_profile(one, one, one, one, None, 1, 8, 2, 32, st, st, -1, -1, 1.0, one, need - 1, None)
    assert rc != 0 and b'workspace' in lib.sconf_last_error() and str(need).encode() in lib.sconf_last_error()
    assert lib.sconf_attn_offset_profile(one, one, None, one, None, 1, 8, 2, 32, st, st, -1, -1, 1.0, one, need, None) != 0
    assert b'null lse' in lib.sconf_last_error()
