"""CPU tests of the evaluation loop: the edit-count references against the brute-force definition, word_error_rate_detail,
the buffered fetch_logits against the reference's own output (buffered_tiny.npz), evaluate() in its three modes, and the host
side of the new C ABI entry points.  The HIP ops are replaced by tests/eval_refs.py (installed here, onto the emulated op layer)."""
import ctypes
import itertools
import math

import numpy as np
import pytest
import torch

import eval_refs as E
from common_model import build_from_fixture
from conftest import load_golden


@pytest.fixture
def eval_ops(emulated_ops, monkeypatch):
    E.attach(monkeypatch, emulated_ops)
    return emulated_ops


# ---- the references and the definition ---------------------------------------------------------------------------------------
def test_edit_references_agree_with_each_other_and_with_the_brute_force_definition():
    rng = np.random.default_rng(0)
    pairs = [([], []), ([1], []), ([], [2, 2]), ([0, 1], [1, 2])]
    for _ in range(300):
        a = int(rng.integers(2, 4))
        pairs.append(tuple(x.tolist() for x in E.random_pair(rng, int(rng.integers(0, 6)), int(rng.integers(0, 6)), a)))
    for h, r in pairs:
        best = E.brute_force_counts(h, r)
        assert len(best) == 1, (h, r, best)                        # the split of the definition is unique
        want = list(best[0])
        assert E._split(E.edit_key_loop(h, r), len(h), len(r)) == want, (h, r)
        assert E._split(E.edit_key_rows(h, r), len(h), len(r)) == want, (h, r)
    seqs = [E.random_pair(rng, int(rng.integers(0, 90)), int(rng.integers(0, 90)), a) for a in (2, 3, 5000) for _ in range(8)]
    seqs.append(E.planted_pair(rng, 200, 50, 17))
    h, ho = E.ragged([s[0] for s in seqs]); r, ro = E.ragged([s[1] for s in seqs])
    a, b = E.edit_counts_loop(h, ho, r, ro), E.edit_counts(h, ho, r, ro)
    assert a.dtype == torch.int64 and a.shape == (len(seqs), 4) and torch.equal(a, b)
    assert int(a[-1, 0]) <= 17 and (a[:, 0] == a[:, 1:].sum(1)).all()
    assert E.edit_counts(*E.ragged([]), *E.ragged([])).shape == (0, 4)


# ---- word_error_rate_detail -------------------------------------------------------------------------------------------------
def test_word_error_rate_detail_hand_made_cases(eval_ops):
    from lcasr_amd.eval.wer import word_error_rate_detail as wer
    assert wer(['the cat sat'], ['the cat sat']) == (0.0, 3, 0.0, 0.0, 0.0)
    assert wer(['a b c'], ['x y z']) == (1.0, 3, 0.0, 0.0, 1.0)                       # all different: three substitutions
    assert wer([''], ['x y z']) == (1.0, 3, 0.0, 1.0, 0.0)                            # empty hypothesis: three deletions
    assert wer(['a b'], ['']) == (float('inf'),) * 1 + (0,) + (float('inf'),) * 3     # no reference words at all
    assert wer(['a b', 'c'], ['', 'c d']) == (1.5, 2, 1.0, 0.5, 0.0)                  # empty reference: its hypothesis is insertions
    w = wer([''], [''])
    assert w[1] == 0 and all(math.isinf(v) for v in (w[0],) + w[2:])
    # "a b" against "b c": distance 2 either as two substitutions or as one deletion + one insertion; the contract takes the latter
    assert wer(['a b'], ['b c']) == (1.0, 2, 0.5, 0.5, 0.0)
    assert wer(['a b', 'the cat sat on mat'], ['b c', 'the cat sat on the mat']) == (3 / 8, 8, 1 / 8, 2 / 8, 0.0)
    assert wer(['  a   b\n'], ['a b']) == (0.0, 2, 0.0, 0.0, 0.0)                     # str.split() tokens
    with pytest.raises(ValueError, match='same number of elements'):
        wer(['a'], ['a', 'b'])
    assert wer([], []) [1] == 0


def test_word_error_rate_detail_characters(eval_ops):
    from lcasr_amd.eval.wer import word_error_rate_detail as wer
    assert wer(['abc'], ['abd'], use_cer=True) == (1 / 3, 3, 0.0, 0.0, 1 / 3)
    assert wer(['a c'], ['a bc'], use_cer=True) == (1 / 4, 4, 0.0, 1 / 4, 0.0)        # the inner space is a character
    e, words, i, d, s = wer([' ab '], ['ab '], use_cer=True)                          # ends stripped, words = len(list(r))
    assert (e, words, i, d, s) == (0.0, 3, 0.0, 0.0, 0.0)
    assert wer(['ab'], [''], use_cer=True)[1] == 0
    assert wer(['ab', 'x'], ['', 'xy'], use_cer=True) == (1.5, 2, 1.0, 0.5, 0.0)


def test_token_error_counts_on_emulated_ops(eval_ops):
    from lcasr_amd.eval.wer import token_error_counts
    g = torch.Generator().manual_seed(3)
    B, N, V = 3, 40, 8
    lp = torch.randn(B, N, V, generator=g).log_softmax(-1)
    lengths = torch.tensor([40, 25, 0], dtype=torch.int32)
    targets = torch.randint(0, V - 1, (B, 12), generator=g)
    tl = torch.tensor([12, 7, 3])
    got = token_error_counts(lp, lengths, targets, tl, blank=V - 1)
    import dyneval_refs
    for b in range(B):
        ids = dyneval_refs.greedy_ids(lp[b, :int(lengths[b])], V - 1)
        tg = targets[b, :int(tl[b])].tolist()
        assert got[b].tolist() == E._split(E.edit_key_loop(ids, tg), len(ids), len(tg))
    assert got[2].tolist() == [3, 0, 3, 0]


# ---- buffered fetch_logits ---------------------------------------------------------------------------------------------------
def test_buffer_plan_quirks():
    from lcasr_amd.eval.buffered_transcription import buffer_plan, buffer_spans
    assert buffer_plan(1000, 1000, 0) == [(0, 1000, 0, 1000)]
    p = buffer_plan(1000, 256, 64)
    assert p[0] == (0, 256, 0, 192) and p[1] == (160, 416, 192, 384)                  # clamped at the start, then centred
    assert p[-1] == (744, 1000, 960, 1000) and len(p) == 6                            # clamped at the end, last chunk cut
    assert all(b1 - b0 == 256 for b0, b1, _, _ in p)
    spans, total = buffer_spans(p, 32, 1000 // 4 + 256)
    assert spans[0] == (0, 24, 0) and spans[1] == (4, 24, 24) and total == sum(s[1] for s in spans)
    with pytest.raises(ValueError, match='buffer_plan'):
        buffer_plan(1000, 256, 256)
    with pytest.raises(ValueError, match='does not fit'):
        buffer_spans(p, 32, 40, 'buffer_plan(spec_n=1000, seq_len=256, overlap=64)')


def test_buffered_fetch_logits_placement_is_exactly_the_reference(eval_ops):
    """Part (b) of the fixture: the stub model's posteriors name (window start, row), so equality is exact."""
    from lcasr_amd.eval.buffered_transcription import fetch_logits
    fx = load_golden('buffered_tiny')
    cases = fx['place.cases'].tolist()
    assert len(cases) >= 100
    stub = E.StubModel()
    for ci, (spec_n, sl, ov) in enumerate(cases):
        for mb in (16, 3):
            got = fetch_logits(E.Args, stub, E.stub_spec(spec_n), sl, ov, E.StubTok(), use_tqdm=False, max_batch=mb)
            want = fx[f'place.rows.{ci}']
            assert got.shape == (len(want), 4) and got.dtype == np.float32, (spec_n, sl, ov)
            assert np.array_equal(got, np.repeat(want[:, None], 4, 1).astype(np.float32)), (spec_n, sl, ov, mb)


def _tiny():
    fx = load_golden('infer_tiny')

    class Tok:
        def vocab_size(self): return int(fx['cfg.vocab_size'])

    return fx, Tok(), torch.from_numpy(fx['spec'].copy())


def test_buffered_fetch_logits_tiny_model_against_the_reference(eval_ops):
    """Part (a): bounds of test_fetch_logits_and_greedy_decode_against_reference_fixture, max < 0.3 and mean < 0.03."""
    from lcasr_amd.eval.buffered_transcription import fetch_logits
    fx, tok, spec = _tiny()
    bx = load_golden('buffered_tiny')
    m = build_from_fixture(fx).eval()
    assert len(bx['tiny.cases']) == 10
    for ci, (sl, ov) in enumerate(bx['tiny.cases'].tolist()):
        got = fetch_logits(E.Args, m, spec, sl, ov, tok, use_tqdm=False, max_batch=3)
        ref = bx[f'tiny.logits.{ci}']
        assert got.shape == ref.shape, (sl, ov, got.shape, ref.shape)
        d = np.abs(got - ref)
        print(f'[buffered tiny cpu seq_len={sl} overlap={ov}] max {float(d.max()):.3f} mean {float(d.mean()):.4f}')
        assert float(d.max()) < 0.3 and float(d.mean()) < 0.03, (sl, ov, float(d.max()), float(d.mean()))
    with pytest.raises(AssertionError, match='multiple of the downsampling factor'):
        fetch_logits(E.Args, m, spec, 256, 60, tok, use_tqdm=False)
    with pytest.raises(ValueError):
        fetch_logits(E.Args, m, spec[0], 256, 64, tok, use_tqdm=False)


# ---- evaluate ---------------------------------------------------------------------------------------------------------------
class WordTok:
    """Toy tokenizer: id i decodes to the word 'w<i % 7>' followed by a space."""
    def __init__(self, V): self.V = V
    def vocab_size(self): return self.V
    def decode(self, ids): return ' '.join(f'w{int(i) % 7}' for i in ids)


def _spy(att, fn):
    """Call fn(att) before every use of an attention module (the layers call forward_prenorm, not forward)."""
    inner = att.forward_prenorm

    def wrapped(*a, **kw):
        fn(att)
        return inner(*a, **kw)

    att.forward_prenorm = wrapped


@pytest.mark.parametrize('mode', ['averaged_moving_window', 'buffered', 'windowed_attention'])
def test_evaluate_modes_on_the_tiny_model(eval_ops, mode):
    from lcasr_amd.eval import run as R
    from lcasr_amd.eval.wer import word_error_rate_detail
    from lcasr_amd.decoding.greedy import GreedyCTCDecoder
    fx, _, spec = _tiny()
    m = build_from_fixture(fx).eval()
    tok = WordTok(int(fx['cfg.vocab_size']))
    att = R._windowed_modules(m)
    assert len(att) == int(fx['cfg.n_layers']) and all(a.left_window == -1 and a.right_window == -1 for a in att)
    seen = []
    for a in att:
        _spy(a, lambda mod: seen.append((mod.left_window, mod.right_window)))
    recs = [('r0', spec, 'w1 w2 w3 w4'), ('r1', spec[:, :, :600].contiguous(), 'W5 w6')]
    data = R.evaluate(m, recs, tok, 256, 64, evaluation_mode=mode, include_per_recording_evaluations=True)
    assert [d['recording'] for d in data] == ['r0', 'r1', 'all']
    assert all(sorted(d) == ['del_rate', 'ins_rate', 'recording', 'sub_rate', 'wer', 'words'] for d in data)
    assert [d['words'] for d in data] == [4, 2, 6]
    assert seen and set(seen) == ({(16, 16)} if mode == 'windowed_attention' else {(-1, -1)})
    assert all(a.left_window == -1 and a.right_window == -1 for a in att)
    # the same number by hand: logits of the mode, greedy decode, lower(), one scoring call over both recordings
    dec = GreedyCTCDecoder(tokenizer=tok, blank_id=m.decoder.num_classes - 1)
    if mode == 'windowed_attention':
        for a in att: a.left_window = a.right_window = 16
        fn, sl = R.moving_average_eval, 3600000
    else:
        fn, sl = (R.buffered_eval if mode == 'buffered' else R.moving_average_eval), 256
    texts = [dec(torch.from_numpy(fn(R._Args(), m, s, sl, 64, tok, use_tqdm=False))).lower() for _, s, _ in recs]
    for a in att: a.left_window = a.right_window = -1
    want = word_error_rate_detail(texts, [g for _, _, g in recs])
    assert (data[-1]['wer'], data[-1]['words'], data[-1]['ins_rate'], data[-1]['del_rate'], data[-1]['sub_rate']) == want
    assert want[0] > 0 and abs(want[0] - (want[2] + want[3] + want[4])) < 1e-12
    only_all = R.evaluate(m, recs, tok, 256, 64, evaluation_mode=mode, normalize=lambda s: s.replace('w', 'v'))
    assert len(only_all) == 1 and only_all[0]['recording'] == 'all'


def test_evaluate_restores_the_windows_when_the_model_raises(eval_ops):
    from lcasr_amd.eval import run as R
    fx, _, spec = _tiny()
    m = build_from_fixture(fx).eval()
    att = R._windowed_modules(m)
    att[0].left_window, att[0].right_window = 5, 7

    def boom(mod):
        assert (mod.left_window, mod.right_window) == (12, 12)
        raise RuntimeError('injected failure')

    _spy(att[-1], boom)
    with pytest.raises(RuntimeError, match='injected failure'):
        R.evaluate(m, [('r0', spec, 'a')], WordTok(int(fx['cfg.vocab_size'])), 200, 0, evaluation_mode='windowed_attention')
    assert (att[0].left_window, att[0].right_window) == (5, 7)
    assert all(a.left_window == -1 and a.right_window == -1 for a in att[1:])
    with pytest.raises(ValueError, match='evaluation_mode'):
        R.evaluate(m, [], WordTok(3), 256, 0, evaluation_mode='beam')


# ---- C ABI, host side ------------------------------------------------------------------------------------------------------
def test_edit_geometry_queries_and_argument_validation_answer_on_the_host():
    from lcasr_amd.hip import _lib
    lib = _lib.load()
    assert lib.sconf_version() >= 210
    S, Pc, R = lib.sconf_edit_strip_cols(), lib.sconf_edit_pass_cols(), lib.sconf_edit_block_rows()
    assert S > 0 and S % 64 == 0 and Pc % S == 0 and Pc >= S and R > 0
    ws = lib.sconf_edit_counts_workspace
    assert ws(0, 100, 10 * Pc) == 0 and ws(7, 100, Pc) == 0                          # one pass parks nothing
    assert ws(7, 100, Pc + 1) == 7 * 101 * 8 and ws(1, 1 << 20, 1 << 20) == ((1 << 20) + 1) * 8
    assert ws(-1, 1, 1) == -1 and ws(1, -1, 1) == -1 and ws(1, 1, -1) == -1
    assert lib.sconf_edit_counts(None, None, None, None, 0, None, None, 0, None) == 0     # P == 0 launches nothing
    assert lib.sconf_edit_counts(None, None, None, None, -1, None, None, 0, None) != 0
    assert b'sconf_edit_counts' in lib.sconf_last_error() and b'P=-1' in lib.sconf_last_error()
    assert lib.sconf_edit_counts(None, None, None, None, 2, None, None, 0, None) != 0 and b'null' in lib.sconf_last_error()
    off = (ctypes.c_int64 * 3)(0, 0, 0); out = (ctypes.c_int64 * 8)()
    rc = lib.sconf_edit_counts(None, ctypes.addressof(off), None, ctypes.addressof(off), 2, ctypes.addressof(out), None, 64, None)
    assert rc != 0 and b'workspace' in lib.sconf_last_error()
    assert lib.sconf_copy_row_spans(None, 0, 8, 8, None, None, 8, None) == 0
    assert lib.sconf_copy_row_spans(None, 1, 8, 6, None, None, 8, None) != 0 and b'multiple of 4' in lib.sconf_last_error()
    assert lib.sconf_copy_row_spans(None, 1, 8, 8, None, None, 8, None) != 0 and b'null' in lib.sconf_last_error()
