"""CPU tests of CTC prefix beam search: the numpy restatement (tests/beam_refs.py) against the enumeration of every frame path and
against hand cases, the host-side queries and refusals of the beam unit (test_cabi.py holds its binding to include/sconf_beam.h), and BeamSearchCTCDecoder / decode_beams_lm / evaluate(beam_width=...) on the tiny fixture model with the
binding replaced by the restatement.  The HIP kernels themselves are tested in test_beam_gpu.py."""
import ctypes
import math

import numpy as np
import pytest
import torch

import beam_refs as BR
import eval_refs as E
from common_model import build_from_fixture
from conftest import load_golden

INF = math.inf


@pytest.fixture
def emulated_beam(monkeypatch):
    """The binding layer (lcasr_amd.hip.beam.ctc_beam) replaced by the numpy restatement: host logic without a GPU."""
    from lcasr_amd.decoding import beam as D
    monkeypatch.setattr(D.beam_kernels, 'ctc_beam', BR.ctc_beam)
    return D


def _lp(probs):
    return np.log(np.asarray(probs, dtype=np.float64)).astype(np.float32)


# ---- 1. the yardstick ---------------------------------------------------------------------------------------------------------
def test_restatement_against_the_enumeration_of_every_frame_path():
    """Token pruning off, W above the number of prefixes, T <= 5, C <= 4: every label sequence is a hypothesis and its score is the
    log-sum of all its alignments."""
    rng = np.random.default_rng(2025)
    worst, sets = 0.0, 0
    for T in range(1, 6):
        for C in (2, 3, 4):
            for _ in range(6):
                x = rng.normal(size=(T, C)) * 2
                lp = (x - np.log(np.exp(x).sum(-1, keepdims=True))).astype(np.float32)
                beams, st = BR.search(lp, C - 1, 2000, -INF, -INF, 16)
                want = BR.enumerate_paths(lp, C - 1)
                assert {b[0] for b in beams} == set(want) and len(beams) == len(want)
                assert [b[2] for b in beams] == sorted((b[2] for b in beams), reverse=True)
                for pre, frames, total in beams:
                    worst = max(worst, abs(total - want[pre]))
                    assert len(frames) == len(pre) and list(frames) == sorted(set(frames)) and all(0 <= f < T for f in frames)
                sets += 1
    print(f'[beam] {sets} emission sets, largest |score - log-sum of the alignments| = {worst:.2e}')
    assert worst <= 1e-13


# ---- 2. hand cases --------------------------------------------------------------------------------------------------------------
def test_two_frames_where_greedy_returns_nothing_and_the_search_returns_a():
    """Classes: 0 = a, 1 = blank.  P(a) = 0.6 both frames: P("a") = 1 - 0.16, greedy finds it too.  P(a) = 0.4: P("a") = 0.64 but the
    per-frame argmax is the blank twice."""
    beams, _ = BR.search(_lp([[0.6, 0.4]] * 2), 1, 4)
    assert beams[0][0] == (0,) and beams[0][2] == pytest.approx(math.log(0.84), abs=1e-7) and beams[0][1] == (0,)
    lp = _lp([[0.4, 0.6]] * 2)
    assert lp.argmax(-1).tolist() == [1, 1]                                # greedy: ""
    beams, _ = BR.search(lp, 1, 4)
    assert [b[0] for b in beams] == [(0,), ()]
    assert beams[0][2] == pytest.approx(math.log(0.64), abs=1e-7) and beams[1][2] == pytest.approx(math.log(0.36), abs=1e-7)
    out = BR.ctc_beam(torch.from_numpy(lp)[None], None, 1, 4, 2, -5.0, -10.0, 16, 2)
    assert out.count.tolist() == [2] and out.tokens.tolist() == [[[0, -1], [-1, -1]]] and out.lengths.tolist() == [[1, 0]]
    assert out.token_frames.tolist() == [[[0, -1], [-1, -1]]]


def test_tie_rules_by_hand():
    """Log-probs that are exact in f32 (multiples of 0.25; not normalised: the contract does not ask for it)."""
    # kept tokens: ties at the cap go to the lower index, the arg-max tie to the lowest index
    row = np.asarray([-1, -1, -1, -9, -1], dtype=np.float32)              # blank = 3
    assert BR.kept_tokens(row, 3, -5.0, 16) == ([0, 1, 2, 4], False)
    assert BR.kept_tokens(row, 3, -5.0, 2) == ([0, 1], True)
    assert BR.kept_tokens(row, 3, -1.0, 16) == ([0, 1, 2, 4], False)       # >=, compared in f32
    assert BR.kept_tokens(np.asarray([-7, -6, -6, -9], dtype=np.float32), 3, -5.0, 16) == ([1], False)      # the arg-max alone
    assert BR.kept_tokens(np.asarray([-7, -6, -6, -6], dtype=np.float32), 3, -5.0, 16) == ([1], False)      # blank ties: lowest index wins
    assert BR.kept_tokens(np.asarray([-7, -8, -8, -6], dtype=np.float32), 3, -5.0, 16) == ([], False)       # the arg-max is the blank
    # selection: a = b = -1 and blank = -1 in one frame: totals all -1; candidate order: stay (index 0), then a (W + 0), then b (W + 1)
    lp = np.asarray([[-1, -1, -1]], dtype=np.float32)
    beams, st = BR.search(lp, 2, 3)
    assert [b[0] for b in beams] == [(), (0,), (1,)] and st['gap'] == 0.0
    beams, _ = BR.search(lp, 2, 2)
    assert [b[0] for b in beams] == [(), (0,)]
    # prune: total < best + prune is dropped, total == best + prune stays
    lp = np.asarray([[-1.0, -3.0, -0.5]], dtype=np.float32)
    assert [b[0] for b in BR.search(lp, 2, 3, beam_prune_logp=-2.5)[0]] == [(), (0,), (1,)]
    assert [b[0] for b in BR.search(lp, 2, 3, beam_prune_logp=-2.25)[0]] == [(), (0,)]
    assert BR.search(lp, 2, 3, beam_prune_logp=-2.25)[1]['pruned'] == 1


def test_a_repeat_with_and_without_a_blank_between():
    """Classes: 0 = a, 1 = blank, probabilities.  "aa" needs a blank between two a; without one, a a collapses to "a"."""
    p = _lp([[0.9, 0.1], [0.9, 0.1]])
    got = {b[0]: b[2] for b in BR.search(p, 1, 8, -INF, -INF)[0]}
    assert set(got) == {(0,), ()}                                          # two frames cannot hold "aa"
    assert got[(0,)] == pytest.approx(math.log(0.81 + 0.09 + 0.09), abs=1e-6)
    p = _lp([[0.9, 0.1], [0.1, 0.9], [0.9, 0.1]])
    beams, st = BR.search(p, 1, 8, -INF, -INF)
    got = {b[0]: b for b in beams}
    assert got[(0, 0)][2] == pytest.approx(math.log(0.9 * 0.9 * 0.9), abs=1e-6) and got[(0, 0)][1] == (0, 2)
    assert beams[0][0] == (0, 0) and st['folds'] >= 1
    want = BR.enumerate_paths(p, 1)
    assert all(b[2] == pytest.approx(want[b[0]], abs=1e-12) for b in beams)


def test_a_last_token_that_is_not_kept_contributes_nothing():
    """Classes: 0 = a, 1 = b, 2 = blank.  Frame 1 gives a the log-prob -6 < token_min_logp and b the arg-max: a is not kept, so the
    beam "a" does not continue through a a - only through a blank."""
    lp = np.asarray([[-0.25, -4.0, -2.0], [-6.0, -0.25, -2.0]], dtype=np.float32)
    assert BR.kept_tokens(lp[1], 2, -5.0, 16) == ([1], False)
    got = {b[0]: b[2] for b in BR.search(lp, 2, 16, beam_prune_logp=-INF)[0]}
    assert got[(0,)] == -0.25 + -2.0                                       # a then blank; NOT lse(a a, a blank)
    assert (0, 0) not in got and got[(0, 1)] == -0.5
    loose = {b[0]: b[2] for b in BR.search(lp, 2, 16, token_min_logp=-7.0, beam_prune_logp=-INF)[0]}
    assert loose[(0,)] == pytest.approx(math.log(math.exp(-2.25) + math.exp(-6.25) + math.exp(-8.0)), abs=1e-12)      # a blank, a a, blank a


def test_batched_restatement_lengths_padding_and_poisoned_samples():
    lp, _ = BR.spiky_case(3, 4, 30, 8, 7, every=2)
    st = []
    out = BR.ctc_beam(lp, torch.tensor([30, 12, 31, 0]), 7, 8, 3, -5.0, -10.0, 4, 5, stats=st)
    assert out.count.dtype == torch.int32 and out.scores.dtype == torch.float64 and out.tokens.shape == (4, 3, 5)
    assert st[2] is None and out.count[2] == 0 and bool(torch.isnan(out.scores[2]).all()) and bool((out.tokens[2] == -1).all())
    assert out.count[3] == 1 and out.scores[3].tolist() == [0.0, -INF, -INF] and out.lengths[3].tolist() == [0, 0, 0]
    assert int(out.lengths[0, 0]) > 5 and bool((out.tokens[0, 0] >= 0).all())          # longer than Lmax: the true length, 5 tokens
    assert bool((out.token_frames[1][out.token_frames[1] >= 0] < 12).all())
    alone = BR.ctc_beam(lp[1:2], torch.tensor([12]), 7, 8, 3, -5.0, -10.0, 4, 5)
    assert all(torch.equal(a[0], b[1]) for a, b in zip(alone, out))


def test_the_recreation_case_exists_among_the_first_40_seeds():
    for W in (2, 3, 4):
        case = BR.recreation_case(W)
        assert case is not None and 0 <= case[0] < 40
        _, st = BR.search(BR.noise_case(case[0], 1, 24, 4, case[1])[0].numpy(), 3, W)
        assert st['recreated'] >= 1


# ---- 3. host side of the beam unit (its header is held to the binding in test_cabi.py) ---------------------------------------
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from lcasr_amd.hip import beam
    return beam.load()


def test_beam_queries(lib):
    from lcasr_amd.hip import beam
    MW, MK = lib.sconf_beam_max_width(), lib.sconf_beam_max_tokens()
    assert MW >= 128 and MK >= 16 and MW == beam.max_width() and MK == beam.max_tokens()
    th, ss = lib.sconf_beam_threads, lib.sconf_beam_sort_size
    R = lib.sconf_beam_rank_limit()
    assert R == 128 and [ss(c) for c in (1, 2, 65, R, R + 1, 256, 257, 1000, 1024, 1025, 2048, 2049, 2176)] == [0, 0, 0, 0, 256, 256, 512, 1024, 1024, 2048, 2048, 4096, 4096]
    assert ss(0) == -1 and ss(MW * (MK + 1) + 1) == -1 and ss(MW * (MK + 1)) > 0
    for W in (1, 2, 7, 63, 64, 65, 100, MW):
        for K in (1, 2, 5, MK):
            t = th(W, K)
            assert t in (64, 128, 256, 512, 1024) and (t == 1024 or t == 64 or t == 1 << (W * (K + 1) - 1).bit_length() - 1)
    assert th(1, 1) == 64 and th(MW, MK) == 1024 and th(8, 16) == 128 and th(16, 16) == 256 and th(32, 16) == 512
    assert th(0, 1) == -1 and th(MW + 1, 1) == -1 and th(1, 0) == -1 and th(1, MK + 1) == -1
    assert lib.sconf_beam_prefetch_frames() >= 1
    ws = lib.sconf_beam_workspace
    assert ws(1, 16384, 100, 16) == 28444672 == beam.beam_workspace(1, 16384, 100, 16)            # the figure in the header
    r256 = lambda n: (n + 255) // 256 * 256
    for B, N, W, K in ((1, 1, 1, 1), (2, 100, 7, 3), (3, 2048, 64, 16), (16, 2048, 100, 16)):
        assert ws(B, N, W, K) == r256(B * N * (8 + 8 * K)) + r256(16 * B * N * W) + r256(16 * B * W) + r256(4 * B)
        assert ws(B, N, W, K) <= ws(B + 1, N, W, K) and ws(B, N, W, K) <= ws(B, N + 1, W, K)
    assert ws(0, 10, 4, 4) == -1 and ws(1, 0, 4, 4) == -1 and ws(1, 10, 0, 4) == -1 and ws(1, 10, MW + 1, 4) == -1
    assert ws(1, 10, 4, 0) == -1 and ws(1, 10, 4, MK + 1) == -1 and ws(-1, 10, 4, 4) == -1 and ws(1 << 20, 1 << 20, 4, 4) == -1
    with pytest.raises(ValueError, match=str(MW)):
        beam.beam_workspace(1, 10, MW + 1, 4)


def test_beam_refusals_launch_nothing(lib):
    from lcasr_amd.hip import beam
    one = ctypes.c_void_p(16)                                              # never dereferenced: every call below is refused on the host
    need = lib.sconf_beam_workspace(1, 10, 8, 4)

    def call(lp=one, ws=need, B=1, N=10, C=32, blank=31, W=8, nbest=2, prune=-10.0, K=4, L=10):
        return lib.sconf_beam_ctc(lp, None, one, one, one, one, one, one, ws, B, N, C, blank, W, nbest, -5.0, prune, K, L, None)

    assert call(blank=32) != 0 and b'blank' in lib.sconf_last_error()
    assert call(blank=-1) != 0 and b'blank' in lib.sconf_last_error()
    assert call(ws=need - 1) != 0 and b'workspace' in lib.sconf_last_error()
    assert call(W=0) != 0 and b'beam_width' in lib.sconf_last_error()
    assert call(W=lib.sconf_beam_max_width() + 1, ws=1 << 40) != 0 and str(lib.sconf_beam_max_width()).encode() in lib.sconf_last_error()
    assert call(nbest=9) != 0 and b'nbest' in lib.sconf_last_error()
    assert call(nbest=0) != 0 and b'nbest' in lib.sconf_last_error()
    assert call(K=0) != 0 and b'max_tokens_per_frame' in lib.sconf_last_error()
    assert call(K=lib.sconf_beam_max_tokens() + 1, ws=1 << 40) != 0 and b'max_tokens_per_frame' in lib.sconf_last_error()
    assert call(prune=0.5) != 0 and b'beam_prune_logp' in lib.sconf_last_error()
    assert call(prune=math.nan) != 0 and b'beam_prune_logp' in lib.sconf_last_error()
    assert call(C=30) != 0 and b'multiple of 4' in lib.sconf_last_error()
    assert call(N=0) != 0 and b'sizes' in lib.sconf_last_error()
    assert call(L=0) != 0 and b'sizes' in lib.sconf_last_error()
    assert call(lp=None) != 0 and b'null' in lib.sconf_last_error()
    assert call(B=0) == 0                                                  # nothing to do, nothing launched


def test_a_cpu_tensor_is_refused_by_the_product_path():
    from lcasr_amd.decoding.beam import BeamSearchCTCDecoder, ctc_beam_search
    lp = BR.noise_case(1, 1, 8, 8)
    with pytest.raises(RuntimeError, match='GPU'):
        ctc_beam_search(lp[0], blank=7)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='GPU'):
            BeamSearchCTCDecoder(blank_id=7)(lp[0])


# ---- 4. the Python layers on the restatement ------------------------------------------------------------------------------------
class PieceTok:
    """A sentencepiece-like stub."""
    PIECES = ['▁the', '▁c', 'at', 's', '▁sat', 'on', '▁']

    def id_to_piece(self, i): return self.PIECES[i]
    def decode(self, ids): return ''.join(self.PIECES[i] for i in ids).replace('▁', ' ').strip()


def _planted(ids, C, blank, gap=3):
    """(N, C) log-probs that spell `ids`: token j at frame gap * j + 1 with probability 0.9, every other token 0.001 (below
    token_min_logp), the blank the rest."""
    N = gap * len(ids) + 2
    p = np.full((N, C), 0.001)
    p[:, blank] = 1 - 0.001 * (C - 1)
    for j, c in enumerate(ids):
        p[gap * j + 1, c] = 0.9
        p[gap * j + 1, blank] = 0.1 - 0.001 * (C - 2)
    return torch.from_numpy(np.log(p).astype(np.float32))


def test_wrapper_shapes_defaults_and_class_padding(emulated_beam):
    D = emulated_beam
    lp = BR.noise_case(4, 2, 12, 7)                                        # 7 classes: padded to 8 with -inf
    a = D.ctc_beam_search(lp[0], blank=6, beam_width=5, nbest=3)
    assert isinstance(a, D.CTCBeams) and a.tokens.shape == (3, 12) and a.scores.shape == (3,) and a.count.shape == ()
    assert int(a.tokens.max()) < 7
    b = D.ctc_beam_search(lp, input_lengths=[12, 9], blank=6, beam_width=5, nbest=3, max_len=4)
    assert b.tokens.shape == (2, 3, 4) and torch.equal(b.tokens[0], a.tokens[:, :4]) and torch.equal(b.scores[0], a.scores)
    want, _ = BR.search(lp[1, :9].numpy(), 6, 5)
    assert b.scores[1].tolist()[:int(b.count[1])] == [w[2] for w in want[:3]]
    with pytest.raises(ValueError):
        D.ctc_beam_search(lp[0, 0], blank=6)


def test_beam_decoder_and_decode_beams_lm(emulated_beam):
    from lcasr_amd.eval.utils import decode_beams_lm
    from lcasr_amd.utils.audio_tools import total_seconds
    D = emulated_beam
    ids = [5, 0, 1, 2, 3, 4]                                               # 'on' 'the' 'c at s' 'sat'
    lp = _planted(ids, 8, 7)
    dec = D.BeamSearchCTCDecoder(tokenizer=PieceTok(), blank_id=7, beam_width=16, nbest=4)
    assert dec(lp) == 'on the cats sat' and dec(lp, decode=False) == ids
    assert D.BeamSearchCTCDecoder(blank_id=7)(lp) == ids                   # no tokenizer: ids, as GreedyCTCDecoder
    beams = dec.decode_beams(lp)
    assert 1 < len(beams) <= 4 and beams[0].tokens == ids and beams[0].text == 'on the cats sat'
    assert beams[0].lm_score == beams[0].logit_score and [b.logit_score for b in beams] == sorted((b.logit_score for b in beams), reverse=True)
    assert beams[0].text_frames == [('on', (1, 2)), ('the', (4, 5)), ('cats', (7, 14)), ('sat', (16, 17))]
    assert len(dec.decode_beams(lp, beam_width=2)) <= 2
    w = D.BeamSearchCTCDecoder(tokenizer=PieceTok(), blank_id=7, word_start=lambda i: i in (0, 4)).decode_beams(lp)[0]
    assert [t for t, _ in w.text_frames] == ['on', 'the cats', 'sat'] and w.text_frames[1][1] == (4, 14)
    with pytest.raises(ValueError, match='max_len'):
        D.BeamSearchCTCDecoder(blank_id=7, max_len=3)(lp)
    with pytest.raises(ValueError):
        dec(lp[None])
    data, best = decode_beams_lm([lp.numpy(), lp], dec, beam_width=8, encoded_lengths=[lp.shape[0], 9], ds_factor=4)
    assert [d['text'] for d in data] == ['on the cats sat', 'on the c'] and best.tokens == [5, 0, 1]
    d = data[0]
    assert sorted(d) == ['am_score', 'frames', 'ngram_score', 'score', 'text'] and d['ngram_score'] == 0 and d['score'] == d['am_score'] < 0
    assert d['frames'][2] == {'word': 'cats', 'start': total_seconds(7 * 4), 'end': total_seconds(14 * 4)}
    assert decode_beams_lm([lp], dec, ds_factor=None)[0][0]['frames'] is None


class WordTok:
    """Toy tokenizer: id i decodes to the word 'w<i % 7>'."""
    def __init__(self, V): self.V = V
    def vocab_size(self): return self.V
    def decode(self, ids): return ' '.join(f'w{int(i) % 7}' for i in ids)


def test_evaluate_with_a_beam_on_the_tiny_model(emulated_ops, emulated_beam, monkeypatch):
    from lcasr_amd.eval import run as R
    from lcasr_amd.eval.wer import word_error_rate_detail
    E.attach(monkeypatch, emulated_ops)
    fx = load_golden('infer_tiny')
    m = build_from_fixture(fx).eval()
    tok = WordTok(int(fx['cfg.vocab_size']))
    spec = torch.from_numpy(fx['spec'].copy())
    recs = [('r0', spec, 'w1 w2 w3 w4'), ('r1', spec[:, :, :600].contiguous(), 'W5 w6')]
    calls = []
    inner = emulated_beam.beam_kernels.ctc_beam
    monkeypatch.setattr(emulated_beam.beam_kernels, 'ctc_beam', lambda *a: (calls.append(a[3]), inner(*a))[1])
    data = R.evaluate(m, recs, tok, 256, 64, include_per_recording_evaluations=True, beam_width=4)
    assert calls == [4, 4] and [d['recording'] for d in data] == ['r0', 'r1', 'all']
    blank = m.decoder.num_classes - 1
    texts = []
    for _, s, _ in recs:
        logits = R.moving_average_eval(R._Args(), m, s, 256, 64, tok, use_tqdm=False, return_numpy=False)
        best = BR.search(logits.float().numpy(), blank, 4)[0][0]
        texts.append(tok.decode(best[0]).lower())
    want = word_error_rate_detail(texts, [g for _, _, g in recs])
    assert (data[-1]['wer'], data[-1]['words'], data[-1]['ins_rate'], data[-1]['del_rate'], data[-1]['sub_rate']) == want
    # beam_width = 1 is today's greedy path: the search is never called and the figures are those of a call without the argument
    del calls[:]
    assert R.evaluate(m, recs, tok, 256, 64, include_per_recording_evaluations=True, beam_width=1) == \
        R.evaluate(m, recs, tok, 256, 64, include_per_recording_evaluations=True)
    assert calls == [] and type(R._decoder(m, tok, 1)).__name__ == 'GreedyCTCDecoder'
    with pytest.raises(ValueError, match='beam_width'):
        R.evaluate(m, recs, tok, 256, 64, beam_width=0)
