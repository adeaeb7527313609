"""CPU tests of CTC forced alignment: the numpy restatement (tests/align_refs.py) against the brute-force definition and against
hand-written tie cases, the host-side queries and refusals of the alignment unit (test_cabi.py holds its binding to
include/sconf_align.h), word_timestamps, and eval.run.align on the tiny fixture model with the binding replaced by the
restatement.  The HIP kernels themselves are tested in test_align_gpu.py."""
import ctypes
import itertools
import re

import numpy as np
import pytest
import torch

import align_refs as AR
import eval_refs as E
from common_model import build_from_fixture
from conftest import load_golden


@pytest.fixture
def emulated_align(monkeypatch):
    """The binding layer (lcasr_amd.hip.align.ctc_align) replaced by the numpy restatement: host logic without a GPU."""
    from lcasr_amd.decoding import align as D
    monkeypatch.setattr(D.align_kernels, 'ctc_align', AR.ctc_align)
    return D


# ---- 1. the yardstick ---------------------------------------------------------------------------------------------------------
def test_restatement_against_every_path_that_collapses_to_the_target():
    """T <= 6, S <= 3, C = 3 (two labels and the blank), every target, 20 emission sets each.  Emissions are log-softmaxes of
    continuous draws, so two different paths tie only by accident of rounding: unique in well over 90 % of the sets (asserted)."""
    rng = np.random.default_rng(2024)
    sets = unique = 0
    for T in range(1, 7):
        for S in range(0, 4):
            for target in itertools.product(range(2), repeat=S):
                for _ in range(20):
                    x = rng.normal(size=(T, 3)) * 2
                    lp = (x - np.log(np.exp(x).sum(-1, keepdims=True))).astype(np.float32)
                    best, arg = AR.brute_force(lp, target, 2)
                    for dtype in (np.float64, np.float32):
                        path, labels, spans, logp, score = AR.align_sample(lp, target, 2, dtype)
                        if not AR.feasible(T, list(target)):
                            assert path is None and score == -np.inf and best == -np.inf and not arg
                            continue
                        assert path is not None and abs(score - best) <= T * (2.0 ** -52 if dtype is np.float64 else 2.0 ** -23) * abs(best)
                        if dtype is np.float64:
                            assert score == pytest.approx(best, rel=1e-14)
                        if len(arg) == 1 and dtype is np.float64:
                            assert tuple(labels.tolist()) == arg[0]
                            assert AR.collapse(labels.tolist(), 2) == list(target)
                            for j, (f, l) in enumerate(spans.tolist()):
                                assert all(path[t] == 2 * j + 1 for t in range(f, l)) and (path == 2 * j + 1).sum() == l - f
                                assert logp[j] == pytest.approx(float(lp[f:l, target[j]].sum()), abs=1e-5)
                    if AR.feasible(T, list(target)):
                        sets += 1
                        unique += len(arg) == 1
    print(f'[align] {sets} feasible emission sets, best path unique in {unique}')
    assert sets > 1000 and unique >= 0.9 * sets


# ---- 2. tie rules ---------------------------------------------------------------------------------------------------------------
def _lp(rows):
    return np.asarray(rows, dtype=np.float32)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_tie_rules_by_hand(dtype):
    """Multiples of 0.25 (exact in f32 and f64).  Classes: 0 = a, 1 = b, 2 = blank."""
    # stay / s-1 and the end: target [a], three equal frames with a = blank = -1.  v0 = [-1, -1, -inf]; v1 = [-2, -2, -2]: state 1 ties
    # between stay and s-1 (stay wins), state 2 has only s-1; v2 = [-3, -3, -3]: state 2 ties between stay and s-1 (stay wins).  The end
    # ties between L-1 = 2 and L-2 = 1: L-1 wins.  Walk: (2, 2) stayed, (1, 2) came from 1: path 1, 2, 2.
    lp = _lp([[-1, -9, -1]] * 3)
    path, labels, spans, _, score = AR.align_sample(lp, [0], 2, dtype)
    assert path.tolist() == [1, 2, 2] and score == -3.0 and spans.tolist() == [[0, 1]]
    # s-1 / s-2: target [a, b], T = 3, built so that v1[2] = v1[1].
    # v0 = [-1, -1, -inf, -inf, -inf]; v1 = [-2, -2, -2, -10, -inf]; frame 2 (b = -1, blank = -4, a = -9): state 3 from stay -10, s-1 = -2
    # (state 2), s-2 = -2 (state 1): s-1 replaces stay, s-2 is not STRICTLY greater: step 1.  v2[3] = -3, v2[4] = max(-inf, -10) - 4 = -14.
    lp = _lp([[-1, -9, -1], [-1, -9, -1], [-9, -1, -4]])
    path, labels, spans, _, score = AR.align_sample(lp, [0, 1], 2, dtype)
    assert score == -3.0 and path.tolist() == [1, 2, 3] and labels.tolist() == [0, 2, 1] and spans.tolist() == [[0, 1], [2, 3]]
    # end L-1 / L-2: target [a], T = 2, frame 1 a = blank = -1: v1[2] = v0[1] - 1 = -2 = v1[1] (stay on the tie): end = L-1 = 2.
    lp = _lp([[-1, -9, -1], [-1, -9, -1]])
    path, labels, spans, _, score = AR.align_sample(lp, [0], 2, dtype)
    assert score == -2.0 and path.tolist() == [1, 2] and spans.tolist() == [[0, 1]]
    # the same with L-2 strictly better: the end moves
    lp = _lp([[-1, -9, -1], [-0.75, -9, -1]])
    path, _, spans, _, score = AR.align_sample(lp, [0], 2, dtype)
    assert score == -1.75 and path.tolist() == [1, 1] and spans.tolist() == [[0, 2]]
    # a repeated label has no s-2 step: [a, a] in 2 frames is infeasible, in 3 frames it goes through the blank
    assert AR.align_sample(_lp([[-1, -9, -1]] * 2), [0, 0], 2, dtype)[0] is None
    assert AR.align_sample(_lp([[-1, -9, -1]] * 3), [0, 0], 2, dtype)[0].tolist() == [1, 2, 3]


def test_batched_restatement_marks_padding_infeasible_and_poisoned_samples():
    lp, tg = AR.random_case(3, 4, 12, 8, 5)
    tg[3, 1] = 8
    out = AR.ctc_align(lp, tg, torch.tensor([12, 9, 4, 12]), torch.tensor([5, 3, 5, 5]), 7)
    assert out.path.dtype == torch.int32 and out.score.dtype == torch.float64 and out.token_logp.dtype == torch.float32
    assert bool((out.path[1, 9:] == -1).all()) and bool((out.path[1, :9] >= 0).all()) and out.spans[1, 3:].tolist() == [[-1, -1]] * 2
    assert float(out.score[2]) == -np.inf and bool((out.path[2] == -1).all()) and bool((out.spans[2] == -1).all())
    assert np.isnan(float(out.score[3])) and bool((out.labels[3] == -1).all()) and bool((out.token_logp[3] == 0).all())
    alone = AR.ctc_align(lp[:1], tg[:1], None, None, 7)
    assert all(torch.equal(a[0], b[0]) for a, b in zip(alone, out))


# ---- 3. host side of the alignment unit (its header is held to the binding in test_cabi.py) --------------------------------
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from lcasr_amd.hip import align
    return align.load()


def test_align_queries(lib):
    from lcasr_amd.hip import align
    M = lib.sconf_align_max_labels()
    assert M == 8191 == align.max_labels()
    sb = lib.sconf_align_state_bytes
    assert sb(0) == 8 and sb(12) == 8 and sb(M) == 4 and sb(M + 1) == -1 and sb(-1) == -1
    first_f32 = next(s for s in range(M + 1) if sb(s) == 4)
    assert all(sb(s) == 4 for s in range(first_f32, M + 1, 97))              # one threshold
    # two rows of f64 with the kernel's guard and slack cells fit 160 KB just below the threshold and not at it
    spt = lib.sconf_align_states_per_thread
    assert 2 * (2 * (first_f32 - 1) + 1 + spt(first_f32 - 1) + 2) * 8 <= 160 * 1024 < 2 * (2 * first_f32 + 1 + spt(first_f32) + 2) * 8
    assert lib.sconf_align_threads(M + 1) == -1 and spt(M + 1) == -1
    for S in range(0, M + 1, 61):
        assert lib.sconf_align_threads(S) * spt(S) >= 2 * S + 1 and spt(S) in (1, 2, 4, 8, 12, 16)
    ws = lib.sconf_align_workspace
    assert ws(1, 16384, 4096) == 403702016 == align.align_workspace(1, 16384, 4096)          # the figure in the header
    assert ws(1, 16384, 4096) <= 256 + 16384 * (2 * 4096 + 1 + 47) + 4 * 16384 * (4096 + 12) + 512   # <= 1 byte per cell + compact emissions
    for B, N, S in ((1, 1, 0), (2, 100, 7), (3, 2048, 512), (1, 16384, 4096)):
        assert 0 < ws(B, N, S) <= ws(B + 1, N, S) and ws(B, N, S) <= ws(B, N + 1, S) and ws(B, N, S) <= ws(B, N, S + 1)
    assert ws(2, 4000, 300) > ws(1, 4000, 300) and ws(1, 4001, 300) > ws(1, 4000, 300) and ws(1, 4000, 324) > ws(1, 4000, 300)
    assert ws(-1, 10, 10) == -1 and ws(1, -1, 10) == -1 and ws(1, 10, -1) == -1 and ws(1, 10, M + 1) == -1 and ws(0, 10, 10) == -1
    with pytest.raises(ValueError):
        align.align_workspace(1, 10, M + 1)
    with pytest.raises(ValueError, match=str(M)):
        align.state_bytes(M + 1)


def test_align_refusals_launch_nothing(lib):
    one = ctypes.c_void_p(16)                                              # never dereferenced: every call below is refused on the host
    need = lib.sconf_align_workspace(1, 10, 3)
    call = lambda blank=31, ws=need, B=1, N=10, C=32, S=3: lib.sconf_align_ctc(one, one, None, None, one, one, one, one, one, one, ws, B, N, C, S,
                                                                               blank, None)
    assert call(blank=32) != 0 and b'blank' in lib.sconf_last_error()
    assert call(blank=-1) != 0 and b'blank' in lib.sconf_last_error()
    assert call(ws=need - 1) != 0 and b'workspace' in lib.sconf_last_error()
    assert call(S=8192, ws=1 << 40) != 0 and b'8191' in lib.sconf_last_error()
    assert call(C=30) != 0 and b'multiple of 4' in lib.sconf_last_error()
    assert call(N=0) != 0 and b'sizes' in lib.sconf_last_error()
    assert lib.sconf_align_ctc(None, one, None, None, one, one, one, one, one, one, need, 1, 10, 32, 3, 31, None) != 0
    assert b'null' in lib.sconf_last_error()
    assert call(B=0) == 0                                                  # nothing to do, nothing launched


def test_a_cpu_tensor_is_refused_by_the_product_path():
    from lcasr_amd.decoding.align import ctc_forced_align
    lp, tg = AR.random_case(1, 1, 8, 8, 3)
    with pytest.raises(RuntimeError, match='GPU'):
        ctc_forced_align(lp[0], tg[0], blank=7)


# ---- 4. word_timestamps ---------------------------------------------------------------------------------------------------------
class PieceTok:
    """A sentencepiece-like stub."""
    PIECES = ['▁the', '▁c', 'at', 's', '▁sat', 'on', '▁']

    def id_to_piece(self, i): return self.PIECES[i]
    def decode(self, ids): return ''.join(self.PIECES[i] for i in ids).replace('▁', ' ').strip()
    def encode(self, text): raise NotImplementedError


class PlainTok:
    def decode(self, ids): return ' '.join(f'w{int(i)}' for i in ids)


def test_word_timestamps():
    from lcasr_amd.decoding.align import word_timestamps
    ids = [5, 0, 1, 2, 3, 4]                                               # 'on' (a leading piece without the marker) 'the' 'c at s' 'sat'
    spans = torch.tensor([[0, 2], [3, 4], [10, 12], [12, 13], [15, 16], [100, 157]])
    logp = torch.tensor([-1.0, -0.5, -2.0, -1.0, -3.0, -5.7])
    w = word_timestamps(ids, spans, PieceTok(), 0.08, token_logp=logp)
    assert [x['word'] for x in w] == ['on', 'the', 'cats', 'sat']
    assert [(x['startTime'], x['endTime']) for x in w] == [('0.00s', '0.16s'), ('0.24s', '0.32s'), ('0.80s', '1.28s'), ('8.00s', '12.56s')]
    assert all(re.fullmatch(r'\d+\.\d\ds', x[k]) and float(x[k][:-1]) >= 0 for x in w for k in ('startTime', 'endTime'))
    assert w[0]['logp'] == pytest.approx(-1.0 / 2) and w[1]['logp'] == pytest.approx(-0.5)
    assert w[2]['logp'] == pytest.approx((-2.0 - 1.0 - 3.0) / (2 + 1 + 1)) and w[3]['logp'] == pytest.approx(-5.7 / 57, rel=1e-6)
    assert 'logp' not in word_timestamps(ids, spans, PieceTok(), 0.08)[0]
    # word_start overrides the pieces; rounding to 2 decimals
    w = word_timestamps(ids, spans.tolist(), PieceTok(), 0.0123, word_start=lambda i: i in (0, 4))
    assert [x['word'] for x in w] == ['on', 'the cats', 'sat'] and w[1]['startTime'] == '0.04s' and w[1]['endTime'] == '0.20s'
    # no id_to_piece: every token is a word, spelt by decode([id])
    w = word_timestamps([3, 3, 9], [[0, 1], [2, 5], [5, 6]], PlainTok(), 0.5, token_logp=[-1.0, -3.0, 0.0])
    assert [(x['word'], x['startTime'], x['endTime'], x['logp']) for x in w] == [('w3', '0.00s', '0.50s', -1.0), ('w3', '1.00s', '2.50s', -1.0),
                                                                                 ('w9', '2.50s', '3.00s', 0.0)]
    assert word_timestamps([], torch.zeros(0, 2), PlainTok(), 0.5) == []
    with pytest.raises(ValueError):
        word_timestamps([1, 2], [[0, 1]], PlainTok(), 0.5)


def test_forced_align_wrapper_shapes(emulated_align):
    D = emulated_align
    lp, tg = AR.random_case(2, 2, 20, 8, 4)
    a = D.ctc_forced_align(lp[0], tg[0].tolist(), blank=7)
    assert isinstance(a, D.CTCAlignment) and a.path.shape == (20,) and a.spans.shape == (4, 2) and a.score.shape == ()
    b = D.ctc_forced_align(lp, tg, input_lengths=[20, 15], target_lengths=torch.tensor([4, 2]), blank=7)
    assert b.path.shape == (2, 20) and torch.equal(b.path[0], a.path) and bool((b.path[1, 15:] == -1).all())
    assert b.spans[1].tolist()[2:] == [[-1, -1]] * 2
    with pytest.raises(ValueError):
        D.ctc_forced_align(lp, tg[0], blank=7)
    with pytest.raises(ValueError):
        D.ctc_forced_align(lp[0, 0], tg[0], blank=7)


# ---- 5. eval.run.align on the tiny fixture model --------------------------------------------------------------------------------
class IdTok:
    """Every token is a word: id i is spelt 't<i>'."""
    def __init__(self, V): self.V = V
    def vocab_size(self): return self.V
    def decode(self, ids): return ' '.join(f't{int(i)}' for i in ids)
    def encode(self, text): return [int(w[1:]) for w in text.split()]


@pytest.mark.parametrize('mode', ['averaged_moving_window', 'buffered', 'windowed_attention'])
def test_align_on_the_tiny_model(emulated_ops, emulated_align, monkeypatch, mode):
    import audio_refs as AUD
    from lcasr_amd.eval import run as R
    from lcasr_amd.utils import audio_tools
    monkeypatch.setattr(audio_tools.audio, 'melspec', AUD.melspec)
    E.attach(monkeypatch, emulated_ops)
    fx = load_golden('infer_tiny')
    m = build_from_fixture(fx).eval()
    V = int(fx['cfg.vocab_size'])
    tok = IdTok(V)
    wave = AUD.test_signal(3 * 16000, seed=3)
    spec = audio_tools.to_spectogram(wave[None])
    att = R._windowed_modules(m)
    text = 't3 t1 t4 t1 t5 t9 t2 t6'
    words = R.align(m, spec, text, tok, 128, 32, evaluation_mode=mode)
    assert all(a.left_window == -1 and a.right_window == -1 for a in att)
    assert [w['word'] for w in words] == text.split()
    times = [float(w[k][:-1]) for w in words for k in ('startTime', 'endTime')]
    assert times == sorted(times) and times[0] >= 0
    assert all(float(w['endTime'][:-1]) > float(w['startTime'][:-1]) and w['logp'] <= 0 for w in words)
    # the same by hand: the logits of the mode, the restatement, word_timestamps
    if mode == 'windowed_attention':
        for a in att: a.left_window = a.right_window = 128 // m.subsampling.subsampling_factor // 2
        fn, sl = R.moving_average_eval, 3600000
    else:
        fn, sl = (R.buffered_eval if mode == 'buffered' else R.moving_average_eval), 128
    logits = fn(R._Args(), m, spec, sl, 32, tok, use_tqdm=False, return_numpy=False)
    for a in att: a.left_window = a.right_window = -1
    blank = m.decoder.num_classes - 1
    ref = AR.ctc_align(logits[None].float(), torch.tensor([tok.encode(text)], dtype=torch.int32), None, None, blank)
    sec = m.subsampling.subsampling_factor * audio_tools.HOP_LENGTH / audio_tools.SR
    assert times[-1] <= logits.shape[0] * sec + 0.005                      # within the recording: its last log-prob frame ends here
    assert [(w['startTime'], w['endTime']) for w in words] == [(f'{f * sec:.2f}s', f'{l * sec:.2f}s') for f, l in ref.spans[0].tolist()]
    assert R.align_waveform(m, wave, text, tok, 128, 32, evaluation_mode=mode) == words
    assert R.align_waveform(m, torch.stack([wave, -wave]), text, tok, 128, 32, evaluation_mode=mode) == words        # left channel
    with pytest.raises(ValueError, match=rf'transcript of {2 * logits.shape[0]} labels cannot be emitted in {logits.shape[0]} frames'):
        R.align(m, spec, tok.decode([1, 2] * logits.shape[0]), tok, 128, 32, evaluation_mode=mode)
    with pytest.raises(ValueError, match='evaluation_mode'):
        R.evaluate(m, [('r', spec, 't1')], tok, 128, 32, evaluation_mode='beam')
    with pytest.raises(ValueError, match='evaluation_mode'):
        R.align(m, spec, text, tok, 128, 32, evaluation_mode='beam')
