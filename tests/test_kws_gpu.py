"""CTC keyword search on the device (csrc/kws.hip through lcasr_amd.hip.kws and decoding/kws.py).

The contract is bit-exact: on every case here the device gives the bits of kws_refs.search32 - the header's formulas per keyword in
np.float32 - frames, scores and counts alike.  Shapes are the smallest at which the kernels can go wrong: frame counts around the
prefetch depth, a ragged batch with a length 0, classes on both sides of the gather's geometries (16 lanes | a wave | a workgroup per
row) with and without 16-byte loads, U = 1, 4, 5 columns, keywords that end on lane 63, more waves than a workgroup holds, and one
sample long enough that a start frame passes 65536."""
import math
import re

import numpy as np
import pytest
import torch

import kws_refs as KR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def D():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from lcasr_amd.decoding import kws
    kws.kws_kernels.load()
    return kws


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _device(D, x, ks, blank, lengths=None, cap=4, classes=None):
    il = None if lengths is None else torch.tensor(lengths, dtype=torch.int32).cuda()
    out = D.kws_kernels.search(torch.from_numpy(x).cuda(), ks.device_image('cuda'), ks.n_waves, ks.U, ks.K, blank, il, cap, classes)
    return tuple(t.cpu().numpy() for t in out)


def _check(D, x, phrases, per_label, blank, lengths=None, cap=4, classes=None, hits_wanted=True):
    """The device against search32, bit for bit; returns the device's outputs."""
    ks = phrases if isinstance(phrases, D.KeywordSet) else D.KeywordSet(phrases, per_label)
    got = _device(D, x, ks, blank, lengths, cap, classes)
    want = KR.search32(x, ks.phrases, ks.thresholds, blank, lengths, cap, classes)
    for name, g, w in zip(('hit_frames', 'hit_score', 'hit_count'), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(_bits(g), _bits(w)), name
    assert not hits_wanted or int(want[2].sum()) > 0
    return got


PHRASES8 = [(0, 1), (2,), (3, 3), (1, 0, 2), (4, 5, 4, 6)]                  # labels of 8 classes, the blank 7


@pytest.mark.parametrize('n', ['1', 'G-1', 'G', 'G+1', '2G+1'])
def test_frame_counts_around_the_prefetch_depth(D, n):
    G = D.kws_kernels.prefetch()
    N = {'1': 1, 'G-1': G - 1, 'G': G, 'G+1': G + 1, '2G+1': 2 * G + 1}[n]
    _check(D, KR.random_case(N, 2, N, 8), PHRASES8, -6.0, 7, [N, max(N - 1, 1)])


def test_ragged_batch_with_a_length_zero(D):
    f, s, c = _check(D, KR.random_case(2, 3, 37, 8), PHRASES8, -5.0, 7, [37, 0, 20])
    assert not c[1].any() and (f[1] == -1).all() and (s[1] == -math.inf).all()


@pytest.mark.parametrize('classes,pad', [(8, 0), (8, 15), (129, 0), (129, 15), (257, 0), (257, 3), (1025, 0), (1025, 3), (4097, 0), (4097, 3)])
def test_classes_across_the_gathers_geometries(D, classes, pad):
    """Rows of C = classes + pad floats, NaN behind `classes`: each class count with rows that allow 16-byte loads (C a multiple
    of 4) and with rows that do not; an invalid row of each kind sits in the middle."""
    N = 64 if classes > 144 else 23
    x = np.full((2, N, classes + pad), np.nan, dtype=np.float32)
    x[..., :classes] = KR.random_case(classes, 2, N, classes, scale=1.0)
    x[0, 5, classes - 1] = np.nan; x[1, 7, 0] = np.inf; x[1, 11, :classes] = -np.inf
    labels = list(range(0, classes - 1, max(1, classes // 9)))
    _check(D, x, KR.random_phrases(classes, 10, labels, 1, 3), -2.0 * math.log(classes), classes - 1, [N, N - 3], classes=classes)


@pytest.mark.parametrize('U,phrases', [(1, [(2,), (2,)]), (4, [(0, 1), (2,), (1, 2, 0)]), (5, [(0, 1), (2,), (3, 3), (1, 0, 2)])])
def test_columns(D, U, phrases):
    ks = D.KeywordSet(phrases, -5.0)
    assert ks.U == U
    _check(D, KR.random_case(U, 1, 30, 8), ks, None, 7)


def test_packing(D):
    x = KR.random_case(4, 1, 20, 40, scale=1.5)
    full = D.KeywordSet([(i % 39,) for i in range(64)], -2.0)
    edge = D.KeywordSet([(0,)] * 61 + [(1, 2), (3, 4)], -2.5)                # a keyword ends exactly on lane 63; the next opens a wave
    longest = D.KeywordSet([tuple(i % 39 for i in range(32)), (1, 2)], -4.0)
    many = D.KeywordSet(KR.random_phrases(8, 150, list(range(39)), 1, 4), -2.5)      # more waves than one workgroup holds
    assert (full.n_waves, edge.n_waves, longest.n_waves) == (1, 2, 2) and many.n_waves > 4
    for ks in (full, edge, many):
        _check(D, x, ks, None, 39)
    x = KR.random_case(5, 1, 90, 40, scale=0.25)                             # 32 labels need 32 frames and more
    _check(D, x, longest, None, 39, cap=2)


@pytest.mark.parametrize('gap', [[], [(6,)]])
def test_a_hot_neighbour_does_not_leak(D, gap):
    """A keyword whose last state is hot (its labels are the arg-max of most frames) ends on lane j; a second keyword starts on lane
    j + 1 (gap []) or j + 2 (one one-label keyword between).  The second's hits are bit-equal to the hits it has alone."""
    x = KR.random_case(6, 1, 50, 8)
    x[0, ::2, 0] += 9; x[0, 1::2, 1] += 9                                    # 0 1 0 1 .. wins almost every frame
    hot, second = (0, 1), (2, 3, 2)
    alone = _check(D, x, [second], -12.0, 7, cap=6)                          # (a threshold the second reaches inside the hot frames too)
    both = _check(D, x, [hot] + gap + [second], -12.0, 7, cap=6)
    assert int(both[2][0, 0]) > 5                                           # the neighbour is hot indeed
    assert all(np.array_equal(_bits(b[:, -1]), _bits(a[:, 0])) for a, b in zip(alone, both))


def test_start_frames_are_full_int32(D):
    """N = 70000: a hit planted past frame 65536 keeps its start."""
    N = 70000
    x = np.full((1, N, 8), -8.0, dtype=np.float32)
    x[0, :, 0] = 0
    x[0, 66000:66004, 0] = -8; x[0, 66000:66003, 1] = 0; x[0, 66003, 2] = 0
    f, s, c = _check(D, x, [(1, 2)], -1.0, 7)
    assert int(c[0, 0]) == 1 and f[0, 0, 0].tolist() == [66000, 66004] and float(s[0, 0, 0]) == 0.0


def _rows(C, *frames):
    x = np.full((1, len(frames), C), -8.0, dtype=np.float32)
    for t, f in enumerate(frames):
        for c, v in f.items(): x[0, t, c] = v
    return x


def test_exact_ties(D):
    """The tie cases of tests/test_kws.py on the device: equal scores go to the smaller start, and the first end that reaches a score
    keeps it."""
    x = _rows(4, {2: 0}, {2: 0}, {0: 0}, {0: 0}, {3: 0}, {1: 0}, {1: 0}, {2: 0})
    f, s, c = _check(D, x, [(0, 1), (0,), (1,)], -1.0, 3)
    assert f[0, :, 0].tolist() == [[2, 6], [2, 3], [5, 6]] and s[0, :, 0].tolist() == [0.0] * 3 and c[0].tolist() == [1, 1, 1]
    f, s, c = _check(D, _rows(4, {0: 0}, {0: 0}, {0: 0}), [(0, 0)], -10.0, 3)
    assert f[0, 0, 0].tolist() == [0, 3] and float(s[0, 0, 0]) == -8.0
    x = _rows(4, {0: -1, 1: 0}, {0: -0.5, 1: 0})
    f, s, c = _check(D, x, [(0,)], -3.0, 3)
    assert f[0, 0, :2].tolist() == [[0, 1], [1, 2]] and s[0, 0, :2].tolist() == [-1.0, -0.5]
    _check(D, KR.exact_case(9, 2, 40, 8), PHRASES8, -1.5, 7)                 # multiples of 1/8: ties everywhere
    x = _rows(4, *([{0: 0.0, 1: -0.0}] * 3))                                 # a maximum that is both +0 and -0: the two tie, scores are +0
    f, s, c = _check(D, x, [(0, 1), (1, 0), (1,)], -1.0, 3)
    assert f[0, :, 0].tolist() == [[0, 2], [0, 2], [0, 1]] and not np.signbit(s[0, :, 0]).any()


def test_two_calls_are_bit_equal(D):
    x = KR.random_case(12, 2, 45, 8)
    ks = D.KeywordSet(PHRASES8, -5.0)
    a, b = _device(D, x, ks, 7), _device(D, x, ks, 7)
    assert all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(a, b))


def test_cap_and_one_more(D):
    x = _rows(4, *([{0: 0}, {1: 0}] * 5))                                    # five hits of label 0
    f, s, c = _check(D, x, [(0,)], -1.0, 3, cap=5)
    assert int(c[0, 0]) == 5 and f[0, 0].tolist() == [[0, 1], [2, 3], [4, 5], [6, 7], [8, 9]]
    f, s, c = _check(D, x, [(0,)], -1.0, 3, cap=4)
    assert int(c[0, 0]) == 5 and f[0, 0].tolist() == [[0, 1], [2, 3], [4, 5], [6, 7]]
    f, s, c = _check(D, x, [(0,)], -1.0, 3, cap=7)
    assert f[0, 0, 5:].tolist() == [[-1, -1]] * 2 and s[0, 0, 5:].tolist() == [-math.inf] * 2


def test_the_planted_case(D):
    """Asserted on search64 first, then on the device: the four real occurrences at their planted frames, not the broken one, and
    nothing for a keyword that never occurs."""
    x, blank, real, broken = KR.planted_case()
    ks = D.KeywordSet([KR.PLANTED_KEYWORD, KR.ABSENT_KEYWORD], -1.0)
    f, s, c, _ = KR.search64(x, ks.phrases, ks.thresholds, blank, None, 8)
    assert c.tolist() == [[4, 0]] and [tuple(v) for v in f[0, 0, :4].tolist()] == real and broken not in real
    hits = D.ctc_keyword_search(torch.from_numpy(x[0]).cuda(), ks, blank, max_hits=8)
    assert hits.count.tolist() == [4, 0] and [tuple(v) for v in hits.frames[0, :4].tolist()] == real
    assert hits.score[0, :4].cpu().numpy() == pytest.approx(s[0, 0, :4], abs=1e-5)
    assert [(r['start'], r['end']) for r in hits.records()] == real
    _check(D, x, ks, None, blank, cap=8)


class IdTok:
    """Every token is a word: id i is spelt 't<i>'."""
    def __init__(self, V): self.V = V
    def vocab_size(self): return self.V
    def decode(self, ids): return ' '.join(f't{int(i)}' for i in ids)
    def encode(self, text): return [int(w[1:]) for w in text.split()]


def test_search_on_the_tiny_model(D):
    import audio_refs as AUD
    from common_model import build_from_fixture
    from conftest import load_golden
    from lcasr_amd.eval import run as R
    from lcasr_amd.utils import audio_tools as A
    fx = load_golden('infer_tiny')
    model = build_from_fixture(fx, device='cuda').eval()
    tok, blank = IdTok(int(fx['cfg.vocab_size'])), model.decoder.num_classes - 1
    wave = AUD.test_signal(3 * 16000, seed=3).cuda()
    spec = A.to_spectogram(wave[None])
    logits = R.moving_average_eval(R._Args(), model, spec, 128, 32, tok, use_tqdm=False, return_numpy=False)
    greedy = [int(c) for c in logits.argmax(-1).tolist()]
    runs = [c for i, c in enumerate(greedy) if c != blank and (i == 0 or greedy[i - 1] != c)]
    words = [tok.decode(runs[:2]), tok.decode(runs[1:2]), tok.decode([1, 2, 3])] if len(runs) >= 2 else ['t1', 't2', tok.decode([1, 2, 3])]
    recs = R.search(model, spec, words, tok, 128, 32, min_score_per_label=-6.0, max_hits=4)
    ks = D.KeywordSet.from_text(words, tok, -6.0)
    hits = D.ctc_keyword_search(logits, ks, blank, max_hits=4)
    sec = model.subsampling.subsampling_factor * A.HOP_LENGTH / A.SR
    assert recs and recs == hits.records(sec)
    for r, q in zip(recs, hits.records()):                                   # times are multiples of the frame period
        assert re.fullmatch(r'\d+\.\d\ds', r['startTime']) and r['startTime'] == f'{q["start"] * sec:.2f}s' and r['endTime'] == f'{q["end"] * sec:.2f}s'
    starts = [float(r['startTime'][:-1]) for r in recs]
    assert starts == sorted(starts) and all(r['score'] <= 0 for r in recs)
    want = KR.search32(logits.float().cpu().numpy()[None], ks.phrases, ks.thresholds, blank, None, 4)
    assert np.array_equal(hits.frames.cpu().numpy(), want[0][0]) and np.array_equal(_bits(hits.score.cpu().numpy()), _bits(want[1][0]))
    assert R.search_waveform(model, wave, words, tok, 128, 32, min_score_per_label=-6.0, max_hits=4) == recs
