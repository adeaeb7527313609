"""CPU tests of CTC keyword search: the numpy restatements (tests/kws_refs.py) against a brute force that shares nothing with them
and against each other, the behaviours the header states by hand, the lane packing of decoding/kws.py, the host side of the
fourteenth ABI unit (include/sconf_kws.h: header against binding, queries, refusals), the Python surface, and eval.run.search on the
tiny fixture model with the binding replaced by the restatement."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import eval_refs as E
import kws_refs as KR
from cabi_header import assert_binding_is_header, header_abi
from common_model import build_from_fixture
from conftest import ROOT, load_golden

HEADER, PREFIX = 'sconf_kws.h', 'sconf_kws_'
NAMES = {'sconf_kws_max_labels', 'sconf_kws_prefetch', 'sconf_kws_max_hits', 'sconf_kws_workspace', 'sconf_kws_search'}
NINF = -math.inf


@pytest.fixture
def emulated_kws(monkeypatch):
    """The binding layer (lcasr_amd.hip.kws.search) replaced by the lane-by-lane restatement: host logic without a GPU."""
    from lcasr_amd.decoding import kws as D
    monkeypatch.setattr(D.kws_kernels, 'search', KR.search)
    return D


def _same(a, b):
    return all(np.array_equal(p, q) for p, q in zip(a, b))


def _rows(C, *frames):
    """Log-scores (1, N, C): a frame is {class: value}; the classes it does not name hold -8."""
    x = np.full((1, len(frames), C), -8.0, dtype=np.float32)
    for t, f in enumerate(frames):
        for c, v in f.items(): x[0, t, c] = v
    return x


# ---- 1. the yardstick -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('blank', [0, 3, 7])
@pytest.mark.parametrize('repeats', [False, True])
def test_restatement_against_brute_force_on_exactly_representable_inputs(blank, repeats):
    """Multiples of 1/8: every sum is exact in f32 and f64, so the two restatements agree bit for bit, and E_t is the best over
    every start of an ordinary Viterbi with b_t the smallest such start."""
    labels = [c for c in range(8) if c != blank]
    n = 0
    for seed, N in enumerate((1, 2, 5, 17, 40)):
        x = KR.exact_case(seed, 1, N, 8)
        d = KR.llr(x[0], 8, np.float64)
        assert np.array_equal(d, KR.llr(x[0], 8, np.float32).astype(np.float64))
        phrases = KR.random_phrases(seed + 10, 6, labels, 1, 4, repeats) + [(labels[0],) * 3, (labels[1], labels[2], labels[1])]
        for p in phrases:
            ext, skip = KR._states(p, blank)
            E64, b64 = KR.walk(d[:, ext], skip, np.float64)
            E32, b32 = KR.walk(d[:, ext].astype(np.float32), skip, np.float32)
            Eb, bb = KR.brute(d, p, blank)
            live = np.isfinite(Eb)
            assert np.array_equal(E64, Eb) and np.array_equal(E32.astype(np.float64), Eb) and E32.dtype == np.float32
            assert np.array_equal(b64[live], bb[live]) and np.array_equal(b32[live], bb[live])
            n += int(live.sum())
        thr = [-1.5 * len(p) for p in phrases]
        a, b = KR.search32(x, phrases, thr, blank, None, 8), KR.search64(x, phrases, thr, blank, None, 8)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].astype(np.float64), b[1]) and np.array_equal(a[2], b[2])
    assert n > 300


def test_f32_against_f64_on_random_inputs():
    """A case whose smallest decision margin in float64 is under 1e-3 moves its seed on (decided here, on the CPU); every case kept
    gives the same hit frames in both precisions and scores within (n + 2) 2^-24 sum |llr| of the path (sum |llr| = -E)."""
    kept, seed = 0, 0
    while kept < 6:
        seed += 1
        assert seed < 200
        x = KR.random_case(seed, 2, 40, 8)
        phrases = KR.random_phrases(seed, 4, [0, 1, 2, 3, 4, 5, 6], 1, 4)
        thr = [-4.0 * len(p) for p in phrases]
        f64, s64, c64, margin = KR.search64(x, phrases, thr, 7, [40, 23], 8)
        if margin < 1e-3:
            continue
        f32, s32, c32 = KR.search32(x, phrases, thr, 7, [40, 23], 8)
        assert np.array_equal(f32, f64) and np.array_equal(c32, c64) and int(c64.sum()) > 0
        live = f64[..., 0] >= 0
        n = (f64[..., 1] - f64[..., 0])[live]
        assert (np.abs(s32[live].astype(np.float64) - s64[live]) <= (n + 2) * 2.0 ** -24 * -s64[live]).all()
        kept += 1


def test_the_lane_by_lane_walk_is_the_per_keyword_walk():
    """image_search32 (the image, lane by lane, as the kernel walks it) gives the bits of search32 (the formulas, per keyword)."""
    from lcasr_amd.decoding.kws import KeywordSet
    for seed in range(4):
        x = KR.random_case(seed, 3, 33, 12)
        x[0, 9] = np.nan; x[1, 4, 2] = np.inf; x[2, 20] = -np.inf
        phrases = KR.random_phrases(seed, 30, list(range(11)), 1, 6)
        ks = KeywordSet(phrases, -3.0)
        assert ks.n_waves > 1
        a = KR.search32(x, phrases, ks.thresholds, 11, [33, 0, 29], 4)
        assert _same(a, KR.image_search32(x, ks.image, ks.n_waves, ks.U, ks.K, 11, [33, 0, 29], 4))
        assert int(a[2].sum()) > 0 and not a[2][1].any()


# ---- 2. behaviours by hand --------------------------------------------------------------------------------------------------------
def _one(x, phrase, thr, blank, cap=4, lengths=None):
    f, s, c = KR.search32(x, [phrase], [thr], blank, lengths, cap)
    n = min(int(c[0, 0]), cap)
    return [tuple(v) for v in f[0, 0, :n].tolist()], s[0, 0, :n].tolist(), int(c[0, 0])


def test_the_argmax_keyword_scores_zero_from_its_first_frame():
    """C = 4 (labels 0 1 2, blank 3).  The keyword [0, 1] is the arg-max over [2, 6): 0 0 _ 1.  Every path over a sub-span scores 0
    too; the tie rule (the smaller start) gives the start 2, and the first frame that reaches the score keeps the end."""
    x = _rows(4, {2: 0}, {2: 0}, {0: 0}, {0: 0}, {3: 0}, {1: 0}, {1: 0}, {2: 0})
    assert _one(x, (0, 1), -1.0, 3) == ([(2, 6)], [0.0], 1)
    assert _one(x, (0,), -1.0, 3) == ([(2, 3)], [0.0], 1)                   # one label: its first frame, the longer ones tie and lose
    assert _one(x, (1,), -1.0, 3) == ([(5, 6)], [0.0], 1)


def test_a_maximum_of_both_zeros():
    """A row whose maximum is +0 in one class and -0 in another: the two tie (llr 0 for both) and no score is -0."""
    x = _rows(4, *([{0: 0.0, 1: -0.0}] * 3))
    f, s, c = KR.search32(x, [(0, 1), (1, 0), (1,)], [-2.0, -2.0, -1.0], 3, None, 4)
    assert f[0, :, 0].tolist() == [[0, 2], [0, 2], [0, 1]] and not np.signbit(s[0, :, 0]).any() and (s[0, :, 0] == 0).all()


def test_a_doubled_label_needs_its_blank():
    x = _rows(4, {0: 0}, {0: 0}, {0: 0})
    assert _one(x, (0, 0), -20.0, 3) == ([(0, 3)], [-8.0], 1)               # 0 _ 0: the blank's -8 is paid
    x = _rows(4, {0: 0}, {3: 0}, {0: 0})
    assert _one(x, (0, 0), -20.0, 3) == ([(0, 3)], [0.0], 1)
    x = _rows(4, {0: 0}, {1: 0})
    assert _one(x, (0, 1), -20.0, 3) == ([(0, 2)], [0.0], 1)                # two different labels skip it
    assert _one(x, (0, 0), -20.0, 3)[2] == 0                                # two frames do not hold 0 _ 0


def test_non_maximum_suppression():
    """One label, class 0, threshold -3: every frame at or above it is a candidate [t, t + 1) or longer."""
    # overlapping worse: [0, 1) scores 0, [0, 2) scores -1 and begins inside it
    assert _one(_rows(4, {0: 0}, {0: -1, 1: 0}, {1: 0}), (0,), -3.0, 3) == ([(0, 1)], [0.0], 1)
    # overlapping better: 0 _ 0' where the first candidate is worse than a later one that begins before its end
    x = _rows(4, {0: -2, 1: 0}, {3: 0}, {0: 0})
    assert _one(x, (0, 0), -3.0, 3) == ([(0, 3)], [-2.0], 1)
    x = _rows(4, {0: -1, 1: 0}, {0: 0}, {1: 0})                              # [0, 1) at -1, then [1, 2) at 0: adjacent, both stay
    assert _one(x, (0,), -3.0, 3) == ([(0, 1), (1, 2)], [-1.0, 0.0], 2)
    x = _rows(4, {0: -1, 1: 0}, {0: -0.5, 1: 0})                             # [0, 2) at -1.5 against [1, 2) at -0.5: the later start wins the cell
    assert _one(x, (0,), -3.0, 3) == ([(0, 1), (1, 2)], [-1.0, -0.5], 2)
    # a better candidate that overlaps replaces cur: 0 1 with the 1 growing better
    x = _rows(4, {0: 0}, {1: -2, 0: 0}, {1: 0, 0: -1}, {2: 0})
    assert _one(x, (0, 1), -3.0, 3) == ([(0, 3)], [0.0], 1)
    # the last one is emitted at the end of the sample
    x = _rows(4, {1: 0}, {1: 0}, {0: 0})
    assert _one(x, (0,), -3.0, 3) == ([(2, 3)], [0.0], 1)
    assert _one(x, (0,), -3.0, 3, lengths=[2])[2] == 0


def test_cap_and_one_more():
    x = _rows(4, *([{0: 0}, {1: 0}] * 5))                                    # five hits of label 0
    hits, _, n = _one(x, (0,), -1.0, 3, cap=5)
    assert n == 5 and hits == [(0, 1), (2, 3), (4, 5), (6, 7), (8, 9)]
    f, s, c = KR.search32(x, [(0,)], [-1.0], 3, None, 4)
    assert int(c[0, 0]) == 5 and f[0, 0].tolist() == [[0, 1], [2, 3], [4, 5], [6, 7]] and s[0, 0].tolist() == [0.0] * 4
    f, s, c = KR.search32(x, [(0,)], [-1.0], 3, None, 7)
    assert f[0, 0, 5:].tolist() == [[-1, -1]] * 2 and s[0, 0, 5:].tolist() == [NINF] * 2


@pytest.mark.parametrize('poison', [math.nan, math.inf, 'all -inf'])
def test_an_invalid_row_kills_the_paths_across_it(poison):
    frames = [{0: 0}, {0: 0}, {1: 0}, {1: 0}]
    x = _rows(4, *frames)
    assert _one(x, (0, 1), -1.0, 3) == ([(0, 3)], [0.0], 1)
    if poison == 'all -inf': x[0, 1] = -np.inf
    else: x[0, 1, 2] = poison
    assert _one(x, (0, 1), -1.0, 3)[2] == 0                                  # 0 at frame 0 cannot reach the 1 at frame 2
    assert _one(x, (0,), -1.0, 3) == ([(0, 1)], [0.0], 1) and _one(x, (1,), -1.0, 3) == ([(2, 3)], [0.0], 1)


def test_length_zero_and_columns_behind_classes():
    x = KR.random_case(3, 2, 12, 8)
    f, s, c = KR.search32(x, [(0, 1), (2,)], [-50.0, -50.0], 5, [0, 12], 3, classes=6)
    assert not c[0].any() and (f[0] == -1).all() and (s[0] == NINF).all() and c[1].all()
    y = x.copy(); y[..., 6:] = np.nan
    assert _same((f, s, c), KR.search32(y, [(0, 1), (2,)], [-50.0, -50.0], 5, [0, 12], 3, classes=6))


def test_a_keyword_beside_another_gives_the_bits_it_gives_alone():
    from lcasr_amd.decoding.kws import KeywordSet
    x = KR.random_case(11, 1, 30, 8)
    hot, second = (0, 1), (2, 3, 2)
    alone = KeywordSet([second], -3.0)
    a = KR.image_search32(x, alone.image, alone.n_waves, alone.U, alone.K, 7, None, 6)
    for before in ([hot], [hot, (4,)], [(5,), hot]):
        both = KeywordSet(before + [second], -3.0)
        assert both.n_waves == 1
        b = KR.image_search32(x, both.image, both.n_waves, both.U, both.K, 7, None, 6)
        assert all(np.array_equal(p[:, -1], q[:, 0]) for p, q in zip(b, a)) and int(a[2].sum()) > 0


# ---- 3. packing -----------------------------------------------------------------------------------------------------------------
def test_packing():
    from lcasr_amd.decoding.kws import FIRST, LAST, SKIP, KeywordSet, MAX_LABELS
    ks = KeywordSet([(i % 5,) for i in range(64)], -1.0)
    assert (ks.n_waves, ks.U, ks.K) == (1, 5, 64) and (ks.lanes[:, 1] == FIRST | LAST).all() and ks.lanes[:, 2].tolist() == list(range(64))
    assert KeywordSet([(i % 5,) for i in range(65)], -1.0).n_waves == 2
    # 61 lanes of one-label keywords, then a 2-label keyword on the lanes 61 .. 63: it ends exactly on lane 63; the next opens a wave
    ks = KeywordSet([(0,)] * 61 + [(1, 2), (3, 4)], -1.0)
    assert ks.n_waves == 2 and ks.lanes[61:64, 2].tolist() == [61] * 3 and ks.lanes[63, 1] == LAST | SKIP and ks.lanes[64:67, 2].tolist() == [62] * 3
    assert (ks.lanes[67:, 0] == -1).all() and ks.columns.tolist() == [0, 1, 2, 3, 4, -1]
    # one lane short: the keyword does not straddle, lane 63 idles
    ks = KeywordSet([(0,)] * 62 + [(1, 2)], -1.0)
    assert ks.n_waves == 2 and ks.lanes[62:64, 0].tolist() == [-1, -1] and ks.lanes[64, 1] == FIRST
    ks = KeywordSet([tuple(range(MAX_LABELS)), (1, 2)], -0.25)
    assert MAX_LABELS == 32 and ks.n_waves == 2 and (ks.lanes[:63, 2] == 0).all() and ks.lanes[63, 0] == -1 and ks.lanes[64, 2] == 1
    assert ks.thresholds.tolist() == [-8.0, -0.5] and KeywordSet([tuple(range(MAX_LABELS)), (1,)], -0.25).n_waves == 1
    with pytest.raises(ValueError, match='33 labels'):
        KeywordSet([tuple(range(33))])
    # states, flags and columns of one keyword with a repeat: 4 4 5 -> 4 _ 4 _ 5, SKIP on the last state only
    ks = KeywordSet([(4, 4, 5)], -1.0)
    assert ks.columns.tolist() == [4, 5, -1] and ks.lanes[:5, 0].tolist() == [0, 2, 0, 2, 1] and ks.lanes[:5, 1].tolist() == [FIRST, 0, 0, 0, SKIP | LAST]
    assert KeywordSet([(4,), (4,)], -1.0).U == 1                            # no blank column where no keyword needs one
    one = KeywordSet([(1, 2), (3,)], -1.0, one_per_wave=True)
    assert one.n_waves == 2 and one.lanes[64, 2] == 1


def test_validate_refuses_each_malformed_image_by_cause():
    from lcasr_amd.decoding.kws import FIRST, LAST, SKIP, KeywordSet
    good = KeywordSet([(1, 2), (3, 3), (4,)], -1.0)
    nw, U, K = good.n_waves, good.U, good.K

    def broken(match, edit=None, **sizes):
        image = good.image.copy()
        if edit: edit(image[:nw * 256].reshape(-1, 4), image[nw * 256:])
        with pytest.raises(ValueError, match=match):
            KeywordSet.from_image(image, **{**dict(n_waves=nw, U=U, K=K), **sizes})

    KeywordSet.from_image(good.image, nw, U, K)
    broken('do not hold', U=U + 1)
    broken('do not hold', n_waves=0)
    broken('column index out of range', lambda ln, c: ln.__setitem__((1, 0), U))
    broken('column index out of range', lambda ln, c: ln.__setitem__((1, 0), -2))
    broken('keyword index out of range', lambda ln, c: ln.__setitem__((6, 2), K))
    broken('flags', lambda ln, c: ln.__setitem__((0, 1), 8))
    broken('flags on an idle lane', lambda ln, c: ln.__setitem__((20, 1), LAST))
    broken('no FIRST lane opens', lambda ln, c: ln.__setitem__((0, 1), 0))
    broken('not closed by a LAST lane', lambda ln, c: ln.__setitem__((2, 1), SKIP))
    broken('an odd number', lambda ln, c: (ln.__setitem__((1, 1), LAST), ln.__setitem__((2, 1), FIRST | LAST)))
    broken('SKIP exactly', lambda ln, c: ln.__setitem__((5, 1), SKIP | LAST))          # 3 _ 3 must not skip its blank
    broken('SKIP exactly', lambda ln, c: ln.__setitem__((2, 1), LAST))
    broken('labels on even states', lambda ln, c: ln.__setitem__((1, 0), 0))
    broken('single finite threshold', lambda ln, c: ln.__setitem__((2, 3), 0x7f800000))
    broken('single finite threshold', lambda ln, c: ln.__setitem__((6, 3), -1))         # a NaN's bits
    broken('present 2 times', lambda ln, c: ln.__setitem__((6, 2), 0))
    broken('not distinct', lambda ln, c: c.__setitem__(0, 2))
    with pytest.raises(ValueError, match='holds the blank'):
        good.validate(blank=3)
    with pytest.raises(ValueError, match='the model has 4 classes'):
        good.validate(num_classes=4)
    good.validate(blank=5, num_classes=6)


# ---- 4. the Python surface --------------------------------------------------------------------------------------------------------
class IdTok:
    """Every token is a word: id i is spelt 't<i>'."""
    def __init__(self, V): self.V = V
    def vocab_size(self): return self.V
    def decode(self, ids): return ' '.join(f't{int(i)}' for i in ids)
    def encode(self, text): return [int(w[1:]) for w in text.split()]


def test_keyword_set_errors_and_from_text():
    from lcasr_amd.decoding.kws import KeywordSet
    for bad, match in (([], 'empty list'), ([[]], 'empty phrase'), ([[1, -2]], 'negative label')):
        with pytest.raises(ValueError, match=match):
            KeywordSet(bad)
    for v in (math.nan, math.inf, -math.inf):
        with pytest.raises(ValueError, match='finite'):
            KeywordSet([[1]], min_score_per_label=v)
    with pytest.raises(ValueError, match='finite'):
        KeywordSet([[1] * 20], min_score_per_label=-3e38)                   # finite per label, not as a float32 total
    tok = IdTok(32)
    ks = KeywordSet.from_text(['t3 t7', 't5'], tok, min_score_per_label=-2.0)
    assert ks.phrases == [(3, 7), (5,)] and ks.words == ['t3 t7', 't5'] and ks.thresholds.tolist() == [-4.0, -2.0] and ks.name(1) == 't5'
    assert KeywordSet([(3, 7)]).name(0) == 0 and 'not tuned' in ' '.join(KeywordSet.__doc__.lower().split())
    with pytest.raises(TypeError, match='not one string'):
        KeywordSet.from_text('t3 t7', tok)
    with pytest.raises(ValueError, match='encodes to no token'):
        KeywordSet.from_text(['t1', ''], tok)
    assert ks.to('cpu') is ks and torch.equal(ks.device_image('cpu'), torch.from_numpy(ks.image))


def test_search_wrapper_and_records(emulated_kws):
    D = emulated_kws
    x, blank, real, broken = KR.planted_case()
    lp = torch.from_numpy(x)
    ks = D.KeywordSet([KR.PLANTED_KEYWORD, KR.ABSENT_KEYWORD], -1.0)
    one = D.ctc_keyword_search(lp[0], ks, blank, max_hits=8)
    assert one.frames.shape == (2, 8, 2) and one.score.shape == (2, 8) and one.count.tolist() == [4, 0]
    recs = one.records()
    assert [(r['start'], r['end']) for r in recs] == real and {r['keyword'] for r in recs} == {0} and all(set(r) == {'keyword', 'start', 'end', 'score'} for r in recs)
    assert [r['score'] for r in recs] == one.score[0, :4].tolist()
    timed = one.records(0.04)
    assert [(r['startTime'], r['endTime']) for r in timed] == [(f'{a * 0.04:.2f}s', f'{b * 0.04:.2f}s') for a, b in real]
    two = D.ctc_keyword_search(torch.cat([lp, lp]), [KR.PLANTED_KEYWORD], blank, input_lengths=[lp.shape[1], real[1][1]], max_hits=3)
    assert two.count.tolist() == [[4], [2]] and two.frames.shape == (2, 1, 3, 2)
    r0, r1 = two.records()
    assert len(r0) == 3 and all(r.get('truncated') is True for r in r0) and len(r1) == 2 and not any('truncated' in r for r in r1)
    with pytest.raises(ValueError, match='holds the blank'):
        D.ctc_keyword_search(lp[0], ks, KR.PLANTED_KEYWORD[1])
    with pytest.raises(ValueError, match='classes'):
        D.ctc_keyword_search(lp[0], ks, blank, classes=12)
    with pytest.raises(ValueError, match='classes = 40'):
        D.ctc_keyword_search(lp[0], ks, blank, classes=40)
    with pytest.raises(ValueError):
        D.ctc_keyword_search(lp[0, 0], ks, blank)


def test_a_cpu_tensor_is_refused_by_the_product_path():
    from lcasr_amd.decoding.kws import ctc_keyword_search
    x, blank, _, _ = KR.planted_case()
    with pytest.raises(RuntimeError, match='GPU'):
        ctc_keyword_search(torch.from_numpy(x[0]), [KR.PLANTED_KEYWORD], blank)


def test_planted_case_with_the_restatement():
    """What the GPU test asserts on the device: with a threshold between them the four real occurrences are found at their planted
    frames, the one with a missing label is not, and a keyword that never occurs gives no hit."""
    x, blank, real, broken = KR.planted_case()
    assert 380 <= x.shape[1] <= 460 and x.shape[2] == 32 and len(real) == 4
    f, s, c, _ = KR.search64(x, [KR.PLANTED_KEYWORD, KR.ABSENT_KEYWORD], [-3.0, -3.0], blank, None, 8)
    assert c.tolist() == [[4, 0]] and [tuple(v) for v in f[0, 0, :4].tolist()] == real
    weak = math.log(0.45 / 0.55)
    assert s[0, 0, :4] == pytest.approx([0.0, 2 * weak, 0.0, weak], abs=1e-6)
    ext, skip = KR._states(KR.PLANTED_KEYWORD, blank)                        # the broken one is there, far below the threshold
    E, st = KR.walk(KR.llr(x[0], 32, np.float64)[:, ext], skip, np.float64)
    assert st[broken[1] - 1] == broken[0] and -20.0 < E[broken[1] - 1] < -8.0


# ---- 5. host side of the unit -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from lcasr_amd.hip import kws
    return kws.load()


def _declared():
    src = open(os.path.join(ROOT, 'include', HEADER)).read()
    return sorted(set(re.findall(r'\b(sconf_kws_[a-z0-9_]+) ?\(', re.sub(r'/\*.*?\*/', '', src, flags=re.S))))


def test_binding_is_the_header_and_the_core_does_not_name_it(lib):
    from lcasr_amd.hip import _lib, kws
    funcs, enums = header_abi(HEADER, PREFIX)
    assert sorted(funcs) == _declared() and set(funcs) == NAMES
    assert enums == {'SCONF_KWS_FIRST': kws.FIRST, 'SCONF_KWS_SKIP': kws.SKIP, 'SCONF_KWS_LAST': kws.LAST} == {'SCONF_KWS_FIRST': KR.FIRST, 'SCONF_KWS_SKIP': KR.SKIP, 'SCONF_KWS_LAST': KR.LAST}
    assert_binding_is_header(funcs, kws.PROTOTYPES, kws.PLAIN, 'hip/kws.py')
    assert not any(n.startswith(PREFIX) for n in list(_lib.PROTOTYPES) + list(_lib.PLAIN))
    for n in NAMES:
        assert hasattr(lib, n) and n in _lib.bound()
    for path in (os.path.join(ROOT, 'long-context-asr_amd', 'hip', '_lib.py'), os.path.join(ROOT, 'include', 'sconf.h'),
                 os.path.join(ROOT, 'long-context-asr_amd', 'hip', '__init__.py')):
        assert PREFIX not in open(path).read() and not re.search(r'\bkws\b', open(path).read()), path
    hip = os.path.join(ROOT, 'long-context-asr_amd', 'hip')
    for f in sorted(os.listdir(hip)):                                        # nothing under hip/ imports this unit
        if f.endswith('.py') and f != 'kws.py':
            assert not re.search(r'import kws\b|from \.kws\b|from \. import [^\n]*\bkws\b', open(os.path.join(hip, f)).read()), f
    assert lib.sconf_version() == 220


def test_queries_answer_on_the_host(lib):
    from lcasr_amd.hip import kws
    assert lib.sconf_kws_max_labels() == 32 == kws.MAX_LABELS == kws.max_labels()
    G = lib.sconf_kws_prefetch()
    assert G == kws.prefetch() and 2 <= G <= 32
    assert lib.sconf_kws_max_hits() == kws.max_hits() >= 64
    ws = lib.sconf_kws_workspace
    for B, N, U, pad in ((1, 1, 1, 4), (3, 100, 4, 4), (2, 45000, 5, 8), (1, 70000, 250, 252)):
        assert ws(B, N, U) == -(-4 * B * N * pad // 256) * 256 == kws.kws_workspace(B, N, U)
    for bad in ((0, 10, 3), (1, 0, 3), (1, 10, 0), (1 << 16, 10, 3), (1 << 15, 1 << 16, 3), (1, 10, (1 << 20) + 1)):
        assert ws(*bad) == -1
    with pytest.raises(ValueError):
        kws.kws_workspace(1, 10, 0)


def test_refusals_launch_nothing(lib):
    """Every refusal happens before a kernel is enqueued, so none needs a GPU: the pointers are host addresses that are never read."""
    one = ctypes.c_void_p(16)
    need = lib.sconf_kws_workspace(2, 10, 3)
    err = lib.sconf_last_error

    def call(x=one, image=one, frames=one, score=one, count=one, wsp=one, n_waves=1, U=3, K=2, cap=4, ws=need, B=2, N=10, C=8, classes=8, blank=7):
        return lib.sconf_kws_search(x, None, image, n_waves, U, K, frames, score, count, cap, wsp, ws, B, N, C, classes, blank, None)

    for null in ('x', 'image', 'frames', 'score', 'count', 'wsp'):
        assert call(**{null: None}) != 0 and b'null' in err(), null
    for k in ('B', 'N', 'K'):
        assert call(**{k: 0}) != 0 and b'sizes' in err(), k
    assert call(classes=0) != 0 and b'classes' in err()
    assert call(classes=9) != 0 and b'classes' in err()
    assert call(blank=-1) != 0 and b'blank' in err()
    assert call(blank=6, classes=6) != 0 and b'blank' in err()              # a blank behind `classes` is no class of the call
    assert call(cap=0) != 0 and b'cap' in err()
    assert call(cap=lib.sconf_kws_max_hits() + 1) != 0 and b'cap' in err()
    assert call(n_waves=0) != 0 and b'waves' in err()
    assert call(U=0) != 0 and b'columns' in err()
    assert call(ws=need - 1) != 0 and b'workspace' in err()
    assert call(B=1 << 16, ws=1 << 50) != 0 and b'sizes' in err()


# ---- 6. eval.run.search on the tiny fixture model -------------------------------------------------------------------------------
def test_search_on_the_tiny_model(emulated_ops, emulated_kws, monkeypatch):
    import audio_refs as AUD
    from lcasr_amd.eval import run as R
    from lcasr_amd.utils import audio_tools
    monkeypatch.setattr(audio_tools.audio, 'melspec', AUD.melspec)
    E.attach(monkeypatch, emulated_ops)
    fx = load_golden('infer_tiny')
    m = build_from_fixture(fx).eval()
    tok = IdTok(int(fx['cfg.vocab_size']))
    wave = AUD.test_signal(3 * 16000, seed=3)
    spec = audio_tools.to_spectogram(wave[None])
    logits = R.moving_average_eval(R._Args(), m, spec, 128, 32, tok, use_tqdm=False, return_numpy=False)
    blank = m.decoder.num_classes - 1
    greedy = [int(c) for c in logits.argmax(-1).tolist()]
    runs = [c for i, c in enumerate(greedy) if c != blank and (i == 0 or greedy[i - 1] != c)]
    words = [tok.decode(runs[:2]), tok.decode(runs[1:2]), tok.decode([1, 2, 3])] if len(runs) >= 2 else ['t1', 't2', tok.decode([1, 2, 3])]
    recs = R.search(m, spec, words, tok, 128, 32, min_score_per_label=-6.0, max_hits=4)
    ref = emulated_kws.ctc_keyword_search(logits, emulated_kws.KeywordSet.from_text(words, tok, -6.0), blank, max_hits=4)
    sec = m.subsampling.subsampling_factor * audio_tools.HOP_LENGTH / audio_tools.SR
    assert recs == ref.records(sec) and recs
    assert all(set(r) - {'truncated'} == {'keyword', 'startTime', 'endTime', 'score'} and r['keyword'] in words and r['score'] <= 0 for r in recs)
    assert all(re.fullmatch(r'\d+\.\d\ds', r[k]) for r in recs for k in ('startTime', 'endTime'))
    starts = [float(r['startTime'][:-1]) for r in recs]
    assert starts == sorted(starts)
    frames = [(r['start'], r['end']) for r in ref.records()]
    assert [(r['startTime'], r['endTime']) for r in recs] == [(f'{a * sec:.2f}s', f'{b * sec:.2f}s') for a, b in frames]
    if len(runs) >= 2:
        assert any(r['keyword'] == words[0] and r['score'] == 0.0 for r in recs)        # the greedy decode of its span
    assert R.search(m, spec, emulated_kws.KeywordSet.from_text(words, tok, -6.0), tok, 128, 32, max_hits=4) == recs
    assert R.search_waveform(m, wave, words, tok, 128, 32, min_score_per_label=-6.0, max_hits=4) == recs
    with pytest.raises(ValueError, match='evaluation_mode'):
        R.search(m, spec, words, tok, 128, 32, evaluation_mode='beam')
