"""CPU tests of CTC segmentation: the numpy restatement (tests/seg_refs.py) against the enumeration of every frame path and against a
direct double loop, the host side of the thirteenth ABI unit (include/sconf_seg.h: header against binding, queries, refusals),
build_targets, the wrappers of decoding/segment.py and eval.run.segment on the tiny fixture model with the binding replaced by the
restatement."""
import ctypes
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch

import align_refs as AR
import eval_refs as E
import seg_refs as SR
from cabi_header import assert_binding_is_header, header_abi
from common_model import build_from_fixture
from conftest import ROOT, load_golden

HEADER, PREFIX = 'sconf_seg.h', 'sconf_seg_'
NAMES = {'sconf_seg_star_label', 'sconf_seg_max_window', 'sconf_seg_score_tile', 'sconf_seg_workspace', 'sconf_seg_align', 'sconf_seg_score'}


@pytest.fixture
def emulated_seg(monkeypatch):
    """The binding layer (lcasr_amd.hip.seg.align / .score) replaced by the numpy restatement: host logic without a GPU."""
    from lcasr_amd.decoding import segment as D
    monkeypatch.setattr(D.seg_kernels, 'align', SR.align)
    monkeypatch.setattr(D.seg_kernels, 'score', SR.score)
    return D


# ---- 1. the yardstick ---------------------------------------------------------------------------------------------------------
def _star_rows(S, star, labels):
    """Every target of S entries over `labels` and the star, with at least one star: stars at every position."""
    return [t for t in itertools.product(list(labels) + [star], repeat=S) if star in t]


@pytest.mark.parametrize('star_logp', [0.0, -1.0])
def test_restatement_against_every_path_that_collapses_to_the_target(star_logp):
    """T <= 6, S <= 3, two labels, the blank and the star: the restated score is the best over every frame path of the extended
    alphabet that collapses to the target - the star's emission in the path score - and the restated path is one of the best."""
    C, blank, star = 3, 2, 3
    rng = np.random.default_rng(5)
    n = 0
    for T in range(1, 7):
        lp = torch.log_softmax(torch.from_numpy(rng.normal(size=(1, T, C)).astype(np.float32)) * 2, -1)
        lp = torch.cat([lp, lp[..., :1]], -1).contiguous()                  # C a multiple of 4 for the op; class 3 is never a label
        ext = SR.extend(lp[..., :C], star_logp)[0].numpy()                  # (T, 4): labels 0 1, blank 2, star 3
        for S in range(1, 4):
            for tgt in _star_rows(S, star, (0, 1)):
                best, arg = AR.brute_force(ext, tgt, blank)
                al = SR.align(lp[..., :C].contiguous(), torch.tensor([tgt], dtype=torch.int32), None, None, blank, star_logp)
                n += 1
                if not AR.feasible(T, tgt):
                    assert best == -np.inf and float(al.score) == -np.inf and bool((al.path == -1).all()) and not bool(al.frame_logp.any())
                    continue
                assert float(al.score) == pytest.approx(best, abs=1e-5)
                assert tuple(al.labels[0].tolist()) in arg or len(arg) > 1
                assert AR.collapse(al.labels[0].tolist(), blank) == list(tgt)
                assert float(al.frame_logp.double().sum()) == pytest.approx(best, abs=1e-5)
                for j, (f, l) in enumerate(al.spans[0].tolist()):
                    if tgt[j] == star:
                        assert l > f and float(al.token_logp[0, j]) == pytest.approx((l - f) * star_logp)
    assert n > 100


def test_star_ties_by_hand():
    """C = 4 (labels 0 1 2, blank 3), the star 4.  Log-probs in exact binary fractions so that ties are ties."""
    blank, star = 3, 4
    row = lambda *v: list(v)
    # 1. a free star beside a label whose frames are free too.  Target [0, *], states b 0 b * b; label 0 and the star emit 0, the
    #    blank -8.  Frame 1: the star's cell has one finite candidate, the skip from label 0 (step 2).  Frame 2: stay (0) and the
    #    skip (0) tie, the earlier candidate keeps the cell: stay.  End: the trailing blank holds -8, the star 0 > -8.  The walk back
    #    is star, star (entered by the skip at frame 1), label: of the three zero-cost paths the star takes two frames.
    lp = torch.tensor([[row(0.0, -8.0, -8.0, -8.0)] * 3])
    al = SR.align(lp, torch.tensor([[0, star]], dtype=torch.int32), None, None, blank, 0.0)
    assert float(al.score) == 0.0 and al.labels[0].tolist() == [0, star, star]
    assert al.spans[0].tolist() == [[0, 1], [1, 3]] and al.token_logp[0].tolist() == [0.0, 0.0] and al.frame_logp[0].tolist() == [0.0, 0.0, 0.0]
    # 2. the same with star_logp = -1: the label keeps every frame it can, the star its one obligatory frame
    al = SR.align(lp, torch.tensor([[0, star]], dtype=torch.int32), None, None, blank, -1.0)
    assert float(al.score) == -1.0 and al.labels[0].tolist() == [0, 0, star] and al.frame_logp[0].tolist() == [0.0, 0.0, -1.0]
    assert al.token_logp[0].tolist() == [0.0, -1.0]
    # 3. two adjacent stars are a repeat: a blank frame must part them, so 2 frames do not fit and 3 do
    lp = torch.tensor([[row(-8.0, -8.0, -8.0, -0.5)] * 3])
    two = torch.tensor([[star, star]], dtype=torch.int32)
    assert float(SR.align(lp[:, :2].contiguous(), two, None, None, blank, 0.0).score) == -np.inf
    al = SR.align(lp, two, None, None, blank, 0.0)
    assert al.labels[0].tolist() == [star, blank, star] and float(al.score) == -0.5
    # 4. a star between an equal pair of labels lifts the repeat: [1, *, 1] fits 3 frames, [1, 1] needs 3 as well but with a blank
    lp = torch.tensor([[row(-8.0, 0.0, -8.0, -8.0)] * 3])
    al = SR.align(lp, torch.tensor([[1, star, 1]], dtype=torch.int32), None, None, blank, -2.0)
    assert al.labels[0].tolist() == [1, star, 1] and float(al.score) == -2.0
    al = SR.align(lp, torch.tensor([[1, 1, 0]], dtype=torch.int32), None, torch.tensor([2], dtype=torch.int32), blank, -2.0)
    assert al.labels[0].tolist() == [1, blank, 1] and float(al.score) == -8.0
    # 5. the star is a label, not a class: label 5 poisons, label 4 does not; star_logp must be finite and <= 0
    bad = SR.align(lp, torch.tensor([[1, 5, 1]], dtype=torch.int32), None, None, blank, 0.0)
    assert math.isnan(float(bad.score)) and bool((bad.labels == -1).all()) and not bool(bad.frame_logp.any())
    for v in (0.5, math.nan, -math.inf):
        with pytest.raises(RuntimeError):
            SR.align(lp, two, None, None, blank, v)


def test_targets_without_a_star_are_the_plain_alignment():
    lp, tg = AR.random_case(3, 3, 30, 8, 6, in_len=[30, 22, 4], tg_len=[6, 3, 6], repeats=2)
    il, tl = torch.tensor([30, 22, 4], dtype=torch.int32), torch.tensor([6, 3, 6], dtype=torch.int32)
    a, b = SR.align(lp, tg, il, tl, 7, -1.0), AR.ctc_align(lp, tg, il, tl, 7)
    for x, y in zip(a[:5], b):
        assert torch.equal(x, y) or (bool(torch.isnan(x).any()) and torch.equal(torch.isnan(x), torch.isnan(y)))
    assert float(a.score[2]) == -np.inf and not bool(a.frame_logp[2].any()) and not bool(a.frame_logp[1, 22:].any())
    assert torch.equal(a.frame_logp[0], lp[0].gather(1, a.labels[0].long()[:, None])[:, 0])


def test_utterance_scores_against_a_direct_double_loop():
    rng = np.random.default_rng(9)
    B, N, Smax = 3, 70, 9
    g = torch.from_numpy(-rng.exponential(2.0, size=(B, N)).astype(np.float32))
    bounds = np.stack([np.sort(rng.choice(np.arange(0, N + 1), size=Smax + 1, replace=False)) for _ in range(B)])   # token j: [bounds[j], bounds[j + 1])
    spans = torch.from_numpy(np.stack([bounds[:, :-1], bounds[:, 1:]], -1).astype(np.int32))
    score = torch.tensor([-3.0, -math.inf, -7.5], dtype=torch.float64)
    utt = torch.tensor([[[0, 1], [1, 4], [0, 9], [4, 4], [5, 10]], [[0, 3]] * 5, [[2, 7], [6, 5], [-1, 3], [0, 9], [8, 9]]], dtype=torch.int32)
    counts = torch.tensor([5, 5, 4], dtype=torch.int32)
    for window in (1, 3, 30, 1000):
        out = SR.score(spans, g, score, None, None, utt, counts, window)
        for b in range(B):
            for u in range(5):
                got = (out.utt_frames[b, u].tolist(), float(out.utt_logp[b, u]), float(out.utt_conf[b, u]))
                j0, j1 = utt[b, u].tolist()
                if u >= int(counts[b]):
                    assert got == ([-1, -1], 0.0, 0.0)
                elif b == 1 or not 0 <= j0 < j1 <= Smax:
                    assert got[0] == [-1, -1] and math.isnan(got[1]) and math.isnan(got[2])
                else:
                    f0, f1 = int(spans[b, j0, 0]), int(spans[b, j1 - 1, 1])
                    n = f1 - f0
                    w = min(window, n)
                    vals = [float(x) for x in g[b, f0:f1]]
                    worst = min(math.fsum(vals[t:t + w]) / w for t in range(n - w + 1))          # the definition, every sum exact
                    assert got[0] == [f0, f1]
                    assert got[1] == pytest.approx(math.fsum(vals) / n, rel=2 ** -23) and got[2] == pytest.approx(worst, rel=2 ** -23)
                    assert got[2] <= got[1] + 1e-6 and (w < n or got[1] == got[2])


def test_planted_case_with_the_restatement():
    """The case the GPU test runs on the device: -1.0 recovers the planted spans exactly, 0.0 does not; without stars the score
    falls by more than the stars paid; a corrupted utterance has the lowest confidence and its mean moves less."""
    from lcasr_amd.decoding.segment import build_targets
    lp, utts, planted, gap_frames = SR.planted_case()
    C, blank = lp.shape[2], lp.shape[2] - 1

    def run(utterances, star_logp, stars=True, window=4):
        row, ranges = build_targets(utterances, C, stars, stars)
        al = SR.align(lp, torch.tensor([row], dtype=torch.int32), None, None, blank, star_logp)
        sc = SR.score(al.spans, al.frame_logp, al.score, None, None, torch.tensor([ranges], dtype=torch.int32), None, window)
        return al, sc

    al, sc = run(utts, -1.0)
    assert [tuple(x) for x in sc.utt_frames[0].tolist()] == planted
    assert sorted(torch.nonzero(al.labels[0] == C)[:, 0].tolist()) == gap_frames
    assert [tuple(x) for x in run(utts, 0.0)[1].utt_frames[0].tolist()] != planted
    plain, _ = run(utts, -1.0, stars=False)
    assert math.isfinite(float(plain.score)) and float(al.score) - float(plain.score) > len(gap_frames) * 1.0
    wrong = [utts[0], [utts[1][0], 6, 7] + utts[1][3:], utts[2]]
    _, sw = run(wrong, -1.0)
    assert int(sw.utt_conf[0].argmin()) == 1
    assert abs(float(sw.utt_logp[0, 1] - sc.utt_logp[0, 1])) < abs(float(sw.utt_conf[0, 1] - sc.utt_conf[0, 1]))


# ---- 2. build_targets and the wrappers ------------------------------------------------------------------------------------------
def test_build_targets():
    from lcasr_amd.decoding.segment import build_targets, star_id
    S = star_id(32)
    assert S == 32
    assert build_targets([[1, 2], [3], [4, 5, 6]], S) == ([S, 1, 2, S, 3, S, 4, 5, 6, S], [(1, 3), (4, 5), (6, 9)])
    assert build_targets([[1, 2], [3]], S, star_between=False) == ([S, 1, 2, 3, S], [(1, 3), (3, 4)])
    assert build_targets([[1, 2], [3]], S, star_ends=False) == ([1, 2, S, 3], [(0, 2), (3, 4)])
    assert build_targets([(1, 2), torch.tensor([3])], S, False, False) == ([1, 2, 3], [(0, 2), (2, 3)])
    assert build_targets([], S) == ([], [])
    with pytest.raises(ValueError, match='utterance 1 is empty'):
        build_targets([[1], [], [2]], S)
    with pytest.raises(ValueError):
        star_id(0)


def test_wrapper_shapes(emulated_seg):
    D = emulated_seg
    lp, utts, planted, _ = SR.planted_case()
    blank = lp.shape[2] - 1
    one = D.ctc_segment(lp[0], utts, blank, star_logp=-1.0, window=4)
    assert isinstance(one, D.CTCSegmentation) and one.utt_frames.shape == (3, 2) and one.utt_conf.shape == (3,) and one.alignment.score.shape == ()
    assert [tuple(x) for x in one.utt_frames.tolist()] == planted and one.frame_logp.shape == (lp.shape[1],)
    two = D.ctc_segment(torch.cat([lp, lp]), [utts, utts[:2]], blank, star_logp=-1.0, window=4)
    assert two.utt_frames.shape == (2, 3, 2) and torch.equal(two.utt_frames[0], one.utt_frames)
    assert two.utt_frames[1, 2].tolist() == [-1, -1] and float(two.utt_conf[1, 2]) == 0.0 and two.alignment.spans.shape[1] == 16
    row, _ = D.build_targets(utts, D.star_id(lp.shape[2]))
    a = D.ctc_forced_align_star(lp[0], row, blank=blank, star_logp=-1.0)
    assert a.path.shape == (lp.shape[1],) and torch.equal(a.spans, one.alignment.spans) and len(a) == 5
    with pytest.raises(ValueError, match='65535'):
        D.ctc_forced_align_star(lp[0], [0] * 65536, blank=blank)
    with pytest.raises(ValueError):
        D.ctc_segment(lp, [utts, utts], blank)
    with pytest.raises(ValueError):
        D.ctc_segment(lp[0, 0], utts, blank)


def test_a_cpu_tensor_is_refused_by_the_product_path():
    from lcasr_amd.decoding.segment import ctc_segment
    lp, utts, _, _ = SR.planted_case()
    with pytest.raises(RuntimeError, match='GPU'):
        ctc_segment(lp[0], utts, lp.shape[2] - 1)


# ---- 3. host side of the unit -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from lcasr_amd.hip import seg
    return seg.load()


def _declared():
    src = open(os.path.join(ROOT, 'include', HEADER)).read()
    return sorted(set(re.findall(r'\b(sconf_seg_[a-z0-9_]+) ?\(', re.sub(r'/\*.*?\*/', '', src, flags=re.S))))


def test_binding_is_the_header_and_the_core_does_not_name_it(lib):
    from lcasr_amd.hip import _lib, seg
    funcs, enums = header_abi(HEADER, PREFIX)
    assert sorted(funcs) == _declared() and set(funcs) == NAMES and not enums
    assert_binding_is_header(funcs, seg.PROTOTYPES, seg.PLAIN, 'hip/seg.py')
    assert not any(n.startswith(PREFIX) for n in list(_lib.PROTOTYPES) + list(_lib.PLAIN))
    for n in NAMES:
        assert hasattr(lib, n) and n in _lib.bound()
    for path in (os.path.join(ROOT, 'long-context-asr_amd', 'hip', '_lib.py'), os.path.join(ROOT, 'include', 'sconf.h')):
        assert PREFIX not in open(path).read(), path
    for mod in ('_lib', 'audio', 'align', 'beam', 'ops'):                   # what tests/test_cabi.py imports does not import this unit
        src = open(os.path.join(ROOT, 'long-context-asr_amd', 'hip', mod + '.py')).read()
        assert not re.search(r'import seg\b|from \.seg\b|from \. import [^\n]*\bseg\b', src), mod
    assert lib.sconf_version() == 220


def test_queries_answer_on_the_host(lib):
    from lcasr_amd.hip import align, align_long, seg
    assert lib.sconf_seg_star_label(32) == 32 == seg.star_label(32) and lib.sconf_seg_star_label(0) == -1
    W, tile = lib.sconf_seg_max_window(), lib.sconf_seg_score_tile()
    assert W == seg.max_window() and W >= 30 and tile == seg.score_tile() and tile >= 64 and tile % 64 == 0
    M = lib.sconf_lalign_max_labels()
    assert M == 65535 == seg.MAX_LABELS
    ws = lib.sconf_seg_workspace
    short = lib.sconf_align_max_labels()
    for B, N, S in ((1, 1, 0), (2, 100, 7), (3, 2048, 512), (1, 40, short)):
        assert ws(B, N, S, 0) == ws(B, N, S, 9) == lib.sconf_align_workspace(B, N, S) == seg.seg_workspace(B, N, S, 3)
    for B, N, S in ((1, 9000, short + 1), (2, 70000, M)):
        assert ws(B, N, S, 4) == lib.sconf_lalign_workspace(B, N, S, 0)
    for bad in ((0, 10, 10, 1), (1, 0, 10, 1), (1, 10, -1, 1), (1, 10, M + 1, 1), (1, 10, 10, -1), (1 << 16, 1 << 16, 10, 1)):
        assert ws(*bad) == -1
    with pytest.raises(ValueError):
        seg.seg_workspace(1, 10, M + 1)


def test_refusals_launch_nothing(lib):
    """Every refusal happens before a kernel is enqueued, so none needs a GPU: the pointers are host addresses that are never read."""
    one = ctypes.c_void_p(16)
    need = lib.sconf_seg_workspace(1, 10, 3, 2)
    al = lambda blank=31, ws=need, B=1, N=10, C=32, S=3, star=0.0: lib.sconf_seg_align(one, one, None, None, one, one, one, one, one, one, one, ws,
                                                                                      B, N, C, S, blank, star, None)
    assert al(star=0.5) != 0 and b'star_logp' in lib.sconf_last_error()
    assert al(star=1e-30) != 0 and b'star_logp' in lib.sconf_last_error()
    assert al(star=math.nan) != 0 and b'star_logp' in lib.sconf_last_error()
    assert al(star=-math.inf) != 0 and b'star_logp' in lib.sconf_last_error()
    assert al(S=65536, ws=1 << 40) != 0 and b'65535' in lib.sconf_last_error()
    assert al(ws=need - 1) != 0 and b'workspace' in lib.sconf_last_error()
    assert al(blank=32) != 0 and b'blank' in lib.sconf_last_error()          # the star's id is no blank
    assert al(C=30) != 0 and b'multiple of 4' in lib.sconf_last_error()
    assert al(N=0) != 0 and b'sizes' in lib.sconf_last_error()
    assert lib.sconf_seg_align(one, one, None, None, one, one, one, one, one, None, one, need, 1, 10, 32, 3, 31, 0.0, None) != 0
    assert b'null' in lib.sconf_last_error()
    assert al(B=0) == 0
    sc = lambda window=30, B=1, N=10, S=3, U=2: lib.sconf_seg_score(one, one, one, None, None, one, None, window, one, one, one, B, N, S, U, None)
    assert sc(window=0) != 0 and b'window' in lib.sconf_last_error()
    assert sc(window=lib.sconf_seg_max_window() + 1) != 0 and b'window' in lib.sconf_last_error()
    assert sc(S=65536) != 0 and b'sizes' in lib.sconf_last_error()
    assert sc(N=0) != 0 and b'sizes' in lib.sconf_last_error()
    assert lib.sconf_seg_score(one, one, one, None, None, None, None, 30, one, one, one, 1, 10, 3, 2, None) != 0 and b'null' in lib.sconf_last_error()
    assert sc(B=0) == 0 and sc(U=0) == 0


# ---- 4. eval.run.segment on the tiny fixture model ------------------------------------------------------------------------------
class IdTok:
    """Every token is a word: id i is spelt 't<i>'."""
    def __init__(self, V): self.V = V
    def vocab_size(self): return self.V
    def decode(self, ids): return ' '.join(f't{int(i)}' for i in ids)
    def encode(self, text): return [int(w[1:]) for w in text.split()]


def test_segment_on_the_tiny_model(emulated_ops, emulated_seg, monkeypatch):
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
    texts = ['t3 t1 t4', 't1 t5', 't9 t2 t6']
    recs = R.segment(m, spec, texts, tok, 128, 32, window=3)
    assert [r['text'] for r in recs] == texts and all(set(r) == {'text', 'startTime', 'endTime', 'confidence', 'logp'} for r in recs)
    assert all(re.fullmatch(r'\d+\.\d\ds', r[k]) for r in recs for k in ('startTime', 'endTime'))
    times = [float(r[k][:-1]) for r in recs for k in ('startTime', 'endTime')]
    assert times == sorted(times) and all(r['confidence'] <= r['logp'] + 1e-6 <= 1e-6 for r in recs)
    # the same by hand: the logits, the restatement, the record strings
    logits = R.moving_average_eval(R._Args(), m, spec, 128, 32, tok, use_tqdm=False, return_numpy=False)
    C = m.decoder.num_classes
    ids = [tok.encode(t) for t in texts]
    ref = emulated_seg.ctc_segment(logits, ids, C - 1, window=3)
    sec = m.subsampling.subsampling_factor * audio_tools.HOP_LENGTH / audio_tools.SR
    assert [(r['startTime'], r['endTime']) for r in recs] == [(f'{a * sec:.2f}s', f'{b * sec:.2f}s') for a, b in ref.utt_frames.tolist()]
    assert [r['confidence'] for r in recs] == ref.utt_conf.tolist() and [r['logp'] for r in recs] == ref.utt_logp.tolist()
    assert bool((ref.alignment.labels == C).any())                        # stars took frames
    # min_confidence drops the records below it
    cut = sorted(r['confidence'] for r in recs)[1]
    kept = R.segment(m, spec, texts, tok, 128, 32, window=3, min_confidence=cut)
    assert kept == [r for r in recs if r['confidence'] >= cut] and 0 < len(kept) < 3
    # words=True: word_timestamps over each utterance's own tokens
    withw = R.segment(m, spec, texts, tok, 128, 32, window=3, words=True)
    ranges = emulated_seg.build_targets(ids, C)[1]
    for r, base, t, (j0, j1) in zip(withw, recs, texts, ranges):
        assert {k: v for k, v in r.items() if k != 'words'} == base
        assert [w['word'] for w in r['words']] == t.split() and r['words'][0]['startTime'] == r['startTime'] and r['words'][-1]['endTime'] == r['endTime']
        assert r['words'] == R.word_timestamps(tok.encode(t), ref.alignment.spans[j0:j1], tok, sec, token_logp=ref.alignment.token_logp[j0:j1])
    assert R.segment_waveform(m, wave, texts, tok, 128, 32, window=3) == recs
    assert R.segment_waveform(m, torch.stack([wave, -wave]), texts, tok, 128, 32, window=3, star_logp=-1.0) == R.segment(m, spec, texts, tok, 128, 32, window=3, star_logp=-1.0)
    with pytest.raises(ValueError, match=rf'cannot be emitted in {logits.shape[0]} frames'):
        R.segment(m, spec, [tok.decode([1, 2] * logits.shape[0])], tok, 128, 32)
    with pytest.raises(ValueError, match='evaluation_mode'):
        R.segment(m, spec, texts, tok, 128, 32, evaluation_mode='beam')
