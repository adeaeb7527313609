"""CTC segmentation on the device (csrc/seg.hip through lcasr_amd.hip.seg and decoding/segment.py).

The alignment with star labels is held to the header's own definition: the five outputs are, bit for bit, what sconf_align_ctc (or
sconf_lalign_ctc above 8191 labels) gives on the device on an explicit (B, N, C + 4) matrix whose column C holds star_logp and whose
other three new columns hold -inf; frame_logp is a gather by `path`.  The utterance scores are held to the float64 restatement
(tests/seg_refs.py) within seg_refs.score_bound: 2^-22 |ref| + 1e-7, derived there from the number formats, not measured.

Shapes are the smallest at which the kernels can go wrong (C = 8 .. 32): the lattice geometry switches 127 | 128 and 255 | 256, the
routing switch 8191 | 8192 between the two lattice forms, utterances around the window and around sconf_seg_score_tile()."""
import math

import numpy as np
import pytest
import torch

import align_refs as AR
import seg_refs as SR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def K():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from lcasr_amd.hip import align, align_long, seg
    seg.load()

    class Units:
        pass
    k = Units()
    k.seg, k.align, k.long = seg, align, align_long
    return k


def _dev(v):
    return None if v is None else torch.tensor(v, dtype=torch.int32).cuda()


def _bits(t):
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()]) if t.dtype.is_floating_point else t


def same_as_the_explicit_matrix(K, lp, tg, il, tl, blank, star_logp, what='', poisoned=()):
    """seg.align on (lp, star_logp) against the plain aligner on the extended matrix, all on the device: five outputs bit for bit
    (a poisoned sample: score NaN, the rest as infeasible), frame_logp as a gather by path.  Returns the device result."""
    B, N, C = lp.shape
    Smax = tg.shape[1]
    lpd, tgd = lp.cuda(), tg.cuda()
    got = K.seg.align(lpd, tgd, _dev(il), _dev(tl), blank, star_logp)
    ext = SR.extend(lpd, star_logp, extra=4)
    ref = (K.align if Smax <= K.align.max_labels() else K.long).ctc_align(ext, tgd, _dev(il), _dev(tl), blank)
    torch.cuda.synchronize()
    keep = torch.tensor([b not in poisoned for b in range(B)]).cuda()
    for name, a, b in zip(('path', 'labels', 'spans', 'token_logp', 'score'), got[:5], ref):
        bad = (_bits(a)[keep] != _bits(b)[keep]).nonzero()
        assert not bad.numel(), f'{what} {name}: {bad.shape[0]} element(s) differ from the explicit matrix, first at {bad[0].tolist()}'
    for b in poisoned:
        assert math.isnan(float(got.score[b])) and bool((got.path[b] == -1).all()) and bool((got.labels[b] == -1).all())
        assert (Smax == 0 or bool((got.spans[b] == -1).all())) and not bool(got.token_logp[b].any())
    # frame_logp: the emission of the state the path occupies, 0 where there is no path
    path = got.path.long()
    on = path >= 0
    tok = tgd.long().gather(1, (path.clamp(min=0) // 2).clamp(max=max(Smax - 1, 0))) if Smax else torch.full_like(path, blank)
    lab = torch.where(path % 2 == 1, tok, torch.full_like(path, blank))
    want = torch.where(on, ext.gather(2, lab.clamp(0, C + 3)[..., None])[..., 0], torch.zeros_like(got.frame_logp))
    assert torch.equal(_bits(got.frame_logp), _bits(want)), f'{what} frame_logp is not the gather by path'
    assert torch.equal(got.labels.long()[on], lab[on])
    return got


C, BLANK = 16, 15
STAR = C
CASES = {
    'star-only': ([[STAR]], [5], [1]),
    'star-first-last-middle': ([[STAR, 3, 4, STAR, 5, STAR]], [17], [6]),
    'two-adjacent-stars': ([[2, STAR, STAR, 3]], [9], [4]),
    'star-beside-an-equal-pair': ([[4, 4, STAR, 4, STAR, 4, 4]], [14], [7]),
    'exactly-enough-frames': ([[STAR, 1, 1, STAR, STAR, 2], [STAR, 1, 1, STAR, STAR, 2]], [8, 7], [6, 6]),      # S + repeats = 8, and one fewer
    'ragged': ([[STAR, 1, 2, STAR, 3, 4, 5, STAR], [6, STAR, 7, 0, 0, 0, 0, 0], [STAR, 9, STAR, 0, 0, 0, 0, 0]], [30, 11, 19], [8, 3, 3]),
}


@pytest.mark.parametrize('star_logp', [0.0, -1.0])
@pytest.mark.parametrize('id', list(CASES))
def test_star_cases_are_the_explicit_matrix(K, id, star_logp):
    rows, il, tl = CASES[id]
    tg = torch.tensor(rows, dtype=torch.int32)
    lp, _ = AR.random_case(11, len(rows), max(il) + (3 if id == 'ragged' else 0), C, tg.shape[1], il, tl, targets=tg)
    got = same_as_the_explicit_matrix(K, lp, tg, il, tl, BLANK, star_logp, id)
    feas = [AR.feasible(T, r[:S]) for r, T, S in zip(rows, il, tl)]
    assert [math.isfinite(s) for s in got.score.tolist()] == feas and (id != 'exactly-enough-frames' or feas == [True, False])
    if id == 'star-only':
        n = int((got.labels[0] == STAR).sum())
        assert n >= 1 and float(got.token_logp[0, 0]) == star_logp * n and got.spans[0, 0, 1] - got.spans[0, 0, 0] == n


def test_a_poisoned_sample_beside_healthy_ones(K):
    tg = torch.tensor([[STAR, 1, 2, STAR], [1, C + 1, 2, 3], [3, STAR, -1, 2], [2, STAR, 4, 5]], dtype=torch.int32)
    lp, _ = AR.random_case(12, 4, 12, C, 4, targets=tg.clamp(0, C - 1))
    got = same_as_the_explicit_matrix(K, lp, tg, None, None, BLANK, -1.0, 'poisoned', poisoned=(1, 2))
    assert bool(torch.isfinite(got.score[[0, 3]]).all()) and not bool(got.frame_logp[1:3].any())


@pytest.mark.parametrize('S', [127, 128, 255, 256])
def test_targets_without_a_star_give_the_plain_aligners_bits_and_with_one_the_explicit_matrix(K, S):
    """Both sides of the geometry switches, ragged, repeats planted."""
    N = S + 40
    il, tl = [N, S + 9, N - 13], [S, S, max(S - 3, 0)]
    lp, tg = AR.random_case(200 + S, 3, N, C, S, il, tl, repeats=4)
    plain = K.align.ctc_align(lp.cuda(), tg.cuda(), _dev(il), _dev(tl), BLANK)
    got = K.seg.align(lp.cuda(), tg.cuda(), _dev(il), _dev(tl), BLANK, -1.0)
    for name, a, b in zip(('path', 'labels', 'spans', 'token_logp', 'score'), got[:5], plain):
        assert torch.equal(_bits(a), _bits(b)), f'S={S} {name}: not the bits of sconf_align_ctc'
    stars = tg.clone()
    stars[:, 0] = STAR; stars[:, S // 2] = STAR; stars[0, S - 1] = STAR; stars[1, S - 1] = STAR; stars[1, S - 2] = STAR
    for star_logp in (0.0, -1.0):
        g = same_as_the_explicit_matrix(K, lp, stars, il, tl, BLANK, star_logp, f'S={S} star_logp={star_logp}')
        assert bool(torch.isfinite(g.score).all())


@pytest.mark.parametrize('S', [8191, 8192])
def test_the_routing_switch_between_the_two_lattice_forms(K, S):
    """8191 labels: the short form (f32 states); 8192: the long form (f64 states, the default slab).  N just above S, C = 8."""
    Cs, N = 8, S + 40
    lp, tg = AR.random_case(300 + S, 1, N, Cs, S, repeats=6)
    tg[0, 0] = Cs; tg[0, S // 3] = Cs; tg[0, S - 1] = Cs
    assert (K.align.state_bytes(S) if S <= K.align.max_labels() else 8) == (4 if S == 8191 else 8)
    got = same_as_the_explicit_matrix(K, lp, tg, None, None, Cs - 1, -1.0, f'S={S}')
    assert math.isfinite(float(got.score[0])) and int((got.labels[0] == Cs).sum()) >= 3


# ---- utterance scores -------------------------------------------------------------------------------------------------------------
def _score_inputs(K, window):
    """Token j of sample 0 holds n_j frames from a_j on (the kernel takes spans as they come: tokens need not tile the frames)."""
    tile, W = K.seg.score_tile(), K.seg.max_window()
    N = W + tile + 50
    ns = [1, max(window - 1, 1), window, window + 1, tile, tile + 1, tile - 1, N]
    Smax = len(ns)
    spans = torch.full((3, Smax, 2), -1, dtype=torch.int32)
    for j, n in enumerate(ns):
        a = 0 if n == N else min(7 * j + 3, N - n)
        spans[0, j] = torch.tensor([a, a + n])
    spans[1] = spans[0]; spans[2] = spans[0]
    g = torch.from_numpy(-np.random.default_rng(window).exponential(2.0, size=(3, N)).astype(np.float32))
    score = torch.tensor([-40.0, -math.inf, -7.0], dtype=torch.float64)          # sample 1: infeasible, beside healthy ones
    utt = [[j, j + 1] for j in range(Smax)] + [[0, 3], [2, 2], [3, Smax + 1], [-1, 2], [4, 3]]
    utt = torch.tensor([utt, utt, utt], dtype=torch.int32)
    counts = torch.tensor([utt.shape[1], utt.shape[1], 0], dtype=torch.int32)       # sample 2: count 0
    return spans, g, score, utt, counts, ns


@pytest.mark.parametrize('window', ['1', '30', 'largest'])
def test_utterance_scores_at_the_derived_bound(K, window):
    window = K.seg.max_window() if window == 'largest' else int(window)
    spans, g, score, utt, counts, ns = _score_inputs(K, window)
    got = K.seg.score(spans.cuda(), g.cuda(), score.cuda(), None, None, utt.cuda(), counts.cuda(), window)
    torch.cuda.synchronize()
    ref = SR.score(spans, g, score, None, None, utt, counts, window)
    SR.assert_scores_close(got, ref, f'window={window}')
    S = len(ns)
    assert ref.utt_frames[0, :S].tolist() == spans[0].tolist() and not bool(torch.isnan(ref.utt_conf[0, :S + 1]).any())
    assert bool(torch.isnan(ref.utt_conf[0, S + 1:]).all()) and bool(torch.isnan(ref.utt_conf[1]).all())       # j0 = j1, j1 > S, j0 < 0, j0 > j1; -inf
    assert not bool(ref.utt_conf[2].any()) and bool((ref.utt_frames[1:] == -1).all())
    assert float(ref.utt_conf[0, 0]) == float(ref.utt_logp[0, 0])                                              # one frame
    # the same with lengths given, one sample cut short: the utterance of every frame no longer fits it
    il, tl = torch.tensor([g.shape[1] - 1, g.shape[1], 5], dtype=torch.int32), torch.tensor([S, S, S], dtype=torch.int32)
    got = K.seg.score(spans.cuda(), g.cuda(), score.cuda(), il.cuda(), tl.cuda(), utt.cuda(), None, window)
    ref = SR.score(spans, g, score, il, tl, utt, None, window)
    SR.assert_scores_close(got, ref, f'window={window} lengths')
    assert math.isnan(float(ref.utt_conf[0, S - 1])) and math.isfinite(float(ref.utt_conf[2, 0]))


def test_no_utterances(K):
    spans, g, score, utt, counts, _ = _score_inputs(K, 30)
    out = K.seg.score(spans.cuda(), g.cuda(), score.cuda(), None, None, utt[:, :0].contiguous().cuda(), None, 30)
    torch.cuda.synchronize()
    assert out.utt_frames.shape == (3, 0, 2) and out.utt_logp.shape == (3, 0) and out.utt_conf.shape == (3, 0)


# ---- the planted case and the tiny model -----------------------------------------------------------------------------------------
def test_the_planted_case(K):
    from lcasr_amd.decoding import segment as D
    lp, utts, planted, gap_frames = SR.planted_case()
    blank = lp.shape[2] - 1
    lpd = lp.cuda()
    seg = D.ctc_segment(lpd[0], utts, blank, star_logp=-1.0, window=4)
    assert [tuple(x) for x in seg.utt_frames.tolist()] == planted
    assert sorted(torch.nonzero(seg.alignment.labels == lp.shape[2])[:, 0].tolist()) == gap_frames
    assert [tuple(x) for x in D.ctc_segment(lpd[0], utts, blank, star_logp=0.0, window=4).utt_frames.tolist()] != planted
    plain = D.ctc_segment(lpd[0], utts, blank, star_between=False, star_ends=False, star_logp=-1.0, window=4)
    gain = float(seg.alignment.score) - float(plain.alignment.score)
    print(f'[seg] planted: score with stars {float(seg.alignment.score):.3f}, without {float(plain.alignment.score):.3f}, stars paid {len(gap_frames)}')
    assert math.isfinite(float(plain.alignment.score)) and gain > len(gap_frames) * 1.0
    wrong = [utts[0], [utts[1][0], 6, 7] + utts[1][3:], utts[2]]
    sw = D.ctc_segment(lpd[0], wrong, blank, star_logp=-1.0, window=4)
    d_logp, d_conf = abs(float(sw.utt_logp[1] - seg.utt_logp[1])), abs(float(sw.utt_conf[1] - seg.utt_conf[1]))
    print(f'[seg] planted, two tokens replaced: utt_conf {sw.utt_conf.tolist()}, utt_logp moves {d_logp:.3f}, utt_conf moves {d_conf:.3f}')
    assert int(sw.utt_conf.argmin()) == 1 and d_logp < d_conf
    # the batch form and the restatement agree with it
    both = D.ctc_segment(torch.cat([lpd, lpd]), [utts, wrong], blank, star_logp=-1.0, window=4)
    assert torch.equal(both.utt_frames[0], seg.utt_frames) and torch.equal(both.utt_conf[1], sw.utt_conf)
    row, ranges = D.build_targets(utts, lp.shape[2])
    al = SR.align(lp, torch.tensor([row], dtype=torch.int32), None, None, blank, -1.0)
    ref = SR.score(al.spans, al.frame_logp, al.score, None, None, torch.tensor([ranges], dtype=torch.int32), None, 4)
    SR.assert_scores_close(type(ref)(seg.utt_frames[None], seg.utt_logp[None], seg.utt_conf[None]), ref, 'planted')


class IdTok:
    """Every token is a word: id i is spelt 't<i>'."""
    def __init__(self, V): self.V = V
    def vocab_size(self): return self.V
    def decode(self, ids): return ' '.join(f't{int(i)}' for i in ids)
    def encode(self, text): return [int(w[1:]) for w in text.split()]


CFG = dict(vocab_size=127, n_layers=2, d_model=64, n_heads=2, head_dim=32, subsampling_conv_channels=32, use_rotary=True,
           rotary_base_freq=1500000, decoder_norm=True, self_conditioning=True, bias_in_ff=False, default_norm='layer_norm')


def test_the_models_own_greedy_transcript_with_the_middle_utterance_removed(K):
    import audio_refs as AUD
    from lcasr_amd.decoding import segment as D
    from lcasr_amd.eval import run as R
    from lcasr_amd.models.sconformer_xl import SCConformerXL
    from lcasr_amd.utils import audio_tools as A
    torch.manual_seed(12345)
    model = SCConformerXL(**CFG).cuda().eval()
    wave = AUD.test_signal(3 * 16000, seed=9).cuda()
    tok, blank = IdTok(127), model.decoder.num_classes - 1
    spec = A.to_spectogram(wave[None])
    logits = R.moving_average_eval(R._Args(), model, spec, 128, 32, tok, use_tqdm=False, return_numpy=False)
    SR.check_greedy_transcript_with_a_gap(logits, blank, lambda lp, utts: D.ctc_segment(lp, utts, blank, star_ends=False, star_logp=-1.0, window=3))
    # and through the evaluation driver: three records in, the times of the segmentation out
    ids, _ = SR.greedy_runs(logits.cpu(), blank)
    k = len(ids) // 3
    texts = [tok.decode(ids[:k]), tok.decode(ids[2 * k:])]
    recs = R.segment(model, spec, texts, tok, 128, 32, window=3)
    seg = D.ctc_segment(logits, [ids[:k], ids[2 * k:]], blank, window=3)
    sec = model.subsampling.subsampling_factor * A.HOP_LENGTH / A.SR
    assert [(r['text'], r['startTime'], r['endTime']) for r in recs] == [(t, f'{a * sec:.2f}s', f'{b * sec:.2f}s') for t, (a, b) in zip(texts, seg.utt_frames.tolist())]
    assert [r['confidence'] for r in recs] == seg.utt_conf.tolist() and R.segment_waveform(model, wave, texts, tok, 128, 32, window=3) == recs
    with pytest.raises(ValueError, match='cannot be emitted'):
        R.segment(model, spec, [tok.decode([1, 2] * logits.shape[0])], tok, 128, 32)
