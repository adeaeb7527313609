"""Numpy restatement of the CTC segmentation contract (include/sconf_seg.h) with the signatures of lcasr_amd.hip.seg.align and
lcasr_amd.hip.seg.score, and what the CPU and GPU segmentation tests share.  TEST INFRASTRUCTURE.

The alignment with star labels is, by the header's own words, align_refs.ctc_align on the log-probs extended by one column that
holds star_logp, so that is how it is restated: nothing of the recursion is written a second time.  The utterance scores are
evaluated in float64, every window summed on its own (no running sum, so no cancellation), and rounded once to float32."""
import math

import numpy as np
import torch

import align_refs as AR

SHORT_FORM_LABELS = 8191


def extend(log_probs, star_logp, extra=1):
    """(B, N, C) -> (B, N, C + extra): column C holds star_logp, the columns behind it -inf."""
    B, N, C = log_probs.shape
    ext = torch.full((B, N, C + extra), -math.inf, dtype=log_probs.dtype, device=log_probs.device)
    ext[..., :C] = log_probs
    ext[..., C] = star_logp
    return ext.contiguous()


def align(log_probs, targets, input_lengths, target_lengths, blank, star_logp=0.0, dtype=None):
    """lcasr_amd.hip.seg.align on any device, in numpy.  dtype: the state type of the short form (None: float64); the long form
    (more than 8191 labels) is always float64."""
    from lcasr_amd.hip.seg import StarAlignment
    if not (star_logp <= 0 and math.isfinite(star_logp)):
        raise RuntimeError(f'sconf_seg_align: star_logp {star_logp}: it must be finite and <= 0')
    B, N, C = log_probs.shape
    dtype = np.float64 if dtype is None or targets.shape[1] > SHORT_FORM_LABELS else dtype
    ext = extend(log_probs.float(), star_logp)
    al = AR.ctc_align(ext, targets, input_lengths, target_lengths, blank, dtype=dtype)
    lab = al.labels.long().clamp(min=0)
    g = ext.gather(2, lab[..., None])[..., 0]
    g = torch.where(al.labels >= 0, g, torch.zeros_like(g))
    return StarAlignment(*al, g.contiguous())


def window_means(g, w):
    """The mean of every w consecutive values of g, each window summed on its own in float64."""
    g = np.asarray(g, dtype=np.float64)
    return np.lib.stride_tricks.sliding_window_view(g, w).sum(-1) / w


def score(spans, frame_logp, score, input_lengths, target_lengths, utt, utt_counts=None, window=30):
    """lcasr_amd.hip.seg.score on any device, in numpy float64."""
    from lcasr_amd.hip.seg import UtteranceScores
    dev = frame_logp.device
    sp, g, sc, ut = spans.cpu().numpy(), frame_logp.cpu().numpy().astype(np.float64), score.cpu().numpy(), utt.cpu().numpy()
    B, N = g.shape
    Smax, Umax = sp.shape[1], ut.shape[1]
    il = [N] * B if input_lengths is None else input_lengths.cpu().tolist()
    tl = [Smax] * B if target_lengths is None else target_lengths.cpu().tolist()
    uc = [Umax] * B if utt_counts is None else [min(max(c, 0), Umax) for c in utt_counts.cpu().tolist()]
    frames = np.full((B, Umax, 2), -1, np.int32)
    logp, conf = np.zeros((B, Umax), np.float32), np.zeros((B, Umax), np.float32)
    for b in range(B):
        for u in range(uc[b]):
            logp[b, u] = conf[b, u] = np.nan
            j0, j1 = int(ut[b, u, 0]), int(ut[b, u, 1])
            if not (0 <= tl[b] <= Smax and 1 <= il[b] <= N and math.isfinite(sc[b]) and 0 <= j0 < j1 <= tl[b]):
                continue
            f0, f1 = int(sp[b, j0, 0]), int(sp[b, j1 - 1, 1])
            if not 0 <= f0 < f1 <= il[b]:
                continue
            n = f1 - f0
            frames[b, u] = (f0, f1)
            logp[b, u] = np.float32(g[b, f0:f1].sum() / n)
            conf[b, u] = np.float32(window_means(g[b, f0:f1], min(window, n)).min())
    return UtteranceScores(*(torch.from_numpy(a).to(dev) for a in (frames, logp, conf)))


def score_bound(ref):
    """The bound of the utterance scores against this restatement: the f32 rounding of the result (2^-24 relative, twice: the
    kernel's and the restatement's roundings may fall to different sides) plus the f64 accumulation error of a running sum,
    n 2^-53 sum|g| / w < 1e-8 at every test size; held as 2^-22 |ref| + 1e-7."""
    return 2.0 ** -22 * ref.double().abs() + 1e-7


def assert_scores_close(got, ref, what=''):
    """utt_frames exact; utt_logp and utt_conf NaN where the restatement is NaN and within score_bound elsewhere."""
    assert torch.equal(got.utt_frames.cpu(), ref.utt_frames.cpu()), f'{what} utt_frames'
    for name in ('utt_logp', 'utt_conf'):
        x, r = getattr(got, name).cpu().double(), getattr(ref, name).cpu().double()
        nan = torch.isnan(r)
        assert torch.equal(torch.isnan(x), nan), f'{what} {name}: NaN in other places'
        err, bd = (x - r).abs()[~nan], score_bound(r)[~nan]
        if err.numel():
            print(f'[seg] {what} {name}: max |x - ref| = {float(err.max()):.3e}, bound there {float(bd[err.argmax()]):.3e}')
        assert bool((err <= bd).all()), f'{what} {name}: {float((err - bd).max()):.3e} over the bound'


def planted_case(C=16, gap_class=None, peak=6.0, seed=0):
    """Three utterances with untranscribed frames before, between and after them.  Returns (log_probs (1, N, C) f32, utterances
    (lists of ids), planted utt_frames [(f0, f1)], the untranscribed frames).  Classes 0..5 make the utterances, the untranscribed
    frames are peaked on classes outside the transcript (8..11), blank = C - 1.  Every token holds 2 frames, a blank frame parts two
    tokens of an utterance."""
    utterances = [[0, 1, 2, 3], [4, 5, 0, 2, 1], [3, 4, 1]]
    gaps = [5, 7, 6, 4]                                                      # before, between, between, after
    blank = C - 1
    g = torch.Generator().manual_seed(seed)
    cls, frames, gap_frames = [], [], []
    for k, u in enumerate(utterances):
        for _ in range(gaps[k]):
            gap_frames.append(len(cls)); cls.append(8 + int(torch.randint(0, 4, (1,), generator=g)) if gap_class is None else gap_class)
        f0 = len(cls)
        for i, tok in enumerate(u):
            if i: cls.append(blank)
            cls += [tok, tok]
        frames.append((f0, len(cls)))
    for _ in range(gaps[-1]):
        gap_frames.append(len(cls)); cls.append(8 + int(torch.randint(0, 4, (1,), generator=g)) if gap_class is None else gap_class)
    N = len(cls)
    x = torch.randn(1, N, C, generator=g) * 0.3
    x[0, torch.arange(N), torch.tensor(cls)] += peak
    return torch.log_softmax(x, -1).contiguous(), utterances, frames, gap_frames


# ---- the model's own greedy transcript with an utterance removed ---------------------------------------------------------------
def greedy_runs(log_probs, blank):
    """(ids, runs) of the greedy CTC collapse of (N, C) log-probs: the labels in order and [first frame, one past the last) of each."""
    idx = log_probs.argmax(-1).tolist()
    ids, runs = [], []
    for t, c in enumerate(idx):
        if c != blank and (t == 0 or idx[t - 1] != c):
            ids.append(c); runs.append([t, t + 1])
        elif c != blank:
            runs[-1][1] = t + 1
    return ids, runs


def check_greedy_transcript_with_a_gap(logits, blank, segment):
    """`logits` (N, C) of a model, on any device; segment(log_probs, utterances) -> CTCSegmentation with star_logp = -1, a star
    between the utterances and none at the ends (a star always takes a frame, and this transcript leaves none over at its ends).

    The greedy transcript is cut into three utterances and the middle one leaves the list.  The tiny test models are untrained and
    their posteriors nearly uniform, so the logits are SHARPENED first: multiplied by k = 64 / (the least top-1 margin over the
    frames), after which the greedy label of every frame has a log-prob above -1e-20 and every other class one below -64.  A star at
    -1 is then dearer than the right class and cheaper than any wrong one, and a kept token cannot bridge to frames of a removed
    token with its label, since a single wrong frame between them costs more than the at most N < 64 frames a star would pay.
    Hence, exactly: the kept utterances lie on the greedy frames of their tokens, token by token, and the star between them covers
    the greedy frames of every removed token."""
    top2 = logits.float().topk(2, -1).values
    margin = float((top2[:, 0] - top2[:, 1]).min())
    assert margin > 0 and logits.shape[0] < 64
    lp = torch.log_softmax(logits.float() * (64.0 / margin), -1)
    ids, runs = greedy_runs(lp.cpu(), blank)
    assert len(ids) >= 3, f'the greedy transcript has {len(ids)} labels'
    k = len(ids) // 3
    kept = [ids[:k], ids[2 * k:]]
    seg = segment(lp, kept)
    C = lp.shape[1]
    row_runs = runs[:k] + [None] + runs[2 * k:]                             # the star row: u0 [*] u2
    spans = seg.alignment.spans.cpu().tolist()
    assert len(spans) == len(row_runs)
    for j, (sp, run) in enumerate(zip(spans, row_runs)):
        if run is not None:
            assert sp == run, f'token {j} of the star row holds {sp}, its greedy frames are {run}'
    assert seg.utt_frames.cpu().tolist() == [[runs[0][0], runs[k - 1][1]], [runs[2 * k][0], runs[-1][1]]]
    f, l = spans[k]                                                         # the star between the two
    assert f <= runs[k][0] and runs[2 * k - 1][1] <= l, f'the star between the utterances holds [{f}, {l}), the removed tokens {runs[k:2 * k]}'
    labels = seg.alignment.labels.cpu()
    for a, b in runs[k:2 * k]:
        assert bool((labels[a:b] == C).all())
    assert float(seg.utt_conf.max()) <= 0.0 and float(seg.utt_conf.min()) > -1e-6
    return ids, runs
