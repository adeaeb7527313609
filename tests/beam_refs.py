"""The contract of include/sconf_beam.h in numpy / Python f64, with prefixes keyed by TUPLES (the kernels use (length, 64-bit hash)):
the yardstick of tests/test_beam.py (which checks it against the enumeration of every frame path) and tests/test_beam_gpu.py.
TEST INFRASTRUCTURE, a plain importable module.

Besides the result, `search` reports what a test needs to know about its own input:
  gap        the smallest decision gap met: over every frame, the difference between a surviving candidate's total and the next
             candidate's (adjacent survivors, and the last survivor against the first one dropped by the width), and the distance of
             every candidate among the W largest from the prune threshold best + beam_prune_logp.  A device result whose totals are
             within gap / 2 of the restatement's takes the same decisions.
  cap, pruned, folds      frames in which more tokens qualified than Kmax / beams dropped by the prune rule / extensions folded
  recreated  how often a prefix that had left the beam was created again while a longer live beam still started with it: the case
             that an identity by trie node (parent pointer) instead of by token sequence gets wrong
  kept       the number of kept tokens per frame;  live: the number of live beams after each frame
  max_score  the largest |total| met;  candidates: the set of candidate counts n (k + 1) of the frames with a kept token"""
import itertools
import math
from typing import NamedTuple

import numpy as np
import torch

NEG = -math.inf


class Beams(NamedTuple):
    count: torch.Tensor
    tokens: torch.Tensor
    lengths: torch.Tensor
    token_frames: torch.Tensor
    scores: torch.Tensor


def lse(a, b):
    m = max(a, b)
    if not m > NEG:
        return m
    return m + math.log1p(math.exp(-abs(a - b)))


def kept_tokens(row, blank, token_min_logp, Kmax):
    """The kept classes of one frame in ascending order (`row` f32, the comparison in f32), and whether the cap was exercised."""
    row = np.asarray(row, dtype=np.float32)
    thr = np.float32(token_min_logp)
    q = [c for c in range(row.shape[0]) if c != blank and row[c] >= thr]
    am = int(np.argmax(row))                                              # the lowest index among equal maxima
    if am != blank and am not in q:
        q.append(am)
    capped = len(q) > Kmax
    if capped:
        q = sorted(q, key=lambda c: (-float(row[c]), c))[:Kmax]
    return sorted(q), capped


def search(lp, blank, W, token_min_logp=-5.0, beam_prune_logp=-10.0, Kmax=16):
    """One sample: lp (T, C) f32.  Returns (beams, stats); beams is the final ranking, a list of (prefix, frames, total)."""
    lp = np.asarray(lp, dtype=np.float32)
    T = lp.shape[0]
    beams = [((), (), 0.0, NEG)]                                           # (prefix, frames, pb, pnb)
    st = dict(gap=math.inf, cap=0, pruned=0, folds=0, recreated=0, kept=[], live=[], max_score=0.0, candidates=set())
    seen = {()}                                                            # every prefix that has ever been live
    for t in range(T):
        row = lp[t]
        slots, capped = kept_tokens(row, blank, token_min_logp, Kmax)
        st['cap'] += capped
        st['kept'].append(len(slots))
        lpb = float(row[blank])
        live = {b[0]: j for j, b in enumerate(beams)}
        spb, spnb = [], []
        for pre, _, pb, pnb in beams:
            spb.append(lse(pb, pnb) + lpb)
            spnb.append(pnb + float(row[pre[-1]]) if pre and pre[-1] in slots else NEG)
        ext = []                                                           # (candidate index, i, class, v)
        for i, (pre, _, pb, pnb) in enumerate(beams):
            for k, c in enumerate(slots):
                v = float(row[c]) + (pb if pre and c == pre[-1] else lse(pb, pnb))
                j = live.get(pre + (c,))
                if j is not None:
                    spnb[j] = lse(spnb[j], v)
                    st['folds'] += 1
                else:
                    ext.append((W + i * Kmax + k, i, c, v))
        cands = [(lse(spb[i], spnb[i]), i, None) for i in range(len(beams))] + [(v, ci, (i, c)) for ci, i, c, v in ext]
        if slots:
            st['candidates'].add(len(beams) * (len(slots) + 1))
        cands = sorted((x for x in cands if x[0] > NEG), key=lambda x: (-x[0], x[1]))
        top = cands[:W]
        floor = top[0][0] + beam_prune_logp if top else NEG
        surv = [x for x in top if not x[0] < floor]
        st['pruned'] += len(top) - len(surv)
        for r in range(len(surv)):
            if r + 1 < len(cands):
                st['gap'] = min(st['gap'], surv[r][0] - cands[r + 1][0])
        if top and floor > NEG:
            st['gap'] = min(st['gap'], min(abs(x[0] - floor) for x in top))
        new = []
        for total, ci, how in surv:
            st['max_score'] = max(st['max_score'], abs(total))
            if how is None:
                pre, fr, _, _ = beams[ci]
                new.append((pre, fr, spb[ci], spnb[ci]))
            else:
                i, c = how
                new.append((beams[i][0] + (c,), beams[i][1] + (t,), NEG, total))
        stays = [b[0] for (_, _, how), b in zip(surv, new) if how is None]
        for (_, _, how), b in zip(surv, new):
            if how is not None:
                p = b[0]
                if p in seen and any(len(q) > len(p) and q[:len(p)] == p for q in stays):
                    st['recreated'] += 1
                seen.add(p)
        beams = new
        st['live'].append(len(beams))
    return [(pre, fr, lse(pb, pnb)) for pre, fr, pb, pnb in beams], st


def ctc_beam(log_probs, input_lengths, blank, beam_width, nbest, token_min_logp, beam_prune_logp, max_tokens_per_frame, max_len,
             stats=None):
    """lcasr_amd.hip.beam.ctc_beam on CPU tensors.  `stats`: a list that receives the per-sample statistics (None for poisoned)."""
    lp = log_probs.detach().cpu().float().numpy()
    B, N, C = lp.shape
    L = int(max_len)
    out = Beams(torch.zeros(B, dtype=torch.int32), torch.full((B, nbest, L), -1, dtype=torch.int32),
                torch.zeros(B, nbest, dtype=torch.int32), torch.full((B, nbest, L), -1, dtype=torch.int32),
                torch.full((B, nbest), NEG, dtype=torch.float64))
    for b in range(B):
        T = N if input_lengths is None else int(input_lengths[b])
        if T > N or T < 0:
            out.scores[b] = math.nan
            if stats is not None: stats.append(None)
            continue
        beams, st = search(lp[b, :T], blank, beam_width, token_min_logp, beam_prune_logp, max_tokens_per_frame)
        if stats is not None: stats.append(st)
        out.count[b] = min(nbest, len(beams))
        for r, (pre, fr, total) in enumerate(beams[:nbest]):
            n = min(len(pre), L)
            out.tokens[b, r, :n] = torch.tensor(pre[:n], dtype=torch.int32)
            out.token_frames[b, r, :n] = torch.tensor(fr[:n], dtype=torch.int32)
            out.lengths[b, r] = len(pre)
            out.scores[b, r] = total
    return out


# ---- the definition: every frame path --------------------------------------------------------------------------------------------
def collapse(frames, blank):
    out, last = [], None
    for c in frames:
        if c != last and c != blank: out.append(c)
        last = c
    return tuple(out)


def enumerate_paths(lp, blank):
    """{label sequence: log of the summed probability of every frame path that collapses to it}, in f64 (math.fsum of the terms)."""
    lp = np.asarray(lp, dtype=np.float64)
    T, C = lp.shape
    terms = {}
    for frames in itertools.product(range(C), repeat=T):
        terms.setdefault(collapse(frames, blank), []).append(math.exp(float(sum(lp[t, c] for t, c in enumerate(frames)))))
    return {k: (math.log(math.fsum(v)) if math.fsum(v) > 0 else NEG) for k, v in terms.items()}


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def noise_case(seed, B, N, C, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.log_softmax(torch.randn(B, N, C, generator=g) * scale, -1).contiguous()


def recreation_case(W):
    """(seed, scale) of the first noise_case(seed, 1, 24, 4, scale), seed below 40, scale 1 then 1/2, that re-creates a prefix under
    a live extension at width W (blank 3); None if there is none."""
    for scale in (1.0, 0.5):
        for seed in range(40):
            if search(noise_case(seed, 1, 24, 4, scale)[0].numpy(), 3, W)[1]['recreated'] >= 1:
                return seed, scale
    return None


def spiky_case(seed, B, N, C, blank, every=6, peak=8.0, quiet=(), hold=1, in_len=None):
    """log_probs (B, N, C) f32: the log-softmax of unit noise with a planted spiky path - a label every `every` frames on average,
    held for `hold` frames, every fourth label a repeat of the one before, the blank elsewhere, each raised by `peak`.  `quiet`:
    frame ranges (first, one past the last) in which the blank is raised by 30 instead (no token reaches token_min_logp there and
    the blank is the arg-max: no kept token).  Returns (log_probs, labels per sample)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, N, C, generator=g)
    labels = []
    nonblank = [c for c in range(C) if c != blank]
    for b in range(B):
        T = N if in_len is None else max(min(int(in_len[b]), N), 0)
        at = torch.zeros(N, dtype=torch.bool)
        if T > 0:
            pick = torch.rand(T, generator=g) < 1.0 / every
            at[:T] = pick
        for f, l in quiet:
            at[f:l] = False
        for f, l in quiet:                                                 # a label on either side: the quiet run is exactly [f, l)
            if f - 1 >= 0: at[f - 1] = True
            if l < T: at[l] = True
        lab, prev, t = [], None, 0
        while t < N:
            if at[t]:
                c = nonblank[int(torch.randint(0, len(nonblank), (1,), generator=g))]
                if prev is not None and len(lab) % 4 == 3: c = prev
                for h in range(hold):
                    if t + h < N: x[b, t + h, c] += peak
                lab.append(c)
                prev = c
                t += hold
            else:
                x[b, t, blank] += peak
                t += 1
        for f, l in quiet:
            x[b, f:l, blank] += 30.0 - peak
        labels.append(lab)
    return torch.log_softmax(x, -1).contiguous(), labels


def eps_of(T, max_score):
    """The tests' score tolerance: a few ulp of the largest total per frame, accumulated linearly."""
    return 8 * T * 2.0 ** -52 * max_score
