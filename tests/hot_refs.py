"""The contract of include/sconf_hot.h in numpy / Python f64, independent of the automaton image: the yardstick of tests/test_hot.py
and tests/test_hot_gpu.py.  TEST INFRASTRUCTURE, a plain importable module.

  BruteHot    the hotword credits WITHOUT an automaton, straight from a prefix tuple and the list of phrases:
                  emit(prefix)      = the summed weights of every phrase that equals the last len(phrase) tokens of the prefix
                  permanent(prefix) = the sum of emit over every position of the prefix (every phrase occurrence)
                  phi(prefix)       = max w_p k / len(p) over phrases p and 1 <= k < len(p) with prefix[-k:] == p[:k], else 0
              emit and phi are rounded to f32 once (the image holds them as f32), in f64 before that.
  search_hot  lm_refs.search_lm extended by the hotwords: per beam the permanent credit `hot`; the key during the search is
              acoustic total + (bonus + weight phi(prefix)); at the end phi is dropped and the survivors are re-ranked (stable) by
              acoustic total + bonus.  lm=None: the LM's per-token term is 0.  weight = 0 or no phrase: no credit, no re-rank.
              The statistics of search_lm (gap includes the final re-rank's adjacent differences; max_score also |hot| and the key
              with phi) plus  revoked: surviving candidates whose phi is below their parent beam's (a hotword stopped matching);
              reranked: whether the final re-rank changed the order;  boosted: created tokens with emit > 0
  ctc_beam_hot  lcasr_amd.hip.hot.ctc_beam_hot on CPU tensors, with a DictLM (or None) and a BruteHot in the place of the images."""
import math
from typing import NamedTuple

import numpy as np
import torch

import beam_refs as BR
import lm_refs as LR
from beam_refs import NEG, lse, kept_tokens


def f32(x):
    return float(np.float32(x))


class BruteHot:
    """phrases: token tuples; weights: relative (default 1.0); duplicates add."""

    def __init__(self, phrases, weights=None):
        weights = [1.0] * len(phrases) if weights is None else list(weights)
        self.table = {}
        for p, w in zip(phrases, weights):
            p = tuple(int(c) for c in p)
            self.table[p] = self.table.get(p, 0.0) + float(w)
        self.max_len = max((len(p) for p in self.table), default=0)
        self._emit, self._phi = {}, {}

    def emit(self, prefix):
        tail = tuple(prefix[-self.max_len:]) if self.max_len else ()
        if tail not in self._emit:
            self._emit[tail] = f32(sum(w for p, w in self.table.items() if len(p) <= len(tail) and tail[len(tail) - len(p):] == p))
        return self._emit[tail]

    def phi(self, prefix):
        tail = tuple(prefix[-self.max_len:]) if self.max_len else ()
        if tail not in self._phi:
            best = 0.0
            for p, w in self.table.items():
                for k in range(1, min(len(p) - 1, len(tail)) + 1):
                    if tail[len(tail) - k:] == p[:k]: best = max(best, w * k / len(p))
            self._phi[tail] = f32(best)
        return self._phi[tail]

    def permanent(self, prefix):
        return sum(self.emit(prefix[:j]) for j in range(1, len(prefix) + 1))


# ---- the search ------------------------------------------------------------------------------------------------------------------
def search_hot(lp, blank, W, hot, weight, lm=None, alpha=0.5, beta=1.5, token_min_logp=-5.0, beam_prune_logp=-10.0, Kmax=16):
    """One sample: lp (T, C) f32, hot a BruteHot, lm a DictLM or None.  Returns (beams, stats); beams is the final ranking, a list of
    (prefix, frames, key, acoustic total, hot)."""
    lp = np.asarray(lp, dtype=np.float32)
    T = lp.shape[0]
    alpha, beta, weight = float(alpha), float(beta), float(weight)
    boost = weight > 0.0 and bool(hot.table)
    w = weight if boost else 0.0
    wphi = (lambda pre: w * hot.phi(pre)) if boost else (lambda pre: 0.0)
    beams = [((), (), 0.0, NEG, 0.0, lm.start if lm is not None else (), 0.0)]                # (prefix, frames, pb, pnb, bonus, lm state, hot)
    st = dict(gap=math.inf, cap=0, pruned=0, folds=0, recreated=0, kept=[], live=[], max_score=0.0, candidates=set(), revoked=0,
              reranked=False, boosted=0)
    d0, u0, l0 = list(getattr(lm, 'depth', [])), getattr(lm, 'unk_hits', 0), getattr(lm, 'lookups', 0)
    seen = {()}
    for t in range(T):
        row = lp[t]
        slots, capped = kept_tokens(row, blank, token_min_logp, Kmax)
        st['cap'] += capped
        st['kept'].append(len(slots))
        lpb = float(row[blank])
        live = {b[0]: j for j, b in enumerate(beams)}
        spb, spnb = [], []
        for pre, _, pb, pnb, _, _, _ in beams:
            spb.append(lse(pb, pnb) + lpb)
            spnb.append(pnb + float(row[pre[-1]]) if pre and pre[-1] in slots else NEG)
        ext = []                                                           # (candidate index, i, class, v)
        for i, (pre, _, pb, pnb, _, _, _) in enumerate(beams):
            for k, c in enumerate(slots):
                v = float(row[c]) + (pb if pre and c == pre[-1] else lse(pb, pnb))
                j = live.get(pre + (c,))
                if j is not None:
                    spnb[j] = lse(spnb[j], v)                              # acoustic mass only: beam j keeps its bonus, state and credit
                    st['folds'] += 1
                else:
                    ext.append((W + i * Kmax + k, i, c, v))
        cands = []                                                         # (key, candidate index, how, acoustic, bonus, state, hot, w phi)
        for i, b in enumerate(beams):
            a = lse(spb[i], spnb[i])
            if a > NEG:
                p = wphi(b[0])
                cands.append((a + (b[4] + p), i, None, a, b[4], b[5], b[6], p))
        for ci, i, c, v in ext:
            if v > NEG:                                                    # (a dropped candidate takes no step)
                term, s2 = 0.0, ()
                if lm is not None:
                    q, s2 = lm.step(beams[i][5], c, True)
                    term = alpha * q + beta
                pre2 = beams[i][0] + (c,)
                e = w * hot.emit(pre2) if boost else 0.0
                nb = (beams[i][4] + term) + e
                p = wphi(pre2)
                cands.append((v + (nb + p), ci, (i, c), v, nb, s2, beams[i][6] + e, p))
        if slots:
            st['candidates'].add(len(beams) * (len(slots) + 1))
        cands = sorted(cands, key=lambda x: (-x[0], x[1]))
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
        for keyv, ci, how, a, nb, s2, h, p in surv:
            st['max_score'] = max(st['max_score'], abs(keyv), abs(a), abs(nb), abs(nb + p), abs(h))
            if how is None:
                pre, fr = beams[ci][0], beams[ci][1]
                new.append((pre, fr, spb[ci], spnb[ci], nb, s2, h))
            else:
                i, c = how
                new.append((beams[i][0] + (c,), beams[i][1] + (t,), NEG, a, nb, s2, h))
                st['revoked'] += p < wphi(beams[i][0])
                st['boosted'] += h > beams[i][6]
        stays = [b[0] for x, b in zip(surv, new) if x[2] is None]
        for x, b in zip(surv, new):
            if x[2] is not None:
                p = b[0]
                if p in seen and any(len(q) > len(p) and q[:len(p)] == p for q in stays):
                    st['recreated'] += 1
                seen.add(p)
        beams = new
        st['live'].append(len(beams))
    if hasattr(lm, 'depth'):
        st['depth'] = [a - b for a, b in zip(lm.depth, d0)]
        st['unk'], st['lookups'] = lm.unk_hits - u0, lm.lookups - l0
    out = []
    for pre, fr, pb, pnb, bonus, _, h in beams:
        a = lse(pb, pnb)
        out.append((pre, fr, a + bonus, a, h))
    if boost:                                                              # phi is dropped: the final key decides, equal keys keep their order
        order = sorted(range(len(out)), key=lambda r: (-out[r][2], r))
        st['reranked'] = order != list(range(len(out)))
        out = [out[r] for r in order]
        for x, y in zip(out, out[1:]):
            st['gap'] = min(st['gap'], x[2] - y[2])
    return out, st


class BeamsHot(NamedTuple):
    count: torch.Tensor
    tokens: torch.Tensor
    lengths: torch.Tensor
    token_frames: torch.Tensor
    scores: torch.Tensor
    logit_scores: torch.Tensor
    hot_scores: torch.Tensor


def ctc_beam_hot(log_probs, input_lengths, lm, hot, weight, blank, beam_width, nbest, token_min_logp, beam_prune_logp, max_tokens_per_frame,
                 max_len, alpha, beta, stats=None):
    """lcasr_amd.hip.hot.ctc_beam_hot on CPU tensors: `lm` (a DictLM or None) in the place of the LM image and its five integers, `hot`
    (a BruteHot) in the place of the hotword image and its three.  `stats`: a list that receives the per-sample statistics (None for
    poisoned)."""
    lp = log_probs.detach().cpu().float().numpy()
    B, N, C = lp.shape
    L = int(max_len)
    out = BeamsHot(torch.zeros(B, dtype=torch.int32), torch.full((B, nbest, L), -1, dtype=torch.int32),
                   torch.zeros(B, nbest, dtype=torch.int32), torch.full((B, nbest, L), -1, dtype=torch.int32),
                   torch.full((B, nbest), NEG, dtype=torch.float64), torch.full((B, nbest), NEG, dtype=torch.float64),
                   torch.full((B, nbest), NEG, dtype=torch.float64))
    for b in range(B):
        T = N if input_lengths is None else int(input_lengths[b])
        if T > N or T < 0:
            out.scores[b] = math.nan
            out.logit_scores[b] = math.nan
            out.hot_scores[b] = math.nan
            if stats is not None: stats.append(None)
            continue
        beams, st = search_hot(lp[b, :T], blank, beam_width, hot, weight, lm, alpha, beta, token_min_logp, beam_prune_logp, max_tokens_per_frame)
        if stats is not None: stats.append(st)
        out.count[b] = min(nbest, len(beams))
        for r, (pre, fr, keyv, a, h) in enumerate(beams[:nbest]):
            n = min(len(pre), L)
            out.tokens[b, r, :n] = torch.tensor(pre[:n], dtype=torch.int32)
            out.token_frames[b, r, :n] = torch.tensor(fr[:n], dtype=torch.int32)
            out.lengths[b, r] = len(pre)
            out.scores[b, r] = keyv
            out.logit_scores[b, r] = a
            out.hot_scores[b, r] = h
    return out


# ---- phrase sets -----------------------------------------------------------------------------------------------------------------
def phrase_set(rng, V, max_len, extra=6):
    """(phrases, weights) over the tokens [0, V): a phrase that is a prefix of another (a b / a b c), one that is a suffix of another's
    interior (b c in a b c d e), a one-token phrase, a phrase given twice, a phrase of max_len tokens, and `extra` random ones of 1 to
    6 tokens.  The weights are multiples of 1/4 (so their sums and w k / len are what they are in f32 wherever len is a power of
    two; elsewhere the f32 rounding is the image's and the restatement's alike)."""
    a, b, c, d, e = (int(x) for x in rng.permutation(V)[:5]) if V >= 5 else (0, 1, 2, 3, 0)
    phrases = [(a, b), (a, b, c), (a, b, c, d, e), (b, c), (d,), (a, b), tuple(int(x) for x in rng.integers(0, V, max_len))]
    for _ in range(extra):
        phrases.append(tuple(int(x) for x in rng.integers(0, V, int(rng.integers(1, 7)))))
    weights = [float(rng.integers(1, 9)) / 4 for _ in phrases]
    return phrases, weights


def hot_pair(phrases, weights=None):
    """(HotwordSet, BruteHot) of the same phrases: the product's image and the independent definition."""
    from lcasr_amd.decoding.hotwords import HotwordSet
    return HotwordSet(phrases, weights), BruteHot(phrases, weights)


# ---- the usefulness case ---------------------------------------------------------------------------------------------------------
USEFUL_PHRASE = (5, 2, 8)
USEFUL_SEEDS = (0, 1, 2, 3)
USEFUL_WEIGHT = 4.0


def usefulness_case(seed, N=96, margin=0.6):
    """An ambiguous spiky input in the style of lm_refs.usefulness_case: 12 tokens, C = 16, the blank 15, classes 12 to 14 at -30;
    unit noise; a label at every frame with t % 3 == 1, the blank raised by 6 elsewhere.  The labels are seeded tokens other than
    the phrase's with USEFUL_PHRASE planted every eighth label; an ordinary label is raised by 6, a token of the phrase is set to 5 and a
    competitor (token 11) to 5 + 0.85 .. 1.15 margin in the same frame: each token of the phrase is second-best by a small margin.
    Returns (log_probs (1, N, 16), labels)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(1, N, 16, generator=g)
    x[..., 12:15] = -30.0
    others = [c for c in range(11) if c not in USEFUL_PHRASE]
    labels = []
    for t in range(N):
        if t % 3 == 1:
            k = len(labels)
            if k % 8 in (2, 3, 4):
                c = USEFUL_PHRASE[k % 8 - 2]
                x[0, t, c] = 5.0                                           # (set, not added: the noise does not decide these frames)
                x[0, t, 11] = 5.0 + margin * (0.85 + 0.3 * ((7 * k) % 11) / 11)            # (no two margins equal: no exact ties)
            else:
                c = others[int(torch.randint(0, len(others), (1,), generator=g))]
                if labels and c == labels[-1]: c = others[(others.index(c) + 1) % len(others)]
                x[0, t, c] += 6.0
            labels.append(c)
        else:
            x[0, t, 15] += 6.0
    return torch.log_softmax(x, -1).contiguous(), labels


edit_distance = LR.edit_distance
