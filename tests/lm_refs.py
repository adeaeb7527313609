"""The contract of include/sconf_lm.h in numpy / Python f64, independent of the automaton image: the yardstick of tests/test_lm.py and
tests/test_lm_gpu.py.  TEST INFRASTRUCTURE, a plain importable module.

  DictLM      an n-gram table keyed by token tuples with the plain ARPA recursion over FULL histories:
                  ln P(w | h) = logp(h w) if h w is a gram, else backoff(h) (0 if h is no gram) + ln P(w | h without its first word),
                  and unk_logp for a token without a unigram.  Values are the f32-rounded natural logs, summed in f64 in the order met.
                  Its "state" is the history itself, cut to the longest suffix that is a gram shorter than the order.
  write_arpa  a small ARPA writer (log10 values printed with 17 digits, so a reader gets the same doubles back)
  train       a count-based trainer: add-one unigrams, absolute discount 0.4 above, back-off weights that normalise
  search_lm   beam_refs.search extended by the LM (bonus, state, key = acoustic total + bonus), with the same `gap` and statistics
              plus  depth: how often a lookup ended after 0, 1, .. back-offs;  unk: lookups of a token without a unigram;
              lookups: all of them;  max_score includes |key|, |acoustic total| and |bonus|
  ctc_beam_lm lcasr_amd.hip.lm.ctc_beam_lm on CPU tensors, with a DictLM in the place of the image and its sizes."""
import math
from typing import NamedTuple

import numpy as np
import torch

import beam_refs as BR
from beam_refs import NEG, lse, kept_tokens

LN10 = math.log(10.0)


def nat32(log10_value):
    """What the ARPA reader makes of a printed log10 value: the natural log, rounded to f32 once."""
    return float(np.float32(float(log10_value) * LN10))


class DictLM:
    """grams: token tuple -> (ln p, ln backoff) (f32 values as Python floats); "<s>" is the id num_tokens."""

    def __init__(self, grams, order, num_tokens, unk_logp=None, use_bos=True):
        self.grams, self.order, self.num_tokens = dict(grams), int(order), int(num_tokens)
        self.unk = None if unk_logp is None else float(np.float32(unk_logp))
        self.start = (num_tokens,) if use_bos and (num_tokens,) in self.grams and order > 1 else ()
        self.depth = [0] * (order + 1)
        self.unk_hits = 0
        self.lookups = 0

    @classmethod
    def from_log10(cls, grams10, order, num_tokens, unk_log10=None, use_bos=True):
        g = {k: (nat32(p), nat32(b) if b is not None else 0.0) for k, (p, b) in grams10.items()}
        return cls(g, order, num_tokens, None if unk_log10 is None else nat32(unk_log10), use_bos)

    def state_of(self, history):
        """The longest suffix of the history that is a gram shorter than the order."""
        h = tuple(history)[-(self.order - 1):] if self.order > 1 else ()
        while h and h not in self.grams: h = h[1:]
        return h

    def cond(self, history, w, count=False):
        """ln P(w | history) by the recursion over the full history (up to order - 1 words)."""
        h = tuple(history)[-(self.order - 1):] if self.order > 1 else ()
        q, backoffs = 0.0, 0
        while True:
            if h + (w,) in self.grams:
                q += self.grams[h + (w,)][0]
                break
            if not h:
                q += self.unk
                if count: self.unk_hits += 1
                break
            if h in self.grams:
                q += self.grams[h][1]
                backoffs += 1                          # (a history that is no gram costs nothing and is no state of the automaton)
            h = h[1:]
        if count:
            self.depth[backoffs] += 1
            self.lookups += 1
        return q

    def step(self, state, token, count=False):
        if not 0 <= token < self.num_tokens:
            return 0.0, ()
        return self.cond(state, token, count), self.state_of(tuple(state) + (token,))

    def score(self, tokens, state=None):
        s = self.start if state is None else tuple(state)
        total = 0.0
        for c in tokens:
            q, s = self.step(s, c)
            total += q
        return total


def write_arpa(grams10, order, num_tokens, unk_log10=None, with_eos=False, word=str):
    """The lines of an ARPA file of {tuple: (log10 p, log10 backoff or None)}: the id num_tokens is written <s>, every other token
    word(token).  unk_log10: an <unk> unigram; with_eos: a </s> unigram and a bigram that ends in </s> (for a reader to drop)."""
    name = lambda w: '<s>' if w == num_tokens else word(w)
    by_n = {n: sorted(g for g in grams10 if len(g) == n) for n in range(1, order + 1)}
    extra = {1: (unk_log10 is not None) + bool(with_eos), 2: int(bool(with_eos and by_n[1]))}
    out = ['', '\\data\\'] + [f'ngram {n}={len(by_n[n]) + extra.get(n, 0)}' for n in range(1, order + 1)] + ['']
    for n in range(1, order + 1):
        out.append(f'\\{n}-grams:')
        if n == 1 and unk_log10 is not None: out.append(f'{unk_log10!r}\t<unk>')
        if n == 1 and with_eos: out.append('-1.5\t</s>')
        if n == 2 and with_eos and by_n[1]: out.append(f'-0.25\t{name(by_n[1][0][0])} </s>')
        for g in by_n[n]:
            pr, bo = grams10[g]
            out.append(f'{pr!r}\t{" ".join(name(w) for w in g)}' + (f'\t{bo!r}' if bo is not None else ''))
        out.append('')
    return out + ['\\end\\']


def train(sequences, order, num_tokens, discount=0.4, bos=False):
    """{tuple: (log10 p, log10 backoff or None)} from token sequences: unigrams (count + 1) / (N + V) for every token, above them
    p(w | h) = (count(h w) - D) / count(h) for seen grams and the back-off weight of h that makes the distribution sum to one.
    bos: each sequence is counted behind "<s>" (= num_tokens), which gets the unigram -99."""
    V = num_tokens
    counts = [dict() for _ in range(order + 1)]
    for seq in sequences:
        s = ([V] if bos else []) + [int(c) for c in seq]
        for n in range(1, order + 1):
            for i in range(len(s) - n + 1):
                g = tuple(s[i:i + n])
                if V in g[1:]: continue
                counts[n][g] = counts[n].get(g, 0) + 1
    N = sum(c for g, c in counts[1].items() if g != (V,))
    p = {(w,): (counts[1].get((w,), 0) + 1) / (N + V) for w in range(V)}
    ctx_count = [dict() for _ in range(order + 1)]                          # count of h as a context = sum of its continuations
    for n in range(2, order + 1):
        for g, c in counts[n].items():
            ctx_count[n - 1][g[:-1]] = ctx_count[n - 1].get(g[:-1], 0) + c
    for n in range(2, order + 1):
        for g, c in counts[n].items():
            p[g] = (c - discount) / ctx_count[n - 1][g[:-1]]
    bo = {}

    def lower(h, w):
        f, h = 1.0, h[1:]
        while h + (w,) not in p:
            f *= bo.get(h, 1.0)
            h = h[1:]
        return f * p[h + (w,)]

    for n in range(1, order):                                              # contexts of length n, shortest first
        for h in ctx_count[n]:
            seen = [g[-1] for g in counts[n + 1] if g[:-1] == h]
            left = 1.0 - sum(p[h + (w,)] for w in seen)
            low = 1.0 - sum(lower(h, w) for w in seen)
            bo[h] = left / low if low > 1e-12 else 1.0
    out = {}
    for g, v in p.items():
        b = bo.get(g)
        out[g] = (math.log10(v), math.log10(b) if b is not None and len(g) < order else None)
    if bos:
        b = bo.get((V,))
        out[(V,)] = (-99.0, math.log10(b) if b is not None and order > 1 else None)
    for g in list(out):                                                    # prefix closure: every context is a gram
        assert len(g) == 1 or g[:-1] in out, g
    return out


# ---- the search ------------------------------------------------------------------------------------------------------------------
def search_lm(lp, blank, W, lm, alpha=0.5, beta=1.5, token_min_logp=-5.0, beam_prune_logp=-10.0, Kmax=16):
    """One sample: lp (T, C) f32, lm a DictLM (anything with .start and .step(state, token, count)).  Returns (beams, stats); beams is
    the final ranking, a list of (prefix, frames, key, acoustic total)."""
    lp = np.asarray(lp, dtype=np.float32)
    T = lp.shape[0]
    alpha, beta = float(alpha), float(beta)
    beams = [((), (), 0.0, NEG, 0.0, lm.start)]                            # (prefix, frames, pb, pnb, bonus, lm state)
    st = dict(gap=math.inf, cap=0, pruned=0, folds=0, recreated=0, kept=[], live=[], max_score=0.0, candidates=set())
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
        for pre, _, pb, pnb, _, _ in beams:
            spb.append(lse(pb, pnb) + lpb)
            spnb.append(pnb + float(row[pre[-1]]) if pre and pre[-1] in slots else NEG)
        ext = []                                                           # (candidate index, i, class, v)
        for i, (pre, _, pb, pnb, _, _) in enumerate(beams):
            for k, c in enumerate(slots):
                v = float(row[c]) + (pb if pre and c == pre[-1] else lse(pb, pnb))
                j = live.get(pre + (c,))
                if j is not None:
                    spnb[j] = lse(spnb[j], v)                              # acoustic mass only: beam j keeps its own bonus
                    st['folds'] += 1
                else:
                    ext.append((W + i * Kmax + k, i, c, v))
        cands = []                                                         # (key, candidate index, how, acoustic, bonus, state)
        for i, b in enumerate(beams):
            a = lse(spb[i], spnb[i])
            if a > NEG: cands.append((a + b[4], i, None, a, b[4], b[5]))
        for ci, i, c, v in ext:
            if v > NEG:                                                    # (a dropped candidate takes no step)
                q, s2 = lm.step(beams[i][5], c, True)
                nb = beams[i][4] + (alpha * q + beta)
                cands.append((v + nb, ci, (i, c), v, nb, s2))
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
        for keyv, ci, how, a, nb, s2 in surv:
            st['max_score'] = max(st['max_score'], abs(keyv), abs(a), abs(nb))
            if how is None:
                pre, fr = beams[ci][0], beams[ci][1]
                new.append((pre, fr, spb[ci], spnb[ci], nb, s2))
            else:
                i, c = how
                new.append((beams[i][0] + (c,), beams[i][1] + (t,), NEG, a, nb, s2))
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
    for pre, fr, pb, pnb, bonus, _ in beams:
        a = lse(pb, pnb)
        out.append((pre, fr, a + bonus, a))
    return out, st


class BeamsLM(NamedTuple):
    count: torch.Tensor
    tokens: torch.Tensor
    lengths: torch.Tensor
    token_frames: torch.Tensor
    scores: torch.Tensor
    logit_scores: torch.Tensor


def ctc_beam_lm(log_probs, input_lengths, lm, blank, beam_width, nbest, token_min_logp, beam_prune_logp, max_tokens_per_frame, max_len,
                alpha, beta, stats=None):
    """lcasr_amd.hip.lm.ctc_beam_lm on CPU tensors, `lm` (a DictLM) in the place of the image and its five integers.  `stats`: a list
    that receives the per-sample statistics (None for poisoned)."""
    lp = log_probs.detach().cpu().float().numpy()
    B, N, C = lp.shape
    L = int(max_len)
    out = BeamsLM(torch.zeros(B, dtype=torch.int32), torch.full((B, nbest, L), -1, dtype=torch.int32),
                  torch.zeros(B, nbest, dtype=torch.int32), torch.full((B, nbest, L), -1, dtype=torch.int32),
                  torch.full((B, nbest), NEG, dtype=torch.float64), torch.full((B, nbest), NEG, dtype=torch.float64))
    for b in range(B):
        T = N if input_lengths is None else int(input_lengths[b])
        if T > N or T < 0:
            out.scores[b] = math.nan
            out.logit_scores[b] = math.nan
            if stats is not None: stats.append(None)
            continue
        beams, st = search_lm(lp[b, :T], blank, beam_width, lm, alpha, beta, token_min_logp, beam_prune_logp, max_tokens_per_frame)
        if stats is not None: stats.append(st)
        out.count[b] = min(nbest, len(beams))
        for r, (pre, fr, keyv, a) in enumerate(beams[:nbest]):
            n = min(len(pre), L)
            out.tokens[b, r, :n] = torch.tensor(pre[:n], dtype=torch.int32)
            out.token_frames[b, r, :n] = torch.tensor(fr[:n], dtype=torch.int32)
            out.lengths[b, r] = len(pre)
            out.scores[b, r] = keyv
            out.logit_scores[b, r] = a
    return out


def random_table(rng, num_tokens, order, bos, density=0.6):
    """A random prefix-closed table {tuple: (log10 p, log10 backoff or None)}: every unigram but possibly one (then <unk> is needed),
    children thinned level by level (so some grams are leaves and some contexts have no children), "<s>" grams if `bos`.  Returns
    (table, unk_log10 or None)."""
    V = num_tokens
    val = lambda: float(-rng.uniform(0.05, 3.0))
    missing = int(rng.integers(0, V)) if rng.random() < 0.5 else None
    level = [(w,) for w in range(V) if w != missing] + ([(V,)] if bos else [])
    table = {}
    for n in range(1, order + 1):
        nxt = []
        for g in level:
            has_bo = n < order and rng.random() < 0.8                       # a missing back-off column now and then
            table[g] = (-99.0 if g == (V,) else val(), val() if has_bo else None)
            if n < order and rng.random() < density:
                for w in range(V):
                    if rng.random() < density: nxt.append(g + (w,))
        level = nxt
    return table, (val() if missing is not None else None)


# ---- shared inputs ---------------------------------------------------------------------------------------------------------------
def lm_pair(table10, order, num_tokens, unk_log10=None, use_bos=True):
    """(NGramLM read from the table's ARPA text, DictLM of the same table): the product's image and the independent definition."""
    from lcasr_amd.decoding.lm import NGramLM
    img = NGramLM.from_arpa(write_arpa(table10, order, num_tokens, unk_log10), num_tokens, use_bos=use_bos)
    return img, DictLM.from_log10(table10, order, num_tokens, unk_log10, use_bos)


USEFUL_SEQ = (3, 7, 1, 9, 4, 10)
USEFUL_SEEDS = (0, 1, 2, 3, 4, 5)


def usefulness_case(seed, N=96, peak=1.0):
    """The ambiguous spiky input of the usefulness case: 12 tokens, C = 16, the blank 15, classes 12 to 14 at -30; unit noise; a label
    at every frame with t % 3 == 1 raised by peak + 2, the blank raised by peak + 4 elsewhere; the labels are USEFUL_SEQ repeated.
    Returns (log_probs (1, N, 16), labels)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(1, N, 16, generator=g)
    x[..., 12:15] = -30.0
    labels = []
    for t in range(N):
        if t % 3 == 1:
            c = USEFUL_SEQ[len(labels) % len(USEFUL_SEQ)]
            x[0, t, c] += peak + 2.0
            labels.append(c)
        else:
            x[0, t, 15] += peak + 4.0
    return torch.log_softmax(x, -1).contiguous(), labels


def usefulness_table():
    """The trigram trained on the label stream."""
    return train([list(USEFUL_SEQ) * 32], 3, 12)


def edit_distance(a, b):
    d = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        prev, d[0] = d[0], i
        for j, y in enumerate(b, 1):
            prev, d[j] = d[j], min(d[j] + 1, d[j - 1] + 1, prev + (x != y))
    return d[len(b)]
