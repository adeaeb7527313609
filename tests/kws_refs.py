"""Restatements of CTC keyword search (include/sconf_kws.h) in numpy.  TEST INFRASTRUCTURE, plain importable module.

  search32 / search64   the header's formulas per keyword, in np.float32 (the contract: the device must give these bits) and in
                        float64; search64 also returns the smallest margin by which any decision that moves a start frame or a hit
                        was taken
  brute                 shares nothing with that recursion: for every start s an ordinary Viterbi over the frames s .. e, forced to
                        begin on l_1 and to end on l_L; no start frame is carried, no pair is compared
  image_search32        the walk as the kernel makes it, lane by lane from the int32 image (shifts by 1 and 2 inside a 64-lane wave,
                        masked by the flags), and `search`, the same behind the signature of lcasr_amd.hip.kws.search on CPU tensors
  planted_case          about 400 frames over 32 classes with five occurrences of a 3-label keyword: two clean, two with a label at
                        0.45 against 0.55, one with a label missing
"""
from typing import NamedTuple

import numpy as np
import torch

FIRST, SKIP, LAST = 1, 2, 4
NO_START = 2 ** 31 - 1


class Hits(NamedTuple):
    hit_frames: torch.Tensor
    hit_score: torch.Tensor
    hit_count: torch.Tensor


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def exact_case(seed, B, N, C):
    """Log-scores that are multiples of 1/8 in [-4, 0]: every llr and every sum of up to 2^17 of them is exact in f32 and f64."""
    rng = np.random.default_rng(seed)
    return (rng.integers(-32, 1, size=(B, N, C)) / 8.0).astype(np.float32)


def random_case(seed, B, N, C, scale=3.0):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(B, N, C)) * scale).astype(np.float32)


def random_phrases(seed, K, labels, lo=1, hi=4, repeats=True):
    """K phrases of lo .. hi labels out of `labels`; repeats: neighbouring labels may be equal (about one pair in three is)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(K):
        L = int(rng.integers(lo, hi + 1))
        p = [int(rng.choice(labels))]
        while len(p) < L:
            c = int(rng.choice(labels))
            if repeats and rng.random() < 1 / 3: c = p[-1]
            if not repeats and c == p[-1]: continue
            p.append(c)
        out.append(tuple(p))
    return out


# ---- the header's formulas ------------------------------------------------------------------------------------------------------
def llr(x, classes, dtype):
    """x (N, C) f32 -> (N, classes) of x - max in `dtype`; a row with a NaN, a +inf or no finite entry is -inf throughout."""
    x = np.asarray(x, dtype=np.float32)[:, :classes]
    with np.errstate(invalid='ignore'):
        m = x.max(1)
        bad = np.isnan(x).any(1) | ~np.isfinite(m)
        out = x.astype(dtype) - np.where(bad, 0, m).astype(dtype)[:, None]
    out[bad] = -np.inf
    return out


def walk(em, skip, dtype, margins=None):
    """em (T, S): llr of the states' classes; skip (S,) bool -> E (T,), b (T,) of the last state.  margins (a list): the gaps
    between the winner and every finite loser with another start frame are appended."""
    T, S = em.shape
    v = np.full(S, -np.inf, dtype=dtype)
    b = np.full(S, NO_START, dtype=np.int64)
    E, st = np.empty(T, dtype=dtype), np.empty(T, dtype=np.int64)
    cv, cb = np.empty((3, S), dtype=dtype), np.empty((3, S), dtype=np.int64)
    zero = dtype(0)
    for t in range(T):
        cv[:] = -np.inf; cb[:] = NO_START
        cv[0] = v; cb[0] = b
        cv[1, 1:] = v[:-1]; cb[1, 1:] = b[:-1]
        if S > 2:
            cv[2, 2:] = np.where(skip[2:], v[:-2], -np.inf); cb[2, 2:] = np.where(skip[2:], b[:-2], NO_START)
        cv[1, 0] = zero; cb[1, 0] = t                                     # the fresh start, state 0 only
        bv = cv.max(0)
        bb = np.where(cv == bv, cb, NO_START).min(0)                      # larger v, then smaller b
        if margins is not None:
            # (two scores that are exactly 0 are sums of exact zeros in either precision: that tie is the tie rule's, not a rounding's)
            with np.errstate(invalid='ignore'):
                gap = np.where((cb != bb) & np.isfinite(cv) & np.isfinite(bv) & ~((cv == 0) & (bv == 0)), bv - cv, np.inf)
            margins.append(float(gap.min()))
        v = (em[t] + bv).astype(dtype)
        b = bb
        E[t], st[t] = v[-1], b[-1]
    return E, st


def nms(E, st, threshold, margins=None):
    """Candidates (E_t, st_t, t + 1) with E > -inf and E >= threshold -> the list of hits (s, e, E) in time order."""
    hits, cur = [], None
    for t in range(len(E)):
        if not E[t] > -np.inf: continue
        if margins is not None: margins.append(abs(float(E[t]) - float(threshold)))
        if not E[t] >= threshold: continue
        cand = (int(st[t]), t + 1, E[t])
        if cur is not None and cand[0] >= cur[1]:
            hits.append(cur); cur = None
        if cur is not None and margins is not None and not (cand[2] == 0 and cur[2] == 0): margins.append(abs(float(cand[2]) - float(cur[2])))
        if cur is None or cand[2] > cur[2]: cur = cand
    if cur is not None: hits.append(cur)
    return hits


def _states(phrase, blank):
    ext = []
    for i, c in enumerate(phrase):
        if i: ext.append(blank)
        ext.append(int(c))
    ext = np.asarray(ext)
    skip = np.zeros(len(ext), dtype=bool)
    for s in range(2, len(ext), 2): skip[s] = ext[s] != ext[s - 2]
    return ext, skip


def _search(x, phrases, thresholds, blank, input_lengths, cap, classes, dtype, margins):
    x = np.asarray(x, dtype=np.float32)
    B, N, C = x.shape
    classes = C if classes is None else classes
    K = len(phrases)
    frames = np.full((B, K, cap, 2), -1, dtype=np.int32)
    score = np.full((B, K, cap), -np.inf, dtype=dtype)
    count = np.zeros((B, K), dtype=np.int32)
    for b in range(B):
        T = N if input_lengths is None else min(max(int(input_lengths[b]), 0), N)
        if T == 0: continue
        d = llr(x[b, :T], classes, dtype)
        for k, p in enumerate(phrases):
            ext, skip = _states(p, blank)
            E, st = walk(d[:, ext], skip, dtype, margins)
            hits = nms(E, st, dtype(np.float32(thresholds[k])), margins)
            count[b, k] = len(hits)
            for i, (s, e, v) in enumerate(hits[:cap]):
                frames[b, k, i] = (s, e); score[b, k, i] = v
    return frames, score, count


def search32(x, phrases, thresholds, blank, input_lengths=None, cap=8, classes=None):
    """x (B, N, C) f32 -> (hit_frames (B, K, cap, 2) int32, hit_score (B, K, cap) f32, hit_count (B, K) int32): THE CONTRACT."""
    return _search(x, phrases, thresholds, blank, input_lengths, cap, classes, np.float32, None)


def search64(x, phrases, thresholds, blank, input_lengths=None, cap=8, classes=None):
    """The same in float64, and the smallest margin of any decision that moves a start frame or a hit."""
    margins = []
    out = _search(x, phrases, thresholds, blank, input_lengths, cap, classes, np.float64, margins)
    return out + (min(margins, default=np.inf),)


# ---- the brute force ------------------------------------------------------------------------------------------------------------
def brute(d, phrase, blank):
    """d (T, classes) llr in float64 -> (E (T,), b (T,)): E_t the best score of any path that ends on the last frame-of-l_L at t,
    over every start; b_t the smallest start that reaches it.  One ordinary Viterbi per start, plain Python floats."""
    T = d.shape[0]
    ext = []
    for i, c in enumerate(phrase):
        if i: ext.append(blank)
        ext.append(int(c))
    S = len(ext)
    ninf = float('-inf')
    val = [[ninf] * T for _ in range(T)]                                  # val[s][t]
    for s in range(T):
        a = [ninf] * S
        a[0] = float(d[s, ext[0]])
        val[s][s] = a[S - 1]
        for t in range(s + 1, T):
            n = [ninf] * S
            for j in range(S):
                best = a[j]
                if j >= 1 and a[j - 1] > best: best = a[j - 1]
                if j >= 2 and j % 2 == 0 and ext[j] != ext[j - 2] and a[j - 2] > best: best = a[j - 2]
                n[j] = best + float(d[t, ext[j]]) if best > ninf else ninf
            a = n
            val[s][t] = a[S - 1]
    E, b = np.full(T, -np.inf), np.full(T, NO_START, dtype=np.int64)
    for t in range(T):
        col = [val[s][t] for s in range(t + 1)]
        E[t] = max(col)
        if E[t] > -np.inf: b[t] = col.index(E[t])
    return E, b


# ---- the walk as the kernel makes it: from the image, lane by lane --------------------------------------------------------------
def image_search32(x, image, n_waves, U, K, blank, input_lengths=None, cap=8, classes=None):
    x = np.asarray(x, dtype=np.float32)
    image = np.asarray(image, dtype=np.int32)
    B, N, C = x.shape
    classes = C if classes is None else classes
    ln, cols = image[:n_waves * 256].reshape(-1, 4), image[n_waves * 256:n_waves * 256 + U]
    idle = ln[:, 0] < 0
    u = np.clip(ln[:, 0], 0, U - 1)
    flags = np.where(idle, 0, ln[:, 1])
    first, skip, last = (flags & FIRST) != 0, (flags & SKIP) != 0, (flags & LAST) != 0
    kw = np.clip(ln[:, 2], 0, K - 1)
    thr = np.ascontiguousarray(ln[:, 3]).view(np.float32)
    cls = np.where(cols < 0, blank, np.minimum(cols, classes - 1))[u]
    L = ln.shape[0]
    lane = np.arange(L) % 64
    up1 = np.where(lane >= 1, np.arange(L) - 1, np.arange(L))            # __shfl_up: a lane below the shift keeps its own value
    up2 = np.where(lane >= 2, np.arange(L) - 2, np.arange(L))
    frames = np.full((B, K, cap, 2), -1, dtype=np.int32)
    score = np.full((B, K, cap), -np.inf, dtype=np.float32)
    count = np.zeros((B, K), dtype=np.int32)
    ninf = np.float32(-np.inf)
    for b in range(B):
        T = N if input_lengths is None else min(max(int(input_lengths[b]), 0), N)
        if T == 0: continue
        em = llr(x[b, :T], classes, np.float32)[:, cls]
        em[:, idle] = -np.inf
        v, st = np.full(L, ninf, dtype=np.float32), np.zeros(L, dtype=np.int64)
        cur = {}
        for t in range(T):
            bv, bb = v.copy(), st.copy()
            for cv, cb, ok in ((v[up1], st[up1], ~first), (v[up2], st[up2], skip), (np.zeros(L, dtype=np.float32), np.full(L, t), first)):
                better = ok & ((cv > bv) | ((cv == bv) & (cb < bb)))
                bv, bb = np.where(better, cv, bv), np.where(better, cb, bb)
            v, st = (em[t] + bv).astype(np.float32), bb
            for i in np.nonzero(last & (v > ninf) & (v >= thr))[0].tolist():
                k = int(kw[i])
                c = cur.get(i)
                if c is not None and st[i] >= c[1]:
                    if count[b, k] < cap: frames[b, k, count[b, k]] = c[:2]; score[b, k, count[b, k]] = c[2]
                    count[b, k] += 1; c = None
                if c is None or v[i] > c[2]: c = (int(st[i]), t + 1, v[i])
                cur[i] = c
        for i, c in cur.items():
            k = int(kw[i])
            if count[b, k] < cap: frames[b, k, count[b, k]] = c[:2]; score[b, k, count[b, k]] = c[2]
            count[b, k] += 1
    return frames, score, count


def search(x, image, n_waves, U, K, blank, input_lengths=None, cap=64, classes=None):
    """lcasr_amd.hip.kws.search on CPU tensors, through image_search32."""
    il = None if input_lengths is None else input_lengths.cpu().numpy()
    f, s, c = image_search32(x.detach().cpu().numpy(), image.cpu().numpy(), int(n_waves), int(U), int(K), int(blank), il, int(cap), classes)
    return Hits(torch.from_numpy(f), torch.from_numpy(s), torch.from_numpy(c))


# ---- the planted case -----------------------------------------------------------------------------------------------------------
PLANTED_KEYWORD, ABSENT_KEYWORD = (3, 7, 11), (5, 9, 13)


def planted_case():
    """-> (x (1, N, 32) f32 log-probs, blank, real, broken): `real` the four planted spans [s, e) of PLANTED_KEYWORD (two clean,
    two with one label at 0.45 against a competitor's 0.55), `broken` the span of an occurrence whose middle label is missing.
    Around them a greedy transcript of other labels (16 .. 30) and blanks; ABSENT_KEYWORD never occurs.  The winner of a frame has
    0.9 (a weak label 0.45, its competitor 0.55), the other classes share the rest.  A keyword's last label holds one frame, so a
    hit's end is its only best end."""
    C, blank = 32, 31
    rng = np.random.default_rng(2024)
    a, b, c = PLANTED_KEYWORD
    rows, real, broken = [], [], None                                       # rows: (winner, weak label or None)

    def filler(n):
        while n > 0:
            tok, run = (int(rng.integers(16, 31)) if rng.random() < 0.6 else blank), int(rng.integers(1, 4))
            rows.extend([(tok, None)] * min(run, n)); n -= run

    def occurrence(kind):
        s = len(rows)
        if kind == 'weak-first': rows.append((20, a))                      # l_1 at 0.45 under label 20 at 0.55
        else: rows.extend([(a, None)] * 2)
        rows.append((blank, None))
        if kind == 'weak-middle': rows.extend([(21, b)] * 2)
        elif kind == 'missing': rows.extend([(22, None)] * 2)              # another label where l_2 should be
        else: rows.extend([(b, None)] * 3)
        rows.append((c, None))
        return (s, len(rows))

    for kind in ('clean', 'weak-middle', 'missing', 'clean', 'weak-first'):
        filler(int(rng.integers(55, 75)))
        span = occurrence(kind)
        if kind == 'missing': broken = span
        else: real.append(span)
    filler(60)
    N = len(rows)
    p = np.empty((N, C))
    for t, (win, weak) in enumerate(rows):
        if weak is None:
            p[t] = 0.1 / (C - 1); p[t, win] = 0.9
        else:
            p[t] = 1e-4; p[t, win] = 0.55; p[t, weak] = 0.45
            p[t] /= p[t].sum()
    return np.log(p).astype(np.float32)[None], blank, real, broken
