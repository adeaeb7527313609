"""Numpy restatement of the forced-alignment contract (include/sconf_align.h) with the signature of lcasr_amd.hip.align.ctc_align, the
brute-force definition it is checked against, and what the CPU and GPU alignment tests share.  TEST INFRASTRUCTURE.

`viterbi` takes the state dtype as a parameter and makes the same single addition per cell, after the same strict comparisons in
the same order, so for finite inputs its path, spans and score are the kernel's bit for bit."""
import itertools

import numpy as np
import torch

NEG = -np.inf


def viterbi(lp, target, blank, dtype=np.float64):
    """One sample: lp (T, C) f32 array, target (S,) ints.  Returns (path (T,) int, score) or (None, -inf) when nothing fits."""
    lp = np.asarray(lp, dtype=np.float32)
    target = np.asarray(target, dtype=np.int64)
    T, S = lp.shape[0], len(target)
    L = 2 * S + 1
    if T == 0:
        return None, NEG
    ext = np.full(L, blank, dtype=np.int64)
    ext[1::2] = target
    skip = np.zeros(L, dtype=bool)                                        # s odd and l'[s] != l'[s - 2]
    skip[3::2] = target[1:] != target[:-1]
    em = lambda t: lp[t, ext].astype(dtype)                               # (L,): (LT) e(t, s)
    v = np.full(L, NEG, dtype=dtype)
    v[:2] = em(0)[:2]
    bp = np.zeros((T, L), dtype=np.uint8)
    neg1, neg2 = np.full(1, NEG, dtype=dtype), np.full(2, NEG, dtype=dtype)
    with np.errstate(invalid='ignore'):
        for t in range(1, T):
            best = v.copy()
            c1 = np.concatenate([neg1, v[:-1]])
            c2 = np.where(skip, np.concatenate([neg2, v[:-2]])[:L], NEG) if L > 2 else np.full(L, NEG, dtype=dtype)
            m1 = c1 > best
            best = np.where(m1, c1, best)
            m2 = c2 > best
            best = np.where(m2, c2, best)
            bp[t] = np.where(m2, 2, np.where(m1, 1, 0))
            v = (best + em(t)).astype(dtype)                              # ONE addition in the state type
    end = L - 1
    if L > 1 and v[L - 2] > v[L - 1]: end = L - 2
    score = float(v[end])
    if not score > NEG:
        return None, score
    path = np.empty(T, dtype=np.int64)
    s = end
    for t in range(T - 1, -1, -1):
        path[t] = s
        if t > 0: s -= int(bp[t, s])
    return path, score


def align_sample(lp, target, blank, dtype=np.float64):
    """(path (T,), labels (T,), spans (S, 2), token_logp (S,) f32 summed in frame order, score) of one sample; path None if infeasible."""
    lp = np.asarray(lp, dtype=np.float32)
    target = np.asarray(target, dtype=np.int64)
    path, score = viterbi(lp, target, blank, dtype)
    S = len(target)
    if path is None:
        return None, None, np.full((S, 2), -1, np.int64), np.zeros(S, np.float32), score
    labels = np.where(path & 1, target[np.minimum(path >> 1, max(S - 1, 0))] if S else blank, blank)
    spans, logp = np.full((S, 2), -1, np.int64), np.zeros(S, np.float32)
    for j in range(S):
        at = np.nonzero(path == 2 * j + 1)[0]
        spans[j] = (at[0], at[-1] + 1)
        acc = np.float32(0)
        for t in at: acc = np.float32(acc + lp[t, target[j]])
        logp[j] = acc
    return path, labels, spans, logp, score


def ctc_align(log_probs, targets, input_lengths, target_lengths, blank, dtype=np.float64):
    """lcasr_amd.hip.align.ctc_align on any device, in numpy: the five tensors of the contract, poisoned samples included."""
    from lcasr_amd.hip.align import Alignment
    dev = log_probs.device
    lp, tg = log_probs.detach().cpu().numpy(), targets.detach().cpu().numpy()
    B, N, C = lp.shape
    Smax = tg.shape[1]
    il = [N] * B if input_lengths is None else input_lengths.cpu().tolist()
    tl = [Smax] * B if target_lengths is None else target_lengths.cpu().tolist()
    path, labels = np.full((B, N), -1, np.int32), np.full((B, N), -1, np.int32)
    spans, logp, score = np.full((B, Smax, 2), -1, np.int32), np.zeros((B, Smax), np.float32), np.zeros(B, np.float64)
    for b in range(B):
        T, S = il[b], tl[b]
        if T > N or S < 0 or S > Smax or bool(((tg[b, :S] < 0) | (tg[b, :S] >= C)).any()):
            score[b] = np.nan
            continue
        p, l, sp, lg, sc = align_sample(lp[b, :T], tg[b, :S], blank, dtype)
        score[b] = sc
        if p is None: continue
        path[b, :T], labels[b, :T], spans[b, :S], logp[b, :S] = p, l, sp, lg
    return Alignment(*(torch.from_numpy(a).to(dev) for a in (path, labels, spans, logp, score)))


def state_dtype(state_bytes):
    return {8: np.float64, 4: np.float32}[state_bytes]


# ---- the definition: every frame path that collapses to the target -------------------------------------------------------------
def collapse(frames, blank):
    out, last = [], None
    for c in frames:
        if c != last and c != blank: out.append(c)
        last = c
    return out


def brute_force(lp, target, blank):
    """(best score in f64, the list of best frame-label sequences) over every label sequence of T frames that collapses to target."""
    lp = np.asarray(lp, dtype=np.float64)
    T, C = lp.shape
    best, arg = NEG, []
    for frames in itertools.product(range(C), repeat=T):
        if collapse(frames, blank) != list(target): continue
        sc = float(sum(lp[t, c] for t, c in enumerate(frames)))
        if sc > best: best, arg = sc, [frames]
        elif sc == best: arg.append(frames)
    return best, arg


def feasible(T, target):
    return T >= len(target) + repeats_of(list(target)) and T > 0


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def random_targets(g, B, Smax, C, repeats=0):
    """(B, Smax) int32 labels in [0, C - 1) (C - 1 is the blank) with NO adjacent equal labels, then `repeats` planted per row."""
    step = torch.randint(1, max(C - 1, 2), (B, Smax), generator=g)
    tg = (torch.randint(0, C - 1, (B, 1), generator=g) + step.cumsum(1)) % (C - 1)
    for b in range(B):
        for j in torch.randperm(max(Smax - 1, 0), generator=g)[:repeats].sort().values.tolist()[::2]:   # (every other: runs of two)
            tg[b, j + 1] = tg[b, j]
    return tg.to(torch.int32)


def repeats_of(target):
    return sum(1 for a, b in zip(target[:-1], target[1:]) if a == b)


def random_case(seed, B, N, C, Smax, in_len=None, tg_len=None, targets=None, peaked=True, repeats=0):
    """log_probs (B, N, C) f32 (a log-softmax; `peaked` plants a plausible path so that the best path is not degenerate), targets."""
    g = torch.Generator().manual_seed(seed)
    if targets is None:
        targets = random_targets(g, B, Smax, C, repeats)
    x = torch.randn(B, N, C, generator=g)
    if peaked and Smax:
        for b in range(B):
            T = N if in_len is None else min(int(in_len[b]), N)
            S = Smax if tg_len is None else max(min(int(tg_len[b]), Smax), 0)
            if T > 0 and S > 0:
                at = (torch.arange(T) * S // T).clamp(max=S - 1)
                x[b, torch.arange(T), targets[b, at].long().clamp(0, C - 1)] += 2.0
    return torch.log_softmax(x, -1).contiguous(), targets.contiguous()
