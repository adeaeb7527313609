"""Numpy float64 restatements of the posterior unit (include/sconf_post.h): the CTC likelihood of every string at edit distance 1
from a hypothesis.  TEST INFRASTRUCTURE, plain importable module.

Two restatements of the same numbers:
  neighbours_plain    a plain CTC forward on every edited string, batched over the neighbours of one kind (the yardstick, checked
                      against torch.nn.functional.ctc_loss in tests/test_post.py)
  neighbours_bridge   the header's recurrences over the stored rows of the hypothesis, vectorised over (slot, class), with a switch
                      for every rule of the recurrences (RULES) so that a test can show that its inputs see each of them
and on top of them the batch form with the kernels' padding and poisoning (neighbours_batch), the summary of the rows (slots), the
cut rule of the long form (cut_pieces), the tolerances of the header's contract, the inputs of the GPU parity tests (parity_case) and
the three ops of lcasr_amd.hip.post on CPU tensors (op_lattice, op_neighbours, op_slots).  All log-likelihoods are natural logs."""
import collections

import numpy as np
import torch

NINF = -np.inf
RULES = ('prev_skip', 'next_skip', 'last_term', 'start', 'del_hop', 'del_first')
STEP_ERROR_CAP = 8.0 * 2.0 ** -23            # the most sconf_post_step_error() may return


def _lae(a, b):
    with np.errstate(invalid='ignore'):
        return np.logaddexp(a, b)


def _lse(x, axis):
    """logsumexp along `axis`; an empty axis or one of -inf throughout gives -inf."""
    x = np.asarray(x, dtype=np.float64)
    if x.shape[axis] == 0:
        return np.full(np.delete(x.shape, axis), NINF)
    m = x.max(axis=axis, keepdims=True)
    m0 = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide='ignore'):
        return np.log(np.exp(x - m0).sum(axis=axis)) + np.squeeze(m0, axis)


# ---------------------------------------------------------------------------------------------------------- the plain form
def ctc_forward(lp, Y, blank):
    """lp (T, C) float64, Y (K, L) labels -> (K,) log-likelihoods of the K strings: the textbook forward recursion, all strings and
    states at once, one step per frame."""
    lp = np.asarray(lp, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.int64)
    K, L = Y.shape
    T, S = lp.shape[0], 2 * L + 1
    if T == 0:
        return np.full(K, 0.0 if L == 0 else NINF)
    ext = np.full((K, S), blank, dtype=np.int64)
    ext[:, 1::2] = Y
    hop = np.zeros((K, S), dtype=bool)
    hop[:, 3::2] = Y[:, 1:] != Y[:, :-1]
    a = np.full((K, S), NINF)
    a[:, :2] = lp[0][ext[:, :2]]
    for t in range(1, T):
        s1 = np.concatenate([np.full((K, 1), NINF), a], axis=1)[:, :S]
        s2 = np.where(hop, np.concatenate([np.full((K, 2), NINF), a], axis=1)[:, :S], NINF)
        a = lp[t][ext] + _lae(_lae(a, s1), s2)
    return _lae(a[:, -1], a[:, -2]) if L else a[:, -1]


def edited_strings(y, C, blank):
    """(substitutions (L, C, L), insertions (L + 1, C, L + 1), deletions (L, L - 1)) of y.  Column `blank` of the first two holds a
    string with a blank label in it: a placeholder the callers overwrite."""
    y = np.asarray(y, dtype=np.int64)
    L = len(y)
    sub = np.broadcast_to(y, (L, C, L)).copy()
    for i in range(L):
        sub[i, :, i] = np.arange(C)
    ins = np.stack([np.insert(np.broadcast_to(y, (C, L)), j, np.arange(C), axis=1) for j in range(L + 1)])
    dele = np.stack([np.delete(y, i) for i in range(L)]) if L else np.zeros((0, 0), dtype=np.int64)
    return sub, ins, dele


def poisoned(lp, y, blank):
    lp = np.asarray(lp)
    y = np.asarray(y, dtype=np.int64)
    return bool(np.isnan(lp).any() or (lp == np.inf).any() or (y < 0).any() or (y >= lp.shape[1]).any() or (y == blank).any())


def _report(ll, sub, ins, blank):
    """Likelihoods -> the reported ratios: NaN throughout where ll is not finite, column `blank` of the gaps 0."""
    if not np.isfinite(ll):
        return ll, np.full(sub.shape, np.nan), np.full(ins.shape, np.nan)
    ins = ins - ll
    ins[:, blank] = 0.0
    return ll, sub - ll, ins


def neighbours_plain(lp, y, blank):
    """lp (T, C), y (L,) -> (ll, sub_llr (L, C), ins_llr (L + 1, C)) by a CTC forward on every edited string."""
    lp = np.asarray(lp, dtype=np.float64)
    y = np.asarray(y, dtype=np.int64)
    L, C = len(y), lp.shape[1]
    if poisoned(lp, y, blank):
        return np.nan, np.full((L, C), np.nan), np.full((L + 1, C), np.nan)
    ll = float(ctc_forward(lp, y[None], blank)[0])
    subs, inss, dels = edited_strings(y, C, blank)
    sub = ctc_forward(lp, subs.reshape(L * C, L), blank).reshape(L, C)
    ins = ctc_forward(lp, inss.reshape((L + 1) * C, L + 1), blank).reshape(L + 1, C)
    if L:
        sub[:, blank] = ctc_forward(lp, dels, blank)
    return _report(ll, sub, ins, blank)


# ---------------------------------------------------------------------------------------------------------- the bridge form
def lattice_rows(lp, y, blank):
    """(alpha (T, S), betahat (T, S)) of y over lp (T, C), T >= 1: betahat_t(s) includes the emission at t (ATen's log_beta)."""
    T, L = lp.shape[0], len(y)
    S = 2 * L + 1
    ext = np.full(S, blank, dtype=np.int64)
    ext[1::2] = y
    fwd = np.zeros(S, dtype=bool)
    fwd[3::2] = y[1:] != y[:-1]
    bwd = np.zeros(S, dtype=bool)
    bwd[1:-2:2] = y[:-1] != y[1:]
    alpha, beta = np.full((T, S), NINF), np.full((T, S), NINF)
    alpha[0, :2] = lp[0][ext[:2]]
    beta[T - 1, -2:] = lp[T - 1][ext[-2:]]
    pad1, pad2 = np.full(1, NINF), np.full(2, NINF)
    for t in range(1, T):
        a = alpha[t - 1]
        alpha[t] = lp[t][ext] + _lae(_lae(a, np.concatenate([pad1, a])[:S]), np.where(fwd, np.concatenate([pad2, a])[:S], NINF))
        g = beta[T - t]
        beta[T - 1 - t] = lp[T - 1 - t][ext] + _lae(_lae(g, np.concatenate([g, pad1])[1:]), np.where(bwd, np.concatenate([g, pad2])[2:], NINF))
    return alpha, beta


def neighbours_bridge(lp, y, blank, off=()):
    """The same three results from the recurrences of include/sconf_post.h.  off: names of RULES to switch off - 'prev_skip' and
    'next_skip' drop the tests c != prev and c != next (the neighbouring state is always bridged), 'last_term' the term a_{T-1},
    'start' the start a_0 = lp_0(c) of p == 0, 'del_hop' the test y_{i-1} != y_{i+1} of the deletion, 'del_first' its term
    betahat_0(3)."""
    assert set(off) <= set(RULES), off
    lp = np.asarray(lp, dtype=np.float64)
    y = np.asarray(y, dtype=np.int64)
    T, C, L = lp.shape[0], lp.shape[1], len(y)
    if poisoned(lp, y, blank):
        return np.nan, np.full((L, C), np.nan), np.full((L + 1, C), np.nan)
    if T == 0:
        return _report(0.0 if L == 0 else NINF, np.full((L, C), NINF), np.full((L + 1, C), NINF), blank)
    S = 2 * L + 1
    alpha, beta = lattice_rows(lp, y, blank)
    ll = float(_lae(alpha[T - 1, S - 1], alpha[T - 1, S - 2]) if L else alpha[T - 1, 0])
    # rows: the L slots, then the L + 1 gaps
    i, j = np.arange(L), np.arange(L + 1)
    P = np.concatenate([2 * i, 2 * j])
    Q = np.concatenate([2 * i + 2, 2 * j])
    at = lambda k: np.where((k >= 0) & (k < L), y[np.clip(k, 0, max(L - 1, 0))] if L else -1, -1)
    prev = np.concatenate([at(i - 1), at(j - 1)])
    nxt = np.concatenate([at(i + 1), at(j)])
    last = np.concatenate([i == L - 1, j == L])
    c = np.arange(C)
    use_prev = (prev >= 0)[:, None] & (('prev_skip' in off) | (c[None] != prev[:, None]))
    use_next = (nxt >= 0)[:, None] & (('next_skip' in off) | (c[None] != nxt[:, None]))
    a = np.where((P == 0)[:, None] & ('start' not in off), lp[0][None], NINF)
    R = np.full((len(P), C), NINF)
    for t in range(T):
        if t > 0:
            A1, A2 = alpha[t - 1, P], alpha[t - 1, np.maximum(P - 1, 0)]
            a = lp[t][None] + _lae(_lae(a, A1[:, None]), np.where(use_prev, A2[:, None], NINF))
        if t < T - 1:
            G1, G2 = beta[t + 1, Q], beta[t + 1, np.minimum(Q + 1, S - 1)]
            R = _lae(R, a + _lae(G1[:, None], np.where(use_next, G2[:, None], NINF)))
        elif 'last_term' not in off:
            R = np.where(last[:, None], _lae(R, a), R)
    sub, ins = R[:L], R[L:]
    if L:                                                                   # the deletions, into column `blank` of the slots
        d = np.full(L, NINF)
        k = np.arange(L - 1)
        hop = (k > 0) & (('del_hop' in off) | (at(k - 1) != at(k + 1)))
        left = _lae(alpha[:T - 1, 2 * k], np.where(hop[None], alpha[:T - 1, np.maximum(2 * k - 1, 0)], NINF))
        d[:L - 1] = _lse(left + beta[1:, 2 * k + 3], axis=0)
        if L > 1 and 'del_first' not in off:
            d[0] = _lae(d[0], beta[0, 3])
        d[L - 1] = _lae(alpha[T - 1, 2 * L - 2], alpha[T - 1, 2 * L - 3] if L > 1 else NINF)
        sub = sub.copy()
        sub[:, blank] = d
    return _report(ll, sub, ins.copy(), blank)


# ---------------------------------------------------------------------------------------------------------- the batch form
def neighbours_batch(log_probs, targets, input_lengths, target_lengths, blank, C=None, off=(), form=neighbours_bridge):
    """log_probs (B, N, >= C), targets (B, Smax), the two length vectors -> (loglik (B,), sub_llr (B, Smax, C), ins_llr (B, Smax + 1, C))
    float64 as the kernels lay them out: NaN in the slots at and past target_lengths[b] and the gaps past it, NaN throughout a sample
    whose loglik is not finite, loglik NaN for a poisoned sample (a length outside its buffer included)."""
    log_probs = np.asarray(log_probs)
    targets = np.asarray(targets, dtype=np.int64)
    B, N = log_probs.shape[:2]
    C = log_probs.shape[2] if C is None else C
    Smax = targets.shape[1]
    ll = np.full(B, np.nan)
    sub, ins = np.full((B, Smax, C), np.nan), np.full((B, Smax + 1, C), np.nan)
    for b in range(B):
        T, L = int(input_lengths[b]), int(target_lengths[b])
        if not (0 <= T <= N and 0 <= L <= Smax):
            continue
        ll[b], sub[b, :L], ins[b, :L + 1] = form(log_probs[b, :T, :C].astype(np.float64), targets[b, :L], blank, **({'off': off} if off else {}))
    return ll, sub, ins


def _summary(rows, own):
    """rows (R, C), own (R,) -> (softmax(row)[own], the first argmax over the other columns, its softmax); a row with a NaN gives
    NaN, -1, NaN."""
    R, C = rows.shape
    post, alt, alt_post = np.full(R, np.nan), np.full(R, -1, dtype=np.int64), np.full(R, np.nan)
    for r in range(R):
        v = rows[r]
        if np.isnan(v).any() or not 0 <= own[r] < C:
            continue
        p = np.exp(v - _lse(v[None], axis=1)[0])
        others = np.where(np.arange(C) == own[r], -np.inf, v)
        k = int(np.flatnonzero(np.arange(C) != own[r])[0]) if np.all(others == -np.inf) else int(np.argmax(others))
        post[r], alt[r], alt_post[r] = p[own[r]], k, p[k]
    return post, alt, alt_post


def slots(sub_llr, ins_llr, targets, blank):
    """(post, alt, alt_post (B, Smax), gap_post, gap_alt, gap_alt_post (B, Smax + 1)) of the two outputs of neighbours_batch."""
    sub_llr, ins_llr = np.asarray(sub_llr, dtype=np.float64), np.asarray(ins_llr, dtype=np.float64)
    targets = np.asarray(targets, dtype=np.int64)
    B, Smax, C = sub_llr.shape
    a = _summary(sub_llr.reshape(B * Smax, C), targets.reshape(-1))
    g = _summary(ins_llr.reshape(B * (Smax + 1), C), np.full(B * (Smax + 1), blank))
    return tuple(v.reshape(B, Smax) for v in a) + tuple(v.reshape(B, Smax + 1) for v in g)


def tied_rows(rows, own, tol):
    """(R,) bool: the best llr among the columns other than own[r] is finite and the second-best within tol[r] of it.  Rows with a
    NaN are not tied, nor are rows whose alternatives are all -inf: those entries agree exactly between any two evaluations, and the
    first of them is the alternative by rule."""
    R, C = rows.shape
    out = np.zeros(R, dtype=bool)
    for r in range(R):
        if np.isnan(rows[r]).any() or not 0 <= own[r] < C or C < 3:
            continue
        v = np.sort(np.delete(rows[r], own[r]))[::-1]
        out[r] = bool(np.isfinite(v[0]) and v[0] - v[1] <= tol[r])
    return out


# ---------------------------------------------------------------------------------------------------------- the contract's tolerances
def loglik_tol(T, step_error):
    return (np.asarray(T, dtype=np.float64) + 1.0) * step_error


def llr_tol(T, llr, step_error):
    with np.errstate(invalid='ignore'):
        return 2.0 * loglik_tol(T, step_error) + 2.0 ** -22 * np.maximum(1.0, np.abs(np.where(np.isfinite(llr), llr, 0.0)))


def post_tol(T, step_error):
    return 4.0 * loglik_tol(T, step_error) + 2.0 ** -22


# ---------------------------------------------------------------------------------------------------------- the long form's cut rule
def cut_pieces(spans, N, max_frames, max_labels):
    """spans: (start, run_end) of every token, in frames -> [(first token, one past the last token, first frame, one past the last
    frame)].  Greedy: the piece that begins with token k0 at frame f0 takes token k while the piece would then hold at most
    max_labels labels and end at most max_frames frames behind f0 - it ends where the next piece begins, at the midpoint
    (run_end[k] + start[k + 1]) // 2 of the pause behind its last token, or at N behind the last token of all.  A piece takes its
    first token whatever its length.  No tokens: the one piece (0, 0, 0, N)."""
    n = len(spans)
    end = lambda k: N if k == n - 1 else (int(spans[k][1]) + int(spans[k + 1][0])) // 2
    if n == 0:
        return [(0, 0, 0, int(N))]
    pieces, k0, f0 = [], 0, 0
    while k0 < n:
        k = k0 + 1
        while k < n and k - k0 + 1 <= max_labels and end(k) - f0 <= max_frames:
            k += 1
        pieces.append((k0, k, f0, end(k - 1)))
        k0, f0 = k, end(k - 1)
    return pieces


def long_form(lp, tokens, spans, blank, max_frames, max_labels):
    """The long form in float64: cut_pieces, every piece on its own frames, the token entries concatenated and of the gaps at a cut
    the one of the piece on its left -> the six vectors of `slots`, (n,) and (n + 1,)."""
    lp = np.asarray(lp, dtype=np.float64)
    tok, gap = [], []
    for p, (k0, k1, f0, f1) in enumerate(cut_pieces(spans, lp.shape[0], max_frames, max_labels)):
        y = np.asarray(tokens[k0:k1], dtype=np.int64)
        _, sub, ins = neighbours_bridge(lp[f0:f1], y, blank)
        out = slots(sub[None], ins[None], y[None], blank)
        tok.append([v[0] for v in out[:3]])
        gap.append([v[0][0 if p == 0 else 1:] for v in out[3:]])
    return tuple(np.concatenate([t[k] for t in tok]) for k in range(3)) + tuple(np.concatenate([g[k] for g in gap]) for k in range(3))


# ---------------------------------------------------------------------------------------------------------- inputs of the parity tests
def parity_case(samples, C, seed, peak=9.0, pad_frames=2, pad_labels=1):
    """A ragged batch for the GPU parity tests.  samples: (T, L) per sample.  A sample with L <= T gets a transcript without equal
    neighbours, and one `aa`-type repeat where L + 1 <= T leaves room for its blank; its rows are peaky along a sampled alignment of
    the transcript - the emitted class gets +peak on top of N(0, 1) scores before the rows are normalised, and 2 % of the other
    entries are -inf - so that the competing strings differ by whole nats and every rule of the recurrences moves some ratio.  A
    sample with L > T has no alignment (ll = -inf).  The buffers are pad_frames frames and pad_labels labels larger than the longest
    sample.  Returns (log_probs (B, N, C) float32, targets (B, Smax) int32, input_lengths, target_lengths int32, blank)."""
    rng = np.random.default_rng(seed)
    B = len(samples)
    N = max(t for t, _ in samples) + pad_frames
    Smax = max(l for _, l in samples) + pad_labels
    blank = C - 1 if seed % 2 else 0
    labels = np.array([c for c in range(C) if c != blank])
    lp = rng.normal(size=(B, N, C))
    keep = np.zeros((B, N, C), dtype=bool)
    targets = rng.choice(labels, size=(B, Smax))
    for b, (T, L) in enumerate(samples):
        y = targets[b]
        for k in range(1, L):
            while y[k] == y[k - 1]:
                y[k] = rng.choice(labels)
        if L >= 2 and L + 1 <= T:
            k = int(rng.integers(1, L))
            y[k] = y[k - 1]
            if k + 1 < L and y[k + 1] == y[k]:
                y[k + 1] = next(c for c in labels if c != y[k] and (k + 2 >= L or c != y[k + 2]))
        if L > T:
            continue
        ext = []
        for k in range(L):
            if k and y[k] == y[k - 1]:
                ext.append(blank)
            ext.append(int(y[k]))
        room = rng.multinomial(T - len(ext), np.ones(len(ext) + 1) / (len(ext) + 1))
        path = []
        for k, e in enumerate(ext):
            path += [blank] * int(room[k]) + [e]
        path += [blank] * int(room[-1])
        lp[b, np.arange(T), np.array(path, dtype=np.int64)] += peak
        keep[b, np.arange(T), np.array(path, dtype=np.int64)] = True
    lp = lp - np.log(np.exp(lp).sum(-1, keepdims=True))
    lp = np.where((rng.random(size=lp.shape) < 0.02) & ~keep, NINF, lp)
    il = np.array([t for t, _ in samples], dtype=np.int32)
    tl = np.array([l for _, l in samples], dtype=np.int32)
    return lp.astype(np.float32), targets.astype(np.int32), il, tl, blank


# The batches of tests/test_post_gpu.py: (samples, C, row stride - C, labels of padding, seed).  B = 3, ragged in both lengths, one
# sample without labels and one without an alignment in each; T over {1, 2, 3, 63, 64, 65, 130, 256} with L over {1, 2, the
# largest feasible} (L = 0 is in every batch), C over {3, 5, 129, 130, 257} and the stride over {C, C + 15}, every C with both
# strides and with short and long T.  Smax follows the longest transcript but for three batches whose padding reaches the other
# geometries of the lattice kernel: 2 states a thread (Smax 40), and 8 on 1024 threads (Smax 2100).
def _parity_table():
    table, n = [], 0
    Cs = (3, 5, 129, 130, 257)
    for T in (1, 2, 3, 63, 64, 65, 130, 256):
        for L in sorted({1, 2, T} & set(range(T + 1))):
            C = Cs[n % 5]
            table.append(([(T, L), (max(T - 1, 1), 0), (max(T - 2, 1), max(T - 2, 1) + 1)], C, 15 * ((n // 5) % 2), 1, 100 + n))
            n += 1
    table.append(([(63, 2), (60, 0), (3, 4)], 130, 0, 36, 200))
    table.append(([(3, 2), (2, 0), (1, 2)], 5, 15, 2096, 201))
    table.append(([(64, 40), (9, 0), (5, 6)], 257, 0, 2060, 202))
    return table


PARITY = _parity_table()


def parity_inputs(k):
    """Batch k of PARITY with its rows laid out at the batch's stride, NaN behind the C columns: (log_probs (B, N, stride) of which
    the kernels may read [:, :, :C], targets, input_lengths, target_lengths, blank, C)."""
    samples, C, pad, pad_labels, seed = PARITY[k]
    lp, tg, il, tl, blank = parity_case(samples, C, seed, pad_labels=pad_labels)
    wide = np.full(lp.shape[:2] + (C + pad,), np.nan, dtype=np.float32)
    wide[:, :, :C] = lp
    return wide, tg, il, tl, blank, C


# ---------------------------------------------------------------------------------------------------------- the ops on CPU tensors
Lattice = collections.namedtuple('Lattice', 'loglik workspace')


def op_lattice(log_probs, targets, input_lengths, target_lengths, blank):
    ll, _, _ = neighbours_batch(log_probs.detach().numpy(), targets.numpy(), input_lengths.tolist(), target_lengths.tolist(), int(blank))
    return Lattice(torch.from_numpy(ll), torch.zeros(0, dtype=torch.uint8))


def op_neighbours(log_probs, targets, input_lengths, target_lengths, blank, lat):
    _, sub, ins = neighbours_batch(log_probs.detach().numpy(), targets.numpy(), input_lengths.tolist(), target_lengths.tolist(), int(blank))
    return torch.from_numpy(sub.astype(np.float32)), torch.from_numpy(ins.astype(np.float32))


def op_slots(sub_llr, ins_llr, targets, blank):
    out = slots(sub_llr.numpy(), ins_llr.numpy(), targets.numpy(), int(blank))
    kinds = (np.float32, np.int32, np.float32) * 2
    return tuple(torch.from_numpy(v.astype(k)) for v, k in zip(out, kinds))
