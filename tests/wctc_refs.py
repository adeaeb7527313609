"""The wild-card CTC loss (include/sconf_wctc.h) restated in numpy, float64, the naive way: one lattice row per frame in log space,
rows vectorised over the states so that T = 2048 runs in seconds.  TEST INFRASTRUCTURE, plain importable module (no fixtures, no
pytest hooks).  tests/test_wctc.py holds it to autograd through the reference's own wctc_loss (tests/golden/wctc_cases.npz) at 1e-10;
the GPU tests and the footprint cases hold the kernels to it.

With ext = [blank, l_1, blank, .., l_L, blank], p_t(c) = exp(lp[t, c]):
    a_t(s) = p_t(ext_s) (a_{t-1}(s) + a_{t-1}(s-1) + [s >= 2, ext_s != ext_{s-2}] a_{t-1}(s-2) + [s <= 1]),   a_{-1} = 0
    E_t = a_t(2L-1) + a_t(2L), e_t = ln E_t;   f = ln sum_t E_t | max_t e_t | sum_t softmax(e)_t e_t;   loss = -f
    b_t(s) = [s in {2L-1, 2L}] w_t / E_t + sum over the successors s' of s of p_{t+1}(ext_s') b_{t+1}(s'),   w_t = df/de_t
    d loss / d lp[t, c] = - sum over s with ext_s = c of a_t(s) b_t(s)
w is signed in soft mode: b is carried as b+ - b-, two non-negative log-space rows (a linear recursion splits over its sources).

The departures from the reference are in: input_length is honoured (frames from there on take no part, zero gradient rows), an
infeasible sample gives +inf and zero gradient rows, frames with E_t = 0 take no part, and target_length = 0 (or a label outside
[0, C), or lengths beyond the tensors) poisons the sample: NaN loss, NaN gradient rows below input_length."""
import numpy as np

MODES = ('soft', 'max_prob', 'sum_prob')
NEG = -np.inf


def _lse(*rows):
    with np.errstate(invalid='ignore', divide='ignore'):
        m = np.max(rows, axis=0)
        m0 = np.where(np.isfinite(m), m, 0.0)
        return np.log(sum(np.exp(r - m0) for r in rows)) + m0


def _shift(row, k):
    out = np.full_like(row, NEG)
    if k > 0: out[k:] = row[:-k]
    else: out[:k] = row[-k:]
    return out


def weights(e, mode):
    """e (T) with -inf where E_t = 0 -> (f, w (T)); f = -inf when no frame is alive."""
    alive = np.isfinite(e)
    w = np.zeros_like(e)
    if not alive.any():
        return NEG, w
    ea = e[alive]
    M = ea.max()
    lse = M + np.log(np.exp(ea - M).sum())
    pi = np.exp(ea - lse)
    if mode == 'sum_prob':
        f, wa = lse, pi
    elif mode == 'max_prob':
        f, wa = M, np.zeros_like(ea)
        wa[int(np.argmax(ea))] = 1.0                     # the first maximum
    elif mode == 'soft':
        f = float((pi * ea).sum())
        wa = pi * (1.0 + ea - f)
    else:
        raise ValueError(f'bad mode {mode!r}')
    w[alive] = wa
    return float(f), w


def wctc_sample(lp, labels, blank, mode):
    """One sample over ALL rows of lp (T, C) float64, labels (L >= 1) -> (loss, grad (T, C), e (T), w (T))."""
    lp = np.asarray(lp, dtype=np.float64)
    T, C = lp.shape
    labels = np.asarray(labels, dtype=np.int64)
    L = len(labels)
    grad = np.zeros((T, C))
    if T == 0:
        return np.inf, grad, np.zeros(0), np.zeros(0)
    ext = np.full(2 * L + 1, blank, dtype=np.int64)
    ext[1::2] = labels
    n = len(ext)
    skip = np.zeros(n, dtype=bool)                       # s may be entered from s - 2
    skip[2:] = ext[2:] != ext[:-2]
    src = np.full(n, NEG)
    src[:2] = 0.0                                        # the wild-card: ln 1 into states 0 and 1 at every frame
    em = lp[:, ext]                                      # (T, n)
    la = np.full((T, n), NEG)
    prev = np.full(n, NEG)
    for t in range(T):
        prev = em[t] + _lse(prev, _shift(prev, 1), np.where(skip, _shift(prev, 2), NEG), src)
        la[t] = prev
    e = _lse(la[:, n - 2], la[:, n - 1])
    f, w = weights(e, mode)
    if f == NEG:
        return np.inf, grad, e, w
    skip_out = np.zeros(n, dtype=bool)                   # s may leave to s + 2
    skip_out[:-2] = skip[2:]
    with np.errstate(divide='ignore', invalid='ignore'):
        sinks = [np.where(w > 0, np.log(np.where(w > 0, w, 1.0)) - e, NEG), np.where(w < 0, np.log(np.where(w < 0, -w, 1.0)) - e, NEG)]
    occ = np.zeros((T, n))
    for sign, sk in ((1.0, sinks[0]), (-1.0, sinks[1])):
        if not np.isfinite(sk).any():
            continue
        g = np.full(n, NEG)                              # g_{t+1}(s) = ln p_{t+1}(ext_s) b_{t+1}(s)
        for t in range(T - 1, -1, -1):
            snk = np.full(n, NEG)
            snk[n - 2:] = sk[t]
            lb = _lse(g, _shift(g, -1), np.where(skip_out, _shift(g, -2), NEG), snk)
            with np.errstate(invalid='ignore'):
                occ[t] += sign * np.exp(np.where(np.isfinite(la[t]) & np.isfinite(lb), la[t] + lb, NEG))
            g = em[t] + lb
    for t in range(T):
        np.add.at(grad[t], ext, -occ[t])
    return -f, grad, e, w


def wctc(lp_bnc, targets, input_lengths, target_lengths, blank, mode, grad_out=None):
    """Batch-major log-probs (B, N, C), targets (B, Smax) with anything past target_lengths -> (nll (B), grad (B, N, C),
    [(e, w) per sample]), float64, with the departures of include/sconf_wctc.h."""
    lp = np.asarray(lp_bnc, dtype=np.float64)
    B, N, C = lp.shape
    targets = np.asarray(targets).reshape(B, -1)
    nll, grad, info = np.zeros(B), np.zeros((B, N, C)), []
    for b in range(B):
        T, L = int(input_lengths[b]), int(target_lengths[b])
        lab = targets[b, :max(L, 0)]
        if T <= 0:
            nll[b] = np.inf; info.append((np.zeros(0), np.zeros(0)))
        elif T > N or L < 1 or L > targets.shape[1] or (lab < 0).any() or (lab >= C).any():
            nll[b] = np.nan; grad[b, :min(T, N)] = np.nan; info.append((np.zeros(0), np.zeros(0)))
        else:
            nll[b], grad[b, :T], e, w = wctc_sample(lp[b, :T], lab, blank, mode)
            info.append((e, w))
        if grad_out is not None:
            grad[b] *= float(grad_out[b])
    return nll, grad, info
