"""The confidence unit (include/sconf_confid.h) restated from its formulas in numpy float64, sharing nothing with the kernels: the frame
measures, the greedy runs, the aggregation of spans and the grouping of tokens into words.  `frames32` evaluates the frame measures
with the contract's m, Z, S_a formulas in np.float32 with pairwise sums; it is used ONLY to set tolerances: for a test input
d32 = max |frames32 - frames|, and the device gets 4 d32 + 1e-6.  `op_*` wrap the restatements with the signatures of
lcasr_amd.hip.confid, on CPU tensors, for the host-logic tests.  TEST INFRASTRUCTURE."""
import math

import numpy as np
import torch

METHODS = ('max_prob', 'shannon', 'tsallis', 'renyi')
NORMS = ('lin', 'exp')
AGGS = ('mean', 'min', 'max', 'prod')
MEASURES = [(m, n) for m in METHODS for n in NORMS if (m, n) != ('max_prob', 'exp')]


def alpha32(alpha):
    """The alpha the ABI carries: a C float."""
    return float(np.float32(alpha))


def _valid(row):
    return not (np.isnan(row).any() or np.isposinf(row).any() or not np.isfinite(row).any())


def _normalise(H, hmax, V, norm, tsallis):
    if norm == 'lin':
        return 1.0 - H / hmax
    if tsallis:
        return (math.exp(-H) - math.exp(-hmax)) / (1.0 - math.exp(-hmax))
    return (V * math.exp(-H) - 1.0) / (V - 1.0)


def frame_row(row, method, norm, alpha):
    """(idx, conf) of one row of log-scores, float64, straight from the table of the header."""
    row = np.asarray(row, dtype=np.float64)
    V = row.shape[0]
    if method == 'max_prob' and norm == 'exp':
        raise ValueError('max_prob has no exp normalisation')
    if not _valid(row):
        return -1, math.nan
    idx = int(np.argmax(row))                                              # the first maximal index
    p = np.exp(row - row.max())
    p = p / p.sum()
    nz = p[p > 0]
    if method == 'max_prob':
        return idx, (V * p.max() - 1.0) / (V - 1.0)
    if method == 'shannon' or alpha == 1.0:
        return idx, _normalise(float(-(nz * np.log(nz)).sum()), math.log(V), V, norm, False)
    if not (0.0 < alpha < 1.0 or 1.0 < alpha <= 4.0):
        raise ValueError(f'alpha={alpha}')
    Sa = float((nz ** alpha).sum())
    if method == 'tsallis':
        return idx, _normalise((1.0 - Sa) / (alpha - 1.0), (1.0 - V ** (1.0 - alpha)) / (alpha - 1.0), V, norm, True)
    return idx, _normalise(math.log(Sa) / (1.0 - alpha), math.log(V), V, norm, False)


def frames(x, classes=None, method='tsallis', norm='exp', alpha=1.0 / 3.0):
    """x (M, >= classes) -> idx (M) int32, conf (M) float64."""
    x = np.asarray(x)
    classes = x.shape[1] if classes is None else classes
    out = [frame_row(r[:classes], method, norm, alpha32(alpha)) for r in x]
    return np.array([o[0] for o in out], dtype=np.int32), np.array([o[1] for o in out], dtype=np.float64)


def _pairwise(v):
    """Pairwise float32 sum along the last axis."""
    v = np.asarray(v, dtype=np.float32)
    while v.shape[-1] > 1:
        if v.shape[-1] % 2:
            v = np.concatenate([v, np.zeros(v.shape[:-1] + (1,), dtype=np.float32)], axis=-1)
        v = (v[..., 0::2] + v[..., 1::2]).astype(np.float32)
    return v[..., 0]


def frames32(x, classes=None, method='tsallis', norm='exp', alpha=1.0 / 3.0):
    """The frame confidences in float32 arithmetic (conf (M) float32, NaN for invalid rows): Z = sum e^(x - m),
    H = ln Z - sum e^(x - m)(x - m) / Z, S_a = sum e^(alpha (x - m)) / Z^alpha, every operation rounded to float32."""
    f = np.float32
    x = np.asarray(x, dtype=np.float32)
    classes = x.shape[1] if classes is None else classes
    x = x[:, :classes]
    V, a = f(classes), f(alpha)
    if method in ('tsallis', 'renyi') and a == f(1):
        method = 'shannon'
    ok = np.array([_valid(r) for r in x])
    conf = np.full(x.shape[0], np.nan, dtype=np.float32)
    if not ok.any():
        return conf
    with np.errstate(all='ignore'):
        r = x[ok]
        d = (r - r.max(axis=1, keepdims=True)).astype(f)
        e = np.exp(d).astype(f)
        Z = _pairwise(e)
        lnz = np.log(Z).astype(f)
        lnv = f(math.log(classes))
        if method == 'max_prob':
            c = ((V / Z).astype(f) - f(1)) / (V - f(1))
        else:
            if method == 'shannon':
                T = _pairwise(np.where(e > 0, e * d, f(0)).astype(f))
                H, hmax = (lnz - (T / Z).astype(f)).astype(f), lnv
            else:
                ln_sa = (np.log(_pairwise(np.exp((a * d).astype(f)).astype(f))).astype(f) - (a * lnz).astype(f)).astype(f)
                am1 = float(a) - 1.0
                if method == 'renyi':
                    H, hmax = (-ln_sa / f(am1)).astype(f), lnv
                else:
                    H, hmax = ((f(1) - np.exp(ln_sa).astype(f)) / f(am1)).astype(f), f((1.0 - math.exp(-am1 * math.log(classes))) / am1)
            if norm == 'lin':
                c = f(1) - (H / hmax).astype(f)
            elif method == 'tsallis':
                eh = f(math.exp(-float(hmax)))
                c = (np.exp(-H).astype(f) - eh) / (f(1) - eh)
            else:
                c = ((V * np.exp(-H).astype(f)).astype(f) - f(1)) / (V - f(1))
    conf[ok] = c.astype(f)
    return conf


def tolerance(x, classes, method, norm, alpha):
    """(tol, d32): the device's absolute tolerance 4 d32 + 1e-6 on this input, and d32 = max |float32 - float64 restatement|."""
    _, c64 = frames(x, classes, method, norm, alpha)
    c32 = frames32(x, classes, method, norm, alpha32(alpha))
    ok = ~np.isnan(c64)
    assert (np.isnan(c32) == ~ok).all()
    d32 = float(np.abs(c32[ok].astype(np.float64) - c64[ok]).max()) if ok.any() else 0.0
    return 4.0 * d32 + 1e-6, d32


def runs_row(idx, length, blank, s_cap):
    """One sequence: (targets (s_cap), spans (s_cap, 3), target_length), as the header defines them."""
    idx = [int(i) for i in idx]
    n = min(max(int(length), 0), len(idx))
    labels = []                                                            # [label, start, run_end]
    t = 0
    while t < n:
        c = idx[t]
        if c < 0 or c == blank:
            t += 1
            continue
        u = t
        while u < n and idx[u] == c:
            u += 1
        labels.append([c, t, u])
        t = u
    targets, spans = np.zeros(s_cap, dtype=np.int32), np.zeros((s_cap, 3), dtype=np.int32)
    for k, (c, a, b) in enumerate(labels[:s_cap]):
        targets[k] = c
        spans[k] = (a, b, labels[k + 1][1] if k + 1 < len(labels) else n)
    return targets, spans, (-1 if len(labels) > s_cap else len(labels))


def runs(idx, lengths, blank, s_cap=None):
    idx = np.asarray(idx)
    B, N = idx.shape
    s_cap = N if s_cap is None else s_cap
    out = [runs_row(idx[b], N if lengths is None else lengths[b], blank, s_cap) for b in range(B)]
    return (np.stack([o[0] for o in out]).reshape(B, s_cap), np.stack([o[1] for o in out]).reshape(B, s_cap, 3),
            np.array([o[2] for o in out], dtype=np.int32))


def aggregate(values, spans, aggregation, idx=None, blank=0):
    """out (S) float64 of values (M) over the half-open spans (S, 2); idx: skip the frames that are blank or negative."""
    values = np.asarray(values, dtype=np.float64)
    M = values.shape[0]
    out = np.full(len(spans), np.nan)
    for s, (a, b) in enumerate(np.asarray(spans).reshape(-1, 2).tolist()):
        if a < 0 or b > M or a >= b:
            continue
        frames_ = list(range(a, b))
        if idx is not None:
            kept = [t for t in frames_ if idx[t] >= 0 and idx[t] != blank]
            frames_ = kept or frames_
        v = values[frames_]
        if np.isnan(v).any():
            continue
        out[s] = {'mean': v.mean, 'min': v.min, 'max': v.max, 'prod': v.prod}[aggregation]()
    return out


def word_groups(ids, starts):
    """Positions of the tokens of each word: token k opens a word where k == 0 or starts(ids[k])."""
    groups = []
    for k, i in enumerate(ids):
        if k == 0 or starts(i):
            groups.append([k])
        else:
            groups[-1].append(k)
    return groups


def greedy(x, blank, method, norm, alpha, aggregation, exclude_blank, lengths=None):
    """x (B, N, C): per sequence (tokens, spans (S, 3), token confidences float64), and the frame confidences (B, N)."""
    x = np.asarray(x)
    B, N, C = x.shape
    idx, conf = frames(x.reshape(B * N, C), C, method, norm, alpha)
    idx, conf = idx.reshape(B, N), conf.reshape(B, N)
    tg, sp, tl = runs(idx, lengths, blank, N)
    out = []
    for b in range(B):
        n = int(tl[b])
        tc = aggregate(conf[b], sp[b, :n][:, [0, 2]], aggregation, idx[b] if exclude_blank else None, blank)
        out.append((tg[b, :n].tolist(), sp[b, :n].tolist(), tc))
    return out, conf


# ---- the ops of lcasr_amd.hip.confid on CPU tensors -----------------------------------------------------------------------------
def op_frames(x, classes=None, method='tsallis', norm='exp', alpha=1.0 / 3.0):
    idx, conf = frames(x.detach().float().numpy(), classes, method, norm, alpha)
    return torch.from_numpy(idx), torch.from_numpy(conf.astype(np.float32))


def op_runs(idx, lengths, blank, s_cap=None):
    return tuple(torch.from_numpy(a) for a in runs(idx.numpy(), None if lengths is None else lengths.tolist(), blank, s_cap))


def op_aggregate(values, spans, aggregation='min', idx=None, blank=0):
    out = aggregate(values.numpy(), spans.numpy(), aggregation, None if idx is None else idx.numpy(), blank)
    return torch.from_numpy(out.astype(np.float32))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def planted(seed=0, tokens=40, corrupted=8, classes=32, blank=31):
    """The usefulness case: `tokens` labels, each over two frames and followed by one blank frame, with peaky posteriors (0.97 on the
    label); `corrupted` of them split their mass 0.55 / 0.45 with a competitor on both frames.  -> (log_probs (N, classes) f32, labels, set of corrupted positions)."""
    rng = np.random.default_rng(seed)
    labels = []
    for _ in range(tokens):
        c = int(rng.integers(0, classes - 1))
        while labels and c == labels[-1]:
            c = int(rng.integers(0, classes - 1))
        labels.append(c)
    bad = set(rng.choice(tokens, corrupted, replace=False).tolist())
    rows = []
    for k, c in enumerate(labels):
        for _ in range(2):
            p = np.full(classes, 0.03 / (classes - 1))
            p[c] = 0.97
            if k in bad:
                other = (c + 1 + int(rng.integers(0, classes - 2))) % (classes - 1)
                rest = 0.03 / (classes - 2)
                p = np.full(classes, rest)
                p[c], p[other] = 0.55 - rest, 0.45 - rest
                p = p / p.sum()
            rows.append(p)
        p = np.full(classes, 0.03 / (classes - 1))
        p[blank] = 0.97
        rows.append(p)
    return np.log(np.array(rows)).astype(np.float32), labels, bad
