"""Numpy restatement of the context-attribution ops (same signatures as lcasr_amd.hip.ctxattr), the NAIVE way: per pair (i, j) the
labels are spliced, collapsed, and scored by eval_refs.edit_counts - no boundary rows, no scan, no decomposition - so the restatement
is independent of the formulation it checks.  The means are the numpy f64 mean cast to f32.  TEST INFRASTRUCTURE."""
from typing import NamedTuple, Optional

import numpy as np
import torch

import eval_refs as E


class Scores(NamedTuple):
    errors: torch.Tensor
    clean_errors: torch.Tensor
    clean_len: torch.Tensor
    mid_len: torch.Tensor
    mid_tokens: Optional[torch.Tensor]


def collapse(labels, blank, prev=None):
    """The CTC collapse of a label sequence whose predecessor is `prev` (None: no predecessor)."""
    out = []
    for a in labels:
        a = int(a)
        if a != blank and a != prev: out.append(a)
        prev = a
    return out


def distance(h, r):
    return int(E.edit_counts(*E.ragged([h]), *E.ragged([r]))[0, 0])


def spliced(clean, row, f, g):
    s = np.array(clean, copy=True)
    s[f:g] = row[f:g]
    return s


def window_means(spec, windows):
    x = spec.cpu().numpy()
    T = x.shape[1]
    out = []
    for s, e in windows.cpu().tolist():
        s, e = min(max(s, 0), T), min(max(e, 0), T)
        out.append(np.float32(x[:, s:e].astype(np.float64).mean()) if e > s else np.float32(0))
    return torch.from_numpy(np.asarray(out, dtype=np.float32).reshape(-1)).to(spec.device)


def mask_fill(spec, windows, means, j0, b):
    T = spec.shape[1]
    dst = spec[None].repeat(b, 1, 1)
    for k in range(b):
        s, e = (min(max(int(v), 0), T) for v in windows[j0 + k].tolist())
        if e > s: dst[k, :, s:e] = means[j0 + k]
    return dst


def score(clean, masked, ref, frame_windows, blank, with_tokens=False):
    dev = clean.device
    a0, am, r = clean.cpu().numpy(), masked.cpu().numpy(), ref.cpu().numpy().tolist()
    N, J, I = len(a0), am.shape[0], len(frame_windows)
    cap = max(1, max(min(g + 1, N) - f for f, g in frame_windows))
    errors, mid_len = np.zeros((I, J), np.int32), np.zeros((I, J), np.int32)
    mid_tokens = np.zeros((I, J, cap), np.int32)
    for i, (f, g) in enumerate(frame_windows):
        ge = min(g + 1, N)
        for j in range(J):
            s = spliced(a0, am[j], f, g)
            errors[i, j] = distance(collapse(s, blank), r)
            mid = collapse(s[f:ge], blank, int(s[f - 1]) if f > 0 else None)
            mid_len[i, j] = len(mid)
            mid_tokens[i, j, :len(mid)] = mid
    hyp = collapse(a0, blank)
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int32)).to(dev)
    return Scores(t(errors), t([distance(hyp, r)]), t([len(hyp)]), t(mid_len), t(mid_tokens) if with_tokens else None)


# ---- cases ---------------------------------------------------------------------------------------------------------------------
def random_labels(rng, J, N, alphabet, blank, p_blank=0.5, p_change=0.15):
    """clean (N) and masked (J, N): clean has runs and blanks; each masked row is clean with a fraction of its frames redrawn."""
    def draw(n):
        x = rng.integers(0, alphabet, n)
        x[rng.random(n) < p_blank] = blank
        keep = rng.random(n) < 0.3                                  # repeats: a frame copies its predecessor
        for t in range(1, n):
            if keep[t]: x[t] = x[t - 1]
        return x.astype(np.int32)
    clean = draw(N)
    masked = np.repeat(clean[None], J, 0)
    for j in range(J):
        at = rng.random(N) < p_change
        masked[j, at] = draw(N)[at]
    return clean, masked


def even_windows(N, I):
    edges = [round(k * N / I) for k in range(I + 1)]
    return [(edges[k], edges[k + 1]) for k in range(I)]


# ---- the end-to-end case shared by the CPU and the GPU test: the first E2E_T frames of infer_tiny's spectrogram ------------------------
E2E_T, E2E_WINDOW = 400, 96                   # five windows, the last of 16 frames; N = 50


def gold_of(hyp, every=3):
    """A reference made from a hypothesis: every third token dropped and one foreign token in front."""
    return [126] + [t for k, t in enumerate(hyp) if k % every != 2]


def condition(errors):
    """What makes the end-to-end matrix worth comparing: some off-diagonal entry differs from the clean column."""
    W = errors.shape[0]
    return any(int(errors[i, j]) != int(errors[i, W]) for i in range(W) for j in range(W) if i != j)
