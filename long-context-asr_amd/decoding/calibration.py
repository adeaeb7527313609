"""Calibration of confidence scores: do the numbers of decoding/confidence.py mean anything?

Two pieces run on the GPU (csrc/calib.hip through hip/calib.py; include/sconf_calib.h holds the exact contracts): the edit alignment
that says WHICH hypothesis tokens are wrong, and the frame confidences at K softmax temperatures from one pass over the log-scores.
The figures on top of them - normalised cross entropy, expected calibration error, the areas under the ROC and the precision-recall
curves - are small tensor arithmetic in float64.

    labels = error_labels(hyp_ids, ref_ids)                          # 1: a hit, 0: substituted or inserted
    idx, conf = frame_confidence_sweep(log_probs, temperatures, cfg) # conf (K, N): row k feeds token_confidence unchanged
    t = fit_temperature(conf_by_temperature, labels, temperatures)   # the grid point with the highest NCE

Posterior confidences are decoding/posterior.py; eval.run.calibrate(posterior=True) scores them with calibration_metrics beside
the measures here.  Not part of it: calibration maps other than a temperature, and n-best or lattice word posteriors."""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import torch

from ..hip import calib as calib_kernels          # the HIP op layer (tests swap its two ops for the numpy restatement)
from .confidence import ConfidenceConfig, _on_device

METRICS = ('n', 'n_nan', 'accuracy', 'nce', 'ece', 'auroc', 'aupr', 'aupr_errors')


def error_labels(hyp_ids: Sequence[int], ref_ids: Sequence[int]) -> torch.Tensor:
    """(len(hyp_ids),) int32 on the device: 1 where the hypothesis token is a hit of the edit alignment against ref_ids, 0 where it
    is substituted or inserted.  One launch of the alignment kernel; the comparison runs on the device as well."""
    from ..eval.wer import edit_alignment_on_device
    h, _, r, _, h2r, _, _ = edit_alignment_on_device([[int(i) for i in hyp_ids]], [[int(i) for i in ref_ids]])
    if h.numel() == 0:
        return torch.zeros(0, dtype=torch.int32, device=h.device)
    if r.numel() == 0:
        return torch.zeros_like(h)
    aligned = h2r >= 0
    return (aligned & (r[h2r.clamp(min=0).long()] == h)).to(torch.int32)


def inverse_temperatures(temperatures: Sequence[float]) -> torch.Tensor:
    """(K,) float32 on the host: 1 / T for every temperature, each finite and positive."""
    ts = [float(t) for t in temperatures]
    if not ts:
        raise ValueError('no temperatures')
    for t in ts:
        if not (math.isfinite(t) and t > 0.0):
            raise ValueError(f'temperature {t!r} must be finite and positive')
    return torch.tensor([1.0 / t for t in ts], dtype=torch.float64).to(torch.float32)


def frame_confidence_sweep(log_probs: torch.Tensor, temperatures: Sequence[float], cfg: ConfidenceConfig = ConfidenceConfig(),
                           classes: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """decoding.confidence.frame_confidence at every temperature of `temperatures` in ONE pass over the rows: log_probs (N, C) or
    (B, N, C) -> (idx of shape (N,) or (B, N), conf of shape (K, N) or (K, B, N)), conf[k] the confidences of
    softmax(log_probs / temperatures[k]).  The argmax does not depend on the temperature; a temperature of exactly 1 gives
    frame_confidence's bits.  Up to sconf_calib_max_temps() temperatures per launch, more in groups."""
    lp = _on_device(log_probs)
    if lp.dim() not in (2, 3):
        raise ValueError(f'log_probs must be (N, C) or (B, N, C), got {tuple(lp.shape)}')
    inv = _on_device(inverse_temperatures(temperatures))
    lp = lp.float()
    rows = lp.reshape(-1, lp.shape[-1]) if lp.is_contiguous() or lp.dim() == 3 else lp
    if rows.stride(-1) != 1:
        rows = rows.contiguous()
    method, norm = cfg.measure
    group = calib_kernels.max_temps()
    idx, parts = None, []
    for k0 in range(0, inv.shape[0], group):
        idx, conf = calib_kernels.frames_sweep(rows, inv[k0:k0 + group].contiguous(), classes, method, norm, float(cfg.alpha))
        parts.append(conf)
    conf = parts[0] if len(parts) == 1 else torch.cat(parts)
    return idx.reshape(lp.shape[:-1]), conf.reshape((inv.shape[0],) + tuple(lp.shape[:-1]))


def _average_precision(score: torch.Tensor, positive: torch.Tensor) -> float:
    """The area under the precision-recall curve as the sum over the distinct thresholds, from the highest score down, of
    (recall_k - recall_(k-1)) precision_k; samples with equal scores enter together."""
    values, inverse = torch.unique(score, return_inverse=True)               # ascending
    pos = torch.zeros(values.shape[0], dtype=torch.float64, device=score.device).index_add_(0, inverse, positive)
    cnt = torch.zeros(values.shape[0], dtype=torch.float64, device=score.device).index_add_(0, inverse, torch.ones_like(positive))
    tp = torch.cumsum(pos.flip(0), 0)
    seen = torch.cumsum(cnt.flip(0), 0)
    return float((pos.flip(0) / positive.sum() * (tp / seen)).sum())


def calibration_metrics(conf, correct, n_bins: int = 10) -> dict:
    """How well `conf` (a confidence per sample) predicts `correct` (1 / 0 per sample), in float64 torch arithmetic:
      n, n_nan     samples used, and samples dropped because their confidence is NaN
      accuracy     the mean of correct
      nce          normalised cross entropy (H(y) - CE) / H(y), conf clamped into [1e-6, 1 - 1e-6]: 1 perfect, 0 no better than
                   the base rate, negative worse than it
      ece          expected calibration error over n_bins equal-width bins of [0, 1]: sum_b n_b / n |accuracy_b - mean conf_b|
      auroc        the probability that a correct sample scores above a wrong one, ties counted as a half
      aupr         area under the precision-recall curve of detecting the correct samples by conf
      aupr_errors  the same for detecting the wrong samples by 1 - conf
    A sample with a single class (all correct or all wrong, or empty) gives NaN for nce and the three areas."""
    c = torch.as_tensor(conf).detach().reshape(-1).to(torch.float64)
    y = torch.as_tensor(correct).detach().reshape(-1).to(device=c.device, dtype=torch.float64)
    if c.shape != y.shape:
        raise ValueError(f'{c.shape[0]} confidences but {y.shape[0]} labels')
    if n_bins < 1:
        raise ValueError(f'n_bins must be at least 1, got {n_bins}')
    keep = ~torch.isnan(c)
    n_nan = int((~keep).sum())
    c, y = c[keep], y[keep]
    n = int(c.shape[0])
    out = {'n': n, 'n_nan': n_nan, 'accuracy': math.nan, 'nce': math.nan, 'ece': math.nan, 'auroc': math.nan, 'aupr': math.nan,
           'aupr_errors': math.nan}
    if n == 0:
        return out
    n_pos = float(y.sum())
    n_neg = n - n_pos
    acc = n_pos / n
    out['accuracy'] = acc
    bins = torch.clamp((c * n_bins).floor().long(), 0, n_bins - 1)
    zeros = torch.zeros(n_bins, dtype=torch.float64, device=c.device)
    cnt = zeros.clone().index_add_(0, bins, torch.ones_like(c))
    gap = (zeros.clone().index_add_(0, bins, y) - zeros.clone().index_add_(0, bins, c)).abs()     # n_b |acc_b - conf_b|
    out['ece'] = float(gap[cnt > 0].sum() / n)
    if n_pos == 0 or n_neg == 0:
        return out
    p = c.clamp(1e-6, 1.0 - 1e-6)
    ce = -float((y * p.log() + (1.0 - y) * (1.0 - p).log()).mean())
    hy = -(acc * math.log(acc) + (1.0 - acc) * math.log(1.0 - acc))
    out['nce'] = (hy - ce) / hy
    values, inverse, counts = torch.unique(c, return_inverse=True, return_counts=True)
    counts = counts.to(torch.float64)
    rank = (torch.cumsum(counts, 0) - counts + (counts + 1.0) / 2.0)[inverse]                     # mid-ranks from 1: a tie is a half
    out['auroc'] = (float(rank[y > 0].sum()) - n_pos * (n_pos + 1.0) / 2.0) / (n_pos * n_neg)
    out['aupr'] = _average_precision(c, y)
    out['aupr_errors'] = _average_precision(1.0 - c, 1.0 - y)
    return out


def fit_temperature(conf_by_temperature, correct, temperatures: Sequence[float], n_bins: int = 10, metrics: Optional[List[dict]] = None) -> float:
    """The temperature of the grid whose confidences (conf_by_temperature[k], any shape with len(temperatures) rows) have the highest
    NCE against `correct`.  Ties go to the temperature nearest 1 and then to the lower one; a NaN NCE loses to any number, and if
    every NCE is NaN (one class only) the rule of the ties alone decides.  metrics: the calibration_metrics of every row where the
    caller has them already."""
    ts = [float(t) for t in temperatures]
    if not ts:
        raise ValueError('no temperatures')
    if metrics is None:
        rows = torch.as_tensor(conf_by_temperature)
        if rows.shape[0] != len(ts):
            raise ValueError(f'{rows.shape[0]} rows of confidences for {len(ts)} temperatures')
        metrics = [calibration_metrics(rows[k], correct, n_bins) for k in range(len(ts))]
    if len(metrics) != len(ts):
        raise ValueError(f'{len(metrics)} metrics for {len(ts)} temperatures')
    nce = [-math.inf if math.isnan(m['nce']) else m['nce'] for m in metrics]
    return min(zip(nce, ts), key=lambda v: (-v[0], abs(v[1] - 1.0), v[1]))[1]
