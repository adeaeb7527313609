"""Confidence scores: how sure the model is of each frame, token and word it decoded.

The measures are those of NeMo's `ConfidenceConfig` (maximum probability, and the Shannon, Tsallis and Renyi entropies of the
frame's posterior, normalised so that a one-hot frame scores 1 and a uniform one 0), computed on the GPU (csrc/confid.hip through
hip/confid.py; include/sconf_confid.h holds the exact contract) with no host loop: one kernel gives every frame's confidence and
argmax, one collapses the argmax vector into labels with their frames, one aggregates spans - frames into tokens, tokens into words.

    cfg = ConfidenceConfig()                                  # Tsallis entropy, alpha 1/3, exp-normalised, min over a token's frames
    g = greedy_confidence(log_probs, blank, cfg)              # tokens, spans, token_confidence, frame_confidence
    words = word_confidence(g.tokens, g.token_confidence, tokenizer, cfg)

`temperature=` on frame_confidence and greedy_confidence takes the confidences of softmax(log_probs / temperature) instead (through the
temperature sweep of csrc/calib.hip with one temperature); decoding/calibration.py holds the calibration against error labels and the
fit of that temperature; decoding/posterior.py holds the posterior confidences, which read the CTC likelihood of the competing
strings instead of the shape of single frames."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, List, NamedTuple, Optional, Tuple

import torch

from ..hip import calib as calib_kernels            # the temperature sweep, reached only where a temperature is given
from ..hip import confid as confid_kernels          # the HIP op layer (tests swap its three ops for the numpy restatement)
from .beam import _word_groups

METHODS = ('entropy', 'max_prob')
ENTROPY_TYPES = ('tsallis', 'renyi', 'shannon')
ENTROPY_NORMS = ('exp', 'lin')
AGGREGATIONS = ('min', 'mean', 'max', 'prod')


@dataclass(frozen=True)
class ConfidenceConfig:
    """method 'entropy' (entropy_type 'tsallis' | 'renyi' | 'shannon' with alpha, normalised entropy_norm 'exp' | 'lin') or 'max_prob'
    (linearly normalised; entropy_type, alpha and entropy_norm are not read).  alpha in (0, 1) or (1, 4]; exactly 1 is Shannon.
    aggregation ('min' | 'mean' | 'max' | 'prod'): frames into a token; exclude_blank: without the token's blank frames (all of its
    frames where it has no other).  word_aggregation: tokens into a word, None: the same as aggregation."""
    method: str = 'entropy'
    entropy_type: str = 'tsallis'
    alpha: float = 1.0 / 3.0
    entropy_norm: str = 'exp'
    aggregation: str = 'min'
    exclude_blank: bool = True
    word_aggregation: Optional[str] = None

    def __post_init__(self):
        if self.method not in METHODS:
            raise ValueError(f'unknown method {self.method!r}; one of {METHODS}')
        if self.entropy_type not in ENTROPY_TYPES:
            raise ValueError(f'unknown entropy_type {self.entropy_type!r}; one of {ENTROPY_TYPES}')
        if self.entropy_norm not in ENTROPY_NORMS:
            raise ValueError(f'unknown norm {self.entropy_norm!r}; one of {ENTROPY_NORMS}')
        for a in (self.aggregation,) + (() if self.word_aggregation is None else (self.word_aggregation,)):
            if a not in AGGREGATIONS:
                raise ValueError(f'unknown aggregation {a!r}; one of {AGGREGATIONS}')
        a = float(self.alpha)
        if self.method == 'entropy' and self.entropy_type != 'shannon' and not (0.0 < a <= 4.0):
            raise ValueError(f'alpha={a:g} must be in (0, 1), 1 or (1, 4]')

    @property
    def measure(self) -> Tuple[str, str]:
        """(method, norm) as the kernel names them."""
        if self.method == 'max_prob':
            return 'max_prob', 'lin'
        return self.entropy_type, self.entropy_norm

    @property
    def words(self) -> str:
        return self.aggregation if self.word_aggregation is None else self.word_aggregation


class GreedyConfidence(NamedTuple):
    """tokens: the greedy labels, a list of ints (a list of such lists for (B, N, C) input); spans: per label (start, run_end, end)
    in frames, lists of the same shape; token_confidence: a float per label; frame_confidence: (N,) or (B, N) f32 on the device
    (NaN where a frame's scores are invalid)."""
    tokens: list
    spans: list
    token_confidence: list
    frame_confidence: torch.Tensor


def _on_device(t) -> torch.Tensor:
    if not torch.is_tensor(t):
        t = torch.as_tensor(t)
    if not t.is_cuda and torch.cuda.is_available():
        t = t.cuda()                                                       # (no GPU: the op layer refuses CPU tensors loudly)
    return t


def _inverse_temperature(temperature: float) -> torch.Tensor:
    t = float(temperature)
    if not (math.isfinite(t) and t > 0.0):
        raise ValueError(f'temperature {temperature!r} must be finite and positive')
    return torch.tensor([1.0 / t], dtype=torch.float64).to(torch.float32)


def frame_confidence(log_probs: torch.Tensor, cfg: ConfidenceConfig = ConfidenceConfig(), classes: Optional[int] = None,
                     temperature: Optional[float] = None):
    """log_probs (N, C) or (B, N, C): logits, log-probs or the log of averaged posteriors (the kernel normalises) -> (idx, conf) of
    shape (N,) or (B, N): the argmax (int32, first index on ties) and the confidence (f32) of every frame over the first `classes`
    (default C) columns.  A frame with a NaN or without a finite score gives idx -1 and conf NaN.
    temperature: the confidences of softmax(log_probs / temperature) (the argmax is the same); None: the call of today."""
    lp = _on_device(log_probs)
    if lp.dim() not in (2, 3):
        raise ValueError(f'log_probs must be (N, C) or (B, N, C), got {tuple(lp.shape)}')
    lp = lp.float()
    rows = lp.reshape(-1, lp.shape[-1]) if lp.is_contiguous() or lp.dim() == 3 else lp
    if rows.stride(-1) != 1:
        rows = rows.contiguous()
    method, norm = cfg.measure
    if temperature is None:
        idx, conf = confid_kernels.frames(rows, classes, method, norm, float(cfg.alpha))
    else:
        idx, conf = calib_kernels.frames_sweep(rows, _on_device(_inverse_temperature(temperature)), classes, method, norm, float(cfg.alpha))
    return idx.reshape(lp.shape[:-1]), conf.reshape(lp.shape[:-1])


def token_confidence(frame_conf: torch.Tensor, idx: Optional[torch.Tensor], spans: torch.Tensor, cfg: ConfidenceConfig = ConfidenceConfig(),
                     blank: int = 0) -> torch.Tensor:
    """frame_conf (N,) f32, idx (N,) int32 (frame_confidence's; may be None where cfg.exclude_blank is off), spans (S, 2) frames
    [first, one past the last) -> (S,) f32 on the device: cfg.aggregation over each span, without its blank frames if
    cfg.exclude_blank.  The spans may come from greedy runs, a forced alignment (CTCAlignment.spans) or spans_from_token_frames."""
    spans = _on_device(spans).to(torch.int32).contiguous()
    if cfg.exclude_blank and idx is None:
        raise ValueError('token_confidence: exclude_blank needs the frames\' idx')
    return confid_kernels.aggregate(frame_conf.contiguous(), spans, cfg.aggregation, idx.contiguous() if cfg.exclude_blank else None, int(blank))


def spans_from_token_frames(frames: torch.Tensor, T: int) -> torch.Tensor:
    """Beam-search token frames (S,) (CTCBeams.token_frames of one hypothesis, the frame each token was emitted at) -> spans (S, 2)
    int32: token i covers [frames[i], frames[i + 1]), the last one up to T."""
    fr = torch.as_tensor(frames).reshape(-1).to(torch.int32)
    end = torch.cat([fr[1:], torch.full((1,), int(T), dtype=torch.int32, device=fr.device)])
    return torch.stack([fr, end], dim=1).contiguous()


def greedy_confidence(log_probs: torch.Tensor, blank: int, cfg: ConfidenceConfig = ConfidenceConfig(), lengths=None,
                      temperature: Optional[float] = None) -> GreedyConfidence:
    """Greedy CTC decoding with confidences, in three launches and one copy to the host (frame_confidence stays on the device).
    temperature: as frame_confidence takes it; the tokens do not depend on it."""
    lp = _on_device(log_probs)
    single = lp.dim() == 2
    idx, conf = frame_confidence(lp[None] if single else lp, cfg, temperature=temperature)
    B, N = idx.shape
    il = None if lengths is None else torch.as_tensor(lengths).reshape(-1).to(device=idx.device, dtype=torch.int32).contiguous()
    targets, spans, tl = confid_kernels.runs(idx.contiguous(), il, int(blank), N)
    flat = (spans[:, :, (0, 2)] + (torch.arange(B, device=idx.device, dtype=torch.int32) * N)[:, None, None]).reshape(-1, 2).contiguous()
    tok = confid_kernels.aggregate(conf.reshape(-1), flat, cfg.aggregation, idx.reshape(-1) if cfg.exclude_blank else None, int(blank))
    packed = torch.cat([tl, targets.reshape(-1), spans.reshape(-1), tok.view(torch.int32)]).cpu()       # the one copy
    S = N
    n, rest = packed[:B].tolist(), packed[B:]
    tg, sp, tc = rest[:B * S].reshape(B, S), rest[B * S:4 * B * S].reshape(B, S, 3), rest[4 * B * S:].view(torch.float32).reshape(B, S)
    tokens = [tg[b, :n[b]].tolist() for b in range(B)]
    span_l = [sp[b, :n[b]].tolist() for b in range(B)]
    tconf = [tc[b, :n[b]].tolist() for b in range(B)]
    if single:
        return GreedyConfidence(tokens[0], span_l[0], tconf[0], conf[0])
    return GreedyConfidence(tokens, span_l, tconf, conf)


def word_confidence(token_ids, token_conf, tokenizer, cfg: ConfidenceConfig = ConfidenceConfig(),
                    word_start: Optional[Callable[[int], bool]] = None) -> List[float]:
    """Token confidences -> one float per word: cfg.word_aggregation (default cfg.aggregation) over the tokens of each word, grouped
    exactly as decoding.align.word_timestamps and BeamSearchCTCDecoder.decode_beams group them.  token_conf: (S,) floats, a list or
    a tensor; the aggregation runs on the device."""
    ids = [int(i) for i in (token_ids.tolist() if torch.is_tensor(token_ids) else token_ids)]
    if not ids:
        return []
    tc = _on_device(torch.as_tensor(token_conf, dtype=torch.float32).reshape(-1)).contiguous()
    if tc.shape[0] < len(ids):
        raise ValueError(f'{len(ids)} tokens but {tc.shape[0]} confidences')
    groups = _word_groups(ids, tokenizer, word_start)
    spans = _on_device(torch.tensor([[g[0], g[-1] + 1] for g in groups], dtype=torch.int32))
    return confid_kernels.aggregate(tc, spans, cfg.words, None, 0).tolist()
