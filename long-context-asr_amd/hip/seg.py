"""ctypes binding and tensor-level ops of CTC segmentation (include/sconf_seg.h), the thirteenth ABI unit of libsconf_hip.so: forced
alignment in which star labels absorb any audio, and a span of frames, a mean log-probability and a confidence per utterance.

Same discipline as the other units under hip/: GPU tensors in and out, outputs and workspace allocated here, the kernels enqueued on
torch's current stream, no host read, no fallback - a CPU tensor, a missing library or a failing call raises.  `tests/seg_refs.py`
restates the ops in numpy float64.  This module is imported by decoding/segment.py only."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import torch

from . import _lib
from ._lib import vp, i64, i32, f32
from .ops import _chk_log_probs, _chk_lengths, _p, _stream, _workspace, require_gpu

# name -> argtypes (status-returning launchers).  Must match include/sconf_seg.h.
PROTOTYPES = {
    'sconf_seg_align': [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, i64, i64, i32, f32, vp],
    'sconf_seg_score': [vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, i64, i64, i64, i64, vp],
}
# name -> (argtypes, restype): the queries
PLAIN = {
    'sconf_seg_star_label': ([i64], C.c_int),
    'sconf_seg_max_window': ([], C.c_int),
    'sconf_seg_score_tile': ([], C.c_int),
    'sconf_seg_workspace': ([i64, i64, i64, i64], C.c_int64),
}

_lib.register(PROTOTYPES, PLAIN)
load = _lib.load

MAX_LABELS = 65535          # sconf_lalign_max_labels(): the widest target row, stars included (held to the query by the tests)


class StarAlignment(NamedTuple):
    """What sconf_seg_align writes: path, labels (B, N) int32; spans (B, Smax, 2) int32; token_logp (B, Smax) f32; score (B) f64;
    frame_logp (B, N) f32."""
    path: torch.Tensor
    labels: torch.Tensor
    spans: torch.Tensor
    token_logp: torch.Tensor
    score: torch.Tensor
    frame_logp: torch.Tensor


class UtteranceScores(NamedTuple):
    """What sconf_seg_score writes: utt_frames (B, Umax, 2) int32; utt_logp, utt_conf (B, Umax) f32."""
    utt_frames: torch.Tensor
    utt_logp: torch.Tensor
    utt_conf: torch.Tensor


def star_label(num_classes: int) -> int:
    return int(load().sconf_seg_star_label(num_classes))


def max_window() -> int:
    return int(load().sconf_seg_max_window())


def score_tile() -> int:
    return int(load().sconf_seg_score_tile())


def seg_workspace(B: int, N: int, Smax: int, Umax: int = 0) -> int:
    n = int(load().sconf_seg_workspace(B, N, Smax, Umax))
    if n < 0:
        raise ValueError(f'seg: invalid sizes B={B} N={N} Smax={Smax} Umax={Umax}')
    return n


def align(log_probs: torch.Tensor, targets: torch.Tensor, input_lengths: Optional[torch.Tensor], target_lengths: Optional[torch.Tensor],
          blank: int, star_logp: float = 0.0) -> StarAlignment:
    """log_probs (B, N, C) f32, targets (B, Smax) int32 with the value C for a star, lengths (B,) int32 or None (= N / Smax) ->
    StarAlignment of device tensors.  See include/sconf_seg.h for the semantics."""
    B, N, Cn = _chk_log_probs(log_probs, 'seg.align')
    require_gpu(targets, 'targets')
    if targets.dtype != torch.int32 or targets.dim() != 2 or targets.shape[0] != B or not targets.is_contiguous():
        raise TypeError('seg.align: targets must be a contiguous (B, Smax) int32 tensor')
    Smax = targets.shape[1]
    if Smax > MAX_LABELS:
        raise ValueError(f'seg.align: {Smax} labels: at most {MAX_LABELS} (a lattice of {2 * MAX_LABELS + 1} states) are supported')
    if B < 1 or N < 1:
        raise ValueError(f'seg.align: empty input B={B} N={N}')
    _chk_lengths(input_lengths, B, 'seg.align', 'input_lengths')
    _chk_lengths(target_lengths, B, 'seg.align', 'target_lengths')
    dev = log_probs.device
    out = StarAlignment(torch.empty(B, N, dtype=torch.int32, device=dev), torch.empty(B, N, dtype=torch.int32, device=dev),
                        torch.empty(B, Smax, 2, dtype=torch.int32, device=dev), torch.empty(B, Smax, dtype=torch.float32, device=dev),
                        torch.empty(B, dtype=torch.float64, device=dev), torch.empty(B, N, dtype=torch.float32, device=dev))
    nbytes = seg_workspace(B, N, Smax)
    ws = _workspace(nbytes, dev)
    _lib.call('sconf_seg_align', _p(log_probs), _p(targets), _p(input_lengths), _p(target_lengths), _p(out.path), _p(out.labels),
              _p(out.spans), _p(out.token_logp), _p(out.score), _p(out.frame_logp), _p(ws), nbytes, B, N, Cn, Smax, int(blank),
              float(star_logp), _stream())
    return out


def score(spans: torch.Tensor, frame_logp: torch.Tensor, score: torch.Tensor, input_lengths: Optional[torch.Tensor],
          target_lengths: Optional[torch.Tensor], utt: torch.Tensor, utt_counts: Optional[torch.Tensor] = None,
          window: int = 30) -> UtteranceScores:
    """spans (B, Smax, 2) int32, frame_logp (B, N) f32, score (B,) f64 of `align`; utt (B, Umax, 2) int32 token ranges [j0, j1);
    utt_counts (B,) int32 or None (= Umax) -> UtteranceScores of device tensors.  See include/sconf_seg.h."""
    for t, what, dt, nd in ((spans, 'spans', torch.int32, 3), (frame_logp, 'frame_logp', torch.float32, 2), (score, 'score', torch.float64, 1),
                            (utt, 'utt', torch.int32, 3)):
        require_gpu(t, what)
        if t.dtype != dt or t.dim() != nd or not t.is_contiguous():
            raise TypeError(f'seg.score: {what} must be a contiguous {nd}-d {dt} tensor')
    B, N = frame_logp.shape
    Smax, Umax = spans.shape[1], utt.shape[1]
    if spans.shape[0] != B or spans.shape[2] != 2 or score.shape[0] != B or utt.shape[0] != B or utt.shape[2] != 2:
        raise ValueError(f'seg.score: spans {tuple(spans.shape)}, score {tuple(score.shape)} and utt {tuple(utt.shape)} do not go with '
                         f'frame_logp {tuple(frame_logp.shape)}')
    _chk_lengths(input_lengths, B, 'seg.score', 'input_lengths')
    _chk_lengths(target_lengths, B, 'seg.score', 'target_lengths')
    _chk_lengths(utt_counts, B, 'seg.score', 'utt_counts')
    dev = frame_logp.device
    out = UtteranceScores(torch.empty(B, Umax, 2, dtype=torch.int32, device=dev), torch.empty(B, Umax, dtype=torch.float32, device=dev),
                          torch.empty(B, Umax, dtype=torch.float32, device=dev))
    _lib.call('sconf_seg_score', _p(spans), _p(frame_logp), _p(score), _p(input_lengths), _p(target_lengths), _p(utt), _p(utt_counts),
              int(window), _p(out.utt_frames), _p(out.utt_logp), _p(out.utt_conf), B, N, Smax, Umax, _stream())
    return out
