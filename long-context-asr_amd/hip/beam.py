"""ctypes binding and tensor-level op of CTC prefix beam search (include/sconf_beam.h), the fourth ABI unit of libsconf_hip.so.

Same discipline as hip/ops.py, hip/audio.py and hip/align.py: GPU tensors in and out, outputs and workspace allocated here, kernels
enqueued on torch's current stream, no fallback - a CPU tensor, a missing library or a failing call raises.  `tests/beam_refs.py`
restates the op in numpy."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import torch

from . import _lib
from ._lib import vp, i64, i32, f32, f64
from .ops import _chk_log_probs, _chk_lengths, _p, _stream, _workspace

# name -> argtypes (status-returning launchers).  Must match include/sconf_beam.h.
PROTOTYPES = {
    'sconf_beam_ctc': [vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, i64, i32, i32, i32, f32, f64, i32, i64, vp],
}
# name -> (argtypes, restype): the queries
PLAIN = {
    'sconf_beam_max_width': ([], C.c_int),
    'sconf_beam_max_tokens': ([], C.c_int),
    'sconf_beam_threads': ([i64, i64], C.c_int),
    'sconf_beam_rank_limit': ([], C.c_int),
    'sconf_beam_sort_size': ([i64], C.c_int),
    'sconf_beam_prefetch_frames': ([], C.c_int),
    'sconf_beam_workspace': ([i64, i64, i64, i64], C.c_int64),
}

_lib.register(PROTOTYPES, PLAIN)
load = _lib.load


class Beams(NamedTuple):
    """What sconf_beam_ctc writes: count (B) int32; tokens, token_frames (B, nbest, Lmax) int32; lengths (B, nbest) int32; scores
    (B, nbest) f64."""
    count: torch.Tensor
    tokens: torch.Tensor
    lengths: torch.Tensor
    token_frames: torch.Tensor
    scores: torch.Tensor


def max_width() -> int:
    return int(load().sconf_beam_max_width())


def max_tokens() -> int:
    return int(load().sconf_beam_max_tokens())


def beam_workspace(B: int, N: int, W: int, Kmax: int) -> int:
    n = int(load().sconf_beam_workspace(B, N, W, Kmax))
    if n < 0:
        raise ValueError(f'ctc_beam: invalid sizes B={B} N={N} beam_width={W} (at most {max_width()}) '
                         f'max_tokens_per_frame={Kmax} (at most {max_tokens()})')
    return n


def ctc_beam(log_probs: torch.Tensor, input_lengths: Optional[torch.Tensor], blank: int, beam_width: int, nbest: int,
             token_min_logp: float, beam_prune_logp: float, max_tokens_per_frame: int, max_len: int) -> Beams:
    """log_probs (B, N, C) f32, input_lengths (B,) int32 or None (= N) -> Beams of device tensors.  See include/sconf_beam.h for
    the semantics."""
    B, N, Cn = _chk_log_probs(log_probs, 'ctc_beam')
    if B < 1 or N < 1:
        raise ValueError(f'ctc_beam: empty input B={B} N={N}')
    _chk_lengths(input_lengths, B, 'ctc_beam', 'input_lengths')
    W, nb, K, L = int(beam_width), int(nbest), int(max_tokens_per_frame), int(max_len)
    if not 1 <= nb <= W or L < 1:
        raise ValueError(f'ctc_beam: nbest={nb} must be in 1..beam_width={W} and max_len={L} at least 1')
    nbytes = beam_workspace(B, N, W, K)
    dev = log_probs.device
    out = Beams(torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, nb, L, dtype=torch.int32, device=dev),
                torch.empty(B, nb, dtype=torch.int32, device=dev), torch.empty(B, nb, L, dtype=torch.int32, device=dev),
                torch.empty(B, nb, dtype=torch.float64, device=dev))
    ws = _workspace(nbytes, dev)
    _lib.call('sconf_beam_ctc', _p(log_probs), _p(input_lengths), _p(out.count), _p(out.tokens), _p(out.lengths), _p(out.token_frames),
              _p(out.scores), _p(ws), nbytes, B, N, Cn, int(blank), W, nb, float(token_min_logp), float(beam_prune_logp), K, L, _stream())
    return out
