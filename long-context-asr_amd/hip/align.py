"""ctypes binding and tensor-level op of CTC forced alignment (include/sconf_align.h), the third ABI unit of libsconf_hip.so.

Same discipline as hip/ops.py and hip/audio.py: GPU tensors in and out, outputs and workspace allocated here, kernels enqueued on
torch's current stream, no fallback - a CPU tensor, a missing library or a failing call raises.  `tests/align_refs.py` restates the
op in numpy."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import torch

from . import _lib
from ._lib import vp, i64, i32
from .ops import _chk_log_probs, _chk_lengths, _p, _stream, _workspace, require_gpu

# name -> argtypes (status-returning launchers).  Must match include/sconf_align.h.
PROTOTYPES = {
    'sconf_align_ctc': [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, i64, i64, i32, vp],
}
# name -> (argtypes, restype): the queries
PLAIN = {
    'sconf_align_max_labels': ([], C.c_int),
    'sconf_align_state_bytes': ([i64], C.c_int),
    'sconf_align_threads': ([i64], C.c_int),
    'sconf_align_states_per_thread': ([i64], C.c_int),
    'sconf_align_walk_window': ([], C.c_int),
    'sconf_align_workspace': ([i64, i64, i64], C.c_int64),
}

_lib.register(PROTOTYPES, PLAIN)
load = _lib.load


class Alignment(NamedTuple):
    """What sconf_align_ctc writes: path, labels (B, N) int32; spans (B, Smax, 2) int32; token_logp (B, Smax) f32; score (B) f64."""
    path: torch.Tensor
    labels: torch.Tensor
    spans: torch.Tensor
    token_logp: torch.Tensor
    score: torch.Tensor


def max_labels() -> int:
    return int(load().sconf_align_max_labels())


def state_bytes(Smax: int) -> int:
    n = int(load().sconf_align_state_bytes(Smax))
    if n < 0:
        raise ValueError(f'ctc_align: {Smax} labels: at most {max_labels()} are supported')
    return n


def align_workspace(B: int, N: int, Smax: int) -> int:
    n = int(load().sconf_align_workspace(B, N, Smax))
    if n < 0:
        raise ValueError(f'ctc_align: invalid sizes B={B} N={N} Smax={Smax}')
    return n


def ctc_align(log_probs: torch.Tensor, targets: torch.Tensor, input_lengths: Optional[torch.Tensor],
              target_lengths: Optional[torch.Tensor], blank: int) -> Alignment:
    """log_probs (B, N, C) f32, targets (B, Smax) int32, lengths (B,) int32 or None (= N / Smax) -> Alignment of device tensors.
    See include/sconf_align.h for the semantics."""
    B, N, Cn = _chk_log_probs(log_probs, 'ctc_align')
    require_gpu(targets, 'targets')
    if targets.dtype != torch.int32 or targets.dim() != 2 or targets.shape[0] != B or not targets.is_contiguous():
        raise TypeError('ctc_align: targets must be a contiguous (B, Smax) int32 tensor')
    Smax = targets.shape[1]
    if Smax > max_labels():
        raise ValueError(f'ctc_align: {Smax} labels: at most {max_labels()} (a lattice of {2 * max_labels() + 1} states) are supported')
    if B < 1 or N < 1:
        raise ValueError(f'ctc_align: empty input B={B} N={N}')
    _chk_lengths(input_lengths, B, 'ctc_align', 'input_lengths')
    _chk_lengths(target_lengths, B, 'ctc_align', 'target_lengths')
    dev = log_probs.device
    out = Alignment(torch.empty(B, N, dtype=torch.int32, device=dev), torch.empty(B, N, dtype=torch.int32, device=dev),
                    torch.empty(B, Smax, 2, dtype=torch.int32, device=dev), torch.empty(B, Smax, dtype=torch.float32, device=dev),
                    torch.empty(B, dtype=torch.float64, device=dev))
    nbytes = align_workspace(B, N, Smax)
    ws = _workspace(nbytes, dev)
    _lib.call('sconf_align_ctc', _p(log_probs), _p(targets), _p(input_lengths), _p(target_lengths), _p(out.path), _p(out.labels),
              _p(out.spans), _p(out.token_logp), _p(out.score), _p(ws), nbytes, B, N, Cn, Smax, int(blank), _stream())
    return out
