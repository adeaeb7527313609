"""ctypes binding and tensor-level ops of the wild-card CTC loss (include/sconf_wctc.h), the eighth ABI unit of libsconf_hip.so:
the loss of transcripts that miss their audio's first and last frames, and its gradient.

Same discipline as the other units under hip/: GPU tensors in and out, outputs and workspace allocated here, kernels enqueued on
torch's current stream, no fallback - a CPU tensor, a missing library or a failing call raises.  `tests/wctc_refs.py` restates the
function in numpy, the naive way.  This module is imported by functional.py (WCTCFn / wctc_nll) only."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import vp, i64, i32
from .ops import _chk, _p, _stream, _workspace

# name -> argtypes (status-returning launchers).  Must match include/sconf_wctc.h.
PROTOTYPES = {
    'sconf_wctc_fwd': [vp, vp, vp, vp, vp, vp, i64, i64, i64, i64, i64, i32, i32, vp],
    'sconf_wctc_bwd': [vp, vp, vp, vp, vp, vp, i64, i64, i64, i64, i64, i32, i32, vp],
}
# name -> (argtypes, restype): the queries
PLAIN = {
    'sconf_wctc_max_labels': ([], C.c_int),
    'sconf_wctc_workspace': ([i64, i64, i64, i32], C.c_int64),
}

_lib.register(PROTOTYPES, PLAIN)
load = _lib.load

MODES = {'soft': 0, 'max_prob': 1, 'sum_prob': 2}    # SCONF_WCTC_* of the header (held to it by the tests)
MAX_LABELS = 2552                                    # sconf_wctc_max_labels(), for callers that check before the library is loaded


def mode_id(mode: str) -> int:
    if mode not in MODES:
        raise ValueError(f"wctc: mode must be one of {', '.join(MODES)}, got {mode!r}")
    return MODES[mode]


def max_labels() -> int:
    return int(load().sconf_wctc_max_labels())


def workspace_bytes(B: int, N: int, Smax: int, mode: str) -> int:
    n = int(load().sconf_wctc_workspace(B, N, Smax, mode_id(mode)))
    if n < 0:
        raise ValueError(f'wctc: invalid sizes B={B} N={N} Smax={Smax} (1 .. {max_labels()} labels)')
    return n


def _chk_args(targets, input_lengths, target_lengths, op: str) -> Tuple[int, int]:
    _chk(targets, 'targets', torch.int32); _chk(input_lengths, 'input_lengths', torch.int32); _chk(target_lengths, 'target_lengths', torch.int32)
    B = input_lengths.shape[0]
    if targets.dim() != 2 or targets.shape[0] != B or tuple(target_lengths.shape) != (B,) or input_lengths.dim() != 1:
        raise ValueError(f'{op}: targets (B, Smax) and lengths (B,): got {tuple(targets.shape)}, {tuple(input_lengths.shape)}, {tuple(target_lengths.shape)}')
    return B, targets.shape[1]


def wctc_fwd(log_probs: torch.Tensor, targets: torch.Tensor, input_lengths: torch.Tensor, target_lengths: torch.Tensor, blank: int,
             mode: str = 'soft') -> Tuple[torch.Tensor, torch.Tensor]:
    """log_probs (B, N, C) f32 with C % 4 == 0; targets (B, Smax) int32; lengths (B,) int32, all on the device.  Returns nll (B,) f32
    and the workspace the backward needs."""
    _chk(log_probs, 'log_probs', torch.float32)
    if log_probs.dim() != 3: raise ValueError(f'wctc_fwd: log_probs must be (B, N, C), got {tuple(log_probs.shape)}')
    B, Smax = _chk_args(targets, input_lengths, target_lengths, 'wctc_fwd')
    if log_probs.shape[0] != B: raise ValueError(f'wctc_fwd: {log_probs.shape[0]} samples of log_probs, {B} lengths')
    _, N, Cn = log_probs.shape
    nbytes = workspace_bytes(B, N, Smax, mode)
    ws = _workspace(nbytes, log_probs.device)
    nll = torch.empty(B, dtype=torch.float32, device=log_probs.device)
    _lib.call('sconf_wctc_fwd', _p(log_probs), _p(targets), _p(input_lengths), _p(target_lengths), _p(nll), _p(ws), nbytes, B, N, Cn, Smax,
              int(blank), mode_id(mode), _stream())
    return nll, ws


def wctc_bwd(shape: Tuple[int, int, int], ws: torch.Tensor, targets: torch.Tensor, input_lengths: torch.Tensor, target_lengths: torch.Tensor,
             grad_out: Optional[torch.Tensor], blank: int, mode: str = 'soft') -> torch.Tensor:
    """grad (B, N, C) f32 = grad_out[b] * d nll[b] / d log_probs from the workspace wctc_fwd filled with the same arguments
    (`shape` = log_probs.shape; the log-probs themselves are not read again).  grad_out (B,) f32 or None (= 1)."""
    B, Smax = _chk_args(targets, input_lengths, target_lengths, 'wctc_bwd')
    _chk(ws, 'workspace', torch.uint8)
    if grad_out is not None:
        _chk(grad_out, 'grad_out', torch.float32)
        if tuple(grad_out.shape) != (B,): raise ValueError(f'wctc_bwd: grad_out must be ({B},), got {tuple(grad_out.shape)}')
    Bn, N, Cn = (int(v) for v in shape)
    if Bn != B: raise ValueError(f'wctc_bwd: {Bn} samples of log_probs, {B} lengths')
    grad = torch.empty(B, N, Cn, dtype=torch.float32, device=ws.device)
    _lib.call('sconf_wctc_bwd', _p(targets), _p(input_lengths), _p(target_lengths), _p(grad_out), _p(grad), _p(ws), ws.numel(), B, N, Cn, Smax,
              int(blank), mode_id(mode), _stream())
    return grad
