"""ctypes binding and tensor-level ops of the posterior unit (include/sconf_post.h), the sixteenth ABI unit of libsconf_hip.so: the
CTC likelihood of every string at edit distance 1 from a hypothesis, as log-likelihood ratios against it, and the slot and gap
posteriors on top of them.

Same discipline as the other units under hip/: GPU tensors in and out, outputs allocated here, the kernels enqueued on torch's
current stream, no host read, no fallback - a CPU tensor, a missing library or a failing call raises.  `tests/post_refs.py`
restates the ops in numpy.  The Python caller (decoding/posterior.py) reaches `lattice`, `neighbours` and `slots` through this
module's attributes, so that a test can replace the three with the restatements."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Tuple

import torch

from . import _lib
from ._lib import vp, i64, i32
from .ops import _p, _stream, require_gpu

# name -> argtypes (status-returning launchers).  Must match include/sconf_post.h.
PROTOTYPES = {
    'sconf_post_lattice': [vp, vp, vp, vp, i64, i64, i64, i64, i64, i32, vp, i64, vp, vp],
    'sconf_post_neighbours': [vp, vp, vp, vp, i64, i64, i64, i64, i64, i32, vp, i64, vp, vp, vp, vp],
    'sconf_post_slots': [vp, vp, vp, i64, i64, i64, i32, vp, vp, vp, vp, vp, vp, vp],
}
# name -> (argtypes, restype): the queries
PLAIN = {
    'sconf_post_max_labels': ([], C.c_int),
    'sconf_post_workspace': ([i64, i64, i64], C.c_int64),
    'sconf_post_step_error': ([vp], C.c_int),
}

_lib.register(PROTOTYPES, PLAIN)
load = _lib.load


class Lattice(NamedTuple):
    """What `lattice` hands to `neighbours`: loglik (B,) f64 in nats, and the workspace that holds the alpha and betahat rows."""
    loglik: torch.Tensor
    workspace: torch.Tensor


def max_labels() -> int:
    return int(load().sconf_post_max_labels())


def step_error() -> float:
    """The per-frame error constant of the kernels in nats (include/sconf_post.h, NUMERICS): every tolerance follows from it."""
    v = C.c_double()
    if load().sconf_post_step_error(C.byref(v)) != 0:
        raise RuntimeError('sconf_post_step_error failed')
    return float(v.value)


def workspace_bytes(B: int, N: int, Smax: int) -> int:
    n = int(load().sconf_post_workspace(int(B), int(N), int(Smax)))
    if n < 0:
        raise ValueError(f'post: a batch of {B} x {N} frames with {Smax} labels; at most {max_labels()} labels, and 16 B N (2 Smax + 1) bytes below 2^62')
    return n


def _checked(log_probs, targets, input_lengths, target_lengths, blank):
    require_gpu(log_probs, 'log_probs'); require_gpu(targets, 'targets')
    require_gpu(input_lengths, 'input_lengths'); require_gpu(target_lengths, 'target_lengths')
    if log_probs.dtype != torch.float32 or log_probs.dim() != 3 or (log_probs.shape[2] > 1 and log_probs.stride(2) != 1):
        raise TypeError('post: log_probs must be a (B, N, C) float32 tensor with unit stride along C')
    B, N, Cc = log_probs.shape
    stride = log_probs.stride(1) if N > 1 else Cc
    if stride < Cc or (B > 1 and log_probs.stride(0) != N * stride):
        raise TypeError('post: the frames of log_probs must lie row_stride >= C apart and the samples N rows apart')
    if targets.dtype != torch.int32 or targets.dim() != 2 or targets.shape[0] != B or not targets.is_contiguous():
        raise TypeError('post: targets must be a contiguous (B, Smax) int32 tensor')
    for t, what in ((input_lengths, 'input_lengths'), (target_lengths, 'target_lengths')):
        if t.dtype != torch.int32 or tuple(t.shape) != (B,) or not t.is_contiguous():
            raise TypeError(f'post: {what} must be a contiguous (B,) int32 tensor')
    if not 0 <= int(blank) < Cc:
        raise ValueError(f'post: blank = {blank} for {Cc} classes')
    return B, N, Cc, stride, targets.shape[1]


def lattice(log_probs: torch.Tensor, targets: torch.Tensor, input_lengths: torch.Tensor, target_lengths: torch.Tensor, blank: int) -> Lattice:
    """log_probs (B, N, C) f32 (unit stride along C, any row stride >= C), targets (B, Smax) int32, input_lengths and target_lengths
    (B,) int32 -> Lattice(loglik (B,) f64, workspace).  One launch.  See include/sconf_post.h."""
    B, N, Cc, stride, Smax = _checked(log_probs, targets, input_lengths, target_lengths, blank)
    ws = torch.empty(workspace_bytes(B, N, Smax), dtype=torch.uint8, device=log_probs.device)
    loglik = torch.empty(B, dtype=torch.float64, device=log_probs.device)
    _lib.call('sconf_post_lattice', _p(log_probs), _p(targets), _p(input_lengths), _p(target_lengths), B, N, Cc, stride, Smax, int(blank),
              _p(ws), ws.numel(), _p(loglik), _stream())
    return Lattice(loglik, ws)


def neighbours(log_probs: torch.Tensor, targets: torch.Tensor, input_lengths: torch.Tensor, target_lengths: torch.Tensor, blank: int,
               lat: Lattice) -> Tuple[torch.Tensor, torch.Tensor]:
    """The arguments of `lattice` and what it returned -> (sub_llr (B, Smax, C), ins_llr (B, Smax + 1, C)) f32.  One launch."""
    B, N, Cc, stride, Smax = _checked(log_probs, targets, input_lengths, target_lengths, blank)
    require_gpu(lat.loglik, 'loglik'); require_gpu(lat.workspace, 'workspace')
    if lat.loglik.dtype != torch.float64 or tuple(lat.loglik.shape) != (B,) or lat.workspace.dtype != torch.uint8 or not lat.workspace.is_contiguous():
        raise TypeError('post.neighbours: lat must be what post.lattice returned for the same batch')
    sub = torch.empty(B, Smax, Cc, dtype=torch.float32, device=log_probs.device)
    ins = torch.empty(B, Smax + 1, Cc, dtype=torch.float32, device=log_probs.device)
    _lib.call('sconf_post_neighbours', _p(log_probs), _p(targets), _p(input_lengths), _p(target_lengths), B, N, Cc, stride, Smax, int(blank),
              _p(lat.workspace), lat.workspace.numel(), _p(lat.loglik), _p(sub), _p(ins), _stream())
    return sub, ins


def slots(sub_llr: torch.Tensor, ins_llr: torch.Tensor, targets: torch.Tensor, blank: int):
    """sub_llr (B, Smax, C), ins_llr (B, Smax + 1, C) f32 and targets (B, Smax) int32 -> (post, alt, alt_post) of shape (B, Smax) and
    (gap_post, gap_alt, gap_alt_post) of shape (B, Smax + 1); the alternatives int32, the posteriors f32.  One launch."""
    require_gpu(sub_llr, 'sub_llr'); require_gpu(ins_llr, 'ins_llr'); require_gpu(targets, 'targets')
    if sub_llr.dtype != torch.float32 or ins_llr.dtype != torch.float32 or sub_llr.dim() != 3 or ins_llr.dim() != 3 \
            or not sub_llr.is_contiguous() or not ins_llr.is_contiguous():
        raise TypeError('post.slots: sub_llr and ins_llr must be contiguous 3-D float32 tensors')
    B, Smax, Cc = sub_llr.shape
    if tuple(ins_llr.shape) != (B, Smax + 1, Cc) or targets.dtype != torch.int32 or tuple(targets.shape) != (B, Smax) or not targets.is_contiguous():
        raise TypeError(f'post.slots: ins_llr must be ({B}, {Smax + 1}, {Cc}) and targets a contiguous ({B}, {Smax}) int32 tensor')
    dev = sub_llr.device
    post, alt_post = torch.empty(B, Smax, dtype=torch.float32, device=dev), torch.empty(B, Smax, dtype=torch.float32, device=dev)
    alt = torch.empty(B, Smax, dtype=torch.int32, device=dev)
    gap_post, gap_alt_post = torch.empty(B, Smax + 1, dtype=torch.float32, device=dev), torch.empty(B, Smax + 1, dtype=torch.float32, device=dev)
    gap_alt = torch.empty(B, Smax + 1, dtype=torch.int32, device=dev)
    _lib.call('sconf_post_slots', _p(sub_llr), _p(ins_llr), _p(targets), B, Cc, Smax, int(blank), _p(post), _p(alt), _p(alt_post), _p(gap_post),
              _p(gap_alt), _p(gap_alt_post), _stream())
    return post, alt, alt_post, gap_post, gap_alt, gap_alt_post
