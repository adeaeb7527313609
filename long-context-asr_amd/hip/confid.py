"""ctypes binding and tensor-level ops of the confidence scores (include/sconf_confid.h), the twelfth ABI unit of libsconf_hip.so: a
confidence and the argmax of every frame, the greedy CTC collapse with the frames of every label, and spans aggregated to one value
each.

Same discipline as the other units under hip/: GPU tensors in and out, outputs allocated here, the kernels enqueued on torch's
current stream, no host read, no fallback - a CPU tensor, a missing library or a failing call raises.  `tests/confid_refs.py`
restates the ops in numpy float64.  This module is imported by decoding/confidence.py only."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import vp, i64, i32, f32
from .ops import _p, _stream, require_gpu

# the enumerators of include/sconf_confid.h (tests hold the two together)
METHOD = {'max_prob': 0, 'shannon': 1, 'tsallis': 2, 'renyi': 3}
NORM = {'lin': 0, 'exp': 1}
AGGREGATION = {'mean': 0, 'min': 1, 'max': 2, 'prod': 3}

# name -> argtypes (status-returning launchers).  Must match include/sconf_confid.h.
PROTOTYPES = {
    'sconf_confid_frames': [vp, i64, i64, i64, i32, i32, f32, vp, vp, vp],
    'sconf_confid_runs': [vp, vp, i64, i64, i32, vp, vp, vp, i64, vp],
    'sconf_confid_aggregate': [vp, vp, i32, i64, vp, i64, i32, vp, vp],
}
# name -> (argtypes, restype): the queries
PLAIN = {
    'sconf_confid_row_capacity': ([], C.c_int),
    'sconf_confid_block_capacity': ([], C.c_int),
    'sconf_confid_scan_chunk': ([], C.c_int),
}

_lib.register(PROTOTYPES, PLAIN)
load = _lib.load


def row_capacity() -> int:
    return int(load().sconf_confid_row_capacity())


def block_capacity() -> int:
    return int(load().sconf_confid_block_capacity())


def scan_chunk() -> int:
    return int(load().sconf_confid_scan_chunk())


def _enum(table: dict, key: str, what: str) -> int:
    if key not in table:
        raise ValueError(f'confid: unknown {what} {key!r}; one of {sorted(table)}')
    return table[key]


def _int32_vector(t: Optional[torch.Tensor], n: int, what: str):
    if t is None:
        return None
    require_gpu(t, what)
    if t.dtype != torch.int32 or t.numel() != n or not t.is_contiguous():
        raise ValueError(f'confid: {what} must be a contiguous int32 tensor of {n} elements')
    return t


def frames(x: torch.Tensor, classes: Optional[int] = None, method: str = 'tsallis', norm: str = 'exp',
           alpha: float = 1.0 / 3.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """x (M, C) f32 with unit stride along C (any row stride >= C) -> (idx (M,) int32, conf (M,) f32) over the first `classes`
    (default C) columns of every row.  See include/sconf_confid.h."""
    require_gpu(x, 'x')
    if x.dtype != torch.float32 or x.dim() != 2 or (x.shape[1] > 1 and x.stride(1) != 1):
        raise TypeError('confid.frames: x must be an (M, C) float32 tensor with unit stride along C')
    M, Cc = x.shape
    classes = Cc if classes is None else int(classes)
    if not 2 <= classes <= Cc:
        raise ValueError(f'confid.frames: classes = {classes} for rows of {Cc}; 2 .. {Cc}')
    idx = torch.empty(M, dtype=torch.int32, device=x.device)
    conf = torch.empty(M, dtype=torch.float32, device=x.device)
    _lib.call('sconf_confid_frames', _p(x), M, classes, x.stride(0) if M > 1 else Cc, _enum(METHOD, method, 'method'),
              _enum(NORM, norm, 'norm'), float(alpha), _p(idx), _p(conf), _stream())
    return idx, conf


def runs(idx: torch.Tensor, lengths: Optional[torch.Tensor], blank: int, s_cap: Optional[int] = None):
    """idx (B, N) int32 -> (targets (B, s_cap) int32, spans (B, s_cap, 3) int32, target_lengths (B,) int32); s_cap defaults to N,
    which always suffices.  See include/sconf_confid.h."""
    require_gpu(idx, 'idx')
    if idx.dtype != torch.int32 or idx.dim() != 2 or not idx.is_contiguous():
        raise TypeError('confid.runs: idx must be a contiguous (B, N) int32 tensor')
    B, N = idx.shape
    lengths = _int32_vector(lengths, B, 'lengths')
    s_cap = N if s_cap is None else int(s_cap)
    targets = torch.empty(B, s_cap, dtype=torch.int32, device=idx.device)
    spans = torch.empty(B, s_cap, 3, dtype=torch.int32, device=idx.device)
    tl = torch.empty(B, dtype=torch.int32, device=idx.device)
    _lib.call('sconf_confid_runs', _p(idx), _p(lengths), B, N, int(blank), _p(targets), _p(spans), _p(tl), s_cap, _stream())
    return targets, spans, tl


def aggregate(values: torch.Tensor, spans: torch.Tensor, aggregation: str = 'min', idx: Optional[torch.Tensor] = None,
              blank: int = 0) -> torch.Tensor:
    """values (M,) f32, spans (S, 2) int32 -> (S,) f32; idx (M,) int32: skip the frames that are `blank` or negative.
    See include/sconf_confid.h."""
    require_gpu(values, 'values')
    if values.dtype != torch.float32 or values.dim() != 1 or not values.is_contiguous():
        raise TypeError('confid.aggregate: values must be a contiguous (M,) float32 tensor')
    require_gpu(spans, 'spans')
    if spans.dtype != torch.int32 or spans.dim() != 2 or spans.shape[1] != 2 or not spans.is_contiguous():
        raise TypeError('confid.aggregate: spans must be a contiguous (S, 2) int32 tensor')
    M, S = values.shape[0], spans.shape[0]
    idx = _int32_vector(idx, M, 'idx')
    out = torch.empty(S, dtype=torch.float32, device=values.device)
    _lib.call('sconf_confid_aggregate', _p(values), _p(idx), int(blank), M, _p(spans), S, _enum(AGGREGATION, aggregation, 'aggregation'),
              _p(out), _stream())
    return out
