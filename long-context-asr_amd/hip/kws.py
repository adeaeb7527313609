"""ctypes binding and tensor-level op of CTC keyword search (include/sconf_kws.h), the fourteenth ABI unit of libsconf_hip.so: a
keyword image and the log-scores of a recording become timed, scored hits.

Same discipline as the other units under hip/: GPU tensors in and out, outputs and workspace allocated here, the kernels enqueued on
torch's current stream, no host read, no fallback - a CPU tensor, a missing library or a failing call raises.  `tests/kws_refs.py`
restates the op in numpy.  This module is imported by decoding/kws.py only."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import torch

from . import _lib
from ._lib import vp, i64, i32
from .ops import _chk_lengths, _p, _stream, _workspace, require_gpu

# the enumerators of include/sconf_kws.h (tests hold the two together)
FIRST, SKIP, LAST = 1, 2, 4
MAX_LABELS = 32             # sconf_kws_max_labels(): 63 states, one wave (held to the query by the tests)

# name -> argtypes (status-returning launchers).  Must match include/sconf_kws.h.
PROTOTYPES = {
    'sconf_kws_search': [vp, vp, vp, i64, i64, i64, vp, vp, vp, i64, vp, i64, i64, i64, i64, i64, i32, vp],
}
# name -> (argtypes, restype): the queries
PLAIN = {
    'sconf_kws_max_labels': ([], C.c_int),
    'sconf_kws_prefetch': ([], C.c_int),
    'sconf_kws_max_hits': ([], C.c_int),
    'sconf_kws_workspace': ([i64, i64, i64], C.c_int64),
}

_lib.register(PROTOTYPES, PLAIN)
load = _lib.load


class Hits(NamedTuple):
    """What sconf_kws_search writes: hit_frames (B, K, cap, 2) int32; hit_score (B, K, cap) f32; hit_count (B, K) int32."""
    hit_frames: torch.Tensor
    hit_score: torch.Tensor
    hit_count: torch.Tensor


def max_labels() -> int:
    return int(load().sconf_kws_max_labels())


def prefetch() -> int:
    return int(load().sconf_kws_prefetch())


def max_hits() -> int:
    return int(load().sconf_kws_max_hits())


def kws_workspace(B: int, N: int, U: int) -> int:
    n = int(load().sconf_kws_workspace(B, N, U))
    if n < 0:
        raise ValueError(f'kws: invalid sizes B={B} N={N} U={U}')
    return n


def search(x: torch.Tensor, image: torch.Tensor, n_waves: int, U: int, K: int, blank: int, input_lengths: Optional[torch.Tensor] = None,
           cap: int = 64, classes: Optional[int] = None) -> Hits:
    """x (B, N, C) f32 with unit stride along C and rows C apart; image: the int32 keyword image of n_waves * 256 + U words on the
    same device; input_lengths (B,) int32 or None (= N) -> Hits of device tensors over the first `classes` (default C) columns.
    See include/sconf_kws.h for the semantics."""
    require_gpu(x, 'log_probs')
    if x.dtype != torch.float32 or x.dim() != 3 or not x.is_contiguous():
        raise TypeError('kws.search: log_probs must be a contiguous (B, N, C) float32 tensor')
    require_gpu(image, 'image')
    if image.dtype != torch.int32 or image.dim() != 1 or not image.is_contiguous() or image.device != x.device:
        raise TypeError('kws.search: the image must be a contiguous 1-d int32 tensor on the device of log_probs')
    n_waves, U, K, cap = int(n_waves), int(U), int(K), int(cap)
    if n_waves < 1 or U < 1 or image.numel() != n_waves * 256 + U:
        raise ValueError(f'kws.search: an image of {image.numel()} words does not hold {n_waves} waves and {U} columns')
    B, N, Cn = x.shape
    if B < 1 or N < 1:
        raise ValueError(f'kws.search: empty input B={B} N={N}')
    classes = Cn if classes is None else int(classes)
    _chk_lengths(input_lengths, B, 'kws.search', 'input_lengths')
    if K < 1 or not 1 <= cap <= max_hits():
        raise ValueError(f'kws.search: K = {K} keywords and cap = {cap}: K at least 1, cap in 1 .. {max_hits()}')
    dev = x.device
    out = Hits(torch.empty(B, K, cap, 2, dtype=torch.int32, device=dev), torch.empty(B, K, cap, dtype=torch.float32, device=dev),
               torch.empty(B, K, dtype=torch.int32, device=dev))
    nbytes = kws_workspace(B, N, U)
    ws = _workspace(nbytes, dev)
    _lib.call('sconf_kws_search', _p(x), _p(input_lengths), _p(image), n_waves, U, K, _p(out.hit_frames), _p(out.hit_score),
              _p(out.hit_count), cap, _p(ws), nbytes, B, N, Cn, classes, int(blank), _stream())
    return out
