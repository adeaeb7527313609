"""ctypes binding and tensor-level op of the long form of CTC forced alignment (include/sconf_align_long.h), the sixth ABI unit of
libsconf_hip.so: the contract of hip/align.py for transcripts of up to 65535 labels, the lattice cut into state slabs.

Same discipline as hip/align.py: GPU tensors in and out, outputs and workspace allocated here, kernels enqueued on torch's current
stream, no fallback - a CPU tensor, a missing library or a failing call raises.  `tests/align_refs.py` restates the op in numpy."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib
from ._lib import vp, i64, i32
from .align import Alignment
from .ops import _chk_log_probs, _chk_lengths, _p, _stream, _workspace, require_gpu

# name -> argtypes (status-returning launchers).  Must match include/sconf_align_long.h.
PROTOTYPES = {
    'sconf_lalign_ctc': [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, i64, i64, i32, i32, vp],
}
# name -> (argtypes, restype): the queries
PLAIN = {
    'sconf_lalign_max_labels': ([], C.c_int),
    'sconf_lalign_default_slab_states': ([], C.c_int),
    'sconf_lalign_threads': ([i32], C.c_int),
    'sconf_lalign_states_per_thread': ([i32], C.c_int),
    'sconf_lalign_slabs': ([i64, i32], C.c_int),
    'sconf_lalign_workspace': ([i64, i64, i64, i32], C.c_int64),
}

_lib.register(PROTOTYPES, PLAIN)
load = _lib.load

MAX_LABELS = 65535          # sconf_lalign_max_labels(), for callers that route before the library is loaded (held to it by the tests)


def max_labels() -> int:
    return int(load().sconf_lalign_max_labels())


def slabs(Smax: int, slab_states: int = 0) -> int:
    n = int(load().sconf_lalign_slabs(Smax, slab_states))
    if n < 0:
        raise ValueError(f'ctc_align: {Smax} labels in slabs of {slab_states} states: at most {max_labels()} labels, slab_states 0 or a '
                         f'power of two in 256..8192')
    return n


def align_workspace(B: int, N: int, Smax: int, slab_states: int = 0) -> int:
    n = int(load().sconf_lalign_workspace(B, N, Smax, slab_states))
    if n < 0:
        raise ValueError(f'ctc_align: invalid sizes B={B} N={N} Smax={Smax} slab_states={slab_states}')
    return n


def ctc_align(log_probs: torch.Tensor, targets: torch.Tensor, input_lengths: Optional[torch.Tensor],
              target_lengths: Optional[torch.Tensor], blank: int, slab_states: int = 0) -> Alignment:
    """log_probs (B, N, C) f32, targets (B, Smax) int32, lengths (B,) int32 or None (= N / Smax) -> Alignment of device tensors, what
    hip.align.ctc_align returns.  slab_states: 0 (the default geometry) or 256 .. 8192; the result does not depend on it.  See
    include/sconf_align_long.h."""
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
    nbytes = align_workspace(B, N, Smax, int(slab_states))
    ws = _workspace(nbytes, dev)
    _lib.call('sconf_lalign_ctc', _p(log_probs), _p(targets), _p(input_lengths), _p(target_lengths), _p(out.path), _p(out.labels),
              _p(out.spans), _p(out.token_logp), _p(out.score), _p(ws), nbytes, B, N, Cn, Smax, int(blank), int(slab_states), _stream())
    return out
