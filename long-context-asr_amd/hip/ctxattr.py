"""ctypes binding and tensor-level ops of context attribution (include/sconf_ctxattr.h), the seventh ABI unit of libsconf_hip.so: the
means of the masked windows, the masked model batch, and the matrix of edit distances of the spliced hypotheses.

Same discipline as hip/lm.py and hip/align_long.py: GPU tensors in and out, outputs and workspace allocated here, kernels enqueued on
torch's current stream, no fallback - a CPU tensor, a missing library or a failing call raises.  `tests/ctxattr_refs.py` restates the
ops in numpy, the naive way.  This module is imported by eval/context_attribution.py only."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import vp, i64, i32
from .ops import _chk, _p, _stream, _workspace

# name -> argtypes (status-returning launchers).  Must match include/sconf_ctxattr.h.
PROTOTYPES = {
    'sconf_ctxattr_window_means': [vp, vp, vp, i64, i64, i64, vp],
    'sconf_ctxattr_mask_fill': [vp, vp, vp, vp, i64, i64, i64, i64, i64, vp],
    'sconf_ctxattr_score': [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, i64, i64, i64, i32, vp],
}
# name -> (argtypes, restype): the queries
PLAIN = {
    'sconf_ctxattr_max_ref': ([], C.c_int),
    'sconf_ctxattr_max_window_frames': ([], C.c_int),
    'sconf_ctxattr_threads': ([i64], C.c_int),
    'sconf_ctxattr_cells_per_thread': ([i64], C.c_int),
    'sconf_ctxattr_score_workspace': ([i64, i64, i64, i64], C.c_int64),
}

_lib.register(PROTOTYPES, PLAIN)
load = _lib.load

MAX_REF = 65535             # sconf_ctxattr_max_ref(), for callers that check before the library is loaded (held to it by the tests)
MAX_WINDOW_FRAMES = 8192    # sconf_ctxattr_max_window_frames(), likewise


class Scores(NamedTuple):
    """What sconf_ctxattr_score writes: errors (I, J), clean_errors (1), clean_len (1), mid_len (I, J) and, if asked for, mid_tokens
    (I, J, mid_cap), all int32 on the device."""
    errors: torch.Tensor
    clean_errors: torch.Tensor
    clean_len: torch.Tensor
    mid_len: torch.Tensor
    mid_tokens: Optional[torch.Tensor]


def max_ref() -> int:
    return int(load().sconf_ctxattr_max_ref())


def max_window_frames() -> int:
    return int(load().sconf_ctxattr_max_window_frames())


def score_workspace(N: int, I: int, J: int, R: int) -> int:
    n = int(load().sconf_ctxattr_score_workspace(N, I, J, R))
    if n < 0:
        raise ValueError(f'ctxattr.score: invalid sizes N={N} I={I} J={J} R={R} (at most {max_ref()} reference ids)')
    return n


def _chk_spec(spec: torch.Tensor, windows: torch.Tensor, op: str) -> Tuple[int, int, int]:
    _chk(spec, 'spec', torch.float32); _chk(windows, 'windows', torch.int32)
    if spec.dim() != 2: raise ValueError(f'{op}: spec must be (features, time), got {tuple(spec.shape)}')
    if windows.dim() != 2 or windows.shape[1] != 2: raise ValueError(f'{op}: windows must be (J, 2), got {tuple(windows.shape)}')
    return spec.shape[0], spec.shape[1], windows.shape[0]


def window_means(spec: torch.Tensor, windows: torch.Tensor) -> torch.Tensor:
    """spec (F, T) f32, windows (J, 2) int32 on the device -> means (J,) f32: the mean of spec[:, s:e], accumulated in f64 in a fixed
    order; 0 for an empty window."""
    F, T, J = _chk_spec(spec, windows, 'ctxattr.window_means')
    means = torch.empty(J, dtype=torch.float32, device=spec.device)
    _lib.call('sconf_ctxattr_window_means', _p(spec), _p(windows), _p(means), F, T, J, _stream())
    return means


def mask_fill(spec: torch.Tensor, windows: torch.Tensor, means: torch.Tensor, j0: int, b: int) -> torch.Tensor:
    """-> (b, F, T) f32: copy k is spec with the frames of window j0 + k set to means[j0 + k].  One launch."""
    F, T, J = _chk_spec(spec, windows, 'ctxattr.mask_fill')
    _chk(means, 'means', torch.float32)
    if tuple(means.shape) != (J,): raise ValueError(f'ctxattr.mask_fill: means must be ({J},), got {tuple(means.shape)}')
    j0, b = int(j0), int(b)
    if j0 < 0 or b < 1 or j0 + b > J: raise ValueError(f'ctxattr.mask_fill: windows {j0} .. {j0 + b} of {J}')
    dst = torch.empty(b, F, T, dtype=torch.float32, device=spec.device)
    _lib.call('sconf_ctxattr_mask_fill', _p(spec), _p(windows), _p(means), _p(dst), F, T, J, j0, b, _stream())
    return dst


def score(clean: torch.Tensor, masked: torch.Tensor, ref: torch.Tensor, frame_windows: Sequence[Tuple[int, int]], blank: int,
          with_tokens: bool = False) -> Scores:
    """clean (N,) int32, masked (J, N) int32, ref (R,) int32 on the device; frame_windows: I pairs (f, g) on the HOST -> Scores of
    device tensors.  See include/sconf_ctxattr.h for the identity that makes a pair cost its middle only."""
    _chk(clean, 'clean', torch.int32); _chk(masked, 'masked', torch.int32); _chk(ref, 'ref', torch.int32)
    if clean.dim() != 1 or masked.dim() != 2 or masked.shape[1] != clean.shape[0] or ref.dim() != 1:
        raise ValueError(f'ctxattr.score: clean (N,), masked (J, N), ref (R,): got {tuple(clean.shape)}, {tuple(masked.shape)}, {tuple(ref.shape)}')
    N, J, R, I = clean.shape[0], masked.shape[0], ref.shape[0], len(frame_windows)
    if R > max_ref(): raise ValueError(f'ctxattr.score: {R} reference ids: at most {max_ref()} are supported')
    for f, g in frame_windows:
        if not 0 <= f <= g <= N or g - f + 1 > max_window_frames():
            raise ValueError(f'ctxattr.score: frame window [{f}, {g}) must be within 0 <= f <= g <= N = {N} and at most '
                             f'{max_window_frames() - 1} frames wide')
    nbytes = score_workspace(N, I, J, R)
    fw =(C.c_int32 * (2 * I))(*[int(v) for pair in frame_windows for v in pair])
    cap = max(1, max(min(int(g) + 1, N) - int(f) for f, g in frame_windows))
    dev = clean.device
    new = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    out = Scores(new(I, J), new(1), new(1), new(I, J), new(I, J, cap) if with_tokens else None)
    ws = _workspace(nbytes, dev)
    _lib.call('sconf_ctxattr_score', _p(clean), _p(masked), _p(ref) if R else None, fw, _p(out.errors), _p(out.clean_errors), _p(out.clean_len),
              _p(out.mid_len), _p(out.mid_tokens), _p(ws), nbytes, N, I, J, R, cap, int(blank), _stream())
    return out
