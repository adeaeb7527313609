"""ctypes binding and tensor-level ops of the calibration unit (include/sconf_calib.h), the fifteenth ABI unit of libsconf_hip.so: the
edit alignment of ragged pairs of id sequences, and the frame confidences at K softmax temperatures from one pass over the rows.

Same discipline as the other units under hip/: GPU tensors in and out, outputs allocated here, the kernels enqueued on torch's
current stream, no host read, no fallback - a CPU tensor, a missing library or a failing call raises.  `tests/calib_refs.py`
restates the ops in numpy.  The Python callers (eval/wer.py, decoding/calibration.py, decoding/confidence.py) reach `edit_align` and
`frames_sweep` through this module's attributes, so that a test can replace the two with the restatements."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import vp, i64, i32, f32
from .ops import _p, _stream, require_gpu

# the enumerators of include/sconf_confid.h, which this unit's sweep takes
METHOD = {'max_prob': 0, 'shannon': 1, 'tsallis': 2, 'renyi': 3}
NORM = {'lin': 0, 'exp': 1}

# name -> argtypes (status-returning launchers).  Must match include/sconf_calib.h.
PROTOTYPES = {
    'sconf_edit_align': [vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp],
    'sconf_calib_frames_sweep': [vp, i64, i64, i64, i32, i32, f32, vp, i64, vp, vp, vp],
}
# name -> (argtypes, restype): the queries
PLAIN = {
    'sconf_edit_align_strip_cols': ([], C.c_int),
    'sconf_edit_align_pass_cols': ([], C.c_int),
    'sconf_edit_align_block_rows': ([], C.c_int),
    'sconf_edit_align_cells_per_word': ([], C.c_int),
    'sconf_edit_align_tile_bytes': ([], C.c_int),
    'sconf_edit_align_max_len': ([], C.c_int),
    'sconf_edit_align_pair_bytes': ([i64, i64], C.c_int64),
    'sconf_calib_max_temps': ([], C.c_int),
}

_lib.register(PROTOTYPES, PLAIN)
load = _lib.load


def strip_cols() -> int:
    return int(load().sconf_edit_align_strip_cols())


def pass_cols() -> int:
    return int(load().sconf_edit_align_pass_cols())


def block_rows() -> int:
    return int(load().sconf_edit_align_block_rows())


def cells_per_word() -> int:
    return int(load().sconf_edit_align_cells_per_word())


def max_len() -> int:
    return int(load().sconf_edit_align_max_len())


def max_temps() -> int:
    return int(load().sconf_calib_max_temps())


def pair_bytes(H: int, R: int) -> int:
    """The exact workspace bytes of a pair of H hypothesis and R reference ids."""
    n = int(load().sconf_edit_align_pair_bytes(int(H), int(R)))
    if n < 0:
        raise ValueError(f'edit_align: a pair of {H} against {R} ids; at most {max_len()} a side')
    return n


def workspace_offsets(hyp_lens: Sequence[int], ref_lens: Sequence[int]) -> list:
    """(P + 1) byte offsets of the pairs' slices, each exactly what its pair needs, from the lengths on the host."""
    off = [0]
    for h, r in zip(hyp_lens, ref_lens):
        off.append(off[-1] + pair_bytes(h, r))
    return off


def _ids(t: torch.Tensor, what: str, dtype) -> torch.Tensor:
    require_gpu(t, what)
    if t.dtype != dtype or t.dim() != 1 or not t.is_contiguous():
        raise TypeError(f'edit_align: {what} must be a contiguous 1-D {dtype} tensor')
    return t


def edit_align(hyp: torch.Tensor, hyp_off: torch.Tensor, ref: torch.Tensor, ref_off: torch.Tensor, ws_off: torch.Tensor,
               ws: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """hyp / ref int32 ids, hyp_off / ref_off (P + 1,) int64 offsets that begin at 0, ws_off (P + 1,) int64 byte offsets of the pairs'
    workspace slices (workspace_offsets), all on the device -> (hyp_to_ref int32 like hyp, ref_to_hyp int32 like ref, counts (P, 4)
    int64).  ws: the uint8 workspace the slices lie in, of at least ws_off[P] bytes (the caller, who made ws_off, knows that figure;
    nothing is read back here to check it); None where no pair needs a byte.  A pair whose slice is too small comes back as -1
    throughout.  One launch.  See include/sconf_calib.h."""
    _ids(hyp, 'hyp', torch.int32); _ids(ref, 'ref', torch.int32)
    _ids(hyp_off, 'hyp_off', torch.int64); _ids(ref_off, 'ref_off', torch.int64); _ids(ws_off, 'ws_off', torch.int64)
    if hyp_off.numel() < 1 or hyp_off.shape != ref_off.shape or hyp_off.shape != ws_off.shape:
        raise ValueError(f'edit_align: hyp_off, ref_off and ws_off must all be (P + 1,), got {tuple(hyp_off.shape)} / {tuple(ref_off.shape)} / {tuple(ws_off.shape)}')
    if ws is not None:
        require_gpu(ws, 'ws')
        if ws.dtype != torch.uint8 or not ws.is_contiguous():
            raise TypeError('edit_align: ws must be a contiguous uint8 tensor')
    P = hyp_off.numel() - 1
    h2r = torch.empty_like(hyp)
    r2h = torch.empty_like(ref)
    counts = torch.empty(P, 4, dtype=torch.int64, device=hyp_off.device)
    _lib.call('sconf_edit_align', _p(hyp), _p(hyp_off), _p(ref), _p(ref_off), P, _p(h2r), _p(r2h), _p(counts), _p(ws), _p(ws_off), _stream())
    return h2r, r2h, counts


def frames_sweep(x: torch.Tensor, inv_temps: torch.Tensor, classes: Optional[int] = None, method: str = 'tsallis', norm: str = 'exp',
                 alpha: float = 1.0 / 3.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """x (M, C) f32 with unit stride along C (any row stride >= C), inv_temps (K,) f32 on the device -> (idx (M,) int32,
    conf (K, M) f32) over the first `classes` (default C) columns of every row.  See include/sconf_calib.h."""
    require_gpu(x, 'x')
    if x.dtype != torch.float32 or x.dim() != 2 or (x.shape[1] > 1 and x.stride(1) != 1):
        raise TypeError('calib.frames_sweep: x must be an (M, C) float32 tensor with unit stride along C')
    require_gpu(inv_temps, 'inv_temps')
    if inv_temps.dtype != torch.float32 or inv_temps.dim() != 1 or not inv_temps.is_contiguous():
        raise TypeError('calib.frames_sweep: inv_temps must be a contiguous (K,) float32 tensor')
    M, Cc = x.shape
    K = inv_temps.shape[0]
    classes = Cc if classes is None else int(classes)
    if not 2 <= classes <= Cc:
        raise ValueError(f'calib.frames_sweep: classes = {classes} for rows of {Cc}; 2 .. {Cc}')
    if method not in METHOD or norm not in NORM:
        raise ValueError(f'calib.frames_sweep: unknown method {method!r} or norm {norm!r}; {sorted(METHOD)} and {sorted(NORM)}')
    idx = torch.empty(M, dtype=torch.int32, device=x.device)
    conf = torch.empty(K, M, dtype=torch.float32, device=x.device)
    _lib.call('sconf_calib_frames_sweep', _p(x), M, classes, x.stride(0) if M > 1 else Cc, METHOD[method], NORM[norm], float(alpha),
              _p(inv_temps), K, _p(idx), _p(conf), _stream())
    return idx, conf
