"""ctypes binding and tensor-level op of the audio front end (include/sconf_audio.h), the second ABI unit of libsconf_hip.so.

Same discipline as hip/ops.py: GPU tensors in and out, outputs allocated here, kernels enqueued on torch's current stream, no
fallback - a CPU tensor, a missing library or a failing call raises.  `tests/audio_refs.py` restates the op in plain torch."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib
from ._lib import vp, i64, i32
from .ops import BF16, F32, _p, _stream, _workspace, require_gpu

# name -> argtypes (status-returning launchers).  Must match include/sconf_audio.h.
PROTOTYPES = {
    'sconf_audio_melspec': [vp, i64, vp, i64, vp, vp, vp, i32, vp, i32, vp, i64, i64, i64, i64, vp],
}
# name -> (argtypes, restype): the queries
PLAIN = {
    'sconf_audio_tile_frames': ([], C.c_int),
    'sconf_audio_melspec_workspace': ([i64, i64, i64], C.c_int64),
}

N_FFT, HOP, WIN, N_BINS, PAD = 512, 160, 400, 257, 256
MAX_MELS = 128

_lib.register(PROTOTYPES, PLAIN)
load = _lib.load


def tile_frames() -> int:
    return int(load().sconf_audio_tile_frames())


def melspec_workspace(B: int, T: int, n_mels: int) -> int:
    n = int(load().sconf_audio_melspec_workspace(B, T, n_mels))
    if n < 0:
        raise ValueError(f'melspec: invalid sizes B={B} T={T} n_mels={n_mels}')
    return n


def filter_ranges(fb: torch.Tensor) -> torch.Tensor:
    """(n_mels, 2) int32: the half-open range of bins where each column of the (257, n_mels) filterbank is not zero."""
    nz = fb != 0
    k = torch.arange(fb.shape[0], device=fb.device)[:, None]
    lo = torch.where(nz, k, fb.shape[0]).amin(0)
    hi = torch.where(nz, k + 1, 0).amax(0)
    return torch.stack([torch.minimum(lo, hi), hi], 1).to(torch.int32).contiguous()


def melspec(wave: torch.Tensor, lengths: Optional[torch.Tensor], fb: torch.Tensor, ranges: torch.Tensor, normalise: bool = True,
            out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """wave (B, L) f32 with unit stride along L (any row stride), lengths (B) int64 or None, fb (257, n_mels) f32, ranges as
    filter_ranges(fb) -> (B, n_mels, 1 + L // 160) in out_dtype.  See include/sconf_audio.h for the semantics."""
    require_gpu(wave, 'waveform')
    if wave.dtype != torch.float32 or wave.dim() != 2 or wave.stride(1) != 1:
        raise TypeError('melspec: waveform must be (B, L) float32 with unit stride along L')
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f'melspec: out_dtype must be float32 or bfloat16, got {out_dtype}')
    B, L = wave.shape
    if L <= PAD:
        raise ValueError(f'melspec: {L} samples: reflect padding needs more than {PAD}')
    n_mels = fb.shape[1]
    if tuple(fb.shape) != (N_BINS, n_mels) or fb.dtype != torch.float32 or not fb.is_contiguous() or not 1 <= n_mels <= MAX_MELS:
        raise ValueError(f'melspec: the filterbank must be a contiguous ({N_BINS}, 1..{MAX_MELS}) float32 tensor')
    if tuple(ranges.shape) != (n_mels, 2) or ranges.dtype != torch.int32 or not ranges.is_contiguous():
        raise ValueError('melspec: ranges must be a contiguous (n_mels, 2) int32 tensor')
    if lengths is not None and (lengths.dtype != torch.int64 or tuple(lengths.shape) != (B,) or not lengths.is_contiguous()):
        raise ValueError('melspec: lengths must be a contiguous (B,) int64 tensor')
    for t, what in ((fb, 'filterbank'), (ranges, 'ranges')) + (((lengths, 'lengths'),) if lengths is not None else ()):
        require_gpu(t, what)
    T = 1 + L // HOP
    spec = torch.empty(B, n_mels, T, dtype=out_dtype, device=wave.device)
    raw = torch.empty(B, n_mels, T, dtype=torch.float32, device=wave.device) if normalise and out_dtype == torch.bfloat16 else None
    nbytes = melspec_workspace(B, T, n_mels)
    ws = _workspace(nbytes, wave.device)
    _lib.call('sconf_audio_melspec', _p(wave), wave.stride(0) if B > 1 else L, _p(lengths), L, _p(fb), _p(ranges), _p(spec),
              F32 if out_dtype == torch.float32 else BF16, _p(raw), int(bool(normalise)), _p(ws), nbytes, B, T, n_mels, _stream())
    return spec
