"""ctypes binding and tensor-level op of the resampler (include/sconf_resample.h), the ninth ABI unit of libsconf_hip.so: a
waveform at any rate to the rate of the audio front end, torchaudio.transforms.Resample's polyphase filter from a compact table.

Same discipline as the other units under hip/: GPU tensors in and out, the output allocated here, the kernel enqueued on torch's
current stream, no fallback - a CPU tensor, a missing library or a failing call raises.  `tests/resample_refs.py` restates the op
in plain torch.  This module is imported by utils/audio_tools.py (resample) only."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib
from ._lib import vp, i64, i32
from .ops import _p, _stream, require_gpu

# name -> argtypes (status-returning launchers).  Must match include/sconf_resample.h.
PROTOTYPES = {
    'sconf_resample_rows': [vp, i64, i64, i32, i32, vp, i64, vp, vp, i64, i64, i64, vp, i64, i64, i64, vp],
}
# name -> (argtypes, restype): the queries
PLAIN = {
    'sconf_resample_tile': ([], C.c_int),
    'sconf_resample_max_table': ([], C.c_int),
    'sconf_resample_out_length': ([i64, i64, i64], C.c_int64),
}

_lib.register(PROTOTYPES, PLAIN)
load = _lib.load


def tile() -> int:
    return int(load().sconf_resample_tile())


def max_table() -> int:
    return int(load().sconf_resample_max_table())


def out_length(L: int, O: int, P: int) -> int:
    n = int(load().sconf_resample_out_length(L, O, P))
    if n < 0:
        raise ValueError(f'resample: invalid sizes L={L} O={O} P={P}')
    return n


def resample_rows(wave: torch.Tensor, lengths: Optional[torch.Tensor], taps: torch.Tensor, first: torch.Tensor, O: int, P: int,
                  mix: bool = False) -> torch.Tensor:
    """wave (B, L) or (B, channels, L) f32 with unit stride along L (any other strides), lengths (B) int64 or None, taps (P, K) f32
    and first (P) int32 as utils.audio_tools.resample_table builds them -> (B, ceil(P L / O)) f32.  A (B, channels, L) input is
    reduced to its channel 0, or with mix to the mean of its channels.  See include/sconf_resample.h for the semantics."""
    require_gpu(wave, 'waveform')
    if wave.dtype != torch.float32 or wave.dim() not in (2, 3) or wave.stride(-1) != 1:
        raise TypeError('resample_rows: waveform must be (B, L) or (B, channels, L) float32 with unit stride along L')
    B, L = wave.shape[0], wave.shape[-1]
    channels = wave.shape[1] if wave.dim() == 3 else 1
    if B < 1 or L < 1 or channels < 1:
        raise ValueError(f'resample_rows: empty waveform {tuple(wave.shape)}')
    if taps.dim() != 2 or taps.shape[0] != P or taps.dtype != torch.float32 or not taps.is_contiguous():
        raise ValueError(f'resample_rows: taps must be a contiguous ({P}, K) float32 tensor')
    K = taps.shape[1]
    if P * K > max_table():
        raise ValueError(f'resample_rows: a table of {P} x {K} taps; at most {max_table()} (sconf_resample_max_table) are kept in LDS')
    if tuple(first.shape) != (P,) or first.dtype != torch.int32 or not first.is_contiguous():
        raise ValueError(f'resample_rows: first must be a contiguous ({P},) int32 tensor')
    if lengths is not None and (lengths.dtype != torch.int64 or tuple(lengths.shape) != (B,) or not lengths.is_contiguous()):
        raise ValueError('resample_rows: lengths must be a contiguous (B,) int64 tensor')
    for t, what in ((taps, 'taps'), (first, 'first')) + (((lengths, 'lengths'),) if lengths is not None else ()):
        require_gpu(t, what)
    L_out = out_length(L, O, P)
    out = torch.empty(B, L_out, dtype=torch.float32, device=wave.device)
    chan_stride = wave.stride(1) if wave.dim() == 3 and channels > 1 else L
    _lib.call('sconf_resample_rows', _p(wave), chan_stride, wave.stride(0) if B > 1 else L * channels, channels, int(bool(mix)), _p(lengths),
              L, _p(taps), _p(first), O, P, K, _p(out), L_out, L_out, B, _stream())
    return out
