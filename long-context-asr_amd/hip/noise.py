"""ctypes binding and tensor-level ops of the noise corruption (include/sconf_noise.h), the tenth ABI unit of libsconf_hip.so: the
mean square of waveform rows, Gaussian noise from the contract's Philox normals and a background clip mixed in at K SNR levels per
launch.

Same discipline as the other units under hip/: GPU tensors in and out, outputs and the workspace allocated here, the kernels
enqueued on torch's current stream, no fallback - a CPU tensor, a missing library or a failing call raises.  `tests/noise_refs.py`
restates the ops in numpy / torch f64.  This module is imported by utils/audio_tools.py only."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib
from ._lib import vp, i64
from .ops import _p, _stream, _workspace, require_gpu

# name -> argtypes (status-returning launchers).  Must match include/sconf_noise.h.
PROTOTYPES = {
    'sconf_noise_power': [vp, i64, i64, vp, vp, vp, i64, i64, vp, vp, i64, vp],
    'sconf_noise_add_gaussian': [vp, i64, vp, i64, i64, vp, vp, i64, i64, i64, i64, vp, i64, vp],
    'sconf_noise_add_background': [vp, i64, vp, i64, i64, vp, i64, i64, vp, vp, vp, vp, vp, i64, vp, i64, vp],
}
# name -> (argtypes, restype): the queries
PLAIN = {
    'sconf_noise_tile': ([], C.c_int),
    'sconf_noise_max_levels': ([], C.c_int),
    'sconf_noise_workspace': ([i64, i64], C.c_int64),
}

_lib.register(PROTOTYPES, PLAIN)
load = _lib.load


def tile() -> int:
    return int(load().sconf_noise_tile())


def max_levels() -> int:
    return int(load().sconf_noise_max_levels())


def workspace(B: int, L: int) -> int:
    n = int(load().sconf_noise_workspace(B, L))
    if n < 0:
        raise ValueError(f'noise: invalid sizes B={B} L={L}')
    return n


def _rows(t: torch.Tensor, what: str):
    require_gpu(t, what)
    if t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1 or t.shape[0] < 1 or t.shape[1] < 1:
        raise TypeError(f'noise: {what} must be a non-empty (rows, L) float32 tensor with unit stride along L')
    return t.shape


def _vector(t: Optional[torch.Tensor], n: int, dtype, what: str):
    if t is None:
        return None
    require_gpu(t, what)
    if t.dtype != dtype or tuple(t.shape) != (n,) or not t.is_contiguous():
        raise ValueError(f'noise: {what} must be a contiguous ({n},) {dtype} tensor')
    return t


def _levels(snr_db: torch.Tensor, B: int) -> int:
    require_gpu(snr_db, 'snr_db')
    if snr_db.dtype != torch.float32 or snr_db.dim() != 2 or snr_db.shape[0] != B or not snr_db.is_contiguous():
        raise ValueError(f'noise: snr_db must be a contiguous ({B}, K) float32 tensor')
    K = snr_db.shape[1]
    if not 1 <= K <= max_levels():
        raise ValueError(f'noise: {K} levels; a call takes 1..{max_levels()} (sconf_noise_max_levels)')
    return K


def power(src: torch.Tensor, lengths: Optional[torch.Tensor] = None, src_lengths: Optional[torch.Tensor] = None,
          offsets: Optional[torch.Tensor] = None, L: Optional[int] = None, B: Optional[int] = None) -> torch.Tensor:
    """src (rows, Ls) f32 with unit stride along Ls -> (B,) f64 mean squares.  Without offsets and src_lengths: of the first
    lengths[b] (or all) samples of row b (B = rows, L = Ls).  With them (both (·,) int64; src_lengths is filled with Ls where only
    offsets are given): of the L-sample stretch (lengths[b] of it) that starts at offsets[b] of row b - of row 0 where rows == 1 -
    and wraps at src_lengths.  See include/sconf_noise.h."""
    rows, Ls = _rows(src, 'waveform')
    wrapped = offsets is not None or src_lengths is not None
    B = rows if B is None else int(B)
    L = Ls if L is None else int(L)
    if rows not in (1, B) or (not wrapped and (L != Ls or B != rows)):
        raise ValueError(f'noise.power: {rows} rows of {Ls} for B = {B}, L = {L}')
    if wrapped and src_lengths is None:
        src_lengths = torch.full((rows,), Ls, dtype=torch.int64, device=src.device)
    lengths, src_lengths, offsets = _vector(lengths, B, torch.int64, 'lengths'), _vector(src_lengths, rows, torch.int64, 'src_lengths'), \
        _vector(offsets, B, torch.int64, 'offsets')
    out = torch.empty(B, dtype=torch.float64, device=src.device)
    nbytes = workspace(B, L)
    ws = _workspace(nbytes, src.device)
    _lib.call('sconf_noise_power', _p(src), src.stride(0) if rows > 1 else Ls, rows, _p(lengths), _p(src_lengths), _p(offsets), L, B, _p(out),
              _p(ws), nbytes, _stream())
    return out


def add_gaussian(wave: torch.Tensor, lengths: Optional[torch.Tensor], power: torch.Tensor, snr_db: torch.Tensor, seed: int,
                 first_row: int = 0, first_sample: int = 0) -> torch.Tensor:
    """wave (B, L) f32, power (B,) f64 (`power` of it), snr_db (B, K) f32 -> (B, K, L) f32: level k of row b is wave[b] plus the
    normals of (seed, first_row + b, first_sample + i) at snr_db[b, k] dB.  See include/sconf_noise.h."""
    B, L = _rows(wave, 'waveform')
    K = _levels(snr_db, B)
    lengths, power = _vector(lengths, B, torch.int64, 'lengths'), _vector(power, B, torch.float64, 'power')
    if first_row < 0 or first_sample < 0:
        raise ValueError(f'noise.add_gaussian: first_row = {first_row} and first_sample = {first_sample} must not be negative')
    seed = int(seed) & (2 ** 64 - 1)
    out = torch.empty(B, K, L, dtype=torch.float32, device=wave.device)
    _lib.call('sconf_noise_add_gaussian', _p(wave), wave.stride(0) if B > 1 else L, _p(lengths), L, B, _p(power), _p(snr_db), K,
              seed - 2 ** 64 if seed >= 2 ** 63 else seed, int(first_row), int(first_sample), _p(out), L, _stream())
    return out


def add_background(wave: torch.Tensor, lengths: Optional[torch.Tensor], noise: torch.Tensor, noise_lengths: Optional[torch.Tensor],
                   offsets: Optional[torch.Tensor], power: torch.Tensor, noise_power: torch.Tensor, snr_db: torch.Tensor) -> torch.Tensor:
    """wave (B, L) f32, noise (1 or B, NL) f32, power and noise_power (B,) f64, snr_db (B, K) f32 -> (B, K, L) f32: wave[b] plus the
    clip from offsets[b] on, wrapped at noise_lengths (NL where None), scaled to snr_db[b, k] dB.  See include/sconf_noise.h."""
    B, L = _rows(wave, 'waveform')
    R, NL = _rows(noise, 'noise')
    if R not in (1, B):
        raise ValueError(f'noise.add_background: {R} clips for {B} rows; one clip or one per row')
    K = _levels(snr_db, B)
    if noise_lengths is None:
        noise_lengths = torch.full((R,), NL, dtype=torch.int64, device=wave.device)
    lengths, noise_lengths, offsets = _vector(lengths, B, torch.int64, 'lengths'), _vector(noise_lengths, R, torch.int64, 'noise_lengths'), \
        _vector(offsets, B, torch.int64, 'offsets')
    power, noise_power = _vector(power, B, torch.float64, 'power'), _vector(noise_power, B, torch.float64, 'noise_power')
    out = torch.empty(B, K, L, dtype=torch.float32, device=wave.device)
    _lib.call('sconf_noise_add_background', _p(wave), wave.stride(0) if B > 1 else L, _p(lengths), L, B, _p(noise),
              noise.stride(0) if R > 1 else NL, R, _p(noise_lengths), _p(offsets), _p(power), _p(noise_power), _p(snr_db), K, _p(out), L,
              _stream())
    return out
