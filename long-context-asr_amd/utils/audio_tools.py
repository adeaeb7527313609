"""Audio front end — mirror of lcasr/utils/audio_tools.py (same names and spellings), with the spectrogram on the device.

`to_spectogram` is the reference's torchaudio MelSpectrogram(win_length 400, hop_length 160, n_fft 512, n_mels 80) followed by the
per-row mean / std normalisation, as one fused HIP path (csrc/audio.hip through hip/audio.py): the waveform is read once, neither
the STFT nor a padded copy of the waveform reaches memory.  Decoding audio files and resampling stay on the host and outside this
package: `processing_chain` takes the decoded waveform and its sample rate, and refuses any rate but 16 kHz."""
from __future__ import annotations

import math
from typing import Optional

import torch

from ..hip import audio

WIN_LENGTH = 400
HOP_LENGTH = 160
SR = 16000
N_FFT = 2 ** math.ceil(math.log2(WIN_LENGTH))  # 512
N_MELS = 80

_tables = {}                                   # (device, n_mels) -> (filterbank, ranges) on that device


def mel_filterbank(n_mels: int = N_MELS) -> torch.Tensor:
    """(257, n_mels) f32 HTK filterbank, 0..8000 Hz, no area normalisation: torchaudio.functional.melscale_fbanks, evaluated on
    the host in f32 in its order of operations."""
    all_freqs = torch.linspace(0, SR // 2, N_FFT // 2 + 1)
    m_max = 2595.0 * math.log10(1.0 + (SR // 2) / 700.0)
    m_pts = torch.linspace(0.0, m_max, n_mels + 2)
    f_pts = 700.0 * (10 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    down = (-1.0 * slopes[:, :-2]) / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    return torch.max(torch.zeros(1), torch.min(down, up)).contiguous()


def _device_tables(device, n_mels: int):
    key = (str(device), int(n_mels))
    if key not in _tables:
        fb = mel_filterbank(n_mels)
        _tables[key] = (fb.to(device), audio.filter_ranges(fb).to(device))
    return _tables[key]


def grab_left_channel(waveform: torch.Tensor) -> torch.Tensor:
    if len(waveform.shape) == 2:
        return waveform[0, None]
    elif len(waveform.shape) == 1:
        return waveform[None]
    else:
        raise ValueError("Waveform must be 1D or 2D")


def take_mean_channel(waveform: torch.Tensor) -> torch.Tensor:
    if len(waveform.shape) == 2:
        return waveform.mean(0, keepdim=True)
    elif len(waveform.shape) == 1:
        return waveform[None]
    else:
        raise ValueError("Waveform must be 1D or 2D")


def spectogram_lengths(sample_lengths):
    """Frames of a recording of that many samples (int or tensor): 1 + n // 160."""
    return 1 + sample_lengths // HOP_LENGTH


def to_spectogram(waveform: torch.Tensor, global_normalisation=True, lengths=None, out_dtype: torch.dtype = torch.float32,
                  n_mels: int = N_MELS) -> torch.Tensor:
    """waveform (L,) or (B, L) f32 on the GPU, 16 kHz -> (n_mels, T) or (B, n_mels, T), T = 1 + L // 160, as the reference returns
    them (feature-major, what SCConformerXL.forward takes).
    lengths: (B,) sample counts of a padded batch (tensor or sequence).  Row b is processed as if it were alone: reflected at its own
    end, statistics over its own 1 + lengths[b] // 160 frames, later frames 0; nothing at or beyond lengths[b] is read.
    out_dtype: float32 or bfloat16."""
    if waveform.dim() not in (1, 2):
        raise ValueError('Waveform must be 1D or 2D')
    if waveform.shape[-1] <= N_FFT // 2:
        raise ValueError(f'to_spectogram: {waveform.shape[-1]} samples: reflect padding of {N_FFT // 2} needs a longer waveform')
    if not 1 <= n_mels <= audio.MAX_MELS:
        raise ValueError(f'to_spectogram: n_mels must be in 1..{audio.MAX_MELS}')
    wave = waveform[None] if waveform.dim() == 1 else waveform
    if wave.dtype != torch.float32:
        raise TypeError(f'to_spectogram: waveform must be float32, got {wave.dtype}')
    if wave.stride(1) != 1:
        wave = wave.contiguous()
    if lengths is not None:
        lengths = torch.as_tensor(lengths)
        if tuple(lengths.shape) != (wave.shape[0],) or lengths.dtype.is_floating_point:
            raise ValueError(f'to_spectogram: lengths must be {wave.shape[0]} integer sample counts')
        if not lengths.is_cuda and (int(lengths.min()) <= N_FFT // 2 or int(lengths.max()) > wave.shape[1]):
            raise ValueError(f'to_spectogram: every length must be in {N_FFT // 2 + 1}..{wave.shape[1]}')
        lengths = lengths.to(device=wave.device, dtype=torch.int64).contiguous()
    fb, ranges = _device_tables(wave.device, n_mels)
    spec = audio.melspec(wave, lengths, fb, ranges, normalise=bool(global_normalisation), out_dtype=out_dtype)
    return spec[0] if waveform.dim() == 1 else spec


def total_seconds(spectogram_length: int) -> float:
    '''converts number of frames to seconds'''
    return (spectogram_length * HOP_LENGTH) / SR


def total_frames(seconds: float) -> int:
    '''inverse of total_seconds'''
    return int((seconds * 16000) / HOP_LENGTH)


def processing_chain(waveform: torch.Tensor, sample_rate: int, normalise: bool = True) -> torch.Tensor:
    """The reference's chain from the decoded file on: left channel, then the spectrogram (1, 80, T).  Resampling is not part of
    this package."""
    if sample_rate != SR:
        raise NotImplementedError(f'processing_chain: sample rate {sample_rate} Hz; resample to {SR} Hz on the host first')
    return to_spectogram(grab_left_channel(waveform), global_normalisation=normalise)
