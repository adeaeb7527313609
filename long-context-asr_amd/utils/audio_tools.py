"""Audio front end — mirror of lcasr/utils/audio_tools.py (same names and spellings), with the spectrogram on the device.

`to_spectogram` is the reference's torchaudio MelSpectrogram(win_length 400, hop_length 160, n_fft 512, n_mels 80) followed by the
per-row mean / std normalisation, as one fused HIP path (csrc/audio.hip through hip/audio.py): the waveform is read once, neither
the STFT nor a padded copy of the waveform reaches memory.

`resample` is the reference's torchaudio.transforms.Resample(orig, new) with its defaults (sinc_interp_hann, lowpass_filter_width 6,
rolloff 0.99), a polyphase windowed-sinc filter, as one HIP kernel (csrc/resample.hip through hip/resample.py): the filter is
evaluated here on the host in f64, cast to f32 as torchaudio does, and handed to the device as a compact table of the taps that
are not clamped to zero; the left channel or the channel mean is taken while the waveform is read, once.  `processing_chain` takes
the decoded waveform and its sample rate: 16 kHz as it is, any other rate with resample_input=True.  Decoding audio files stays on
the host and outside this package."""
from __future__ import annotations

import math
from typing import Optional

import torch

from ..hip import audio
from ..hip import resample as resampler

WIN_LENGTH = 400
HOP_LENGTH = 160
SR = 16000
N_FFT = 2 ** math.ceil(math.log2(WIN_LENGTH))  # 512
N_MELS = 80

LOWPASS_FILTER_WIDTH = 6
ROLLOFF = 0.99

_tables = {}                                   # (device, n_mels) -> (filterbank, ranges) on that device
_resample_tables = {}                          # (device, orig, new) -> (taps, first, O, P) on that device


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


def resample_table(orig_sr: int, new_sr: int):
    """The kernel of torchaudio.transforms.Resample(orig_sr, new_sr) as a compact table: (taps (P, K) f32, first (P) int32, O, P).
    With g = gcd, O = orig / g, P = new / g, base = min(O, P) * 0.99 and width = ceil(6 O / base), tap i of phase p of the dense kernel
    (i = 0 .. 2 width + O - 1, over the row padded with `width` zeros on the left) is sinc(t) cos^2(pi t / 12) base / O at
    t = ((i - width) / O - p / P) base clamped to [-6, 6], evaluated in f64 and cast to f32.  Clamped taps are below 2e-49 and 0 in
    f32; the others of a phase are consecutive.  taps[p] holds them from dense index first[p] + width on, K = the largest count,
    shorter phases padded with 0: output q P + p = sum_k taps[p][k] x[q O + first[p] + k]."""
    g = math.gcd(orig_sr, new_sr)
    O, P = orig_sr // g, new_sr // g
    base = min(O, P) * ROLLOFF
    width = math.ceil(LOWPASS_FILTER_WIDTH * O / base)
    idx = torch.arange(-width, width + O, dtype=torch.float64)[None] / O
    raw = (torch.arange(0, -P, -1, dtype=torch.float64)[:, None] / P + idx) * base
    live = raw.abs() < LOWPASS_FILTER_WIDTH
    t = raw.clamp(-LOWPASS_FILTER_WIDTH, LOWPASS_FILTER_WIDTH)
    window = torch.cos(t * math.pi / LOWPASS_FILTER_WIDTH / 2) ** 2
    t = t * math.pi
    dense = (torch.where(t == 0, torch.ones_like(t), t.sin() / t) * window * (base / O)).float()          # (P, 2 width + O)
    count = live.sum(1)
    start = live.float().argmax(1)
    K = int(count.max())
    cols = start[:, None] + torch.arange(K)[None]
    inside = torch.arange(K)[None] < count[:, None]
    taps = torch.where(inside, dense.gather(1, cols.clamp(max=dense.shape[1] - 1)), torch.zeros(1))
    return taps.contiguous(), (start - width).to(torch.int32).contiguous(), O, P


def _device_resample_table(device, orig_sr: int, new_sr: int):
    key = (str(device), int(orig_sr), int(new_sr))
    if key not in _resample_tables:
        g = math.gcd(orig_sr, new_sr)
        O, P = orig_sr // g, new_sr // g
        # a phase's live taps are the integers of an open interval of length 12 O / base: at least that many less one.  Refused
        # before the dense kernel (P x (2 width + O) in f64) is evaluated: for rates without a common factor it would not fit memory.
        least = math.ceil(2 * LOWPASS_FILTER_WIDTH * O / (min(O, P) * ROLLOFF)) - 1
        if P * least > resampler.max_table():
            raise ValueError(f'resample: {orig_sr} -> {new_sr} Hz needs a table of {P} x {least} taps or more; at most '
                             f'{resampler.max_table()} (sconf_resample_max_table) are kept in LDS')
        taps, first, O, P = resample_table(orig_sr, new_sr)
        if taps.numel() > resampler.max_table():
            raise ValueError(f'resample: {orig_sr} -> {new_sr} Hz needs a table of {P} x {taps.shape[1]} taps; at most '
                             f'{resampler.max_table()} (sconf_resample_max_table) are kept in LDS')
        _resample_tables[key] = (taps.to(device), first.to(device), O, P)
    return _resample_tables[key]


def _check_rates(orig_sr, new_sr):
    for r in (orig_sr, new_sr):
        if isinstance(r, bool) or not isinstance(r, int) or r <= 0:
            raise ValueError(f'resample: sample rates must be positive integers, got {orig_sr!r} -> {new_sr!r}')


def resampled_lengths(sample_lengths, orig_sr: int, new_sr: int):
    """Samples of a recording of that many samples (int or integer tensor) after resample: ceil(new * n / orig)."""
    _check_rates(orig_sr, new_sr)
    g = math.gcd(orig_sr, new_sr)
    O, P = orig_sr // g, new_sr // g
    if torch.is_tensor(sample_lengths):
        sample_lengths = sample_lengths.to(torch.int64)                    # an hour at 44.1 kHz times 160 is past int32
    return (sample_lengths * P + (O - 1)) // O


def resample(waveform: torch.Tensor, orig_sr: int, new_sr: int, lengths=None, mix: Optional[str] = None) -> torch.Tensor:
    """torchaudio.transforms.Resample(orig_sr, new_sr)(waveform) on the device: waveform (L,) or (rows, L) f32 on the GPU, every row
    resampled on its own -> (L',) or (rows, L'), L' = ceil(new_sr * L / orig_sr).
    lengths: (rows,) sample counts of a padded batch (tensor or sequence).  Row b is processed as if it were alone: nothing at or
    beyond lengths[b] is read, outputs behind resampled_lengths(lengths[b], orig_sr, new_sr) are 0.
    mix: 'left' or 'mean' takes the rows as the channels of ONE recording, (channels, L) -> (1, L'): resample(grab_left_channel(w)) and
    resample(take_mean_channel(w)) in one pass over the waveform, without the mono copy (lengths: one count, or None).
    Equal rates return the waveform (the mixed channel with mix)."""
    _check_rates(orig_sr, new_sr)
    if mix not in (None, 'left', 'mean'):
        raise ValueError(f"resample: mix must be None, 'left' or 'mean', got {mix!r}")
    if waveform.dim() not in (1, 2):
        raise ValueError('Waveform must be 1D or 2D')
    if waveform.dtype != torch.float32:
        raise TypeError(f'resample: waveform must be float32, got {waveform.dtype}')
    if orig_sr == new_sr:
        return waveform if mix is None else grab_left_channel(waveform) if mix == 'left' else take_mean_channel(waveform)
    if waveform.shape[-1] < 1 or waveform.shape[0] < 1:
        raise ValueError(f'resample: empty waveform {tuple(waveform.shape)}')
    wave = waveform[None] if waveform.dim() == 1 else waveform
    if wave.stride(1) != 1:
        wave = wave.contiguous()
    rows = 1 if mix is not None else wave.shape[0]
    if lengths is not None:
        lengths = torch.as_tensor(lengths).reshape(-1) if mix is not None else torch.as_tensor(lengths)
        if tuple(lengths.shape) != (rows,) or lengths.dtype.is_floating_point:
            raise ValueError(f'resample: lengths must be {rows} integer sample counts')
        if not lengths.is_cuda and (int(lengths.min()) < 0 or int(lengths.max()) > wave.shape[1]):
            raise ValueError(f'resample: every length must be in 0..{wave.shape[1]}')
        lengths = lengths.to(device=wave.device, dtype=torch.int64).contiguous()
    taps, first, O, P = _device_resample_table(wave.device, orig_sr, new_sr)
    out = resampler.resample_rows(wave[None] if mix is not None else wave, lengths, taps, first, O, P, mix=mix == 'mean')
    return out[0] if waveform.dim() == 1 and mix is None else out


def total_seconds(spectogram_length: int) -> float:
    '''converts number of frames to seconds'''
    return (spectogram_length * HOP_LENGTH) / SR


def total_frames(seconds: float) -> int:
    '''inverse of total_seconds'''
    return int((seconds * 16000) / HOP_LENGTH)


def processing_chain(waveform: torch.Tensor, sample_rate: int, normalise: bool = True, resample_input: bool = False) -> torch.Tensor:
    """The reference's chain from the decoded file on: left channel, resampled to 16 kHz, then the spectrogram (1, 80, T).  The
    resampling step is taken only with resample_input=True; without it any rate but 16 kHz is refused, as before."""
    if sample_rate != SR:
        if not resample_input:
            raise NotImplementedError(f'processing_chain: sample rate {sample_rate} Hz; pass resample_input=True to resample to {SR} Hz '
                                      f'on the device')
        return to_spectogram(resample(waveform, sample_rate, SR, mix='left'), global_normalisation=normalise)
    return to_spectogram(grab_left_channel(waveform), global_normalisation=normalise)
