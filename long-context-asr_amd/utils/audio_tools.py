"""Audio front end — mirror of lcasr/utils/audio_tools.py (same names and spellings), with the spectrogram on the device.

`to_spectogram` is the reference's torchaudio MelSpectrogram(win_length 400, hop_length 160, n_fft 512, n_mels 80) followed by the
per-row mean / std normalisation, as one fused HIP path (csrc/audio.hip through hip/audio.py): the waveform is read once, neither
the STFT nor a padded copy of the waveform reaches memory.

`resample` is the reference's torchaudio.transforms.Resample(orig, new) with its defaults (sinc_interp_hann, lowpass_filter_width 6,
rolloff 0.99), a polyphase windowed-sinc filter, as one HIP kernel (csrc/resample.hip through hip/resample.py): the filter is
evaluated here on the host in f64, cast to f32 as torchaudio does, and handed to the device as a compact table of the taps that
are not clamped to zero; the left channel or the channel mean is taken while the waveform is read, once.  `processing_chain` takes
the decoded waveform and its sample rate: 16 kHz as it is, any other rate with resample_input=True.

`wave_power`, `add_gaussian_snr` and `add_background_noise` are the corruptions of the reference's noise-robustness drivers
(audiomentations' AddGaussianSNR and AddBackgroundNoise; csrc/noise.hip through hip/noise.py) between `resample` and `to_spectogram`:
the mean square of every row in one pass, then one launch that mixes all the SNR levels asked for from one noise sequence.
Decoding audio files stays on the host and outside this package."""
from __future__ import annotations

import math
from typing import Optional

import torch

from ..hip import audio
from ..hip import noise as noiser
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


def _noise_rows(waveform: torch.Tensor, lengths, what: str):
    """((rows, L) view with unit stride along L, lengths (rows,) int64 on the device or None)."""
    if waveform.dim() not in (1, 2):
        raise ValueError('Waveform must be 1D or 2D')
    if waveform.dtype != torch.float32:
        raise TypeError(f'{what}: waveform must be float32, got {waveform.dtype}')
    if waveform.shape[-1] < 1 or waveform.shape[0] < 1:
        raise ValueError(f'{what}: empty waveform {tuple(waveform.shape)}')
    wave = waveform[None] if waveform.dim() == 1 else waveform
    if wave.stride(1) != 1:
        wave = wave.contiguous()
    return wave, _row_counts(lengths, wave.shape[0], 0, wave.shape[1], wave.device, what, 'lengths')


def _row_counts(v, rows: int, lo: int, hi: int, device, what: str, name: str):
    """None, or `rows` integers as an int64 device vector; a host-given one must lie in lo..hi."""
    if v is None:
        return None
    v = torch.as_tensor(v)
    if tuple(v.shape) != (rows,) or v.dtype.is_floating_point:
        raise ValueError(f'{what}: {name} must be {rows} integers')
    if not v.is_cuda and (int(v.min()) < lo or int(v.max()) > hi):
        raise ValueError(f'{what}: every one of {name} must be in {lo}..{hi}')
    return v.to(device=device, dtype=torch.int64).contiguous()


def _snr_levels(snr_db, rows: int, device, what: str):
    """snr_db as the (rows, K) f32 device tensor of a launch, and whether it was a single number (no level axis in the result).
    A number, a sequence of K numbers shared by the rows, or a (rows, K) tensor; NaN in a host-given value is refused."""
    single = not torch.is_tensor(snr_db) and not hasattr(snr_db, '__len__')
    t = torch.as_tensor([snr_db] if single else snr_db)
    if torch.is_tensor(snr_db) and snr_db.dim() == 2:
        if snr_db.shape[0] != rows:
            raise ValueError(f'{what}: snr_db of shape {tuple(snr_db.shape)} for {rows} rows')
    elif t.dim() != 1:
        raise ValueError(f'{what}: snr_db must be a number, a sequence of K numbers or a (rows, K) tensor')
    if not 1 <= t.shape[-1] <= noiser.max_levels():
        raise ValueError(f'{what}: {t.shape[-1]} SNR levels; a call takes 1..{noiser.max_levels()} (sconf_noise_max_levels)')
    if not t.is_cuda and bool(torch.isnan(t.double()).any()):
        raise ValueError(f'{what}: snr_db holds NaN')
    t = t.to(device=device, dtype=torch.float32)
    return (t[None].expand(rows, -1) if t.dim() == 1 else t).contiguous(), single


def _shaped(out: torch.Tensor, waveform: torch.Tensor, single: bool) -> torch.Tensor:
    """(rows, K, L) -> the input's shape for a single level, (K, L) for a 1-D input."""
    out = out[:, 0] if single else out
    return out[0] if waveform.dim() == 1 else out


def wave_power(waveform: torch.Tensor, lengths=None) -> torch.Tensor:
    """Mean square of every row, f64 (rows,) on the device ((1,) for a 1-D waveform): waveform (L,) or (rows, L) f32 on the GPU; with
    lengths (rows,) over the first lengths[b] samples of row b, 0 for an empty row.  Exact squares summed in f64 in a fixed order:
    the same bits on every call, and for a row of a batch the bits of the row alone."""
    wave, lengths = _noise_rows(waveform, lengths, 'wave_power')
    return noiser.power(wave, lengths)


def add_gaussian_snr(waveform: torch.Tensor, snr_db, lengths=None, seed: int = 17925, first_row: int = 0, first_sample: int = 0) -> torch.Tensor:
    """audiomentations' AddGaussianSNR at a set SNR, on the device: y = x + sigma z with sigma = sqrt(mean x^2) 10^(-snr_db / 20) per
    row.  waveform (L,) or (rows, L) f32 on the GPU.  snr_db: a number -> the input's shape; a sequence of K numbers shared by the
    rows or a (rows, K) tensor -> (rows, K, L), or (K, L) for a 1-D input, every level from the SAME standard normals z (as the
    reference's per-file re-seeding gives them), in one launch.
    z is a function of (seed, first_row + row, first_sample + i) alone (include/sconf_noise.h): a row of a batch gets the noise it
    would get alone with first_row = its index, a piece of a recording the noise of the whole with first_sample = its start.
    lengths: (rows,) sample counts of a padded batch; the power is taken over them and samples behind them are 0.  A silent row,
    or snr_db = +inf, returns the input bit for bit."""
    wave, lengths = _noise_rows(waveform, lengths, 'add_gaussian_snr')
    snr, single = _snr_levels(snr_db, wave.shape[0], wave.device, 'add_gaussian_snr')
    out = noiser.add_gaussian(wave, lengths, noiser.power(wave, lengths), snr, int(seed), int(first_row), int(first_sample))
    return _shaped(out, waveform, single)


def add_background_noise(waveform: torch.Tensor, noise: torch.Tensor, snr_db, lengths=None, noise_lengths=None, offsets=None) -> torch.Tensor:
    """audiomentations' AddBackgroundNoise at a set SNR, on the device: y = x + g v, v[i] = noise[(offset + i) mod its length] - the clip
    cropped at `offsets` where it is longer than the row, repeated where it is shorter - and g = sqrt(mean x^2 / mean v^2)
    10^(-snr_db / 20), the clip's mean square over the samples actually used.  A clip with an rms below 1e-9 leaves the input as it
    is, bit for bit, and so does a silent row.
    noise: (NL,) or (1, NL) f32 on the GPU, one clip for all rows, or (rows, NL), one per row; noise_lengths and offsets (one per
    clip, one per row; tensors or sequences) default to NL and 0.  snr_db, lengths and the result's shape as for add_gaussian_snr."""
    wave, lengths = _noise_rows(waveform, lengths, 'add_background_noise')
    rows = wave.shape[0]
    if noise.dim() not in (1, 2) or noise.dtype != torch.float32 or noise.shape[-1] < 1:
        raise TypeError('add_background_noise: noise must be a non-empty (NL,) or (clips, NL) float32 tensor')
    clip = noise[None] if noise.dim() == 1 else noise
    if clip.shape[0] not in (1, rows):
        raise ValueError(f'add_background_noise: {clip.shape[0]} clips for {rows} rows; one clip or one per row')
    if clip.stride(1) != 1:
        clip = clip.contiguous()
    NL = clip.shape[1]
    noise_lengths = _row_counts(noise_lengths, clip.shape[0], 1, NL, wave.device, 'add_background_noise', 'noise_lengths')
    if noise_lengths is None:
        noise_lengths = torch.full((clip.shape[0],), NL, dtype=torch.int64, device=wave.device)
    offsets = _row_counts(offsets, rows, 0, NL - 1, wave.device, 'add_background_noise', 'offsets')      # the kernel wraps one past its clip
    snr, single = _snr_levels(snr_db, rows, wave.device, 'add_background_noise')
    p_noise = noiser.power(clip, lengths, noise_lengths, offsets, L=wave.shape[1], B=rows)
    out = noiser.add_background(wave, lengths, clip, noise_lengths, offsets, noiser.power(wave, lengths), p_noise, snr)
    return _shaped(out, waveform, single)


def processing_chain(waveform: torch.Tensor, sample_rate: int, normalise: bool = True, resample_input: bool = False, corrupt=None) -> torch.Tensor:
    """The reference's chain from the decoded file on: left channel, resampled to 16 kHz, then the spectrogram (1, 80, T).  The
    resampling step is taken only with resample_input=True; without it any rate but 16 kHz is refused, as before.
    corrupt: a callable (waveform (1, L) at 16 kHz, sample_rate=16000) -> waveform of that shape, applied before the spectrogram - an
    utils.augmentation.AddGaussianSNR, say, where the reference's noise experiments corrupt the file."""
    if sample_rate != SR:
        if not resample_input:
            raise NotImplementedError(f'processing_chain: sample rate {sample_rate} Hz; pass resample_input=True to resample to {SR} Hz '
                                      f'on the device')
        left = resample(waveform, sample_rate, SR, mix='left')
    else:
        left = grab_left_channel(waveform)
    if corrupt is not None:
        left = corrupt(left, sample_rate=SR)
    return to_spectogram(left, global_normalisation=normalise)
