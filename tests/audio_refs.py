"""Plain-torch CPU restatement of the audio front end (include/sconf_audio.h, lcasr_amd.utils.audio_tools.to_spectogram).

The reference itself is torchaudio.transforms.MelSpectrogram(win_length=400, hop_length=160, n_fft=512, n_mels=80) followed by
(spec - mean) / std per row; torchaudio is not a dependency here, so the contract is restated on torch.stft, parameterised by the
working dtype: float64 is the yardstick of the GPU tests, float32 (what the reference computes in) calibrates their tolerance.
The filterbank is always evaluated in f32 in torchaudio's order of operations and then cast.  TEST INFRASTRUCTURE, plain module."""
import math

import torch

N_FFT, HOP, WIN, N_BINS, PAD, SR = 512, 160, 400, 257, 256, 16000


def mel_filterbank(n_mels=80, dtype=torch.float32):
    """torchaudio.functional.melscale_fbanks(257, 0, 8000, n_mels, 16000, norm=None, mel_scale='htk'), in f32, then cast."""
    all_freqs = torch.linspace(0, SR // 2, N_BINS)
    m_pts = torch.linspace(0.0, 2595.0 * math.log10(1.0 + (SR // 2) / 700.0), n_mels + 2)
    f_pts = 700.0 * (10 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None, :] - all_freqs[:, None]
    fb = torch.clamp(torch.min(-slopes[:, :-2] / f_diff[:-1], slopes[:, 2:] / f_diff[1:]), min=0)
    assert fb.dtype == torch.float32 and fb.shape == (N_BINS, n_mels)
    return fb.to(dtype)


def filter_ranges(fb):
    """(n_mels, 2) int32: half-open range of the non-zero bins of every filter, by a loop."""
    out = []
    for m in range(fb.shape[1]):
        nz = fb[:, m].nonzero().flatten().tolist()
        out.append([nz[0], nz[-1] + 1] if nz else [0, 0])
    return torch.tensor(out, dtype=torch.int32)


def test_signal(L, seed=0):
    """0.3 sin(2 pi 440 t) + 0.05 randn (1 + sin(2 pi 1.3 t)), f32: a tone over noise whose level moves, so that no mel row is flat."""
    t = torch.arange(L, dtype=torch.float64) / SR
    n = torch.randn(L, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    return (0.3 * torch.sin(2 * math.pi * 440 * t) + 0.05 * n * (1 + torch.sin(2 * math.pi * 1.3 * t))).float()


def mel_row(wave, n_mels=80, dtype=torch.float64):
    """(n_mels, 1 + L // 160) raw mel power spectrogram of one (L,) waveform."""
    L = wave.shape[0]
    if L <= PAD:
        raise ValueError(f'{L} samples: reflect padding of {PAD} needs more')
    x = wave.to(dtype)
    st = torch.stft(x, N_FFT, hop_length=HOP, win_length=WIN, window=torch.hann_window(WIN, periodic=True, dtype=dtype), center=True,
                    pad_mode='reflect', normalized=False, onesided=True, return_complex=True)
    power = st.real ** 2 + st.imag ** 2                                   # (257, T)
    return (power.transpose(0, 1) @ mel_filterbank(n_mels, dtype)).transpose(0, 1).contiguous()


def normalise_row(spec):
    return (spec - spec.mean(-1, keepdim=True)) / spec.std(-1, keepdim=True)


def to_spectogram(waveform, global_normalisation=True, lengths=None, out_dtype=None, n_mels=80, dtype=torch.float64):
    """The contract of lcasr_amd.utils.audio_tools.to_spectogram on the CPU: (L,) -> (n_mels, T), (B, L) -> (B, n_mels, T),
    T = 1 + L // 160; with lengths every row is computed from its own samples alone and is 0 behind its own frames.
    out_dtype None keeps the working dtype."""
    wave = waveform[None] if waveform.dim() == 1 else waveform
    B, L = wave.shape
    if L <= PAD:
        raise ValueError(f'{L} samples: reflect padding of {PAD} needs more')
    T = 1 + L // HOP
    out = torch.zeros(B, n_mels, T, dtype=dtype)
    for b in range(B):
        n = L if lengths is None else int(lengths[b])
        s = mel_row(wave[b, :n], n_mels, dtype)
        out[b, :, :s.shape[1]] = normalise_row(s) if global_normalisation else s
    if out_dtype is not None:
        out = out.to(out_dtype)
    return out[0] if waveform.dim() == 1 else out


def melspec(wave, lengths, fb, ranges, normalise=True, out_dtype=torch.float32):
    """lcasr_amd.hip.audio.melspec on the CPU, in f32 (the emulated binding of the host-logic tests)."""
    assert wave.dim() == 2 and wave.dtype == torch.float32 and tuple(fb.shape) == (N_BINS, ranges.shape[0])
    return to_spectogram(wave, normalise, lengths, out_dtype, n_mels=fb.shape[1], dtype=torch.float32)


def direct_dft_mel(wave, n_mels=80):
    """Independent of torch.stft: frames cut from an explicitly reflected copy, windowed, multiplied with the DFT matrix in f64."""
    x = wave.double()
    L = x.shape[0]
    idx = torch.arange(-PAD, L + PAD)
    idx = torch.where(idx < 0, -idx, idx)
    idx = torch.where(idx >= L, 2 * (L - 1) - idx, idx)
    padded = x[idx]
    T = 1 + L // HOP
    win = torch.zeros(N_FFT, dtype=torch.float64)
    n = torch.arange(WIN, dtype=torch.float64)
    win[(N_FFT - WIN) // 2:(N_FFT + WIN) // 2] = 0.5 - 0.5 * torch.cos(2 * math.pi * n / WIN)
    frames = torch.stack([padded[t * HOP:t * HOP + N_FFT] for t in range(T)]) * win          # (T, 512)
    k = torch.arange(N_BINS, dtype=torch.float64)[:, None] * torch.arange(N_FFT, dtype=torch.float64)[None, :]
    ang = 2 * math.pi * (k % N_FFT) / N_FFT
    re, im = frames @ torch.cos(ang).T, frames @ torch.sin(ang).T                            # (T, 257)
    return ((re ** 2 + im ** 2) @ mel_filterbank(n_mels, torch.float64)).T.contiguous()


def row_error(x, r):
    """E(x): max over rows (b, mel) of max_t |x - r| / max_t |r|, r the f64 restatement.  A row that is exactly 0 in r (an empty
    filter: 128 mels have some below 100 Hz) must be exactly 0 in x and does not enter the maximum."""
    x, r = x.detach().double().cpu(), r.detach().double().cpu()
    x, r = x.reshape(-1, x.shape[-1]), r.reshape(-1, r.shape[-1])
    num, den = (x - r).abs().amax(1), r.abs().amax(1)
    flat = den == 0
    assert not bool((num[flat] != 0).any()), 'a row that is exactly 0 in the restatement is not 0 in the output'
    return float((num[~flat] / den[~flat]).max()) if bool((~flat).any()) else 0.0
