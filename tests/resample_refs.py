"""Plain-torch CPU restatement of the resampler (include/sconf_resample.h, lcasr_amd.utils.audio_tools.resample).

The reference itself is torchaudio.transforms.Resample(orig, new) with its defaults (sinc_interp_hann, lowpass_filter_width 6,
rolloff 0.99); torchaudio is not a dependency here, so the contract is restated on conv1d the way torchaudio computes it - a dense
(P, 1, 2 width + O) kernel at stride O over the zero-padded row - parameterised by the working dtype: float64 taps and sums are
the yardstick of the GPU tests, float32 (the f64 kernel cast to f32, f32 conv1d: what the reference computes) shows how far the
reference itself is from it.  `bound` is the per-sample error bound of an f32 evaluation, derived below.  TEST INFRASTRUCTURE,
plain module."""
import math

import torch

WIDTH, ROLLOFF = 6, 0.99
# the rate pairs of the tests: (orig, new) -> (O, P, K), K the largest count of taps of a phase that are not clamped
PAIRS = {(44100, 16000): (441, 160, 34), (22050, 16000): (441, 320, 17), (11025, 16000): (441, 640, 13), (48000, 16000): (3, 1, 37),
         (32000, 16000): (2, 1, 25), (24000, 16000): (3, 2, 19), (8000, 16000): (1, 2, 13), (44100, 48000): (147, 160, 13)}


def ratio(orig, new):
    g = math.gcd(orig, new)
    return orig // g, new // g


def kernel(orig, new, dtype=torch.float64):
    """torchaudio.functional._get_sinc_resample_kernel: (P, 2 width + O) taps evaluated in f64 and cast, the raw (unclamped) filter
    times t of every tap, and width."""
    O, P = ratio(orig, new)
    base = min(O, P) * ROLLOFF
    width = math.ceil(WIDTH * O / base)
    idx = torch.arange(-width, width + O, dtype=torch.float64)[None] / O
    raw = (torch.arange(0, -P, -1, dtype=torch.float64)[:, None] / P + idx) * base
    t = raw.clamp(-WIDTH, WIDTH)
    window = torch.cos(t * math.pi / WIDTH / 2) ** 2
    t = t * math.pi
    k = torch.where(t == 0, torch.tensor(1.0, dtype=torch.float64), t.sin() / t) * window * (base / O)
    return k.to(dtype), raw, width


def out_length(L, orig, new):
    O, P = ratio(orig, new)
    return -(-(P * L) // O)


def _apply(x, k, width, O, L_out):
    """rows x (R, L) through the dense kernel k (P, taps) of the dtype of x."""
    xp = torch.nn.functional.pad(x, (width, width + O))
    y = torch.nn.functional.conv1d(xp[:, None], k[:, None], stride=O)              # (R, P, Q)
    return y.transpose(1, 2).reshape(x.shape[0], -1)[:, :L_out]


def resample(waveform, orig, new, lengths=None, dtype=torch.float64):
    """The contract of lcasr_amd.utils.audio_tools.resample on the CPU: (L,) -> (L',), (R, L) -> (R, L'), L' = ceil(new L / orig); with
    lengths every row is computed from its own samples alone and is 0 behind its own ceil(new lengths[b] / orig)."""
    if orig == new:
        return waveform
    wave = waveform[None] if waveform.dim() == 1 else waveform
    k, _, width = kernel(orig, new, dtype)
    O, P = ratio(orig, new)
    R, L = wave.shape
    out = torch.zeros(R, out_length(L, orig, new), dtype=dtype)
    for b in range(R):
        n = L if lengths is None else int(lengths[b])
        if n > 0:
            out[b, :out_length(n, orig, new)] = _apply(wave[b:b + 1, :n].to(dtype), k, width, O, out_length(n, orig, new))[0]
    return out[0] if waveform.dim() == 1 else out


def compact(orig, new):
    """The f32 kernel as (taps (P, K), first (P), K) by loops over its phases: the taps with |t| < 6, from dense index first[p] + width
    on.  Asserts what the compact form relies on: the other taps are exactly 0 in f32 and the live ones are consecutive."""
    k, raw, width = kernel(orig, new, torch.float32)
    rows, first = [], []
    for p in range(k.shape[0]):
        live = (raw[p].abs() < WIDTH).nonzero().flatten().tolist()
        assert live and live == list(range(live[0], live[-1] + 1)), (orig, new, p)
        assert not bool(k[p, :live[0]].any()) and not bool(k[p, live[-1] + 1:].any()), (orig, new, p)
        rows.append(k[p, live[0]:live[-1] + 1])
        first.append(live[0] - width)
    K = max(len(r) for r in rows)
    taps = torch.zeros(len(rows), K)
    for p, r in enumerate(rows): taps[p, :len(r)] = r
    return taps, torch.tensor(first, dtype=torch.int32), K


def bound(waveform, orig, new, lengths=None, channels=0):
    """Per-sample bound of |y_f32 - y_f64| for an output summed in f32 from f32 taps: (K + C + 2) 2^-24 sum_k |h[p][k]| |x[..]|.
    A K-term f32 sum of products in any order, with or without fused multiply-adds, is within (K + 1) u sum |h x| of the exact sum
    (u = 2^-24; K - 1 additions and one product rounding per term, to first order, rounded up by the spare unit); the cast of a tap
    to f32 adds one more u, and a mean of C channels C more (C - 1 additions and the division), relative to the mean of |x_c|, which
    the caller passes as `waveform` then.  channels = 0: no mean.  Derived, not tuned.
    The cast of a CLAMPED tap is no rounding but an underflow: below 2e-49 in f64, exactly 0 in f32.  The f64 yardstick keeps those
    taps, so their whole products, sum over clamped k of |h[p][k]| |x[..]| <= 2e-49 sum |x|, are added: it matters only where every
    live tap of an output lies on exact zeros and a clamped one on a sample (the outputs just before a signal that follows silence)."""
    wave = (waveform[None] if waveform.dim() == 1 else waveform).double().abs()
    K = compact(orig, new)[2]
    k64, raw, width = kernel(orig, new)
    k64 = k64.abs() * ((K + channels + 2) * 2.0 ** -24) + k64.abs() * (raw.abs() >= WIDTH)
    O, P = ratio(orig, new)
    R, L = wave.shape
    out = torch.zeros(R, out_length(L, orig, new), dtype=torch.float64)
    for b in range(R):
        n = L if lengths is None else int(lengths[b])
        if n > 0:
            out[b, :out_length(n, orig, new)] = _apply(wave[b:b + 1, :n], k64, width, O, out_length(n, orig, new))[0]
    return out[0] if waveform.dim() == 1 else out


def test_signal(L, sr, seed=0):
    """0.3 sin(2 pi 440 t) + 0.05 randn (1 + sin(2 pi 1.3 t)) at `sr` Hz, f32: the signal of audio_refs at any rate."""
    t = torch.arange(L, dtype=torch.float64) / sr
    n = torch.randn(L, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    return (0.3 * torch.sin(2 * math.pi * 440 * t) + 0.05 * n * (1 + torch.sin(2 * math.pi * 1.3 * t))).float()


def rows_from_table(x, lengths, taps, first, O, P, dtype=torch.float64):
    """include/sconf_resample.h restated from the compact table: y[q P + p] = sum_k taps[p][k] x[q O + first[p] + k], x (R, L), zero
    outside a row's length; 0 behind ceil(P len / O).  By a dense kernel rebuilt from the table."""
    R, L = x.shape
    K = taps.shape[1]
    left = max(0, -int(first.min()))
    D = int(first.max()) + left + K
    dense = torch.zeros(P, D, dtype=dtype)
    for p in range(P): dense[p, int(first[p]) + left:int(first[p]) + left + K] = taps[p].to(dtype)
    L_out = -(-(P * L) // O)
    out = torch.zeros(R, L_out, dtype=dtype)
    for b in range(R):
        n = L if lengths is None else max(0, min(L, int(lengths[b])))
        if n > 0:
            n_out = -(-(P * n) // O)
            xp = torch.nn.functional.pad(x[b:b + 1, :n].to(dtype), (left, D + O))
            y = torch.nn.functional.conv1d(xp[:, None], dense[:, None], stride=O).transpose(1, 2).reshape(-1)
            out[b, :n_out] = y[:n_out]
    return out


def resample_rows(wave, lengths, taps, first, O, P, mix=False):
    """lcasr_amd.hip.resample.resample_rows on the CPU, in f32 (the emulated binding of the host-logic tests)."""
    assert wave.dtype == torch.float32 and wave.dim() in (2, 3) and tuple(first.shape) == (P,) and taps.shape[0] == P
    if wave.dim() == 3:
        wave = wave.mean(1) if mix else wave[:, 0]
    return rows_from_table(wave, lengths, taps, first, O, P, dtype=torch.float32)
