"""numpy / torch float64 restatement of the noise corruption (include/sconf_noise.h, lcasr_amd.utils.audio_tools.wave_power,
add_gaussian_snr, add_background_noise): Philox4x32-10, the contract's normals, the mean square through exact_sums.checksums, both
mixes, and the per-sample bounds the GPU tests hold the kernels to.  TEST INFRASTRUCTURE, plain module.

The bounds, with u = 2^-24 (derived, not tuned):
  power       |got - exact| <= len 2^-53 exact + 2^-52 exact: the squares are exact in f64, every one of at most len - 1 additions of
              non-negative terms rounds by at most 2^-53 of the final sum, and the division by len and the spare unit make up the rest.
  gaussian    |got - y64| <= u (|y64| + 10 sigma r), r = sqrt(-2 ln u0) of that sample in f64.  The uniforms and 2 U are exact; logf,
              sqrtf and sincospif are documented to at most 2 ulp each, and |cospi|, |sinpi| <= 1, so the f32 normal is off by a
              multiple of u r: half of log's relative error (it passes through the square root), the square root's own, one
              product, and sincospi's against a factor of at most 1.  The f32 rounding of sigma adds u sigma r and the final fma
              u |y|.  The 10 covers these at the documented accuracies; the GPU tests print max err / bound, and a ratio above 1
              is a finding about one of the three functions or the code, not a reason to widen it.
  background  |got - y64| <= u |y64| + 2 u |g v|: the rounding of g to f32 (and of the f64 power behind it, far below) on the product,
              one rounding of the fma.
"""
import math

import numpy as np
import torch

from exact_sums import checksums

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
U24 = 2.0 ** -24
SILENT = 1e-18                                  # mean square below which a clip counts as silent (rms 1e-9)


def philox4x32_10(counter, key):
    """counter (n, 4) and key (2,) or (n, 2) of integers below 2^32 -> (n, 4) uint32: Philox4x32 with 10 rounds, as Random123."""
    c = [np.asarray(counter, dtype=np.uint64)[:, i].copy() for i in range(4)]
    key = np.broadcast_to(np.asarray(key, dtype=np.uint64), (c[0].shape[0], 2))
    k0, k1 = key[:, 0].copy(), key[:, 1].copy()
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]            # 32 x 32 -> 64 bits: exact in uint64
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & mask, p1 & mask, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & mask, p0 & mask]
        k0, k1 = (k0 + np.uint64(W0)) & mask, (k1 + np.uint64(W1)) & mask
    return np.stack(c, 1).astype(np.uint32)


def normals(seed, row_id, first_sample, n):
    """(z, r): the n standard normals of samples first_sample .. first_sample + n - 1 of row `row_id` under `seed`, in f64, and the
    radius r = sqrt(-2 ln u0) each was made from."""
    seed, row_id = int(seed) & (2 ** 64 - 1), int(row_id)
    q0, q1 = first_sample >> 2, (first_sample + n - 1) >> 2
    q = np.arange(q0, q1 + 1, dtype=np.uint64)
    lo, hi = np.uint64(0xFFFFFFFF), np.uint64(32)
    ctr = np.stack([q & lo, q >> hi, np.full_like(q, row_id & 0xFFFFFFFF), np.full_like(q, row_id >> 32)], 1)
    w = (philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)) >> np.uint32(9)).astype(np.float64)        # (quads, 4)
    rad = np.sqrt(-2.0 * np.log((w[:, 0::2] + 0.5) * 2.0 ** -23))      # (quads, 2): R(r0), R(r2)
    ang = math.pi * (w[:, 1::2] * 2.0 ** -22)                          # pi * 2 U
    z = np.stack([rad * np.cos(ang), rad * np.sin(ang)], 2).reshape(-1)                                  # z0 z1 z2 z3 per quad
    r = np.repeat(rad, 2, axis=1).reshape(-1)
    a = first_sample - 4 * q0
    return torch.from_numpy(z[a:a + n].copy()), torch.from_numpy(r[a:a + n].copy())


def _len(lengths, b, L):
    return L if lengths is None else max(0, min(L, int(lengths[b])))


def stretch(src, b, n, src_lengths=None, offsets=None):
    """The n samples s_b[(off_b + i) mod sl_b] of include/sconf_noise.h: row b of src (row 0 where it has one row)."""
    r = 0 if src.shape[0] == 1 else b
    sl = src.shape[1] if src_lengths is None else int(src_lengths[r])
    off = 0 if offsets is None else int(offsets[b])
    return src[r, (off + torch.arange(n)) % sl]


def power(src, lengths=None, src_lengths=None, offsets=None, L=None, B=None):
    """(B,) f64: the mean square, exact up to the final rounding (exact_sums.checksums adds with math.fsum)."""
    B, L = src.shape[0] if B is None else B, src.shape[1] if L is None else L
    out = torch.zeros(B, dtype=torch.float64)
    for b in range(B):
        n = _len(lengths, b, L)
        if n > 0:
            out[b] = float(checksums(stretch(src, b, n, src_lengths, offsets))[1]) / n
    return out


def power_bound(exact, lengths, L):
    n = torch.tensor([_len(lengths, b, L) for b in range(exact.shape[0])], dtype=torch.float64)
    return n * 2.0 ** -53 * exact + 2.0 ** -52 * exact


def _levels(snr_db, B):
    s = torch.as_tensor(snr_db, dtype=torch.float64)
    s = s.reshape(1, 1) if s.dim() == 0 else s[None] if s.dim() == 1 else s
    return s.expand(B, -1)


def gaussian(x, snr_db, lengths=None, seed=17925, first_row=0, first_sample=0):
    """(y (B, K, L) f64, bound (B, K, L), sigma (B, K)) of add_gaussian_snr on rows x (B, L); snr_db a number, K numbers or (B, K)."""
    B, L = x.shape
    snr = _levels(snr_db, B)
    sigma = power(x, lengths).sqrt()[:, None] * 10.0 ** (-snr / 20.0)
    y, bd = torch.zeros(B, snr.shape[1], L, dtype=torch.float64), torch.zeros(B, snr.shape[1], L, dtype=torch.float64)
    for b in range(B):
        n = _len(lengths, b, L)
        z, r = normals(seed, first_row + b, first_sample, n)
        y[b, :, :n] = x[b, :n].double()[None] + sigma[b, :, None] * z[None]
        bd[b, :, :n] = U24 * (y[b, :, :n].abs() + 10.0 * sigma[b, :, None] * r[None])
    return y, bd, sigma


def background(x, noise, snr_db, lengths=None, noise_lengths=None, offsets=None):
    """(y (B, K, L) f64, bound, g (B, K)) of add_background_noise on rows x (B, L) with clips noise (1 or B, NL)."""
    B, L = x.shape
    snr = _levels(snr_db, B)
    px, pv = power(x, lengths), power(noise, lengths, noise_lengths, offsets, L=L, B=B)
    g = torch.where((pv >= SILENT) & (px > 0), (px / pv.clamp(min=1e-300)).sqrt(), torch.zeros(()).double())[:, None] * 10.0 ** (-snr / 20.0)
    y, bd = torch.zeros(B, snr.shape[1], L, dtype=torch.float64), torch.zeros(B, snr.shape[1], L, dtype=torch.float64)
    for b in range(B):
        n = _len(lengths, b, L)
        gv = g[b, :, None] * stretch(noise, b, n, noise_lengths, offsets).double()[None]
        y[b, :, :n] = x[b, :n].double()[None] + gv
        bd[b, :, :n] = U24 * y[b, :, :n].abs() + 2 * U24 * gv.abs()
    return y, bd, g


def test_signal(L, seed=0):
    """0.3 sin(2 pi 440 t) + 0.05 randn (1 + sin(2 pi 1.3 t)) at 16 kHz, f32: the signal of audio_refs."""
    t = torch.arange(L, dtype=torch.float64) / 16000
    n = torch.randn(L, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    return (0.3 * torch.sin(2 * math.pi * 440 * t) + 0.05 * n * (1 + torch.sin(2 * math.pi * 1.3 * t))).float()


# ---- the binding's ops on the CPU, in f32: the emulated kernels of the host-logic tests and of the footprint harness ---------------
def op_power(src, lengths=None, src_lengths=None, offsets=None, L=None, B=None):
    return power(src, lengths, src_lengths, offsets, L, B)


def op_add_gaussian(wave, lengths, pw, snr_db, seed, first_row=0, first_sample=0):
    B, L = wave.shape
    out = torch.zeros(B, snr_db.shape[1], L)
    for b in range(B):
        n = _len(lengths, b, L)
        z = normals(seed, first_row + b, first_sample, n)[0]
        sigma = (pw[b].double().sqrt() * 10.0 ** (-snr_db[b].double() / 20.0)).float()
        out[b, :, :n] = torch.where(sigma[:, None] == 0, wave[b, :n][None], (wave[b, :n].double()[None] + sigma.double()[:, None] * z.float().double()[None]).float())
    return out


def op_add_background(wave, lengths, noise, noise_lengths, offsets, pw, noise_pw, snr_db):
    B, L = wave.shape
    out = torch.zeros(B, snr_db.shape[1], L)
    for b in range(B):
        n = _len(lengths, b, L)
        ok = bool(noise_pw[b] >= SILENT) and bool(pw[b] > 0)
        g = ((pw[b] / noise_pw[b]).sqrt() * 10.0 ** (-snr_db[b].double() / 20.0)).float() if ok else torch.zeros(snr_db.shape[1])
        v = stretch(noise, b, n, noise_lengths, offsets)
        out[b, :, :n] = torch.where(g[:, None] == 0, wave[b, :n][None], (wave[b, :n].double()[None] + g.double()[:, None] * v.double()[None]).float())
    return out
