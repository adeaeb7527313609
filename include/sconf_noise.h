/* sconf_noise.h — C ABI of the noise corruption of libsconf_hip.so: Gaussian noise and a background clip mixed into a 16 kHz waveform
 * at a set signal-to-noise ratio, on the MI355X (gfx950).
 *
 * A tenth ABI unit beside sconf.h, with the same conventions: plain DEVICE pointers + sizes, caller-owned buffers borrowed for the
 * enqueued work, kernels enqueued on `stream` without synchronising, allocating or freeing; launchers return 0 on success and
 * non-zero with a message in sconf_last_error().  All positions and strides are 64-bit.
 *
 * Replaces audiomentations' AddGaussianSNR and AddBackgroundNoise as the reference's noise-robustness drivers use them
 * (eval/rev16_gaussian_noise/run.py, eval/rev16_background_noise/run.py).  For a row x of len samples, P(x) = mean_i x[i]^2:
 *     Gaussian     y[i] = x[i] + sigma z[i],   sigma = sqrt(P(x)) 10^(-snr / 20),  z standard normal
 *     background   y[i] = x[i] + g v[i],       v[i] = n[(off + i) mod nlen],  g = sqrt(P(x) / P(v)) 10^(-snr / 20),
 * P(v) over the len samples used; P(v) < 1e-18 (a silent clip) gives g = 0, and so does P(x) == 0.  Where the factor is 0 the output
 * is x bit for bit.  One call mixes K levels snr[b][0..K-1] of every row from one z (one v): a sweep over the SNR is one launch.
 *
 * THE NORMALS are fixed by contract.  Sample s = first_sample + i of row id = first_row + b is output s & 3 of (z0, z1, z2, z3), made
 * from the four words r0..r3 of Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57, Weyl constants 0x9E3779B9, 0xBB67AE85) with key
 * (seed lo32, seed hi32) and counter (q lo32, q hi32, id lo32, id hi32), q = s >> 2:
 *     z0 = R(r0) cospi(2 U(r1)),  z1 = R(r0) sinpi(2 U(r1)),  z2 = R(r2) cospi(2 U(r3)),  z3 = R(r2) sinpi(2 U(r3)),
 *     R(r) = sqrt(-2 ln(((r >> 9) + 0.5) 2^-23)),  U(r) = (r >> 9) 2^-23,
 * in f32 with the HIP math library's logf, sqrtf and sincospif (no fast-math).  |z| <= sqrt(48 ln 2) = 5.77.  A row of a batch gets
 * the bits it would get alone with first_row = b; a recording in pieces gets the bits of one pass with first_sample = the piece's start.
 */
#ifndef SCONF_NOISE_H
#define SCONF_NOISE_H
#include <stdint.h>
#include "sconf.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Samples one workgroup handles: the tile of all three kernels, and the span of one partial sum of sconf_noise_power. */
int sconf_noise_tile(void);
/* The largest K (levels per row and call) the two mixing launchers take; at least 16. */
int sconf_noise_max_levels(void);
/* Bytes of workspace sconf_noise_power needs for B rows of L samples: one f64 per tile per row.  -1 for B < 0, L < 0 or
 * B * ceil(L / tile) >= 2^31. */
int64_t sconf_noise_workspace(int64_t B, int64_t L);

/* power (B) f64: power[b] = (1 / len_b) sum_{i < len_b} s_b[(off_b + i) mod sl_b]^2, and 0 for len_b == 0 (or sl_b < 1).
 * src: f32, row r at src + r * row_stride, src_rows == B or 1; s_b is row b, or row 0 when src_rows == 1.
 * lengths (B) int64 or NULL (len = L; values clamped into 0..L).  src_lengths (src_rows) int64 or NULL (sl = L).  offsets (B) int64
 * or NULL (0); an offset outside 0..sl-1 is taken mod sl.  With offsets == src_lengths == NULL and src_rows == B this is P(x); with
 * them set it is P(v) of the background mix.
 * Two stages: per tile of sconf_noise_tile() samples an f64 sum of the exact squares in an order that depends on (len, tile) only,
 * written to ws; then the tile sums of a row are added in tile order and divided by len.  No atomics: the same bits on every
 * call, whatever the alignment of src, and for a row of a batch the bits of the row alone.  Nothing at or beyond len_b of a row
 * without offsets, and nothing at or beyond sl_b, is read.  Only power and ws (ws_bytes >= sconf_noise_workspace(B, L)) are written. */
int sconf_noise_power(const float* src, int64_t row_stride, int64_t src_rows, const int64_t* lengths, const int64_t* src_lengths,
                      const int64_t* offsets, int64_t L, int64_t B, double* power, void* ws, int64_t ws_bytes, sconf_stream_t stream);

/* out row b * K + k (at out + (b * K + k) * out_stride, L elements) = fmaf(sigma_bk, z, x) of row b of wave (at wave + b * row_stride),
 * sigma_bk = (float)(sqrt(power[b]) * 10^(-snr_db[b * K + k] / 20)) computed in f64; sigma_bk == 0 (power 0, snr +inf) copies x.
 * power (B) f64 as sconf_noise_power writes it; snr_db (B, K) f32 contiguous; 1 <= K <= sconf_noise_max_levels().
 * lengths (B) int64 or NULL: samples at or beyond len_b are written as 0 and never read.  seed: all 64 bits are the Philox key;
 * first_row >= 0 and first_sample >= 0 place the call in the (row id, sample) plane of the normals, see above.
 * Every element of the B * K rows of L is written, nothing else is; out must not overlap wave; out_stride >= L.  Each group of four
 * samples costs one Philox call, whatever K is.  16-byte loads and stores where wave, out, the strides and first_sample are
 * multiples of four elements, single elements elsewhere: the same bits either way. */
int sconf_noise_add_gaussian(const float* wave, int64_t row_stride, const int64_t* lengths, int64_t L, int64_t B, const double* power,
                             const float* snr_db, int64_t K, int64_t seed, int64_t first_row, int64_t first_sample, float* out,
                             int64_t out_stride, sconf_stream_t stream);

/* The same layout with fmaf(g_bk, v, x): v[i] = n_b[(offsets[b] + i) mod nl_b], n_b row b of noise (at noise + b * noise_stride), or
 * row 0 when noise_rows == 1; noise_rows is 1 or B.  noise_lengths (noise_rows) int64 or NULL (nl = L); offsets (B) int64 or NULL (0),
 * each in 0 .. nl - 1 (anything else is taken mod nl).  g_bk = (float)(sqrt(power[b] / noise_power[b]) * 10^(-snr_db[b * K + k] / 20))
 * in f64, 0 where noise_power[b] < 1e-18, power[b] == 0 or nl_b < 1; noise_power (B) f64 = sconf_noise_power of the clip with these
 * lengths, noise_lengths and offsets.  Nothing at or beyond nl_b of a clip is read. */
int sconf_noise_add_background(const float* wave, int64_t row_stride, const int64_t* lengths, int64_t L, int64_t B, const float* noise,
                               int64_t noise_stride, int64_t noise_rows, const int64_t* noise_lengths, const int64_t* offsets,
                               const double* power, const double* noise_power, const float* snr_db, int64_t K, float* out,
                               int64_t out_stride, sconf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SCONF_NOISE_H */
