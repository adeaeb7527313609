/* sconf_resample.h — C ABI of the resampler of libsconf_hip.so: a waveform at any rate -> the 16 kHz (or any other) waveform of the
 * audio front end, on the MI355X (gfx950).
 *
 * A ninth ABI unit beside sconf.h, with the same conventions: plain DEVICE pointers + sizes, caller-owned buffers borrowed for the
 * enqueued work, kernels enqueued on `stream` without synchronising, allocating or freeing; launchers return 0 on success and
 * non-zero with a message in sconf_last_error().
 *
 * Replaces the resample step of lcasr/utils/audio_tools.py:22-23, 67-72 = torchaudio.transforms.Resample(orig, new) with its
 * defaults (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99): a polyphase windowed-sinc filter.  With g = gcd(orig, new),
 * O = orig / g and P = new / g, output j = q P + p of a row x of len samples is
 *     y[j] = sum_{k = 0 .. K-1} taps[p][k] * x[q O + first[p] + k],      x[i] = 0 outside 0 <= i < len,
 * for j < ceil(P len / O).  The caller supplies the filter as a compact table: taps (P, K) f32, the K consecutive taps of phase p
 * that can be non-zero (shorter phases padded with 0), and first (P) int32, the position of tap 0 of phase p relative to sample
 * q O (negative at the head of the filter).  utils/audio_tools.py builds the table of the reference's kernel in f64 and casts it.
 * The sum runs over k in ascending order in f32 with fused multiply-adds: the same bits on every call, and for a row of a batch
 * the bits of the same row processed alone.
 */
#ifndef SCONF_RESAMPLE_H
#define SCONF_RESAMPLE_H
#include <stdint.h>
#include "sconf.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Outputs one workgroup of sconf_resample_rows produces at a time: the tile of the kernel. */
int sconf_resample_tile(void);
/* The largest P * K sconf_resample_rows takes: the table is kept in LDS.  A larger one is refused. */
int sconf_resample_max_table(void);
/* ceil(P L / O), the samples L samples become, in 64-bit integers; -1 for L < 0, O < 1, P < 1 or a product past int64. */
int64_t sconf_resample_out_length(int64_t L, int64_t O, int64_t P);
/* out (B, L_out) f32, row stride out_stride >= L_out elements: out[b] = the resampling of row b of wave, as defined above, with
 * L_out == sconf_resample_out_length(L, O, P).
 * wave: f32; sample i of channel c of row b is wave[b * row_stride + c * chan_stride + i], i < L.  mix == 0: the row is its channel
 * 0 and nothing of the other channels is read (chan_stride is not used); mix == 1: the row is the f32 mean of its `channels`
 * channels, added in channel order and divided by `channels`, taken while the samples are staged (no mono copy is written).
 * 1 <= channels <= 64.
 * lengths (B) int64 or NULL: row b holds lengths[b] <= L samples (clamped into 0..L) and is processed as if it were alone - nothing
 * at or beyond its length is read, outputs behind its own ceil(P lengths[b] / O) are written as 0.
 * taps (P, K) f32 contiguous, first (P) int32, 1 <= K, P * K <= sconf_resample_max_table().  The kernel stages the span of a tile
 * in LDS; it is sized for tables whose q O + first[p] does not decrease with j and advances by at most ceil(O / P) per output, as
 * the reference's does.  Outputs whose taps fall outside the staged span are summed from memory instead, in the same order: any
 * table gives the defined result.  O, P and K for which table and span do not fit 160 KiB of LDS are refused.
 * Every element of out (B rows of L_out) is written, nothing else is; no workspace.  All positions are 64-bit: L, L_out and the
 * row offsets may exceed 2^31.  B * ceil(L_out / tile) must stay below 2^31. */
int sconf_resample_rows(const float* wave, int64_t chan_stride, int64_t row_stride, int channels, int mix, const int64_t* lengths,
                        int64_t L, const float* taps, const int32_t* first, int64_t O, int64_t P, int64_t K, float* out,
                        int64_t out_stride, int64_t L_out, int64_t B, sconf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SCONF_RESAMPLE_H */
