/* sconf_audio.h — C ABI of the audio front end of libsconf_hip.so: 16 kHz waveform -> mel spectrogram on the MI355X (gfx950).
 *
 * A second ABI unit beside sconf.h, with the same conventions: plain DEVICE pointers + sizes, caller-owned buffers borrowed for the
 * enqueued work, kernels enqueued on `stream` without synchronising, allocating or freeing; launchers return 0 on success and
 * non-zero with a message in sconf_last_error(); dtype enums as in sconf.h (0 = float32, 1 = bfloat16).
 *
 * Replaces lcasr/utils/audio_tools.py:44-57 to_spectogram = torchaudio.transforms.MelSpectrogram(win_length 400, hop_length 160,
 * n_fft 512, n_mels, normalized False) followed by (spec - spec.mean(-1)) / spec.std(-1).  Fixed at compile time: frames of 512
 * samples every 160, center = True with 256 reflected samples at either end (sample i < 0 reads -i, i >= len reads 2 (len - 1) - i),
 * a periodic Hann window of 400 samples in the middle of the frame, the one-sided power spectrum |X_k|^2, k = 0..256.
 */
#ifndef SCONF_AUDIO_H
#define SCONF_AUDIO_H
#include <stdint.h>
#include "sconf.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Frames one workgroup of sconf_audio_melspec turns into mel values: the time tile of the kernel and of its statistics partials. */
int sconf_audio_tile_frames(void);
/* Bytes of workspace sconf_audio_melspec needs for B rows of T frames: the twiddle and window table, (mean, std) in f64 per
 * (row, mel), and one (n, mean, M2) f64 partial per (row, mel, tile).  -1 for invalid sizes. */
int64_t sconf_audio_melspec_workspace(int64_t B, int64_t T, int64_t n_mels);
/* spec (B, n_mels, T) = mel spectrogram of wave (B rows of L f32 samples, row stride wave_stride elements), T = 1 + L / 160, L > 256.
 * lengths (B) int64 or NULL: row b holds lengths[b] <= L samples and is processed as if it were alone - reflected at its own end,
 * nothing at or beyond lengths[b] is read, statistics over its own 1 + lengths[b] / 160 frames, later frames written as 0 (a row of
 * 256 samples or fewer has no frame).  fb (257, n_mels) f32: the filterbank; ranges (n_mels, 2) int32: the half-open range of bins
 * where column m of fb is not zero (at most 1024 taps in total are used; bins outside [0, 257) are never read).  1 <= n_mels <= 128.
 * normalise != 0: spec = (mel - mean) / std per (row, mel) over the row's own frames, std with divisor frames - 1 (zero variance gives
 * non-finite values, as the reference does); mean and M2 come from per-tile f64 partials merged in a fixed order (Chan): the same
 * bits every call.  spec_dtype SCONF_F32 or SCONF_BF16.  raw: f32 (B, n_mels, T) scratch, needed only for normalise with bf16
 * output (the f32 output is normalised in place), else NULL.  Every element of spec is written; workspace_bytes must be at least
 * sconf_audio_melspec_workspace(B, T, n_mels). */
int sconf_audio_melspec(const float* wave, int64_t wave_stride, const int64_t* lengths, int64_t L, const float* fb,
                        const int32_t* ranges, void* spec, int spec_dtype, float* raw, int normalise, void* workspace,
                        int64_t workspace_bytes, int64_t B, int64_t T, int64_t n_mels, sconf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SCONF_AUDIO_H */
