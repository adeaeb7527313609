/* sconf_ctxattr.h — C ABI of CONTEXT ATTRIBUTION in libsconf_hip.so on the MI355X (gfx950): the masked-window error-rate matrix of
 * the reference's eval/bin/run_context_attribution.py, without its square.  Entry (i, j) of that matrix is the error count of the
 * transcript whose frames of window i come from a forward with window j of the spectrogram replaced by its mean.
 *
 * A seventh ABI unit beside sconf.h, sconf_audio.h, sconf_align.h, sconf_beam.h, sconf_lm.h and sconf_align_long.h, with their
 * conventions: plain DEVICE pointers + sizes (one HOST array, named as such below), caller-owned buffers borrowed for the enqueued
 * work, kernels enqueued on `stream` without synchronising, allocating, freeing or reading device memory on the host (graph-capture
 * safe); launchers return 0 on success and non-zero with a message in sconf_last_error().  Invalid sizes are refused on the host and
 * nothing is launched.
 *
 * THE IDENTITY.  Labels are per-frame class indices (>= 0), as sconf_argmax_rows writes them.  Let a0 = clean (N), aj = masked[j]
 * (N), window i = frames [f, g) and ge = min(g + 1, N).  The labels of pair (i, j) are a0 with aj[f:g] spliced in (the reference
 * splices the log-probs and takes the argmax, lines 110-114: the same labels), and the hypothesis is their CTC collapse: the label of
 * frame t is emitted when it is not `blank` and t = 0 or it differs from the label of frame t - 1.  It is  pre_i ++ mid_ij ++ suf_i:
 *   pre_i    the clean tokens emitted at frames < f
 *   mid_ij   the tokens the spliced labels emit at frames [f, ge): frame g belongs to the middle because whether it emits depends on
 *            aj[g - 1]
 *   suf_i    the clean tokens emitted at frames >= ge, the same for every j.
 * With F_i[k] = distance(pre_i, ref[:k]), B_i[k] = distance(suf_i, ref[k:]) and M = F_i advanced by the tokens of mid_ij, the unit-cost
 * Levenshtein distance of pair (i, j) is exactly  min_k M[k] + B_i[k]  (every alignment cuts the reference somewhere behind the
 * middle).  The reference pays one full-length distance per pair (line 116); here the two boundary rows of every window come from
 * two DPs over the clean hypothesis and a pair costs |mid_ij| rows.  An empty window (f = g) scores as the clean hypothesis.
 *
 * GEOMETRY.  A DP row has R + 1 cells.  It lives in the registers of one workgroup of sconf_ctxattr_threads(R) threads, each holding
 * sconf_ctxattr_cells_per_thread(R) adjacent cells: 64 .. 1024 threads (a power of two) of 1 cell up to R + 1 = 1024, then 1024
 * threads of 2, 4, .. 64 cells.  One row is a min-plus prefix scan, with V[k] = D[k] - k:
 *   U[k] = min(V[k] + 1, V[k-1] - (ref[k-1] == x)),  U[0] = V[0] + 1,  V'[k] = min over k' <= k of U[k']
 * done as a serial scan of the thread's cells, a prefix-min over the lanes of a wave and at most 16 wave partials through LDS, which
 * are double-buffered by row parity: one barrier per row.  Cells are 32-bit (a distance is at most H + R).
 */
#ifndef SCONF_CTXATTR_H
#define SCONF_CTXATTR_H
#include <stdint.h>
#include "sconf.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The largest R accepted: 65535 reference ids, the bound of sconf_align_long.h. */
int sconf_ctxattr_max_ref(void);
/* The largest g - f + 1 of a frame window: 8192 (the collapsed middle is held in LDS, 4 bytes per frame). */
int sconf_ctxattr_max_window_frames(void);
/* Launch geometry of the DP kernels for a reference of R ids (see GEOMETRY); -1 for R outside 0 .. sconf_ctxattr_max_ref().
 * threads * cells_per_thread >= R + 1, and both are non-decreasing in R. */
int sconf_ctxattr_threads(int64_t R);
int sconf_ctxattr_cells_per_thread(int64_t R);
/* Bytes of workspace of sconf_ctxattr_score, -1 for invalid sizes (N < 1, I outside 1 .. 65535, J < 1, N J >= 2^31, R outside 0 ..
 * sconf_ctxattr_max_ref()).  With P = threads * cells_per_thread, four parts, each rounded up to 256 bytes:
 *   the windows and their two orders      16 I bytes
 *   the reference, padded, both ways      8 P bytes
 *   the forward boundary rows F_i         4 I P bytes
 *   the backward boundary rows B_i        4 I P bytes
 * At N = 45000, I = J = 176, R = 13000 (P = 16384): 2816 + 131 072 + 2 x 11 534 336 = 23 202 560 bytes. */
int64_t sconf_ctxattr_score_workspace(int64_t N, int64_t I, int64_t J, int64_t R);

/* means[j] = the mean of spec[:, s:e] over all F (e - s) elements, (s, e) = windows[j] clamped to 0 <= s, e <= T; an empty window
 * gives 0.  Accumulated in f64 in a fixed order and rounded once to f32, the same bits on every call.  Replaces
 * audio_spec[:, :, mask_start:mask_end].mean() of the reference (line 107), which sums in f32: the two can differ in the last bit.
 * spec (F, T) f32, windows (J, 2) int32 ON THE DEVICE, means (J) f32.  One workgroup per window.  J = 0 returns 0 and launches
 * nothing. */
int sconf_ctxattr_window_means(const float* spec, const int32_t* windows, float* means, int64_t F, int64_t T, int64_t J,
                               sconf_stream_t stream);
/* dst[k] = spec with the frames of window j0 + k set to means[j0 + k], bit-equal to spec elsewhere, for k < b: one launch builds a
 * whole model batch.  Replaces the reference's clone and slice assignment per pair (lines 106-108).  dst (b, F, T) f32; windows and
 * means as above; 0 <= j0, 1 <= b, j0 + b <= J, b F <= 65535.  b = 0 returns 0 and launches nothing. */
int sconf_ctxattr_mask_fill(const float* spec, const int32_t* windows, const float* means, float* dst, int64_t F, int64_t T, int64_t J,
                            int64_t j0, int64_t b, sconf_stream_t stream);
/* The error counts of all I x J pairs (see THE IDENTITY).  Replaces lines 102-123 of the reference less the forwards and the text.
 *   clean (N) int32, masked (J, N) int32, ref (R) int32 (may be NULL when R = 0): device.
 *   frame_windows (I, 2) int32: a HOST array of (f, g) with 0 <= f <= g <= N and g - f + 1 <= sconf_ctxattr_max_window_frames(),
 *       read during the call (not borrowed) and carried to the device as kernel arguments.  In any order; may overlap.
 *   errors (I, J) int32: the Levenshtein distance of pair (i, j) against ref.
 *   clean_errors (1) int32, clean_len (1) int32: the distance and the length H of the clean hypothesis.
 *   mid_len (I, J) int32: |mid_ij|.
 *   mid_tokens (I, J, mid_cap) int32 or NULL: mid_ij, elements past mid_len written as 0.  mid_cap must be at least the largest
 *       min(g + 1, N) - f (and at least 1); ignored when mid_tokens is NULL.
 * Every element of the outputs is written by every call, from the inputs alone; the workspace content is unspecified before and
 * after.  workspace_bytes must be at least sconf_ctxattr_score_workspace(N, I, J, R).
 * Launches: one per 224 windows that plants the windows (and, the first, the padded reference) in the workspace; then
 *   1. the boundary rows: two workgroups, the forward DP over the clean hypothesis and the backward DP over both sequences reversed,
 *      each dumping its row when its frame reaches a window edge; the forward one ends with clean_errors and clean_len;
 *   2. one workgroup per pair: collapses the middle into LDS, loads F_i, advances it by the middle's tokens, reduces
 *      min_k M[k] + B_i[k]. */
int sconf_ctxattr_score(const int32_t* clean, const int32_t* masked, const int32_t* ref, const int32_t* frame_windows, int32_t* errors,
                        int32_t* clean_errors, int32_t* clean_len, int32_t* mid_len, int32_t* mid_tokens, void* workspace,
                        int64_t workspace_bytes, int64_t N, int64_t I, int64_t J, int64_t R, int64_t mid_cap, int blank,
                        sconf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SCONF_CTXATTR_H */
