/* sconf_align.h — C ABI of CTC forced alignment in libsconf_hip.so: the best frame path of a transcript through (B, N, C) log-probs,
 * with token spans, on the MI355X (gfx950).  What torchaudio.functional.forced_align computes, for batches, ragged lengths and
 * lattices of up to 16383 states.
 *
 * A third ABI unit beside sconf.h and sconf_audio.h, with the same conventions: plain DEVICE pointers + sizes, caller-owned buffers
 * borrowed for the enqueued work, kernels enqueued on `stream` without synchronising, allocating, freeing or reading anything on
 * the host (graph-capture safe); launchers return 0 on success and non-zero with a message in sconf_last_error().
 *
 * SEMANTICS.  Sample b has T = input_lengths[b] frames and S = target_lengths[b] labels y_0..y_{S-1} (row b of targets); the
 * lattice has L = 2 S + 1 states, l'[2 j] = blank, l'[2 j + 1] = y_j, and e(t, s) = log_probs[b][t][l'[s]] (f32).  LT is the state
 * type: double where sconf_align_state_bytes(Smax) == 8, float where it is 4.
 *
 *   Recursion   v[0][0] = (LT) e(0, 0),  v[0][1] = (LT) e(0, 1),  every other v[0][s] = -inf;
 *               v[t][s] = max*(v[t-1][s], v[t-1][s-1], v[t-1][s-2] if s is odd and l'[s] != l'[s-2]) + (LT) e(t, s).
 *               The predecessors are compared first and ONE addition in LT follows: this order fixes the bits.  max* takes its
 *               candidates in the order stay, s-1, s-2; a later candidate replaces an earlier one only when it is STRICTLY
 *               greater.  The back-pointer of a cell is the step taken: 0, 1 or 2.
 *   End         among the states (L-1, L-2), in that order, under the same strict rule; state 0 when S = 0.  The back-pointers are
 *               walked from (T-1, end) to frame 0.
 *   path        (B, N) int32: the state per frame; -1 at t >= T.
 *   labels      (B, N) int32: l'[path]; -1 at t >= T (torchaudio's aligned tokens).
 *   spans       (B, Smax, 2) int32: [first frame, one past the last frame) in which state 2 j + 1 is occupied; (-1, -1) for j >= S.
 *   token_logp  (B, Smax) f32: the sum, in frame order, of log_probs[b][t][y_j] over the span of token j; 0 for j >= S.
 *   score       (B) f64: v[T-1][end].
 *   Infeasible  (T = 0, or T < S + the number of adjacent equal labels; detected as score = -inf): score = -inf, path and labels
 *               all -1, spans all -1, token_logp all 0.
 *   Poisoned    as sconf_ctc_fwd defines it (T > N, S < 0 or S > Smax, a label outside [0, C)): score = NaN, the rest as for an
 *               infeasible sample; nothing is indexed with the bad value, and the other samples of the batch are not affected.
 *   Every element of the five outputs is written by every call, from the inputs alone.  The workspace content is unspecified.
 *   Non-finite log-probs give an unspecified path, never an out-of-range one (0 <= path < L, labels from l').
 *
 * GEOMETRY.  One workgroup walks one sample's lattice serially in time; each thread owns sconf_align_states_per_thread(Smax)
 * ADJACENT states of a workgroup of sconf_align_threads(Smax) threads: 256 x 1 up to 127 labels, 512 x 1 up to 255, then 1024
 * threads with 1, 2, 4, 8, 12 and 16 states each up to 511, 1023, 2047, 4095, 6143 and 8191 labels.  Two rows of LT live in the
 * 160 KB LDS: double up to 5112 labels, float above.
 */
#ifndef SCONF_ALIGN_H
#define SCONF_ALIGN_H
#include <stdint.h>
#include "sconf.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The largest Smax accepted: 8191 labels = 16383 states, the limit of sconf_ctc_fwd. */
int sconf_align_max_labels(void);
/* Bytes of one lattice state for targets of up to Smax labels: 8 (double) while two rows fit the LDS, else 4 (float); -1 for
 * Smax < 0 or Smax > sconf_align_max_labels(). */
int sconf_align_state_bytes(int64_t Smax);
/* Launch geometry of the lattice kernel (see GEOMETRY); -1 for an invalid Smax. */
int sconf_align_threads(int64_t Smax);
int sconf_align_states_per_thread(int64_t Smax);
/* Frames whose back-pointers the walk back fetches together (K frames lie in a window of 2 K - 1 cells per row). */
int sconf_align_walk_window(void);
/* Bytes of workspace for B samples of N frames and up to Smax labels, -1 for invalid sizes (B < 1, N < 1, Smax outside
 * 0..sconf_align_max_labels()).  Three parts, each rounded up to 256 bytes:
 *   end state per sample                 4 B bytes
 *   emissions, compact                   4 B N (round8(Smax) + 12) bytes: per frame the Smax label log-probs, then the blank's
 *                                        (every blank state shares one emission, so half of the (N, 2 Smax + 1) lattice is not stored)
 *   back-pointers, ONE BYTE per cell     B N round48(2 Smax + 1) bytes (a thread's adjacent cells leave as one vector store)
 * At B = 1, N = 16384, Smax = 4096: 256 + 269 221 888 + 134 479 872 = 403 702 016 bytes. */
int64_t sconf_align_workspace(int64_t B, int64_t N, int64_t Smax);
/* The alignment (see SEMANTICS).  log_probs (B, N, C) f32 and targets (B, Smax) int32 as sconf_ctc_fwd takes them (C a multiple of
 * 4, at most 16384); input_lengths / target_lengths (B) int32 or NULL (= N / Smax); Smax = 0 is allowed (targets is then never read).
 * Outputs path, labels (B, N) int32, spans (B, Smax, 2) int32, token_logp (B, Smax) f32, score (B) f64; workspace_bytes must be at
 * least sconf_align_workspace(B, N, Smax).  0 <= blank < C.  B = 0 returns 0 and launches nothing. */
int sconf_align_ctc(const float* log_probs, const int32_t* targets, const int32_t* input_lengths, const int32_t* target_lengths,
                    int32_t* path, int32_t* labels, int32_t* spans, float* token_logp, double* score, void* workspace,
                    int64_t workspace_bytes, int64_t B, int64_t N, int64_t C, int64_t Smax, int blank, sconf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SCONF_ALIGN_H */
