/* sconf_post.h — C ABI of the posterior unit of libsconf_hip.so: the exact CTC likelihood of every string at edit distance 1 from a
 * hypothesis, as log-likelihood ratios against the hypothesis itself, and the token and gap posteriors that follow from them, on the
 * MI355X (gfx950).
 *
 * A sixteenth ABI unit beside sconf.h, with the same conventions: plain DEVICE pointers + sizes, caller-owned buffers borrowed for the
 * enqueued work, kernels enqueued on `stream` without synchronising, allocating or freeing; launchers return 0 on success and
 * non-zero with a message in sconf_last_error().  Nothing is read back to the host.  A refused call launches nothing.
 *
 * THE QUANTITIES.  lp (T, C) log-scores per frame (natural logs), b the blank, y[0..L) labels other than b.  Lattice states 0..2L:
 * 2i the blank in front of y_i, 2i + 1 y_i, 2L the last blank.  alpha_t(s) is the CTC forward row; betahat_t(s) the log-probability
 * of frames t..T-1 starting in s at t, the emission at t included (ATen's log_beta); ll = logsumexp(alpha_{T-1}(2L), alpha_{T-1}(2L-1)).
 * alpha_t(s), s <= 2i, depends only on y[0..i), and betahat_t(s), s >= 2i, only on y[i..L): an edited string shares the rows of y in
 * front of and behind the edit, and one chain over a single bridge state joins them.
 *     Bridge(p, q, prev, next, c, last):
 *         a_0 = lp_0(c) if p == 0 else -inf
 *         a_t = lp_t(c) + logsumexp(a_{t-1}, alpha_{t-1}(p), [prev exists and c != prev] alpha_{t-1}(p-1))
 *         result = logsumexp over t < T-1 of a_t + logsumexp(betahat_{t+1}(q), [next exists and c != next] betahat_{t+1}(q+1)),
 *                  and the term a_{T-1} if last
 *     substitute y_i -> c          Bridge(2i, 2i+2, y_{i-1}, y_{i+1}, c, i == L-1)
 *     insert c at gap j (0..L)     Bridge(2j, 2j,   y_{j-1}, y_j,     c, j == L)         gap j lies between y_{j-1} and y_j
 *     delete y_i, i < L-1          logsumexp over t < T-1 of logsumexp(alpha_t(2i), [i > 0 and y_{i-1} != y_{i+1}] alpha_t(2i-1))
 *                                  + betahat_{t+1}(2i+3), and the term betahat_0(3) if i == 0
 *     delete y_{L-1}               logsumexp(alpha_{T-1}(2L-2), [L > 1] alpha_{T-1}(2L-3))
 * With T == 0 every neighbour has probability 0.
 *
 * WHAT IS REPORTED.  Log-likelihood ratios against ll, in f32 (an absolute f32 log-likelihood of magnitude 1e4 would carry 1e-3 of
 * rounding).  sub_llr (B, Smax, C): row i, column c != b is the substitution y_i -> c, column b the DELETION of y_i, so a row is the
 * unnormalised log-distribution of slot i over C distinct strings; column y_i is computed like any other and is 0 to rounding.
 * ins_llr (B, Smax + 1, C): column c != b is the insertion of c at gap j, column b is 0 (nothing inserted).  A ratio does not change
 * when a constant is added to a frame's row, so unnormalised, averaged and temperature-scaled rows are valid input; ll itself means a
 * likelihood for normalised rows only.  A neighbour of probability 0 gives -inf.  Slots at and past target_lengths[b] and gaps past it
 * are NaN.  If ll is not finite every output of the sample is NaN and ll says why: -inf for a y no alignment produces, NaN for a
 * POISONED sample - input_lengths[b] outside [0, N], target_lengths[b] outside [0, Smax], a label outside [0, C) or equal to the
 * blank, or a NaN or +inf among the first C columns of a frame t < input_lengths[b].  A poisoned sample touches nothing of its
 * neighbours in the batch.
 *
 * NUMERICS.  The state of every recursion is f64, in log2 units.  A log-sum-exp takes its maximum and its differences in f64 and its
 * exponentials (v_exp_f32), their sum and its logarithm (v_log_f32) in f32: with both instructions accurate to 1 ulp, the largest
 * term exactly 1 and the sum in [1, 3], one log-sum-exp is off by at most 2.9 * 2^-23 nats whatever the magnitude of its arguments.
 * A reported log-likelihood passes through at most one log-sum-exp per frame on its way through the rows (alpha in front of the
 * bridge frame, betahat behind it) and one more per frame in the running sum over the bridge frames: 2 * 2.9 * 2^-23 per frame, stated
 * as 6 * 2^-23 nats; sconf_post_step_error() returns this constant.  Against the float64 evaluation of the definitions above on the
 * same f32 input:
 *     every log-likelihood (ll, and ll + llr before its rounding)   E(T) = (T + 1) * step_error
 *     every finite llr                                              2 E(T) + 2^-22 * max(1, |llr|)
 *     every posterior                                               4 E(T) + 2^-22, absolute
 * Results are bit-reproducible: every sum has a fixed order.
 */
#ifndef SCONF_POST_H
#define SCONF_POST_H
#include <stdint.h>
#include "sconf.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The largest Smax (4095): two f64 lattice rows of 2 Smax + 1 states are held in the LDS. */
int sconf_post_max_labels(void);
/* The bytes of the workspace of a batch: the alpha rows and the betahat rows, f64 (B, N, 2 Smax + 1) each, 16 B N (2 Smax + 1) in
 * all; -1 where a size is negative, Smax exceeds sconf_post_max_labels() or the figure passes 2^62. */
int64_t sconf_post_workspace(int64_t B, int64_t N, int64_t Smax);
/* *nats = the per-frame error constant of NUMERICS (6 * 2^-23), on the host; returns 0.  (Through a pointer: the entry points of
 * this library return int, int64_t or a string.) */
int sconf_post_step_error(double* nats);

/* Common to the two launchers below, laid out as for sconf_ctc_fwd:
 *   log_probs (B, N, row_stride) f32, row_stride >= C: only the first C columns of a row are read
 *   targets (B, Smax) int32; input_lengths, target_lengths (B) int32
 *   workspace: sconf_post_workspace(B, N, Smax) bytes, 16-byte aligned; workspace_bytes: what the caller has there
 *   loglik (B) f64: ll in nats
 * 2 <= C < 2^30, 0 <= blank < C, 0 <= Smax <= sconf_post_max_labels(), B and N below 2^31, B N row_stride below 2^62. */

/* Fills the workspace with the alpha and betahat rows of every sample (rows t < input_lengths[b], states s <= 2 target_lengths[b];
 * the rest of the workspace is not written) and writes loglik, every element.  One workgroup per (sample, direction), the row in the
 * LDS in f64, one barrier per frame. */
int sconf_post_lattice(const float* log_probs, const int32_t* targets, const int32_t* input_lengths, const int32_t* target_lengths,
                       int64_t B, int64_t N, int64_t C, int64_t row_stride, int64_t Smax, int blank, void* workspace,
                       int64_t workspace_bytes, double* loglik, sconf_stream_t stream);

/* sub_llr (B, Smax, C) and ins_llr (B, Smax + 1, C) f32 from the rows sconf_post_lattice left in the workspace and its loglik, both
 * read only; the other arguments are those of that call.  One lane per (slot or gap, class): a wave runs the chains of 64 consecutive
 * classes of one slot, frames at which the bridge state cannot be reached or the string no longer finished are skipped (they add
 * exactly 0), and the deletion of a slot is summed by the wave that owns column `blank`.  Every element of sub_llr and ins_llr is
 * written, nothing else. */
int sconf_post_neighbours(const float* log_probs, const int32_t* targets, const int32_t* input_lengths, const int32_t* target_lengths,
                          int64_t B, int64_t N, int64_t C, int64_t row_stride, int64_t Smax, int blank, const void* workspace,
                          int64_t workspace_bytes, const double* loglik, float* sub_llr, float* ins_llr, sconf_stream_t stream);

/* The summary of every row of sub_llr and ins_llr, one wave per row:
 *   post (B, Smax) f32          softmax(row i of sub_llr)[y_i]: the posterior of the decoded token among its alternatives
 *   alt (B, Smax) int32         the column other than y_i with the largest llr, the first on ties; `blank` means "delete"
 *   alt_post (B, Smax) f32      its softmax
 *   gap_post, gap_alt, gap_alt_post (B, Smax + 1): the same of row j of ins_llr with column `blank` (nothing inserted) in y_i's place
 * A row that holds a NaN (a padded slot or gap, a sample whose ll is not finite) gives NaN, -1, NaN.  The maximum is taken in f32,
 * the exponentials and their sum in f64 in a fixed order.  Every element of the six outputs is written, nothing else. */
int sconf_post_slots(const float* sub_llr, const float* ins_llr, const int32_t* targets, int64_t B, int64_t C, int64_t Smax, int blank,
                     float* post, int32_t* alt, float* alt_post, float* gap_post, int32_t* gap_alt, float* gap_alt_post,
                     sconf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SCONF_POST_H */
