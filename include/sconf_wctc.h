/* sconf_wctc.h — C ABI of the WILD-CARD CTC LOSS (W-CTC) in libsconf_hip.so on the MI355X (gfx950): the loss of the reference's
 * lcasr/losses/wctc.py (wctc_loss / WCTCLoss, modes soft, max_prob, sum_prob) and its gradient, for transcripts that do not cover the
 * first and last frames of their audio.  A wild-card lets the alignment start at any frame, and the last lattice row is tracked over
 * all frames so the alignment may stop at any frame.
 *
 * An eighth ABI unit, with the conventions of the others: plain DEVICE pointers + sizes, caller-owned buffers borrowed for the
 * enqueued work, kernels enqueued on `stream` without synchronising, allocating, freeing or reading device memory on the host
 * (graph-capture safe); launchers return 0 on success and non-zero with a message in sconf_last_error().  Invalid sizes, a bad mode,
 * null pointers and a short workspace are refused on the host and nothing is launched.
 *
 * THE FUNCTION (natural-log probabilities; one sample; L labels; T = its input_length).  The lattice is
 * ext = [blank, l_1, blank, l_2, .., l_L, blank], states s = 0 .. 2L, p_t(c) = exp(lp[t, c]):
 *   a_t(s) = p_t(ext_s) ( a_{t-1}(s) + a_{t-1}(s-1) + [s >= 2 and ext_s != ext_{s-2}] a_{t-1}(s-2) + [s <= 1] 1 ),   a_{-1} = 0
 *   E_t    = a_t(2L-1) + a_t(2L),   e_t = ln E_t                  (t = 0 .. T-1)
 *   f      = ln sum_t E_t                     SCONF_WCTC_SUM_PROB
 *          = max_t e_t                        SCONF_WCTC_MAX_PROB
 *          = sum_t pi_t e_t, pi = softmax(e)  SCONF_WCTC_SOFT
 *   nll    = -f
 * The [s <= 1] term is the wild-card.  With w_t = df/de_t  (sum_prob: pi_t; max_prob: one-hot at the FIRST maximum; soft:
 * pi_t (1 + e_t - f)) the gradient is
 *   b_t(s) = [s in {2L-1, 2L}] w_t / E_t + p_{t+1}(ext_s) b_{t+1}(s) + p_{t+1}(ext_{s+1}) b_{t+1}(s+1)
 *            + [ext_{s+2} != ext_s] p_{t+1}(ext_{s+2}) b_{t+1}(s+2),          b_T = 0
 *   d nll / d lp[t, c] = - sum over s with ext_s = c of a_t(s) b_t(s)
 * the plain derivative with respect to lp (what autograd through the reference gives), NOT the exp(lp) - occupancy convention of
 * sconf_ctc_bwd; a class that is not in ext gets 0.  Frames with E_t = 0 (the last label cannot be reached yet) take no part in any
 * mode: pi_t = w_t = 0.  In soft mode w_t is negative wherever e_t < f - 1: the backward carries w = w+ - w- as two non-negative
 * lattices through the same pass.
 *
 * WHERE THIS DEPARTS FROM THE REFERENCE
 *   - input_lengths is honoured: the recursion and the reduction over time stop at input_lengths[b], and the gradient rows from
 *     there on are 0.  The reference ignores it and runs every sample over all N frames; with every input_length == N the two agree.
 *   - An infeasible sample (no frame with E_t > 0: T < labels + repeats, or T = 0) gives nll = +inf and zero gradient rows.  The
 *     reference returns 3.4028e38.
 *   - target_lengths[b] = 0 has no last label to track: the sample is poisoned, as are input_lengths[b] > N, target_lengths[b] >
 *     Smax and a label outside [0, C) among the first target_lengths[b]: nll = NaN and NaN gradient rows for t < input_lengths[b].
 *     The reference reads its wild-card column as a terminal state for an empty transcript.
 *   - f32 log-probs only.
 * targets beyond target_lengths[b] are never used as labels and may be negative padding.
 *
 * STATE.  As the CTC kernels: the recursion's state is f64 (log2 units) in LDS, its transcendental part f32, one barrier per frame,
 * the emissions gathered once into contiguous rows and prefetched.  The a rows are stored in f64 too, not as the CTC kernels store
 * theirs (f32 relative to an f64 offset per frame): the wild-card keeps the first states of every row at O(1) while the states the
 * gradient lives on lie thousands of nats below, where an f32 relative to any per-frame offset resolves 2.4e-4 .. 4.9e-4.  The
 * reduction over t is accumulated in f64 in a fixed order: the same inputs give the same bits on every call.
 */
#ifndef SCONF_WCTC_H
#define SCONF_WCTC_H
#include <stdint.h>
#include "sconf.h"
#ifdef __cplusplus
extern "C" {
#endif

enum { SCONF_WCTC_SOFT = 0, SCONF_WCTC_MAX_PROB = 1, SCONF_WCTC_SUM_PROB = 2 };

/* The largest Smax accepted: 2552 labels.  Two f64 lattices (w+ and w-) of two rows of 2 Smax + 1 states fill the 160 KB of LDS. */
int sconf_wctc_max_labels(void);
/* Bytes of workspace shared by sconf_wctc_fwd and sconf_wctc_bwd, -1 for invalid sizes (B < 1, N < 1, Smax outside 1 ..
 * sconf_wctc_max_labels(), mode not one of the three).  With W = 2 Smax + 1 and K = 2 in soft mode, else 1, seven parts, each
 * rounded up to 256 bytes:
 *   the gathered emissions           f32 [B][N][W]     lp[b, t, ext_s]
 *   the a rows                       f64 [B][N][W]     log2 a_t(s), -1e300 where a_t(s) = 0
 *   the products a_t(s) b_t(s)       f32 [B][N][W]     written by the backward
 *   e_t                              f64 [B][N]        -inf where E_t = 0
 *   w_t                              f64 [B][N]
 *   the sinks log2(w_t / E_t)        f64 [K][B][N]     of w+ and, in soft mode, of w-
 *   f                                f64 [B]           -inf for an infeasible sample, NaN for a poisoned one
 * Elements at frames >= input_lengths[b] or states >= 2 target_lengths[b] + 1 are unspecified. */
int64_t sconf_wctc_workspace(int64_t B, int64_t N, int64_t Smax, int mode);

/* nll[b] = -f of sample b.  log_probs (B, N, C) f32 batch-major with C % 4 == 0 and C <= 16384; targets (B, Smax) int32;
 * input_lengths, target_lengths (B) int32; nll (B) f32; 0 <= blank < C.  Writes nll and the workspace (all parts but the
 * products).  Two launches: the emission gather (one workgroup per frame), then one workgroup per sample that runs the a lattice
 * over time, reduces over t and writes w_t. */
int sconf_wctc_fwd(const float* log_probs, const int32_t* targets, const int32_t* input_lengths, const int32_t* target_lengths,
                   float* nll, void* workspace, int64_t workspace_bytes, int64_t B, int64_t N, int64_t C, int64_t Smax, int blank,
                   int mode, sconf_stream_t stream);
/* grad (B, N, C) f32 = grad_out[b] * d nll[b] / d log_probs (grad_out (B) f32, NULL = 1).  Every element is written: zeros for t >=
 * input_lengths[b] and for infeasible samples.  The workspace must be the one a sconf_wctc_fwd call with the same arguments filled;
 * the call writes its products part and leaves the rest as it is (it may be called again).  Two launches: one workgroup per sample
 * that runs the b lattice(s) backwards over time and stores a_t(s) b_t(s), then one workgroup per frame that sums the products by
 * class, every sum in a fixed order. */
int sconf_wctc_bwd(const int32_t* targets, const int32_t* input_lengths, const int32_t* target_lengths, const float* grad_out,
                   float* grad, void* workspace, int64_t workspace_bytes, int64_t B, int64_t N, int64_t C, int64_t Smax, int blank,
                   int mode, sconf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SCONF_WCTC_H */
