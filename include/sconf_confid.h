/* sconf_confid.h — C ABI of the confidence scores of libsconf_hip.so: how sure the model is of each frame, token and word it decoded,
 * on the MI355X (gfx950).
 *
 * A twelfth ABI unit beside sconf.h, with the same conventions: plain DEVICE pointers + sizes, caller-owned buffers borrowed for the
 * enqueued work, kernels enqueued on `stream` without synchronising, allocating or freeing; launchers return 0 on success and
 * non-zero with a message in sconf_last_error().  Nothing is read back to the host.
 *
 * Three entry points that chain: sconf_confid_frames (a confidence and the argmax of every frame), sconf_confid_runs (the greedy CTC
 * collapse of the argmax vector with the frames of every label) and sconf_confid_aggregate (one value per span of frames - or of
 * tokens, for words).
 *
 * THE MEASURES.  A row x of V = classes entries is a vector of unnormalised log-scores (logits, log-probs, the log of averaged
 * posteriors alike): p = softmax(x), an entry of -inf has p = 0 and adds 0 to every sum.  With S_a = sum_c p_c^alpha:
 *
 *     method     entropy H                    H_max                             lin             exp
 *     MAX_PROB   -                            -                                 (V max p - 1) / (V - 1)           refused
 *     SHANNON    -sum p ln p                  ln V                              1 - H / ln V    (V e^-H - 1) / (V - 1)
 *     TSALLIS    (1 - S_a) / (alpha - 1)      (1 - V^(1 - alpha)) / (alpha - 1) 1 - H / H_max   (e^-H - e^-H_max) / (1 - e^-H_max)
 *     RENYI      ln S_a / (1 - alpha)         ln V                              1 - H / ln V    (V e^-H - 1) / (V - 1)
 *
 * Every measure is 1 for a one-hot row and 0 for a uniform one.  TSALLIS and RENYI take alpha in (0, 1) or (1, 4]; at alpha == 1
 * exactly both are the SHANNON row, chosen on the host (the kernel divides by no alpha - 1: the host hands it 1 / (alpha - 1)).
 * MAX_PROB and SHANNON do not read alpha.  Any other alpha, and SCONF_CONFID_EXP with MAX_PROB, is refused.
 *
 * In f32, relative to the row maximum m, sums in a fixed order (two calls give the same bits):
 *     Z = sum e^(x - m),   H = ln Z - sum e^(x - m) (x - m) / Z,   ln S_a = ln sum e^(alpha (x - m)) - alpha ln Z,   max p = 1 / Z
 * The per-element e^d, d <= 0, is the hardware's 2^(d log2 e): the rounding of d log2 e moves a term by |d| e^d 2^-24 < 2^-25 at most.
 * The per-row logarithms and exponentials are the HIP math library's logf and expf (the file is built without fast-math).
 *
 * INVALID ROWS.  A row that holds a NaN or +inf, or no finite entry, gives conf = NaN and idx = -1.  Nothing else depends on it.
 */
#ifndef SCONF_CONFID_H
#define SCONF_CONFID_H
#include <stdint.h>
#include "sconf.h"
#ifdef __cplusplus
extern "C" {
#endif

enum { SCONF_CONFID_MAX_PROB = 0, SCONF_CONFID_SHANNON = 1, SCONF_CONFID_TSALLIS = 2, SCONF_CONFID_RENYI = 3 };
enum { SCONF_CONFID_LIN = 0, SCONF_CONFID_EXP = 1 };
enum { SCONF_CONFID_MEAN = 0, SCONF_CONFID_MIN = 1, SCONF_CONFID_MAX = 2, SCONF_CONFID_PROD = 3 };

/* The largest `classes` for which sconf_confid_frames keeps a row in the registers of one wave: 16 lanes per row (four rows per
 * wave) up to 256 classes, a wave per row above.  A longer row takes one workgroup. */
int sconf_confid_row_capacity(void);
/* The largest `classes` for which that workgroup keeps the row in its registers; a longer row still is read twice, the second
 * time out of the cache. */
int sconf_confid_block_capacity(void);
/* Frames one workgroup of sconf_confid_runs scans per step; a longer sequence takes several steps with the label count carried. */
int sconf_confid_scan_chunk(void);

/* idx (M) int32, conf (M) f32: the argmax (first index on ties) and the confidence of each of the M rows of x, as defined above.
 * x: f32, row r at x + r * row_stride, row_stride >= classes elements; only the first `classes` columns of a row are read (the
 * columns behind them may hold anything).  classes >= 2, not necessarily a multiple of 4; M >= 0; M * row_stride < 2^62.
 * method, norm: the enumerators above; alpha: see above.  Where classes % 4 == 0 and the row is finite, idx is what
 * sconf_argmax_rows writes.  Each row is read once from memory (up to sconf_confid_block_capacity() classes), with at most two
 * exponentials per element (one for MAX_PROB and SHANNON).  16-byte loads where x and row_stride are multiples of four elements,
 * single elements elsewhere: the same bits.
 * Every element of idx and conf is written, nothing else. */
int sconf_confid_frames(const float* x, int64_t M, int64_t classes, int64_t row_stride, int method, int norm, float alpha,
                        int32_t* idx, float* conf, sconf_stream_t stream);

/* The greedy CTC collapse of idx (B, N) int32, contiguous (the idx of sconf_confid_frames), with the frames of every label.
 * lengths (B) int32 or NULL (N): clamped into 0..N; frames at or past lengths[b] are ignored.  A frame opens a label where its idx
 * is neither `blank` nor negative and differs from the frame before it (or it is frame 0): idx = -1, an invalid row, breaks a run
 * and is dropped like a blank.  Per sequence b:
 *   targets (B, S_cap) int32          the labels in order, repeats merged, blanks dropped (those of sconf_ctc_collapse), 0 behind them
 *   spans (B, S_cap, 3) int32         (start, run_end, end) of each label: [start, run_end) its own run of frames, end the start of
 *                                     the next label, or lengths[b] for the last; 0 behind the labels
 *   target_lengths (B) int32          the number of labels; -1 where there are more than S_cap (then the first S_cap are written
 *                                     and nothing past the buffers)
 * Every element of the three outputs is written.  One workgroup per sequence scans sconf_confid_scan_chunk() frames per step.
 * 0 <= N < 2^31, B >= 0, 0 <= S_cap < 2^31 / 3. */
int sconf_confid_runs(const int32_t* idx, const int32_t* lengths, int64_t B, int64_t N, int blank, int32_t* targets, int32_t* spans,
                      int32_t* target_lengths, int64_t S_cap, sconf_stream_t stream);

/* out (S) f32: out[s] = the `aggregation` (an enumerator above) of values[a..b) for span s = (a, b) of spans (S, 2) int32, contiguous.
 * values (M) f32.  idx (M) int32 or NULL: where given, frames whose idx is `blank` or negative are skipped; if that leaves none,
 * all frames of the span are used.  An empty span (a == b) gives NaN.  A span that leaves [0, M), or has a > b, is refused on the
 * device: it gives NaN and nothing outside values and idx is read.  A NaN among the frames used gives NaN.  Spans may overlap and be
 * of any length.  One wave per span with a lane-strided loop and a fixed order of reduction: MIN and MAX return one of the values
 * bit for bit, MEAN is the f32 sum over the f32 count, PROD the f32 product.  The same entry point makes token confidences from
 * frame confidences and word confidences from token confidences (idx == NULL, spans over token positions).
 * Every element of out is written, nothing else.  0 <= M < 2^31, S >= 0. */
int sconf_confid_aggregate(const float* values, const int32_t* idx, int blank, int64_t M, const int32_t* spans, int64_t S,
                           int aggregation, float* out, sconf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SCONF_CONFID_H */
