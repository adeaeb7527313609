/* sconf_seg.h — C ABI of CTC segmentation in libsconf_hip.so: a loose transcript (a list of utterances with unknown times, which may
 * skip parts of the recording and may hold wrong utterances) becomes utterances with times and a confidence each, on the MI355X
 * (gfx950).  The job of Kürzinger et al. 2020 ("CTC-Segmentation of Large Corpora for German End-to-end Speech Recognition") and of
 * torchaudio.functional.forced_align with a <star> token.
 *
 * A thirteenth ABI unit beside sconf.h, with the same conventions: plain DEVICE pointers + sizes, caller-owned buffers borrowed for
 * the enqueued work, kernels enqueued on `stream` without synchronising, allocating, freeing or reading anything on the host
 * (graph-capture safe); launchers return 0 on success and non-zero with a message in sconf_last_error().
 *
 * Two entry points that chain: sconf_seg_align (forced alignment in which STAR labels absorb any audio) and sconf_seg_score (one
 * span of frames, a mean log-probability and a confidence per utterance).
 *
 * STAR LABELS.  The label value C, the first id past the classes, is the star: sconf_seg_star_label(C).  Its emission is `star_logp`
 * at every frame.  The five outputs that sconf_align.h defines are exactly what sconf_align_ctc (Smax <= sconf_align_max_labels())
 * or sconf_lalign_ctc with the default slab (above) gives on log-probs (B, N, C') with C' > C whose column C holds star_logp: the
 * same recursion, tie rules, end rule and state type.  So:
 *   - a star is a label: it occupies at least one frame, and two adjacent stars are a repeat (a blank must part them);
 *   - a label outside [0, C] poisons the sample; the label C does not;
 *   - token_logp of a star is star_logp added once per frame of its span, in frame order, in f32;
 *   - labels holds C on the frames of a star;
 *   - targets without a star give the bits of sconf_align_ctc / sconf_lalign_ctc on the same inputs.
 * The star costs no pass over the log-probs and no (B, N, C') copy: it enters where the emissions of the target's labels are gathered.
 *
 * With star_logp = 0 a star is free, so it also takes the frames of its neighbours that cost anything at all: a token next to a star
 * shrinks towards one frame (torchaudio's behaviour too).  A negative star_logp makes a star win only over frames that match
 * nothing in the transcript.  No value has been tuned on real recordings here.
 *
 * UTTERANCE SCORES.  With g = frame_logp of sconf_seg_align, an utterance of the tokens [j0, j1) of a sample's target row covers the
 * frames [f0, f1), f0 = spans[j0][0], f1 = spans[j1 - 1][1]; with n = f1 - f0 and w = min(window, n):
 *     utt_logp = (sum of g over [f0, f1)) / n
 *     utt_conf = min over f0 <= t <= f1 - w of (sum of g over [t, t + w)) / w
 * the sums in f64, each result rounded once to f32.  utt_conf is Kürzinger's rule: an utterance is as good as its worst stretch of w
 * frames, so one wrong word sinks it while the mean hardly moves.  The window sums are differences of an f64 running sum that
 * starts at f0: against an exact evaluation the results are off by the f32 rounding (2^-24 relative) and at most
 * n 2^-53 (sum of |g| over the utterance) / w.
 */
#ifndef SCONF_SEG_H
#define SCONF_SEG_H
#include <stdint.h>
#include "sconf.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The star's label value for C classes: C.  -1 for C < 1. */
int sconf_seg_star_label(int64_t C);
/* The largest `window` sconf_seg_score accepts. */
int sconf_seg_max_window(void);
/* Frames of an utterance that one workgroup of sconf_seg_score handles per round; a longer utterance takes several rounds with the
 * running sum carried. */
int sconf_seg_score_tile(void);
/* Bytes of workspace of sconf_seg_align for B samples of N frames, up to Smax labels (stars included) and up to Umax utterances per
 * sample; -1 for invalid sizes (B < 1, N < 1, B N >= 2^31, Smax outside 0..sconf_lalign_max_labels(), Umax < 0).  It is
 * sconf_align_workspace(B, N, Smax) up to sconf_align_max_labels() labels and sconf_lalign_workspace(B, N, Smax, 0) above.
 * sconf_seg_score works in LDS and registers alone, so Umax adds nothing. */
int64_t sconf_seg_workspace(int64_t B, int64_t N, int64_t Smax, int64_t Umax);

/* The alignment with star labels (see STAR LABELS).  Arguments as sconf_align_ctc takes them (log_probs (B, N, C) f32, C a multiple
 * of 4 and at most 16384; targets (B, Smax) int32 with values in [0, C]; lengths (B) int32 or NULL; Smax = 0 allowed), Smax up to
 * sconf_lalign_max_labels(); star_logp finite and <= 0, anything else is refused.
 * Outputs: path, labels (B, N) int32, spans (B, Smax, 2) int32, token_logp (B, Smax) f32, score (B) f64 as sconf_align.h defines
 * them, and
 *   frame_logp (B, N) f32: the f32 emission of the state the path occupies at frame t (the label's log-prob, the blank's, or
 *                          star_logp); 0 at t >= T and for infeasible or poisoned samples.  Its sum over a sample is the score, up
 *                          to the order and type of the additions.
 * Every element of the six outputs is written by every call.  workspace_bytes must be at least sconf_seg_workspace(B, N, Smax, .).
 * B = 0 returns 0 and launches nothing. */
int sconf_seg_align(const float* log_probs, const int32_t* targets, const int32_t* input_lengths, const int32_t* target_lengths,
                    int32_t* path, int32_t* labels, int32_t* spans, float* token_logp, double* score, float* frame_logp, void* workspace,
                    int64_t workspace_bytes, int64_t B, int64_t N, int64_t C, int64_t Smax, int blank, float star_logp,
                    sconf_stream_t stream);

/* The utterance scores (see UTTERANCE SCORES).  spans (B, Smax, 2) int32, frame_logp (B, N) f32 and score (B) f64 as sconf_seg_align
 * wrote them; input_lengths / target_lengths (B) int32 or NULL (= N / Smax), the ones given to sconf_seg_align.
 * utt (B, Umax, 2) int32: token ranges [j0, j1) into the sample's target row; utt_counts (B) int32 or NULL (= Umax), clamped into
 * 0..Umax.  1 <= window <= sconf_seg_max_window().  Outputs utt_frames (B, Umax, 2) int32, utt_logp, utt_conf (B, Umax) f32:
 *   u >= utt_counts[b]                                         frames (-1, -1), both values 0
 *   a valid utterance (0 <= j0 < j1 <= S, score[b] finite)     as defined above
 *   anything else (a bad range, score[b] -inf or NaN, lengths outside 0..Smax / 1..N, spans that are not 0 <= f0 < f1 <= T)
 *                                                              frames (-1, -1), both values NaN
 * Nothing is indexed with a bad value.  Every element of the three outputs is written by every call, nothing else.  One workgroup
 * per utterance.  B = 0 or Umax = 0 returns 0 and launches nothing.  B <= 65535, N >= 1, B N < 2^31, 0 <= Smax <= 65535. */
int sconf_seg_score(const int32_t* spans, const float* frame_logp, const double* score, const int32_t* input_lengths,
                    const int32_t* target_lengths, const int32_t* utt, const int32_t* utt_counts, int window, int32_t* utt_frames,
                    float* utt_logp, float* utt_conf, int64_t B, int64_t N, int64_t Smax, int64_t Umax, sconf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SCONF_SEG_H */
