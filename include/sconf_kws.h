/* sconf_kws.h — C ABI of CTC keyword search in libsconf_hip.so: a list of keywords (token sequences) and the posteriors of a
 * recording become timed, scored hits, on the MI355X (gfx950).  "Where in these hours does anyone say X?" for hundreds or thousands
 * of X at once, answered from the (N, C) log-scores and not from a 1-best transcript.
 *
 * A fourteenth ABI unit beside sconf.h, with the same conventions: plain DEVICE pointers + sizes, caller-owned buffers borrowed for
 * the enqueued work, kernels enqueued on `stream` without synchronising, allocating, freeing or reading anything on the host
 * (graph-capture safe); the launcher returns 0 on success and non-zero with a message in sconf_last_error().
 *
 * THE FUNCTION.  x (B, N, C) f32 holds rows of unnormalised log-scores; only the first `classes` columns of a row are read.  Per
 * frame t, m_t = max_c x[t, c] and llr_t(c) = x[t, c] - m_t: <= 0, and exactly 0 for the arg-max class.  A row with a NaN, a +inf
 * or no finite entry makes every llr_t = -inf: no path crosses that frame.
 * A keyword of L labels l_1 .. l_L (1 <= L <= sconf_kws_max_labels()) has the lattice ext = [l_1, blank, l_2, blank, .., l_L] of the
 * states s = 0 .. 2L - 2.  There is no leading or trailing blank: a hit starts on the first frame of l_1 and ends on the last frame
 * of l_L.  Each state carries a pair (v, b): the score and the start frame of the best path into it.  Pairs are ordered
 * lexicographically by (larger v, then smaller b); that order is the whole tie rule.
 *
 *     cand_t(s) = { (v, b)_{t-1}(s),  (v, b)_{t-1}(s - 1) [s >= 1],
 *                   (v, b)_{t-1}(s - 2) [s even, s >= 2, ext_s != ext_{s-2}],
 *                   (0, t) [s == 0] }
 *     (v, b)_t(s) = (llr_t(ext_s) + best.v, best.b)              everything before frame 0 is (-inf, -)
 *
 * All arithmetic is f32: one subtraction for llr, one addition per step, nothing to contract or reassociate.  The results are
 * therefore defined to the bit.  (An llr of -0, which only a row whose maximum is +0 in one class and -0 in another produces,
 * counts as +0; best.v is never -0, so no v depends on it and no score is -0.)
 *
 * HITS.  At frame t keyword k has a candidate (E, s, e) = (v_t(2L - 2), b_t(2L - 2), t + 1) when E > -inf and E >= threshold_k; the
 * span is the half-open [s, e).  One pass of non-maximum suppression per keyword and sample keeps `cur`:
 *     no cur                        the candidate becomes cur
 *     candidate.s <  cur.e          it replaces cur only if its E is strictly larger
 *     candidate.s >= cur.e          cur is emitted and the candidate becomes cur
 *     after the sample's last frame cur is emitted
 * Hits come out in time order and never overlap.  E is the total log-likelihood ratio of the keyword's best path over [s, e)
 * against the greedy path over the same frames: 0 means the keyword IS the greedy decode of that span.
 *
 * THE KEYWORD IMAGE.  One int32 buffer, built on the host and uploaded once (decoding/kws.py):
 *     lanes   (n_waves * 64, 4)   per lane of a 64-lane wave: (u, flags, keyword, threshold)
 *                                   u          the lane's column in `columns`; -1 = idle lane
 *                                   flags      SCONF_KWS_FIRST: state 0 of a keyword (takes the fresh start, reads no neighbour)
 *                                              SCONF_KWS_SKIP:  may take the state two lanes below
 *                                              SCONF_KWS_LAST:  state 2L - 2: forms candidates and writes the keyword's hits
 *                                   keyword    the keyword's index in 0 .. K - 1
 *                                   threshold  the keyword's threshold on E, as f32 bits
 *     columns (U)                 the class id of each compact column: the distinct labels of the set, and -1 for the blank of the
 *                                 call where a keyword of two labels or more needs it
 * The states of a keyword lie on neighbouring lanes in order; several keywords lie end to end in one wave; no keyword straddles two
 * waves (the longest, 63 states, has a wave to itself).  Every index read from the image is clamped to the sizes passed to the
 * call: a malformed image gives unspecified hits and no access outside the buffers.  The outputs of a keyword that no LAST lane
 * names are not written.
 */
#ifndef SCONF_KWS_H
#define SCONF_KWS_H
#include <stdint.h>
#include "sconf.h"
#ifdef __cplusplus
extern "C" {
#endif

enum { SCONF_KWS_FIRST = 1, SCONF_KWS_SKIP = 2, SCONF_KWS_LAST = 4 };

/* The most labels of one keyword (32: 63 states, one wave). */
int sconf_kws_max_labels(void);
/* Frames whose llr a lane of the walk holds in registers ahead of the frame it works on. */
int sconf_kws_prefetch(void);
/* The largest `cap`. */
int sconf_kws_max_hits(void);
/* Bytes of workspace for B samples of N frames and an image of U columns: the compact table (B, N, Upad) f32 with Upad = U rounded
 * up to 4, rounded up to 256 bytes.  -1 for invalid sizes (B < 1 or > 65535, N < 1, B N >= 2^31 - 16, U < 1 or > 2^20). */
int64_t sconf_kws_workspace(int64_t B, int64_t N, int64_t U);

/* The search.  x (B, N, C) f32 (C the row stride; the first `classes` columns are read); input_lengths (B) int32 or NULL (= N),
 * clamped into 0 .. N, a length 0 gives no hits; image: n_waves * 256 + U int32 as above; K keywords; blank in [0, classes).
 * Outputs, every element written by every call when every keyword 0 .. K - 1 has its LAST lane:
 *   hit_frames (B, K, cap, 2) int32   [s, e) of the first `cap` hits in time order; (-1, -1) in unused slots
 *   hit_score  (B, K, cap)    f32     their E; -inf in unused slots
 *   hit_count  (B, K)         int32   the TRUE number of hits, which may exceed cap
 * workspace_bytes must be at least sconf_kws_workspace(B, N, U).  Refused on the host before any launch: a null pointer (x, image,
 * the outputs, workspace), B, N or K below 1, classes outside 1 .. C, blank outside [0, classes), cap outside
 * 1 .. sconf_kws_max_hits(), n_waves or U below 1, sizes sconf_kws_workspace refuses, a short workspace.  Two kernels: one pass over
 * x that writes the compact table, then one wave per 64 image lanes and sample that walks the frames in order. */
int sconf_kws_search(const float* x, const int32_t* input_lengths, const int32_t* image, int64_t n_waves, int64_t U, int64_t K,
                     int32_t* hit_frames, float* hit_score, int32_t* hit_count, int64_t cap, void* workspace, int64_t workspace_bytes,
                     int64_t B, int64_t N, int64_t C, int64_t classes, int blank, sconf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SCONF_KWS_H */
