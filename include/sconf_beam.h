/* sconf_beam.h — C ABI of CTC prefix beam search in libsconf_hip.so: the n best transcripts of (B, N, C) log-probs with the frame of
 * every token, on the MI355X (gfx950).  The textbook two-score prefix search (Graves / Hannun) without a language model: what the
 * reference's evaluation drivers run through pyctcdecode's build_ctcdecoder(vocab, kenlm_model_path=None), less its word heuristics.
 *
 * A fourth ABI unit beside sconf.h, sconf_audio.h and sconf_align.h, with the same conventions: plain DEVICE pointers + sizes,
 * caller-owned buffers borrowed for the enqueued work, kernels enqueued on `stream` without synchronising, allocating, freeing or
 * reading anything on the host (graph-capture safe); launchers return 0 on success and non-zero with a message in sconf_last_error().
 *
 * SEMANTICS, per sample; T = input_lengths[b] frames, lp[t][c] = log_probs[b][t][c] (f32); every score is f64 and
 * lse(a, b) = max(a, b) + log1p(exp(-|a - b|)), with -inf neutral.  W = beam_width, Kmax = max_tokens_per_frame.
 *
 *   Kept tokens of frame t.  The non-blank classes c with lp[t][c] >= token_min_logp (compared in f32), plus the row's argmax if it is
 *               not the blank (ties: the lowest index).  If more than Kmax qualify, the Kmax largest stay (ties: the lower index).
 *               The kept tokens in ascending class order are the slots k = 0, 1, ...  The blank is always considered.  A class that
 *               is not kept contributes nothing in that frame, also not as the repeat of a beam's last token.
 *   Beams       are ranked 0 .. n-1; each has a token prefix, pb (log-mass of its alignments that end in the blank) and pnb (of
 *               those that end in a token); its total is lse(pb, pnb).  Start: one beam, the empty prefix, pb = 0, pnb = -inf.
 *   Frame step  Beam i stays (candidate index i):  pb' = lse(pb, pnb) + lp[blank];  pnb' = pnb + lp[last] if the prefix is not empty
 *               and its last token is kept, else -inf.
 *               Beam i is extended by slot k, class c (candidate index W + i Kmax + k):  v = lp[c] + (pb if c == last else
 *               lse(pb, pnb)).  If prefix_i + c EQUALS the prefix of a live beam j, v is folded into that beam's stay candidate,
 *               pnb'_j = lse(pnb'_j, v), and no candidate is made (at most one extension reaches a given j).  Otherwise the
 *               candidate has pb = -inf, pnb = v.
 *               Selection: candidates with total -inf are dropped; the W largest totals survive (ties: the lower candidate index);
 *               survivors with total < best + beam_prune_logp are dropped; the surviving order is the new ranking.  A surviving
 *               extension records t as the frame of its token.
 *               "Equals" is equality of token sequences; the kernels identify a prefix by (length, 64-bit hash).
 *   count       (B) int32: min(nbest, live beams after frame T - 1).
 *   tokens      (B, nbest, Lmax) int32: the first min(length, Lmax) tokens of the hypothesis of each rank, -1 behind them.
 *   lengths     (B, nbest) int32: the true length, also above Lmax; 0 at rank >= count.
 *   token_frames(B, nbest, Lmax) int32: the frame at which each token was created, filled like tokens.
 *   scores      (B, nbest) f64: the totals, best first; -inf at rank >= count.
 *   T = 0       one empty hypothesis with score 0.
 *   Poisoned    (T > N or T < 0): count 0, every score NaN, tokens and token_frames -1, lengths 0; nothing is indexed with the bad
 *               value, and the other samples of the batch are bit-equal to a call of their own.
 *   Every element of the five outputs is written by every call, from the inputs alone.  The workspace content is unspecified.
 *   Non-finite log-probs give unspecified hypotheses, never a token outside [0, C) or an access out of range; -inf entries are
 *   ordinary input (the padded classes of a decoder whose class count is rounded up carry them).
 *
 * GEOMETRY.  Compaction: one workgroup of 256 threads per (sample, frame).  Search: one workgroup of sconf_beam_threads(W, Kmax)
 * threads per sample, serial in time; a frame with n live beams and k kept tokens has n (k + 1) candidates: up to
 * sconf_beam_rank_limit() of them are selected by counting ranks, more by a sort of sconf_beam_sort_size(n (k + 1)) keys; a frame
 * with no kept token selects nothing.  Records are fetched sconf_beam_prefetch_frames() frames at a time, one chunk ahead.
 * Backtrace: one wave per (sample, rank).
 */
#ifndef SCONF_BEAM_H
#define SCONF_BEAM_H
#include <stdint.h>
#include "sconf.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The largest beam_width accepted (128) and the largest max_tokens_per_frame (16). */
int sconf_beam_max_width(void);
int sconf_beam_max_tokens(void);
/* Threads of the search workgroup: half the next power of two of W (Kmax + 1), the most candidates a frame can have, within
 * 64 .. 1024; -1 for a W or Kmax outside 1 .. the maxima. */
int sconf_beam_threads(int64_t W, int64_t Kmax);
/* The largest candidate count of a frame that is selected by counting ranks instead of sorting (128). */
int sconf_beam_rank_limit(void);
/* Keys sorted in a frame with `candidates` = n (k + 1) candidates: 0 up to sconf_beam_rank_limit() (nothing is sorted), else the
 * next power of two; -1 for candidates < 1 or above max_width (max_tokens + 1). */
int sconf_beam_sort_size(int64_t candidates);
/* Frames whose compact records the search fetches together (one chunk is in flight while the previous one is searched). */
int sconf_beam_prefetch_frames(void);
/* Bytes of workspace, -1 for invalid sizes (B < 1, N < 1, W or Kmax outside 1 .. the maxima, B N W >= 2^31).  Four parts, each
 * rounded up to 256 bytes:
 *   compact records      B N (8 + 8 Kmax) bytes: per frame the blank's log-prob (f32), the slot count (int32) and Kmax (class
 *                        int32, log-prob f32) pairs in slot order
 *   prefix trie          16 B N W bytes: node t W + rank = (parent node or -1, token, frame, unused), written by the extension that
 *                        survives frame t at that rank
 *   final beams          16 B W bytes: (leaf node, length, total f64) per rank
 *   live beams           4 B bytes: per sample the number of live beams, -1 for a poisoned sample
 * At B = 1, N = 16384, W = 100, Kmax = 16: 2 228 224 + 26 214 400 + 1792 + 256 = 28 444 672 bytes. */
int64_t sconf_beam_workspace(int64_t B, int64_t N, int64_t W, int64_t Kmax);
/* The search (see SEMANTICS).  log_probs (B, N, C) f32 as sconf_align_ctc takes them (C a multiple of 4, at most 16384);
 * input_lengths (B) int32 or NULL (= N); 0 <= blank < C; 1 <= nbest <= beam_width <= sconf_beam_max_width();
 * beam_prune_logp <= 0 (-inf: no pruning; NaN is refused); 1 <= max_tokens_per_frame <= sconf_beam_max_tokens(); Lmax >= 1.
 * Outputs count (B) int32, tokens and token_frames (B, nbest, Lmax) int32, lengths (B, nbest) int32, scores (B, nbest) f64;
 * workspace_bytes must be at least sconf_beam_workspace(B, N, beam_width, max_tokens_per_frame).  B = 0 returns 0 and launches
 * nothing. */
int sconf_beam_ctc(const float* log_probs, const int32_t* input_lengths, int32_t* count, int32_t* tokens, int32_t* lengths,
                   int32_t* token_frames, double* scores, void* workspace, int64_t workspace_bytes, int64_t B, int64_t N, int64_t C,
                   int blank, int beam_width, int nbest, float token_min_logp, double beam_prune_logp, int max_tokens_per_frame,
                   int64_t Lmax, sconf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SCONF_BEAM_H */
