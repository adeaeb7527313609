/* sconf_hot.h — C ABI of CTC prefix beam search with hotword boosting, in libsconf_hip.so on the MI355X (gfx950): what pyctcdecode's
 * decode_beams(logits, hotwords=[...], hotword_weight=w) adds to the search of sconf_lm.h, for hotwords given as TOKEN sequences
 * (a phrase is the token ids of its spelling), less pyctcdecode's matching on decoded text, negative weights and </s> scoring.
 *
 * An eleventh ABI unit, with the conventions of the others: plain DEVICE pointers + sizes, caller-owned buffers borrowed for the
 * enqueued work, kernels enqueued on `stream` without synchronising, allocating, freeing or reading anything on the host
 * (graph-capture safe); launchers return 0 on success and non-zero with a message in sconf_last_error().
 *
 * THE IMAGE.  The hotword set is one flat read-only buffer of 32-bit words, 16-byte aligned, and three integers.  It is the
 * Aho-Corasick automaton of the phrases over tokens: its states are the nodes of the phrases' trie, state 0 the root.  Three arrays,
 * in this order:
 *
 *   states   hot_states records of 16 bytes  (int32 first_child, int32 n_children, int32 fail_state, int32 0)
 *            first_child / n_children select the state's slice of `entries`.  fail_state is the state of the longest PROPER suffix
 *            of the node's path that is a node (0 for the root and for the nodes of depth 1): a chain of failure arcs loses at
 *            least a token per arc and ends in state 0.
 *   credit   hot_states records of 8 bytes   (f32 emit, f32 phi)
 *            emit(s): the sum of the relative weights of every phrase that is a SUFFIX of the path to s - the phrase that ends
 *            exactly at s and every phrase met over the failure chain.  phi(s) = max(own(s), phi(fail_state(s))), phi(root) = 0,
 *            with own(s) = the maximum, over the phrases p of which the path to s is a PROPER prefix, of w_p depth(s) / len(p)
 *            (0 if there is none): pyctcdecode's partial-match credit, the part of the shortest matching hotword that is spelt so
 *            far.  Both are computed in f64 and rounded to f32 once, on the host.
 *   entries  hot_entries records of 8 bytes  (int32 token, int32 next_state)
 *            The children of every state, sorted by token inside a state.
 *
 *   bytes = 24 hot_states + 8 hot_entries (32-bit words: 6 hot_states + 2 hot_entries).
 *
 *   step(state, token) -> next_state
 *            Repeat: binary-search the state's sorted children for the token; found: its next_state, stop; not found at state 0:
 *            0, stop; not found elsewhere: state = fail_state.  (A token that no phrase holds - also a class the phrases' vocabulary
 *            does not know - ends in state 0.)
 *   hot_max_len  the length of the longest phrase = the depth of the trie (0 .. sconf_hot_max_len()).
 *
 *   Every index read from the image is clamped to the sizes passed to the call, the failure loop is bounded by hot_max_len + 1 rounds
 *   and the binary search of a state's children by 32 probes: an image that does not describe an automaton gives unspecified scores,
 *   never an access out of range.  The caller sees to it that no phrase holds the blank or a token >= C (decoding.hotwords does).
 *
 * SEMANTICS.  Exactly those of sconf_lm.h - kept tokens, stay, extension, fold, tie rules, trie, LM step, T = 0, poisoned samples -
 * with these changes:
 *
 *   LM          lm_image may be NULL with n_states = 0 (then n_entries = num_tokens = order = start_state = 0): the LM's per-token
 *               term (alpha q + beta) is 0 and no LM access is made.
 *   Beams       carry two more values: hot_state (0 for the empty prefix) and hot (f64, 0 for the empty prefix), the PERMANENT
 *               hotword credit of the prefix.
 *   Extension   of beam i by class c that is NOT folded: h' = step(hot_state_i, c); hot' = hot_i + weight (double)emit[h'];
 *               bonus' = (bonus_i + (alpha q + beta)) + weight (double)emit[h'] (each product and each sum rounded on its own);
 *               hot_state' = h'.  A folded extension has the target's prefix, hence its state and credit, and takes no walk.  A
 *               stay keeps everything.
 *   Key         of a candidate during the search = acoustic total + (bonus + weight (double)phi[hot_state]), the parenthesis summed
 *               first.  Selection, the width cut, the tie rules and beam_prune_logp act on this key: a hotword in progress holds
 *               partial credit, and loses it in the frame it stops matching (phi belongs to the state, it is not accumulated).  A
 *               frame without a kept token moves every key by lp[blank] and changes no order.
 *   At the end  phi is dropped: scores = acoustic total + bonus.  The survivors of the last frame are re-ranked by this final key,
 *               larger first; equal keys keep the order of the last frame's ranking.  A transcript that ends inside a hotword gets
 *               no credit for the unfinished part.  With weight = 0 or an image of the root alone there is no phi and no re-rank:
 *               the ranking is the last frame's.
 *   scores      (B, nbest) f64: the final keys, best first.   logit_scores (B, nbest) f64: the acoustic totals, as sconf_lm.h.
 *   hot_scores  (B, nbest) f64: hot of the same hypotheses (weight times the summed relative weights of every phrase occurrence in
 *               the transcript); -inf / NaN placed as in scores.
 *   T = 0       one empty hypothesis, scores = logit_scores = hot_scores = 0.
 *   Every element of the seven outputs is written by every call, from the inputs alone.
 *   With weight = 0, or an image that holds only the root, the first six outputs are those of sconf_lm_beam_ctc bit for bit (with an
 *   LM), or the first five those of sconf_beam_ctc and logit_scores equals scores (without one); hot_scores is 0 where scores is finite.
 *
 * GEOMETRY.  As sconf_lm.h: one workgroup of sconf_hot_beam_threads(W, Kmax) threads per sample.  The thread that owns the candidate
 * of extension (i, k) walks both automata after the fold is known; the new hotword state of every candidate stays in LDS beside its
 * new bonus and LM state until the survivors are known, and a survivor reads the credit record of its new state once more for hot'.
 * Dynamic LDS of the search at W = 128, Kmax = 16: 143 760 bytes (of 160 KB; the LM search: 122 192).
 */
#ifndef SCONF_HOT_H
#define SCONF_HOT_H
#include <stdint.h>
#include "sconf.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The longest phrase an image may hold, in tokens (32). */
int sconf_hot_max_len(void);
/* The largest beam_width (128) and max_tokens_per_frame (16) this unit accepts: those of sconf_beam.h, the search fits LDS with them. */
int sconf_hot_max_width(void);
int sconf_hot_max_tokens(void);
/* Threads of the search workgroup: sconf_beam_threads(W, Kmax); -1 for a W or Kmax outside 1 .. the maxima. */
int sconf_hot_beam_threads(int64_t W, int64_t Kmax);
/* Bytes of workspace, -1 for invalid sizes (as sconf_beam_workspace).  Four parts, each rounded up to 256 bytes: the compact records
 * (B N (8 + 8 Kmax)), the prefix trie (16 B N W), the final beams (32 B W: leaf node, length, key f64, acoustic total f64, hot f64)
 * and the live beams (4 B).  At B = 1, N = 16384, W = 100, Kmax = 16: 2 228 224 + 26 214 400 + 3328 + 256 = 28 446 208 bytes. */
int64_t sconf_hot_beam_workspace(int64_t B, int64_t N, int64_t W, int64_t Kmax);
/* The search (see SEMANTICS).  Everything but lm_image .. weight and hot_scores: as sconf_lm_beam_ctc, except that lm_image may be
 * NULL with n_states = n_entries = num_tokens = 0 (order and start_state are then ignored).  hot_image: see THE IMAGE (16-byte
 * aligned, never NULL; hot_states >= 1, hot_entries >= 0, 6 hot_states + 2 hot_entries < 2^31 words, 0 <= hot_max_len <=
 * sconf_hot_max_len()).  weight: finite, >= 0.  hot_scores (B, nbest) f64.  workspace_bytes must be at least
 * sconf_hot_beam_workspace(B, N, beam_width, max_tokens_per_frame).  B = 0 returns 0 and launches nothing. */
int sconf_hot_beam_ctc(const float* log_probs, const int32_t* input_lengths, const void* lm_image, int64_t n_states, int64_t n_entries,
                       int64_t num_tokens, int order, int start_state, const void* hot_image, int64_t hot_states, int64_t hot_entries,
                       int hot_max_len, double weight, int32_t* count, int32_t* tokens, int32_t* lengths, int32_t* token_frames,
                       double* scores, double* logit_scores, double* hot_scores, void* workspace, int64_t workspace_bytes, int64_t B,
                       int64_t N, int64_t C, int blank, int beam_width, int nbest, float token_min_logp, double beam_prune_logp,
                       int max_tokens_per_frame, int64_t Lmax, double alpha, double beta, sconf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SCONF_HOT_H */
