/* sconf_lm.h — C ABI of CTC prefix beam search with a back-off n-gram language model fused in, in libsconf_hip.so on the MI355X
 * (gfx950): what pyctcdecode's build_ctcdecoder(vocab, kenlm_model_path, alpha, beta) adds to the LM-free search of sconf_beam.h,
 * for a TOKEN-level model (one LM word = one CTC class), less pyctcdecode's word-level merging, hotwords and </s> scoring.
 *
 * A fifth ABI unit beside sconf.h, sconf_audio.h, sconf_align.h and sconf_beam.h, with the same conventions: plain DEVICE pointers +
 * sizes, caller-owned buffers borrowed for the enqueued work, kernels enqueued on `stream` without synchronising, allocating, freeing
 * or reading anything on the host (graph-capture safe); launchers return 0 on success and non-zero with a message in
 * sconf_last_error().
 *
 * THE IMAGE.  The language model is one flat read-only buffer of 32-bit words, 16-byte aligned, and five integers.  It is the
 * back-off automaton of the n-gram table: its states are the contexts, with failure (back-off) arcs.  Three arrays, in this order:
 *
 *   states   n_states records of 16 bytes   (int32 first_child, int32 n_children, f32 backoff, int32 backoff_state)
 *            One state per gram of length < order; state 0 is the empty context (its record is 0, 0, 0.0f, 0: its children are the
 *            dense table below).  first_child / n_children select the state's slice of `entries`.  backoff is the gram's back-off
 *            weight (natural log; 0 where the table gives none) and backoff_state the state of the context without its first word -
 *            the longest proper suffix of the context that is a state - so a chain of back-off arcs loses a word per arc and ends
 *            in state 0.
 *   entries  n_entries records of 16 bytes  (int32 token, f32 logp, int32 next_state, int32 0)
 *            The children of every state but state 0, sorted by token inside a state: the gram "context token" with its natural-log
 *            probability and next_state = the longest suffix of that gram that is a state (computed on the host).
 *   dense    num_tokens records of 8 bytes  (f32 logp, int32 next_state)
 *            The unigram level, indexed by token; a token without a unigram holds (unk_logp, 0).
 *
 *   bytes = 16 n_states + 16 n_entries + 8 num_tokens.  All values were rounded to f32 once, on the host.
 *
 *   step(state, token) -> (q, next_state)
 *            token >= num_tokens (a class the model does not know; never the blank, which is never looked up): q = 0, next = 0.
 *            Else, repeat: at state 0 read dense[token]: q += logp, next = its next_state, stop.  At another state binary-search the
 *            state's sorted children for the token; found: q += logp, next = its next_state, stop; not found: q += backoff, state =
 *            backoff_state.  q is the f64 sum of the f32 values in the order met.
 *   order    the longest gram (1 .. sconf_lm_max_order()); start_state is the state of the empty prefix ("<s>", or 0).
 *
 *   Every index read from the image is clamped to the sizes passed to the call, the back-off loop is bounded by `order` and the binary
 *   search of a state's children by 32 steps: an image that does not describe an automaton gives unspecified scores, never an access out of range.
 *
 * SEMANTICS.  Exactly those of sconf_beam.h - kept tokens, stay, extension, fold by equality of token sequences, tie rules, trie,
 * outputs, T = 0, poisoned samples - with these changes:
 *
 *   Beams       carry two more values: bonus (f64; 0 for the empty prefix) and lm_state (start_state for the empty prefix).
 *   Extension   of beam i by class c that is NOT folded: (q, s') = step(lm_state_i, c); bonus' = bonus_i + (alpha q + beta);
 *               lm_state' = s'.  (pyctcdecode's per-unit alpha ln P + beta.)  A folded extension adds only its acoustic mass to beam
 *               j: it has j's prefix, hence j's bonus and state, and no step is taken.  A stay keeps bonus and state.
 *   Key         of a candidate = acoustic total + bonus (the acoustic total is that of sconf_beam.h; this sum is done last).
 *               Selection, the width cut, the tie rules and beam_prune_logp act on the key; candidates whose ACOUSTIC total is -inf
 *               (or NaN) are dropped.  A frame without a kept token moves every key by lp[blank] and changes no order.
 *   scores      (B, nbest) f64: the keys, best first.
 *   logit_scores(B, nbest) f64: the acoustic totals of the same hypotheses; -inf / NaN placed as in scores.
 *   T = 0       one empty hypothesis, scores = logit_scores = 0.
 *   Every element of the six outputs is written by every call, from the inputs alone.  With alpha = beta = 0 the first five outputs
 *   are those of sconf_beam_ctc bit for bit and logit_scores equals scores.
 *
 * GEOMETRY.  As sconf_beam.h (the compaction and the candidate selection are the same code): one workgroup of
 * sconf_lm_beam_threads(W, Kmax) threads per sample.  The thread that owns the candidate of extension (i, k) takes its step, after
 * the fold is known: a chain of at most order (2 + ceil(log2(children))) dependent 16-byte loads.  New bonus and state of every
 * candidate stay in LDS beside its key until the survivors are known.  Dynamic LDS of the search at W = 128, Kmax = 16: 122 192 bytes
 * (of 160 KB; the LM-free search: 69 904).
 */
#ifndef SCONF_LM_H
#define SCONF_LM_H
#include <stdint.h>
#include "sconf.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The longest gram an image may hold (5). */
int sconf_lm_max_order(void);
/* Threads of the search workgroup: sconf_beam_threads(W, Kmax); -1 for a W or Kmax outside 1 .. the maxima of sconf_beam.h. */
int sconf_lm_beam_threads(int64_t W, int64_t Kmax);
/* Bytes of workspace, -1 for invalid sizes (as sconf_beam_workspace).  Four parts, each rounded up to 256 bytes: the compact records
 * (B N (8 + 8 Kmax)), the prefix trie (16 B N W), the final beams (24 B W: leaf node, length, key f64, acoustic total f64) and the
 * live beams (4 B).  At B = 1, N = 16384, W = 100, Kmax = 16: 2 228 224 + 26 214 400 + 2560 + 256 = 28 445 440 bytes. */
int64_t sconf_lm_beam_workspace(int64_t B, int64_t N, int64_t W, int64_t Kmax);
/* The search (see SEMANTICS).  log_probs, input_lengths, blank, beam_width, nbest, token_min_logp, beam_prune_logp,
 * max_tokens_per_frame, Lmax, count, tokens, lengths, token_frames, scores: as sconf_beam_ctc.  image: see THE IMAGE (16-byte
 * aligned; n_states >= 1, n_entries >= 0, 1 <= num_tokens <= C, 1 <= order <= sconf_lm_max_order(), 0 <= start_state < n_states,
 * an image of 4 (n_states + n_entries) + 2 num_tokens < 2^31 32-bit words).  logit_scores (B, nbest) f64.  alpha, beta: finite.  workspace_bytes must
 * be at least sconf_lm_beam_workspace(B, N, beam_width, max_tokens_per_frame).  B = 0 returns 0 and launches nothing. */
int sconf_lm_beam_ctc(const float* log_probs, const int32_t* input_lengths, const void* image, int64_t n_states, int64_t n_entries,
                      int64_t num_tokens, int order, int start_state, int32_t* count, int32_t* tokens, int32_t* lengths,
                      int32_t* token_frames, double* scores, double* logit_scores, void* workspace, int64_t workspace_bytes, int64_t B,
                      int64_t N, int64_t C, int blank, int beam_width, int nbest, float token_min_logp, double beam_prune_logp,
                      int max_tokens_per_frame, int64_t Lmax, double alpha, double beta, sconf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SCONF_LM_H */
