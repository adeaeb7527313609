// CTC forced alignment (include/sconf_align.h): the Viterbi path of a transcript through (B, N, C) log-probs, token spans and
// per-token log-probabilities.  The lattice is the one of ctc.hip in the (max, +) semiring, plus back-pointers and a walk back.
//
// Structure (serial in time, B-way batch parallelism, as the loss):
//   1. gather    em[b][t] = [log-prob of label 0 .. S-1 | pad | log-prob of the blank]: every blank state has the same emission, so
//                the compact row is half of the loss's (N, 2 S + 1) one, and a thread's adjacent states read CONTIGUOUS labels.
//   2. lattice   one workgroup per sample; a thread owns MAXS adjacent states, the row lives in LDS (double-buffered, one raw barrier
//                per frame), emissions are prefetched G frames ahead into registers with unconditional, clamped vector loads.  The
//                step is LDS read, two compares, one add in the state type, LDS write - no transcendental; what leaves per frame is
//                one BYTE per cell (the step taken), the thread's MAXS bytes as one vector store.  Waves whose states are all
//                unreachable (s > 2 i + 1) or can no longer reach the end (s < L - 2 (T - i)) skip the arithmetic and the store.
//                The loss's long-lattice form stages emissions by LDS-DMA because MAXS strided dword loads and MAXS strided f32
//                stores per thread and frame filled the memory pipeline; here a thread's emissions are MAXS / 2 contiguous floats
//                (one or two 16-byte loads) and its output is at most 16 bytes, so the register prefetch is kept for every length.
//   3. walk back one wave per sample.  The state falls by at most 2 per frame, so the back-pointers of K frames lie within 2 K - 1
//                cells per row below the current state: the wave fetches K rows x 32 cells at once and lane 0 walks them in LDS.
//   4. frames    one thread per frame: labels, and the span boundaries where the path changes state.
//   5. tokens    one thread per token: spans of absent tokens, and the token's log-probabilities summed in frame order.
// Steps 1, 3, 4 and 5 are in align_common.h, shared with the long form of the same contract (align_long.hip); step 2 is in
// align_lattice.h, shared with the alignment with star labels (seg.hip).
#include "align_lattice.h"
#include "../../include/sconf_align.h"

SCONF_API int sconf_align_max_labels(void) { return ALIGN_MAX_LABELS; }
SCONF_API int sconf_align_state_bytes(int64_t Smax) { return Smax < 0 || Smax > ALIGN_MAX_LABELS ? -1 : geometry(Smax).state_bytes; }
SCONF_API int sconf_align_threads(int64_t Smax) { return Smax < 0 || Smax > ALIGN_MAX_LABELS ? -1 : geometry(Smax).nt; }
SCONF_API int sconf_align_states_per_thread(int64_t Smax) { return Smax < 0 || Smax > ALIGN_MAX_LABELS ? -1 : geometry(Smax).maxs; }
SCONF_API int sconf_align_walk_window(void) { return WALK_K; }

SCONF_API int64_t sconf_align_workspace(int64_t B, int64_t N, int64_t Smax) {
    if (B < 1 || N < 1 || Smax < 0 || Smax > ALIGN_MAX_LABELS || B * N > 0x7fffffff) return -1;
    return round256(4 * B) + round256(4 * B * N * (label_pitch(Smax) + 4)) + round256(B * N * bp_pitch(Smax));
}

SCONF_API int sconf_align_ctc(const float* log_probs, const int32_t* targets, const int32_t* input_lengths, const int32_t* target_lengths,
                              int32_t* path, int32_t* labels, int32_t* spans, float* token_logp, double* score, void* workspace,
                              int64_t workspace_bytes, int64_t B, int64_t N, int64_t C, int64_t Smax, int blank, sconf_stream_t stream) {
    if (B == 0) return 0;
    SCONF_REQUIRE(Smax >= 0 && Smax <= ALIGN_MAX_LABELS, "sconf_align_ctc: %ld labels: at most %d (16383 lattice states)", (long)Smax, ALIGN_MAX_LABELS);
    SCONF_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && B * N <= 0x7fffffff, "sconf_align_ctc: bad sizes B = %ld, N = %ld", (long)B, (long)N);
    SCONF_REQUIRE(C >= 4 && C % 4 == 0 && C * 4 <= 64 * 1024, "sconf_align_ctc: C must be a multiple of 4 and one row must fit LDS (%ld classes)", (long)C);
    SCONF_REQUIRE(blank >= 0 && blank < C, "sconf_align_ctc: blank %d out of range", blank);
    SCONF_REQUIRE(log_probs && path && labels && score && workspace && (Smax == 0 || (targets && spans && token_logp)), "sconf_align_ctc: null pointer");
    SCONF_REQUIRE(workspace_bytes >= sconf_align_workspace(B, N, Smax), "sconf_align_ctc: workspace of %ld bytes, %ld needed",
                  (long)workspace_bytes, (long)sconf_align_workspace(B, N, Smax));
    const int LP = label_pitch(Smax), BPW = bp_pitch(Smax);
    int* endst = (int*)workspace;
    float* em = (float*)((char*)workspace + round256(4 * B));
    unsigned char* bp = (unsigned char*)em + round256(4 * B * N * (LP + 4));
    launch_align_gather<false>(log_probs, targets, input_lengths, target_lengths, em, B, N, C, Smax, LP, blank, 0.f, stream);
    launch_align_lattice(em, targets, input_lengths, target_lengths, bp, endst, score, B, N, C, Smax, LP, BPW, stream);
    launch_align_outputs<false>(log_probs, targets, input_lengths, target_lengths, bp, endst, path, labels, spans, token_logp, B, N, C, Smax, BPW,
                                blank, 0.f, stream);
    SCONF_LAUNCH_OK("sconf_align_ctc");
    return 0;
}
