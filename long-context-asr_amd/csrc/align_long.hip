// CTC forced alignment, long form (include/sconf_align_long.h): the contract of include/sconf_align.h for transcripts of up to 65535
// labels, the state always f64.  One workgroup cannot hold such a lattice row in LDS, so the 2 Smax + 1 states are cut into SLABS of
// `slab_states` adjacent states and the slabs are launched one after the other on the stream, one workgroup per sample in each.
//
// v[t][s] depends on v[t-1][s], v[t-1][s-1] and v[t-1][s-2] only, so slab k needs nothing of the slabs above it and, of the slab below,
// only the two cells under its first state, frame by frame: the EDGE COLUMN, 2 f64 per frame, which slab k - 1 wrote during its own
// launch.  The kernel boundary is the only hand-off: no workgroup ever waits for another one, there is no flag and no spin.
//
//   0. sample    one workgroup per sample decides ONCE whether it is poisoned and what its T and S are (info[b]); a poisoned or
//                frameless sample gets its score and end state here and every slab launch returns at once for it.
//   1. gather    align_common.h: the compact emission rows, as the short form.
//   2. slabs     slab k = states [k w, k w + w): align.hip's lattice step (two rows in LDS, one raw barrier behind lgkmcnt(0) per
//                frame, emissions prefetched into registers, one back-pointer byte per cell leaving as one vector store per thread)
//                over the slab's LIVE frames only: [s0, s1] is live at frame i while s0 <= 2 i + 1 and s1 >= L - 2 (T - i).  The
//                threads that own the slab's first two states take the cells below them from registers, prefetched from the edge
//                column with the emissions; the threads that own its last two states store them to the other edge column.  An edge
//                cell of a frame at which the lower slab was not live reads as -inf whatever the workspace holds: before its first
//                live frame nothing of it is reachable, after its last nothing of it reaches the end, and a live cell's three
//                predecessors are live.  The sample's last slab takes the end state among (L-1, L-2); L-2 may sit in the edge column.
//   3-5.         align_common.h: walk back, frames, tokens.  The back-pointer rows keep their pitch over the whole 2 Smax + 1.
// Steps 0 and 2 are in align_slabs.h, shared with the alignment with star labels (seg.hip).
#include "align_slabs.h"
#include "../../include/sconf_align_long.h"

SCONF_API int sconf_lalign_max_labels(void) { return LALIGN_MAX_LABELS; }
SCONF_API int sconf_lalign_default_slab_states(void) { return LALIGN_DEFAULT_SLAB; }
SCONF_API int sconf_lalign_threads(int slab_states) { return slab_ok(slab_states) ? threads_of(slab_of(slab_states)) : -1; }
SCONF_API int sconf_lalign_states_per_thread(int slab_states) {
    return slab_ok(slab_states) ? slab_of(slab_states) / threads_of(slab_of(slab_states)) : -1;
}
SCONF_API int sconf_lalign_slabs(int64_t Smax, int slab_states) {
    return smax_ok(Smax) && slab_ok(slab_states) ? cdiv(2 * Smax + 1, slab_of(slab_states)) : -1;
}

SCONF_API int64_t sconf_lalign_workspace(int64_t B, int64_t N, int64_t Smax, int slab_states) {
    if (B < 1 || N < 1 || !smax_ok(Smax) || !slab_ok(slab_states) || B * N > 0x7fffffff) return -1;
    const Parts p = parts(B, N, Smax);
    return p.endst + p.info + p.edge + p.em + p.bp;
}

SCONF_API int sconf_lalign_ctc(const float* log_probs, const int32_t* targets, const int32_t* input_lengths, const int32_t* target_lengths,
                               int32_t* path, int32_t* labels, int32_t* spans, float* token_logp, double* score, void* workspace,
                               int64_t workspace_bytes, int64_t B, int64_t N, int64_t C, int64_t Smax, int blank, int slab_states,
                               sconf_stream_t stream) {
    if (B == 0) return 0;
    SCONF_REQUIRE(smax_ok(Smax), "sconf_lalign_ctc: %ld labels: at most %d (131071 lattice states)", (long)Smax, LALIGN_MAX_LABELS);
    SCONF_REQUIRE(slab_ok(slab_states), "sconf_lalign_ctc: slab_states %d: 0 (= %d) or 256, 512, 1024, 2048, 4096, 8192", slab_states, LALIGN_DEFAULT_SLAB);
    SCONF_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && B * N <= 0x7fffffff, "sconf_lalign_ctc: bad sizes B = %ld, N = %ld", (long)B, (long)N);
    SCONF_REQUIRE(C >= 4 && C % 4 == 0 && C * 4 <= 64 * 1024, "sconf_lalign_ctc: C must be a multiple of 4 and one row must fit LDS (%ld classes)", (long)C);
    SCONF_REQUIRE(blank >= 0 && blank < C, "sconf_lalign_ctc: blank %d out of range", blank);
    SCONF_REQUIRE(log_probs && path && labels && score && workspace && (Smax == 0 || (targets && spans && token_logp)), "sconf_lalign_ctc: null pointer");
    SCONF_REQUIRE(workspace_bytes >= sconf_lalign_workspace(B, N, Smax, slab_states), "sconf_lalign_ctc: workspace of %ld bytes, %ld needed",
                  (long)workspace_bytes, (long)sconf_lalign_workspace(B, N, Smax, slab_states));
    const int LP = label_pitch(Smax), BPW = bp_pitch(Smax);
    const Sections s = sections(workspace, B, N, Smax);
    launch_lalign_sample(targets, input_lengths, target_lengths, s, score, B, N, C, Smax, stream);
    launch_align_gather<false>(log_probs, targets, input_lengths, target_lengths, s.em, B, N, C, Smax, LP, blank, 0.f, stream);
    launch_lalign_slabs(targets, s, score, B, N, Smax, LP, BPW, slab_states, stream);
    launch_align_outputs<false>(log_probs, targets, input_lengths, target_lengths, s.bp, s.endst, path, labels, spans, token_logp, B, N, C, Smax,
                                BPW, blank, 0.f, stream);
    SCONF_LAUNCH_OK("sconf_lalign_ctc");
    return 0;
}
