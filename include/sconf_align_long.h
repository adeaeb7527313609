/* sconf_align_long.h — C ABI of the LONG FORM of CTC forced alignment in libsconf_hip.so: the contract of sconf_align.h for whole
 * recordings, transcripts of up to 65535 labels (131071 lattice states), on the MI355X (gfx950).
 *
 * A sixth ABI unit, with the conventions of the others: plain DEVICE pointers + sizes, caller-owned buffers borrowed for the
 * enqueued work, kernels enqueued on `stream` without synchronising, allocating, freeing or reading anything on the host
 * (graph-capture safe); launchers return 0 on success and non-zero with a message in sconf_last_error().
 *
 * SEMANTICS.  Those of sconf_align.h, word for word, with LT = double for every size: the same recursion with its one addition
 * per cell, the same strict tie rules in the order stay, s-1, s-2, the same end among (L-1, L-2), the same five outputs, the same
 * infeasible and poisoned samples.  Every element of the five outputs is written by every call, from the inputs alone; the workspace
 * content is unspecified before and after.  Wherever sconf_align_state_bytes(Smax) == 8 the two units give the same bits.
 *
 * GEOMETRY.  The 2 Smax + 1 states are cut into sconf_lalign_slabs(Smax, slab_states) SLABS of slab_states adjacent states, and the
 * slabs are launched one after the other on the stream, one workgroup per sample in each launch: sconf_lalign_threads(slab_states) =
 * min(1024, slab_states) threads of sconf_lalign_states_per_thread(slab_states) = slab_states / threads (1, 2, 4 or 8) adjacent
 * states, two f64 rows in LDS with one cell of padding behind each thread's cells from 2 states per thread on, which keeps the lanes
 * of a wave in different banks (147 504 bytes at 8192).  A slab runs over the frames at which one of its
 * states can be reached from the start and can still reach the end; per frame it takes the two cells below its first state from an
 * EDGE COLUMN that the launch of the slab below wrote, and writes its own top two cells to a second one (the two columns swap roles
 * from slab to slab).  No workgroup waits for another inside a launch: the kernel boundary is the only hand-off.  slab_states is 256,
 * 512, 1024, 2048, 4096 or 8192; 0 stands for sconf_lalign_default_slab_states() = 8192.  The result does not depend on it.
 */
#ifndef SCONF_ALIGN_LONG_H
#define SCONF_ALIGN_LONG_H
#include <stdint.h>
#include "sconf.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The largest Smax accepted: 65535 labels = 131071 states. */
int sconf_lalign_max_labels(void);
/* What slab_states = 0 stands for: 8192 (1024 threads x 8 states). */
int sconf_lalign_default_slab_states(void);
/* Launch geometry of one slab (see GEOMETRY); -1 for a slab_states that is neither 0 nor one of the six sizes. */
int sconf_lalign_threads(int slab_states);
int sconf_lalign_states_per_thread(int slab_states);
/* Slab launches of one call: ceil((2 Smax + 1) / slab_states); -1 for Smax outside 0..sconf_lalign_max_labels() or a bad slab_states. */
int sconf_lalign_slabs(int64_t Smax, int slab_states);
/* Bytes of workspace for B samples of N frames and up to Smax labels, -1 for invalid sizes (B < 1, N < 1, B N >= 2^31, Smax outside
 * 0..sconf_lalign_max_labels(), a bad slab_states).  Five parts, each rounded up to 256 bytes; none depends on slab_states:
 *   end state per sample                 4 B bytes
 *   T, S and status per sample           16 B bytes (decided once, read by every slab launch)
 *   edge columns, two                    2 x 16 B N bytes: per frame the top two f64 cells of the slab that wrote the column
 *   emissions, compact                   4 B N (round8(Smax) + 12) bytes, as sconf_align_workspace
 *   back-pointers, ONE BYTE per cell     B N round48(2 Smax + 1) bytes, as sconf_align_workspace
 * At B = 1, N = 45000, Smax = 12288: 256 + 256 + 1 440 000 + 2 214 000 128 + 1 108 080 128 = 3 323 520 768 bytes. */
int64_t sconf_lalign_workspace(int64_t B, int64_t N, int64_t Smax, int slab_states);
/* The alignment: the arguments of sconf_align_ctc, with slab_states (see GEOMETRY) in front of the stream.  workspace_bytes must be
 * at least sconf_lalign_workspace(B, N, Smax, slab_states).  B = 0 returns 0 and launches nothing. */
int sconf_lalign_ctc(const float* log_probs, const int32_t* targets, const int32_t* input_lengths, const int32_t* target_lengths,
                     int32_t* path, int32_t* labels, int32_t* spans, float* token_logp, double* score, void* workspace,
                     int64_t workspace_bytes, int64_t B, int64_t N, int64_t C, int64_t Smax, int blank, int slab_states,
                     sconf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SCONF_ALIGN_LONG_H */
