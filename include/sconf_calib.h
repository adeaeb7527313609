/* sconf_calib.h — C ABI of the calibration unit of libsconf_hip.so: which hypothesis words are wrong (the edit alignment itself, not
 * only its counts) and the frame confidences of sconf_confid.h at K softmax temperatures from one pass over the rows, on the MI355X
 * (gfx950).
 *
 * A fifteenth ABI unit beside sconf.h, with the same conventions: plain DEVICE pointers + sizes, caller-owned buffers borrowed for the
 * enqueued work, kernels enqueued on `stream` without synchronising, allocating or freeing; launchers return 0 on success and
 * non-zero with a message in sconf_last_error().  Nothing is read back to the host.
 *
 * THE ALIGNMENT.  For a hypothesis of H ids and a reference of R ids, E(i, j) is the lexicographic minimum of (errors, substitutions)
 * over three moves,
 *     diagonal  E(i-1, j-1) + ((0, 0) if hyp[i-1] == ref[j-1] else (1, 1))
 *     up        E(i-1, j) + (1, 0)        an insertion: hypothesis id i-1 is aligned to nothing
 *     left      E(i, j-1) + (1, 0)        a deletion: reference id j-1 is aligned to nothing
 * with E(i, 0) = (i, 0) and E(0, j) = (j, 0).  The backtrace runs from (H, R) and takes the FIRST move that reproduces E(i, j), in
 * the order diagonal, up, left; at j == 0 it goes up, at i == 0 left.  The alignment is therefore unique: the primary cost is the
 * Levenshtein distance, among its optimal alignments the rule picks one with the fewest substitutions (the split sconf_edit_counts
 * documents), and among those the listed order decides.  `a b` against `b c` is insertion, hit, deletion, not two substitutions.
 *
 * STORAGE.  The forward pass keeps 2 bits per cell (0 diagonal, 1 up, 2 left) in the pair's slice of the workspace.  The cells are
 * cut into tiles of sconf_edit_align_block_rows() rows by sconf_edit_align_strip_cols() columns, tile (b, s) of the pair at tile index
 * b * ceil(R / strip_cols) + s.  Inside a tile, lane t of the wave that computes it owns the sconf_edit_align_cells_per_word() = 8
 * consecutive columns 8 t .. 8 t + 7 and packs the directions of one row of them into one 16-bit word (column c of the run in bits
 * 2 c, 2 c + 1): a lane writes whole words only, no word is shared.  Rows pass the lanes in skew, so the word of row r (inside the
 * tile) and lane t is stored at 16-bit index (r + t) * 64 + t: the 64 words a wave stores in one step are one 128-byte line.  A tile
 * takes (block_rows + 63) * 128 bytes whatever part of it is inside the pair.  Where R exceeds sconf_edit_align_pass_cols() the slice
 * begins with the parked keys of the pass boundary, H + 1 64-bit keys rounded up to 16 bytes; the tiles follow.  So
 *     pair_bytes(H, R) = 0 if H == 0 or R == 0, else
 *                        (R > pass_cols ? round16(8 (H + 1)) : 0) + ceil(H / block_rows) ceil(R / strip_cols) (block_rows + 63) 128
 * The backtrace is run by the pair's workgroup after its forward pass: the tile under the path is copied into LDS by all lanes, one
 * lane walks it to the tile's edge and writes the map entries it passes.
 */
#ifndef SCONF_CALIB_H
#define SCONF_CALIB_H
#include <stdint.h>
#include "sconf.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Geometry of sconf_edit_align: reference columns per wave (a tile's width), reference columns per pass of a workgroup (a longer
 * reference takes several passes with one parked key per row between them), hypothesis rows between two barriers (a tile's height),
 * cells packed per stored 16-bit word, and the bytes of one tile. */
int sconf_edit_align_strip_cols(void);
int sconf_edit_align_pass_cols(void);
int sconf_edit_align_block_rows(void);
int sconf_edit_align_cells_per_word(void);
int sconf_edit_align_tile_bytes(void);
/* The largest H or R a pair may have (65535). */
int sconf_edit_align_max_len(void);
/* The exact bytes (a multiple of 16) a pair of H hypothesis and R reference ids needs in the workspace, as stated above; -1 where
 * H or R is negative or above sconf_edit_align_max_len(). */
int64_t sconf_edit_align_pair_bytes(int64_t H, int64_t R);

/* The alignment of P ragged pairs hyp[hyp_off[p] .. hyp_off[p+1]) against ref[ref_off[p] .. ref_off[p+1]), laid out as for
 * sconf_edit_counts: ids int32, offsets int64 with P + 1 entries, all on the device.
 *   ws, ws_off (P + 1) int64    pair p may use the bytes [ws_off[p], ws_off[p+1]) of ws and touches no others; ws and every ws_off[p]
 *                               of a pair that needs bytes are multiples of 16
 *   hyp_to_ref int32, one per hypothesis id, at the id's position in hyp: the index inside the pair's reference of the id this one
 *                               is aligned to (a hit or a substitution), -1 for an insertion
 *   ref_to_hyp int32, one per reference id, at the id's position in ref: the index inside the pair's hypothesis, -1 for a deletion
 *   counts (P, 4) int64         [errors, substitutions, deletions, insertions]: the bits sconf_edit_counts writes for the same pairs
 * A pair whose slice is smaller than sconf_edit_align_pair_bytes(H, R) (or misaligned), or whose H or R exceeds
 * sconf_edit_align_max_len(), gets -1 in all its map entries and counts = -1, -1, -1, -1, and touches nothing else.  Empty
 * hypotheses and empty references are valid (all insertions, all deletions; they need no workspace); P == 0 launches nothing.
 * One workgroup per pair.  Every element of hyp_to_ref, ref_to_hyp and counts is written; of ws only bytes inside the pairs' slices;
 * nothing else.  0 <= P < 2^31. */
int sconf_edit_align(const int32_t* hyp, const int64_t* hyp_off, const int32_t* ref, const int64_t* ref_off, int64_t P,
                     int32_t* hyp_to_ref, int32_t* ref_to_hyp, int64_t* counts, void* ws, const int64_t* ws_off, sconf_stream_t stream);

/* The most temperatures one call of sconf_calib_frames_sweep takes (16). */
int sconf_calib_max_temps(void);

/* idx (M) int32 and conf (K, M) f32, row k at conf + k * M: conf[k][r] is the measure of sconf_confid.h (methods, norms, alpha and
 * invalid rows all as there) of softmax(inv_temps[k] * x_r); idx is the argmax of sconf_confid_frames, which no temperature moves.
 * x, M, classes, row_stride, method, norm, alpha: as for sconf_confid_frames.  inv_temps (K) f32 on the device, 1 / temperature,
 * each finite and > 0; an entry that is not gives a column of NaN, decided on the device (idx is not touched by it).
 * 1 <= K <= sconf_calib_max_temps(), refused on the host otherwise.
 * In f32, relative to the row maximum m, with c_k = fl(inv_temps[k] * log2 e): the per-element exponential is the hardware's
 * 2^((x - m) c_k) (and 2^((alpha (x - m)) c_k) for the S_a of TSALLIS and RENYI), the sum of the entropy is that of e (x - m), scaled
 * by inv_temps[k] once per row, and the order of summation is that of sconf_confid_frames: the column with inv_temps[k] == 1.0f is
 * sconf_confid_frames on the same input bit for bit.  Each row is read once from memory whatever K is (up to
 * sconf_confid_block_capacity() classes; a longer row is read K + 1 times, all but the first out of the cache), with at most 2 K
 * exponentials per element (K for MAX_PROB and SHANNON).  Row k of conf feeds sconf_confid_aggregate unchanged.
 * Every element of idx and conf is written, nothing else. */
int sconf_calib_frames_sweep(const float* x, int64_t M, int64_t classes, int64_t row_stride, int method, int norm, float alpha,
                             const float* inv_temps, int64_t K, int32_t* idx, float* conf, sconf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SCONF_CALIB_H */
