// bf16 MFMA GEMM, 256x256x64 block tile, 8 waves, for the large projections of the SConformerXL path (same contract and
// epilogues as gemm.hip; chosen by sconf_gemm_bf16 when M and N are multiples of 256 and K of 64).
//
// Why a second kernel: a 128x128 tile moves 2 x 128 x 64 x 2 B = 32 KiB through the CU's 64 B/clk vector-memory path
// for 2 x 128 x 128 x 64 flop, i.e. exactly the time the four SIMDs need for the MFMAs: the load path and the matrix
// cores are co-critical and any stall shows.  A 256x256 tile halves the bytes per flop, and a 128x64 wave tile cuts the
// LDS fragment reads per MFMA from 0.5 to 0.375.
//
// Structure (one workgroup per CU, 128 KiB LDS = 2 K-tile buffers x {A0, A1, B0, B1} half-tile images of 128 x 64):
//  * waves 2 (M) x 4 (N); a wave owns rows {64wr..+63} of BOTH A halves and 32 + 32 columns from the two B halves, so
//    each half-tile image is read in exactly one of the four phases of a K-tile and can be restaged right after it;
//  * a K-tile is 4 phases (one 64 x 32 quadrant of the wave tile each): { fragment ds_reads, one half-tile of LDS-DMA
//    prefetch, counted s_waitcnt vmcnt } -> s_barrier -> 16 MFMA -> s_barrier.  The DMA stream runs 5 phases ahead of
//    its consumer and is never drained inside the loop (raw s_barrier, never __syncthreads);
//  * the two wave rows run one barrier apart (wr = 1 executes one extra s_barrier per work item), so that while one
//    half of the waves is in its MFMA cluster the other half issues its LDS reads and DMA;
//  * persistent workgroups walk (K-split, tile) work items; the prefetch cursor crosses item boundaries, so an item's
//    epilogue stores overlap the next item's first loads.
//
// Hazards, by construction (phase P = 4 * k_tile + q; both wave rows issue their share of a half-tile in their own L_P):
//   WAR  an image read in L_P is restaged in L_(P+2) at the earliest: every reader has passed the lgkmcnt(0) that
//        precedes its MFMAs of phase P, and two barriers lie in between even for the lagging wave row;
//   RAW  the wait at the end of L_P leaves the 4 youngest half-tiles (8 DMA instructions per wave) in flight, so every
//        half-tile issued in phases <= P-4 has landed for the issuing wave; the barrier that ends L_P (L_P of the lagging
//        row included) makes that true for all waves before any L_(P+1) read.  Issue phases: A0, B0 of K-tile s+2 in
//        (s, q2), (s, q3); B1, A1 of K-tile s+1 in (s, q0), (s, q1); read phases: A0/B0 q0, B1 q1, A1 q2 - always >= 5
//        phases after the issue.
//   DMA issue (dma_voff, Cursor below): `buffer_load_dwordx4 ... offen lds` from inline asm (gfx950.h dma_pieces / dma_piece), one
//        statement per half-tile.  Per lane ONE loop-invariant 32-bit offset per operand; the descriptor (one per operand and work
//        ITEM, based at the item's corner of the operand, num_records = what the operand has left from there), the K-tile's offset
//        from that corner, the piece / half steps on top of it and the LDS destination (M0) are scalar: a K-tile step is one scalar
//        add per operand and one subtraction for the LDS slot.  What the asm form changes for the hazards above: nothing in the ORDER - the statements clobber "memory", so the
//        compiler moves no LDS read and no epilogue load or store across an issue or a wait, and every issue sits where the builtin
//        sat - but the compiler no longer counts these loads: vmcnt is in order and shared, the loop holds no vector-memory
//        operation of the compiler's own, and the epilogue's loads are issued after the item's last DMA, so a wait the compiler
//        emits for them also retires the older DMA (it over-waits, never under-waits).  M0 is saved and restored inside each
//        statement; SCC is named as clobbered.
//   Steady loop and tail (ktile in the kernels): the ORDER of issues, waits, barriers, reads and MFMAs above is that of every K-tile;
//        the K-tile exists in two forms that differ only in what surrounds the issues.  A K-tile whose prefetch cursor, two K-tiles
//        ahead, stays inside ITS work item is known to issue all four half-tiles through descriptors that are already built: the
//        steady form has no validity test, a constant vmcnt window, Cursor::step as its advance, and the issue forms without the
//        leading s_nop 4 (its listing holds no VALU write of an SGPR, and 24 LDS reads lie between its entry and the first issue).
//        The run lengths are scalar and known at each crossing; after each run comes ONE K-tile in the general form, in which
//        the cursor crosses into its next item (item_coords' divisions, two 64-bit products, two descriptors) or runs out:
//   Tail  past the workgroup's last item the cursor is invalid: nothing is issued and the wait drains (vmcnt(0)).  The test is one
//        scalar compare and branch per phase of the general form.  (A zero-record descriptor would turn the issue into a no-op with the same vmcnt
//        accounting, but it writes zeros through the LDS-DMA path into the next K-tile's images while the other wave row may still
//        be two barriers behind: safe by the WAR rule above, yet it buys one branch and costs 8 zero-fill pieces per K-tile of the
//        tail - not taken.)
#ifdef SCONF_GEMM_STAMP
#define SCONF_STAMPS                 // gfx950.h: STAMP_DECL / STAMP are live in this file
#endif
#include "gemm_tile.h"
#include <algorithm>
#include <type_traits>
#include <stdio.h>

namespace {
using namespace gemm_tile;

// Tile = 256 rows x (128 + 64 * JH) columns: JH = 2 -> 256x256 (gemm256_kernel); JH = 1 -> 256x192 (gemm192_kernel, NT only),
// which turns the 384 tiles of an N = 768 projection (1.5 rounds over 256 CUs) into 512 (exactly 2 rounds).
constexpr int TM = 256, TK = 64;
constexpr int HT = 128 * 64 * 2;                   // one half-tile image, 16 KiB (B1 of the 192-wide tile uses half of it)
constexpr int BUF = 4 * HT;                        // A0 | A1 | B0 | B1
constexpr int GM2 = 4;                             // row panels per L2 patch (4 x 8 tiles = the 32 workgroups of one XCD);
                                                   // 8 x 4 when the output is >= 8 tiles wide (measured +2-4 % at N >= 2304)

// K-contiguous images are [rows][64 k] with a 16-B-chunk XOR swizzle per row.
// A image: the half's 128 rows in natural order, read 16 consecutive rows at a time.
// B images: a wave owns WC = 32 + 16 * JH tile columns, WC * wc + (0 .. WC-1): the first 32 live in B0 (row 32wc + c), the
//   rest in B1 (row 16 JH wc + c - 32).  A wave reads the PERMUTED row set  base + 8 * (a >> 2) + 4j + (a & 3)  (a = lane & 15;
//   B1 of the 192-wide tile: base + 4 * (a >> 2) + (a & 3)) for column tile j, so that with the MFMA issued operand-swapped
//   lane (r, g) accumulates the 8 consecutive columns 8g .. 8g+7 of the wave's B0 part (and 8 or 4 of its B1 part): each
//   epilogue store instruction then writes 64 contiguous bytes per row.
__device__ __forceinline__ int swz_a(int row) { return (row >> 1) & 7; }
__device__ __forceinline__ int swz_b(int row) { return ((row >> 1) & 1) | (((row >> 3) & 3) << 1); }
__device__ __forceinline__ int swz_b1n(int row) { return ((row >> 1) & 1) | (((row >> 2) & 3) << 1); }   // 64-row B1 image

// ---- LDS-DMA prefetch: one buffer descriptor per operand, everything but one 32-bit offset per lane in scalar registers ----
// A half-tile image is 2 pieces of 512 lanes x 16 B (B1 of the 192-wide tile: 1); piece i of half h reads, for thread tid,
// chunk c = tid + 512 i.  The per-lane source offset of piece 0 of half 0 (dma_voff) is the only per-lane part of the address:
//   K-contiguous (row = c >> 3, 8 chunks of 16 B per row):
//     A           mrow = 128 h + row, swizzle swz_a(row) = (row >> 1) & 7:   piece +64 rows, half +128 rows - bits 1..3 of row untouched;
//     B0 / B1     mrow = WC (row >> 5) + 32 h + (row & 31), swz_b(row) uses bits 1, 3, 4:   piece +64 image rows = +2 WC operand rows, half +32;
//     B, rotary   mrow = 128 (row >> 6) + 32 ((row >> 5) & 1) + 64 h + (row & 31):   piece +128 rows, half +64;
//     B1 of the 192-wide tile is a 64-row image with its own row map and swizzle (swz_b1n): a second per-lane offset, one piece;
//   K-strided (kr = c >> 4, 16 chunks per k-row): kr ld + 128 h + 8 (pos ^ swz_strided(kr)); swz_strided uses bits 0, 1, 3 of kr:
//     piece +32 k-rows, half +256 B.
// Every step is wave-uniform and leaves the XOR swizzle alone, so it lives in an SGPR (the piece step goes through dma_pieces'
// soffset, the half step is the soffset it starts from).  The LDS destination is wave-uniform too: par * BUF + image * HT +
// wave * 1024 (+ 8192 for the second piece), written to M0 from SGPRs.
template <bool KS, bool BOP, int JH> __device__ __forceinline__ unsigned dma_voff(long ld, int tid, bool rot = false, bool narrow_b1 = false) {
    constexpr int WC = 32 + 16 * JH;
    if (KS) {
        const int kr = tid >> 4, pos = tid & 15, rc = pos ^ swz_strided(kr);
        return (unsigned)(((long)kr * ld + rc * 8) * 2);
    }
    const int row = tid >> 3, pos = tid & 7;                       // row < 64
    int kc, mrow;
    if (!BOP)           { kc = pos ^ swz_a(row); mrow = row; }
    else if (narrow_b1) { kc = pos ^ swz_b1n(row); mrow = WC * (row >> 4) + 32 + (row & 15); }
    else                { kc = pos ^ swz_b(row); mrow = rot ? 32 * (row >> 5) + (row & 31) : WC * (row >> 5) + (row & 31); }
    return (unsigned)(((long)mrow * ld + kc * 8) * 2);
}
// wave-uniform byte steps of one operand's images: second piece of a half, second half (A: twice the piece step; K-strided: 256 B -
// derived at the issue, not kept in registers of their own)
template <bool KS, bool BOP, int JH> struct DmaSteps {
    unsigned piece, bhalf;
    __device__ __forceinline__ void set(long ld, bool rot = false) {
        constexpr int WC = 32 + 16 * JH;
        if (KS)        { piece = (unsigned)(32 * ld * 2); bhalf = 256; }
        else if (!BOP) { piece = (unsigned)(64 * ld * 2); bhalf = 0; }
        else           { piece = (unsigned)((rot ? 128 : 2 * WC) * ld * 2); bhalf = (unsigned)((rot ? 64 : 32) * ld * 2); }
    }
    __device__ __forceinline__ unsigned half() const { return KS ? 256u : !BOP ? 2 * piece : bhalf; }
};

// Transposed LDS read as inline asm.  Through the builtin, hipcc puts an unconditional `s_waitcnt vmcnt(0)` in front of the
// reads (it cannot tell them from the in-flight LDS-DMA destinations), which drains the whole prefetch pipeline twice per
// K-tile - the reason the K-strided (weight-gradient) kernel sat parked 57 % of its wave-cycles.  The asm form is invisible to
// that logic AND to the compiler's lgkmcnt tracking: the consumer must run wait_lgkm0() and tie() the result before using it.
__device__ __forceinline__ bf16x4 lds_read_tr(const char* p) {
    bf16x4 v;
    asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(v) : "v"(lds_addr(p)));
    return v;
}
template <int OFF> __device__ __forceinline__ bf16x4 lds_read_tr_off(unsigned a) {
    bf16x4 v;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(a), "n"(OFF));
    return v;
}
// Both k-steps' fragments of one 16-wide block of a K-strided image from ONE per-lane base address: k-step 1 is +32 k-rows
// (8192 B) and the second half of each fragment +4 k-rows (1024 B); the XOR swizzle depends on (k & 3, (k >> 3) & 1), which
// those offsets leave unchanged, so all four reads are base + immediate.
__device__ __forceinline__ void frag_pair_ks(const char* s, int col, int lane, bf16x8& f0, bf16x8& f1) {
    const int a = lane & 15, q = a >> 2, g = lane >> 4;
    const int chunk = col >> 3, sub = (col & 4) * 2, k0 = 8 * g + q;
    const unsigned base = lds_addr(s + k0 * 256 + ((chunk ^ swz_strided(k0)) << 4) + sub);
    const bf16x4 l0 = lds_read_tr_off<0>(base), h0 = lds_read_tr_off<1024>(base);
    const bf16x4 l1 = lds_read_tr_off<8192>(base), h1 = lds_read_tr_off<9216>(base);
    f0 = __builtin_shufflevector(l0, h0, 0, 1, 2, 3, 4, 5, 6, 7);
    f1 = __builtin_shufflevector(l1, h1, 0, 1, 2, 3, 4, 5, 6, 7);
}
// 16 x 32 MFMA fragments.  K-contiguous: one ds_read_b128; K-strided ([64 k][128 cols] image): two transposed reads.
template <bool KS> __device__ __forceinline__ bf16x8 frag_a(const char* s, int wr, int i, int kk, int lane) {
    if (!KS) {
        const int r = 64 * wr + 16 * i + (lane & 15), c = kk * 4 + (lane >> 4);
        return *reinterpret_cast<const bf16x8*>(s + r * 128 + ((c ^ swz_a(r)) << 4));
    } else {
        const int a = lane & 15, q = a >> 2, pp = a & 3, g = lane >> 4;
        const int col = 64 * wr + 16 * i + 4 * pp, chunk = col >> 3, sub = (col & 4) * 2;
        const int k0 = kk * 32 + 8 * g + q, k1 = k0 + 4;
        bf16x4 lo = lds_read_tr(s + k0 * 256 + ((chunk ^ swz_strided(k0)) << 4) + sub);
        bf16x4 hi = lds_read_tr(s + k1 * 256 + ((chunk ^ swz_strided(k1)) << 4) + sub);
        return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    }
}
template <bool KS, bool NARROW> __device__ __forceinline__ bf16x8 frag_b(const char* s, int wc, int j, int kk, int lane) {
    if (!KS) {
        const int a = lane & 15, c = kk * 4 + (lane >> 4);
        if (!NARROW) {
            const int r = 32 * wc + 8 * (a >> 2) + 4 * j + (a & 3);
            return *reinterpret_cast<const bf16x8*>(s + r * 128 + ((c ^ swz_b(r)) << 4));
        } else {
            const int r = 16 * wc + 4 * (a >> 2) + (a & 3);
            return *reinterpret_cast<const bf16x8*>(s + r * 128 + ((c ^ swz_b1n(r)) << 4));
        }
    } else {
        const int a = lane & 15, q = a >> 2, pp = a & 3, g = lane >> 4;
        const int col = 32 * wc + 16 * j + 4 * pp, chunk = col >> 3, sub = (col & 4) * 2;
        const int k0 = kk * 32 + 8 * g + q, k1 = k0 + 4;
        bf16x4 lo = lds_read_tr(s + k0 * 256 + ((chunk ^ swz_strided(k0)) << 4) + sub);
        bf16x4 hi = lds_read_tr(s + k1 * 256 + ((chunk ^ swz_strided(k1)) << 4) + sub);
        return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    }
}

// Work items (K-split, 256x256 tile): XCD-contiguous ids, split-major, GM2 x tiles_n patches (see gemm.hip tile_coords).
struct Item { int m0, n0, kbeg, nkt, split; };
struct Sched { int total, ntiles, tiles_m, tiles_n, tn, gm; };
__device__ __forceinline__ Item item_coords(const GemmParams& p, const Sched& sc, int v) {
    const int qx = sc.total >> 3, rx = sc.total & 7, xcd = v & 7;
    const int lid = (xcd < rx ? xcd * (qx + 1) : rx * (qx + 1) + (xcd - rx) * qx) + (v >> 3);
    const int split = lid / sc.ntiles, t = lid - split * sc.ntiles;
    const int per_group = sc.gm * sc.tiles_n;
    const int g = t / per_group, r = t - g * per_group;
    const int first_m = g * sc.gm, gm = min(sc.gm, sc.tiles_m - first_m);
    Item w;
    w.m0 = (first_m + r % gm) * TM; w.n0 = (r / gm) * sc.tn;
    w.split = split;
    w.kbeg = split * p.k_per_split;
    w.nkt = (min(p.K, w.kbeg + p.k_per_split) - w.kbeg) / TK;
    return w;
}
// One past the last byte of each operand, the K-tile steps of the prefetch stream and the sum of the wave's two LDS slots
// (wave-uniform, set once per launch).
template <bool KS> struct DmaGeom {
    const char* aend; const char* bend; unsigned astep, bstep, ldsum;
    __device__ __forceinline__ void set(const GemmParams& p, unsigned ldsw) {
        aend = reinterpret_cast<const char*>(p.A) + (KS ? (long)(p.K - 1) * p.lda + p.M : (long)(p.M - 1) * p.lda + p.K) * 2;
        bend = reinterpret_cast<const char*>(p.B) + (KS ? (long)(p.K - 1) * p.ldb + p.N : (long)(p.N - 1) * p.ldb + p.K) * 2;
        astep = KS ? (unsigned)(TK * p.lda * 2) : TK * 2; bstep = KS ? (unsigned)(TK * p.ldb * 2) : TK * 2;   // (not used by far launches)
        ldsum = 2 * ldsw + BUF;
    }
};
// descriptor over [base, end), num_records clamped to 4 GiB - 1 by the high word of the distance.  The high word passes through
// tie_s: written as a plain 64-bit comparison it becomes v_cmp_lt_u64 (there is no scalar one) - two VALU instructions per descriptor.
__device__ __forceinline__ srd_t dma_srd(const char* base, const char* end) {
    const unsigned long left = (unsigned long)(end - base);
    const unsigned hi = tie_s((unsigned)(left >> 32));
    return make_srd_uniform(base, hi ? 0xffffffffL : (long)(unsigned)left);
}
// Position in the workgroup's stream of K-tiles (all wave-uniform, i.e. SGPRs; `valid` is an int so that it is tested as a scalar, not
// as a lane mask).  The DMA is issued through ONE buffer descriptor per operand and work item, da / db, built by seek() (the stream's
// only multiplies) and based at the ITEM's corner of the operand.  The prefetch runs into the next item while the current one is
// still being computed, so the descriptors belong to the cursor.  Inside an item a K-tile step is one scalar add on the operand's
// offset from that corner, oa / ob (K-contiguous: the same 128 bytes for both, kept once), which goes into the instruction's scalar
// offset with the half and piece steps on top; `lds` is the wave's slot in the buffer the K-tile lands in, flipped by one subtraction.
// num_records is what the operand has left from the item's corner, and the range check takes the scalar offset in (a descriptor
// shortened by the item's K-tile steps reads zeros for the last rows of the operand's last tile - measured): an indexing error in
// any part of the offset reads zeros, never memory past the tensor - the guarantee the per-K-tile descriptors gave.
// FAR launches (far_launch below, decided on the host; an instantiation of their own): an item's offsets do not fit 32 bits.  There
// pa / pb follow the K-TILE's corner with 64-bit adds, the descriptors are rebuilt from them per K-tile and oa / ob stay 0 - paid by
// those launches only: operands of any size, and K-strided items whose k-range times ld passes 4 GiB, stay on this kernel.
// step() is advance() for a K-tile that is known to stay inside the cursor's item of a launch that is not far: no test, no branch; it
// leaves kt to the caller, who adds a whole run of steps at once.
template <bool KS, bool FAR> struct Cursor {
    int v, kt, valid; Item it;
    unsigned lds, oa, ob;
    srd_t da, db;
    const char* pa; const char* pb;                                   // FAR only
    __device__ __forceinline__ unsigned offb() const { return KS ? ob : oa; }
    __device__ __forceinline__ void seek(const GemmParams& p, const DmaGeom<KS>& g) {
        const char* ca = reinterpret_cast<const char*>(p.A) + (KS ? (long)it.kbeg * p.lda + it.m0 : (long)it.m0 * p.lda + it.kbeg) * 2;
        const char* cb = reinterpret_cast<const char*>(p.B) + (KS ? (long)it.kbeg * p.ldb + it.n0 : (long)it.n0 * p.ldb + it.kbeg) * 2;
        da = dma_srd(ca, g.aend); db = dma_srd(cb, g.bend);
        oa = 0; ob = 0;
        if (FAR) { pa = ca; pb = cb; }
    }
    __device__ __forceinline__ void step(const DmaGeom<KS>& g) {
        lds = g.ldsum - lds;
        oa += g.astep;
        if (KS) ob += g.bstep;
    }
    __device__ __forceinline__ void advance(const GemmParams& p, const Sched& sc, const DmaGeom<KS>& g) {
        lds = g.ldsum - lds;
        if (++kt < it.nkt) {
            if (!FAR) { oa += g.astep; if (KS) ob += g.bstep; }
            else {
                pa += (KS ? (long)TK * p.lda * 2 : (long)TK * 2); pb += (KS ? (long)TK * p.ldb * 2 : (long)TK * 2);
                da = dma_srd(pa, g.aend); db = dma_srd(pb, g.bend);
            }
            return;
        }
        kt = 0; v += gridDim.x;
        if (v < sc.total) { it = item_coords(p, sc, v); seek(p, g); } else valid = 0;
    }
    // how many step()s may follow from here: K-tiles left in the cursor's item after this one
    __device__ __forceinline__ int run() const { return valid && !FAR ? it.nkt - 1 - kt : 0; }
};

// Epilogue of one work item for one wave (ACT and the presence of a residual fixed at compile time).  All loads are issued
// before the stores they could queue behind: the bias run once, the aux tile (bf16) per half of 4 row blocks, the residual
// (f32) per pair of row blocks - as far ahead as the 256-VGPR budget beside the 128 accumulator registers allows.
template <int W> struct RawBf;
template <> struct RawBf<8> { typedef bf16x8 type; };
template <> struct RawBf<4> { typedef bf16x4 type; };
template <int ACT, bool RES, bool KS, int JH, int FL = -1, bool ROT = false, int DEEP = 0>
__device__ __forceinline__ void epilogue256(const GemmParams& p, const f32x4 (&acc)[2][4][2 + JH], const Item& it, int wr, int wc, int lane) {
    constexpr int WC = 32 + 16 * JH, WH = 4 * JH;
    constexpr bool AUX = ACT == SCONF_ACT_DGELU || ACT == SCONF_ACT_DSILU || ACT == SCONF_ACT_MULAUX || ACT == SCONF_ACT_SMAXBWD;
    constexpr bool SMB = ACT == SCONF_ACT_SMAXBWD;    // softmax backward: per-row scalar in, column sums out
    const int g = lane >> 4, mbase = it.m0 + 64 * wr + (lane & 15);
    if constexpr (ROT) {
        // qkv projection with the rotary rotation: with the rot row permutation (dma_voff) the lane's lo run is (head, d0 .. d0 + 7)
        // and its hi run (head, d0 + 64 ..): out[d] = x[d] cos - x[d + 64] sin, out[d + 64] = x[d + 64] cos + x[d] sin
        // (apply_rotary_pos_emb, rotary_emb.py:61-73) on the f32 accumulators - one bf16 rounding instead of two.  Tiles past
        // rot_cols (the v block) are stored as they are.  cos / sin of the next row block are requested before this one is stored.
        static_assert(JH == 2 && !RES && !AUX && ACT == SCONF_ACT_NONE && FL >= 0 && !(FL & 2), "rotary epilogue: 256-wide tile, plain bf16 output");
        const int d0 = 32 * (wc & 1) + 8 * g;
        const int nlo = it.n0 + 128 * (wc >> 1) + d0, nhi = nlo + 64;
        float blo[8], bhi[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { blo[e] = 0.f; bhi[e] = 0.f; }
        if (FL & 1) { loadv<8>(p.bias + nlo, blo); loadv<8>(p.bias + nhi, bhi); }
        const bool rot = it.n0 < p.rot_cols;                                       // uniform over the workgroup
        const long crow0 = (long)mbase * p.ldc;
        float cs[2][8], sn[2][8];
        auto fetch = [&](int rb, int slot) {
            const int pos = (mbase + 128 * (rb >> 2) + 16 * (rb & 3)) % p.rot_n;
            loadv<8>(p.rot_cos + (long)pos * 64 + d0, cs[slot]); loadv<8>(p.rot_sin + (long)pos * 64 + d0, sn[slot]);
        };
        if (rot) fetch(0, 0);
#pragma unroll
        for (int rb = 0; rb < 8; ++rb) {
            if (rot && rb + 1 < 8) fetch(rb + 1, (rb + 1) & 1);
            const int h = rb >> 2, i = rb & 3, sl = rb & 1;
            float lo[8], hi[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) { lo[e] = acc[h][i][e >> 2][e & 3] + blo[e]; hi[e] = acc[h][i][2 + (e >> 2)][e & 3] + bhi[e]; }
            if (rot) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float a = lo[e], b = hi[e];
                    lo[e] = a * cs[sl][e] - b * sn[sl][e]; hi[e] = b * cs[sl][e] + a * sn[sl][e];
                }
            }
            const long crow = crow0 + (long)(128 * h + 16 * i) * p.ldc;
            storev<8>(reinterpret_cast<bf16*>(p.C) + crow + nlo, lo); storev<8>(reinterpret_cast<bf16*>(p.C) + crow + nhi, hi);
        }
        return;
    }
    if constexpr (!KS) {
        const int nlo = it.n0 + WC * wc + 8 * g, nhi = it.n0 + WC * wc + 32 + WH * g;
        float blo[8], bhi[WH];
#pragma unroll
        for (int e = 0; e < 8; ++e) blo[e] = 0.f;
#pragma unroll
        for (int e = 0; e < WH; ++e) bhi[e] = 0.f;
        if (FL >= 0 ? (FL & 1) != 0 : p.bias != nullptr) { loadv<8>(p.bias + nlo, blo); loadv<WH>(p.bias + nhi, bhi); }
        const long crow0 = (long)mbase * p.ldc, prow0 = (long)mbase * p.ldpre;      // per-lane row offsets; the rest is wave-uniform
        if constexpr (FL >= 0 && (RES || ACT == SCONF_ACT_MULAUX || SMB)) {
            // Software-pipelined over the 8 row blocks: residual / aux loads are issued blocks ahead of the math and stores that
            // use them, so by the time they are needed the stores they queue behind have long drained.  (Loading each pair of blocks right after the previous pair's stores made every pair wait for a full
            // store round trip: 38-41 k cycles for an f32 + residual tile against ~8 k for a bf16 one.)
            constexpr int NB = 8;                             // row blocks
            // register slots for blocks in flight (f32 residual: 16 VGPRs per block, aux: 8).  DEEP (the one-epilogue kernels, which have
            // ~30 VGPRs to spare): all aux blocks / 3-4 residual blocks requested up front - one exposed round trip instead of two.
            constexpr int NS = DEEP ? (RES ? (JH == 2 ? 4 : 5) : 8) : (RES ? (JH == 2 ? 2 : 3) : 5);
            constexpr bool FIXED = RES || DEEP;              // fixed look-ahead of NS - 1 blocks
            float rl[NS][8], rh[NS][WH];
            typename RawBf<8>::type xl[NS];
            typename RawBf<WH>::type xh[NS];
            float rowv[NS], cslo[8], cshi[WH];
            if constexpr (SMB) {
#pragma unroll
                for (int e = 0; e < 8; ++e) cslo[e] = 0.f;
#pragma unroll
                for (int e = 0; e < WH; ++e) cshi[e] = 0.f;
            }
            auto fetch = [&](int rb, int slot) {
                const int row = mbase + 128 * (rb >> 2) + 16 * (rb & 3);
                if constexpr (SMB) rowv[slot] = p.rowv[row];
                if constexpr (RES) { const float* q = p.resid + (long)row * p.ldr; loadv<8>(q + nlo, rl[slot]); loadv<WH>(q + nhi, rh[slot]); }
                if constexpr (AUX) {
                    const bf16* q = p.aux + (long)row * p.ldaux;
                    xl[slot] = *reinterpret_cast<const typename RawBf<8>::type*>(q + nlo);
                    xh[slot] = *reinterpret_cast<const typename RawBf<WH>::type*>(q + nhi);
                }
            };
#pragma unroll
            for (int nb = 0; nb < (FIXED ? NS - 1 : 1); ++nb) fetch(nb, nb);
            // Aux tiles (bf16, 8 VGPRs per block): the look-ahead GROWS - blocks 1 | 2,3 | 4,5 | 6,7 are requested before blocks
            // 0 | 1 | 2 | 3 are processed, so after the first two round trips every remaining load is already in flight (one block
            // ahead throughout left 8 exposed round trips: 25 k cycles for the aux tile of an FF dgrad item).
#pragma unroll
            for (int rb = 0; rb < NB; ++rb) {
                {
                    // residual (arch-VGPR bound): fixed look-ahead of NS - 1 blocks; aux only: the growing schedule
                    const int lo_b = FIXED ? rb + NS - 1 : (rb == 0 ? 1 : 2 * rb), hi_b = FIXED ? rb + NS - 1 : 2 * rb + 1;
#pragma unroll
                    for (int nb = lo_b; nb <= hi_b; ++nb) if (nb < NB) fetch(nb, nb % NS);
                }
                const int h = rb >> 2, i = rb & 3, sl = rb % NS;
                float vlo[8], vhi[WH], alo[8], ahi[WH], zlo[8], zhi[WH];
#pragma unroll
                for (int e = 0; e < 8; ++e) { vlo[e] = acc[h][i][e >> 2][e & 3]; alo[e] = AUX ? (float)xl[sl][e] : 0.f; zlo[e] = RES ? rl[sl][e] : (SMB ? rowv[sl] : 0.f); }
#pragma unroll
                for (int e = 0; e < WH; ++e) { vhi[e] = acc[h][i][2 + (e >> 2)][e & 3]; ahi[e] = AUX ? (float)xh[sl][e] : 0.f; zhi[e] = RES ? rh[sl][e] : (SMB ? rowv[sl] : 0.f); }
                const long crow = crow0 + (long)(128 * h + 16 * i) * p.ldc, prow = prow0 + (long)(128 * h + 16 * i) * p.ldpre;
                epi_math_store_at<8, ACT, FL>(p, vlo, blo, alo, zlo, crow + nlo, prow + nlo, it.split);
                epi_math_store_at<WH, ACT, FL>(p, vhi, bhi, ahi, zhi, crow + nhi, prow + nhi, it.split);
                if constexpr (SMB) {                           // (epi_math_store_at leaves the stored values in vlo / vhi)
#pragma unroll
                    for (int e = 0; e < 8; ++e) cslo[e] += vlo[e];
#pragma unroll
                    for (int e = 0; e < WH; ++e) cshi[e] += vhi[e];
                }
            }
            if constexpr (SMB) {
                // column sums of the wave's 128 rows: the 16 lanes of a DPP row hold 16 different rows of the same columns - butterfly
                // (quad swaps, half-row mirror, row mirror), then lane 0 of each row stores its 8 + WH sums to the wave row's slab line
                auto row_sum = [](float v) {
                    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true));
                    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, true));
                    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, true));
                    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, true));
                    return v;
                };
#pragma unroll
                for (int e = 0; e < 8; ++e) cslo[e] = row_sum(cslo[e]);
#pragma unroll
                for (int e = 0; e < WH; ++e) cshi[e] = row_sum(cshi[e]);
                if ((lane & 15) == 0) {
                    float* q = p.colslab + (long)(2 * (it.m0 / TM) + wr) * p.N;
                    storev<8>(q + nlo, cslo); storev<WH>(q + nhi, cshi);
                }
            }
            return;
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            typename RawBf<8>::type axlo[4];
            typename RawBf<WH>::type axhi[4];
            if constexpr (AUX) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const bf16* q = p.aux + (long)(mbase + 128 * h + 16 * i) * p.ldaux;
                    axlo[i] = *reinterpret_cast<const typename RawBf<8>::type*>(q + nlo);
                    axhi[i] = *reinterpret_cast<const typename RawBf<WH>::type*>(q + nhi);
                }
            }
#pragma unroll
            for (int i2 = 0; i2 < 4; i2 += 2) {
                float rlo[2][8], rhi[2][WH];
#pragma unroll
                for (int ii = 0; ii < 2; ++ii) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) rlo[ii][e] = 0.f;
#pragma unroll
                    for (int e = 0; e < WH; ++e) rhi[ii][e] = 0.f;
                    if constexpr (RES) {
                        const float* q = p.resid + (long)(mbase + 128 * h + 16 * (i2 + ii)) * p.ldr;
                        loadv<8>(q + nlo, rlo[ii]); loadv<WH>(q + nhi, rhi[ii]);
                    }
                }
#pragma unroll
                for (int ii = 0; ii < 2; ++ii) {
                    const int i = i2 + ii;
                    float vlo[8], vhi[WH], alo[8], ahi[WH];
#pragma unroll
                    for (int e = 0; e < 8; ++e) { vlo[e] = acc[h][i][e >> 2][e & 3]; alo[e] = AUX ? (float)axlo[i][e] : 0.f; }
#pragma unroll
                    for (int e = 0; e < WH; ++e) { vhi[e] = acc[h][i][2 + (e >> 2)][e & 3]; ahi[e] = AUX ? (float)axhi[i][e] : 0.f; }
                    const long crow = crow0 + (long)(128 * h + 16 * i) * p.ldc, prow = prow0 + (long)(128 * h + 16 * i) * p.ldpre;
                    epi_math_store_at<8, ACT, FL>(p, vlo, blo, alo, rlo[ii], crow + nlo, prow + nlo, it.split);
                    epi_math_store_at<WH, ACT, FL>(p, vhi, bhi, ahi, rhi[ii], crow + nhi, prow + nhi, it.split);
                }
            }
        }
    } else {
        // K-strided operands keep natural column order: 4 consecutive columns per lane and 16x16 tile (plain epilogue only)
        const int nb = it.n0 + 32 * wc + 4 * g;
        const int ncol[4] = {nb, nb + 16, nb + 128, nb + 144};
        float zero[4] = {0.f, 0.f, 0.f, 0.f}, bs[4][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int e = 0; e < 4; ++e) bs[j][e] = 0.f;
            if (p.bias) loadv<4>(p.bias + ncol[j], bs[j]);
        }
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float v[4] = {acc[h][i][j][0], acc[h][i][j][1], acc[h][i][j][2], acc[h][i][j][3]};
                    epi_math_store<4, ACT>(p, v, bs[j], zero, zero, mbase + 128 * h + 16 * i, ncol[j], it.split);
                }
    }
}

// One specialised, contiguous epilogue per (activation, residual, bias, output type) combination the model's NT GEMMs use;
// `kind` is computed once per launch (wave-uniform), everything else takes the runtime-flag path.
//   0 bf16 plain   1 bf16 + bias   2 f32 + residual   3 f32 + residual + bias   4 gelu' save (no bias)   5 * aux   6 generic
//   7 bf16 + rotary   8 bf16 + bias + rotary   (256-wide tile only)
//   9 f32 + residual + bias, acc + bias also saved in bf16 (the self-conditioning reprojection)   10 softmax backward: (acc - rowv) * aux + column sums
//   11 f32 plain   12 f32 + bias   (the head's logits, the subsampler's output projection)
//   - 9 .. 12 live only in kernel instantiations of their own (template parameter EK): in the common kernels their register needs made
//     hipcc spill loop-carried values around EVERY item's epilogue (18 VGPRs to scratch, reloaded behind a vmcnt(0))
__host__ __device__ __forceinline__ int epilogue_kind(const GemmParams& p) {
    if (p.rot_cos) return p.bias ? 8 : 7;                        // (the launcher has checked everything else)
    const bool b = p.bias != nullptr, unit = p.alpha == 1.f;   // kinds 0, 1, 4 skip the alpha * v + residual step (the FF dgrad, kind 5, carries the branch scale in alpha)
    if (p.act == SCONF_ACT_GELU_DSAVE) return (!b && !p.out_f32 && !p.resid && unit) ? 4 : 6;
    if (p.act == SCONF_ACT_MULAUX) return (!b && !p.out_f32 && !p.resid && !p.pre) ? 5 : 6;
    if (p.act == SCONF_ACT_SMAXBWD) return 10;                  // (the launcher has checked everything else)
    if (p.act == SCONF_ACT_NONE && p.pre && p.out_f32 && p.resid && b) return 9;
    if (p.act != SCONF_ACT_NONE || p.pre) return 6;
    if (!p.out_f32 && !p.resid) return unit ? (b ? 1 : 0) : 6;
    if (p.out_f32 && p.resid) return b ? 3 : 2;
    if (p.out_f32 && unit) return b ? 12 : 11;
    return 6;
}
#define EPILOGUE_NT(JH_)                                                                                              \
    switch (ekind) {                                                                                                  \
        case 0: epilogue256<SCONF_ACT_NONE, false, false, JH_, 4>(p, acc, cit, wr, wc, lane); break;                  \
        case 1: epilogue256<SCONF_ACT_NONE, false, false, JH_, 5>(p, acc, cit, wr, wc, lane); break;                  \
        case 2: epilogue256<SCONF_ACT_NONE, true, false, JH_, 2>(p, acc, cit, wr, wc, lane); break;                   \
        case 3: epilogue256<SCONF_ACT_NONE, true, false, JH_, 3>(p, acc, cit, wr, wc, lane); break;                   \
        case 4: epilogue256<SCONF_ACT_GELU_DSAVE, false, false, JH_, 4>(p, acc, cit, wr, wc, lane); break;            \
        case 5: epilogue256<SCONF_ACT_MULAUX, false, false, JH_, 0>(p, acc, cit, wr, wc, lane); break;                \
        case 7: if constexpr (JH_ == 2) epilogue256<SCONF_ACT_NONE, false, false, JH_, 0, true>(p, acc, cit, wr, wc, lane); break;  \
        case 8: if constexpr (JH_ == 2) epilogue256<SCONF_ACT_NONE, false, false, JH_, 1, true>(p, acc, cit, wr, wc, lane); break;  \
        default:                                                                                                      \
            if (p.act == SCONF_ACT_GELU_DSAVE)  epilogue256<SCONF_ACT_GELU_DSAVE, false, false, JH_>(p, acc, cit, wr, wc, lane); \
            else if (p.act == SCONF_ACT_MULAUX) epilogue256<SCONF_ACT_MULAUX, false, false, JH_>(p, acc, cit, wr, wc, lane);     \
            else if (p.resid)                   epilogue256<SCONF_ACT_NONE, true, false, JH_>(p, acc, cit, wr, wc, lane);        \
            else                                epilogue256<SCONF_ACT_NONE, false, false, JH_>(p, acc, cit, wr, wc, lane);       \
    }

// One kernel instantiation per specialised epilogue (template parameter EK = the kind): a kernel that holds ONE epilogue is allocated
// for that epilogue alone (206-226 VGPRs, no SGPR spills, against 255 + 6 for the kernel that switches between all of them).
#ifndef DEEPV
#define DEEPV 1
#endif
#define EPILOGUE_ONE(EK_, JH_)                                                                                        \
    do {                                                                                                              \
        if constexpr (EK_ == 0) epilogue256<SCONF_ACT_NONE, false, false, JH_, 4>(p, acc, cit, wr, wc, lane);         \
        else if constexpr (EK_ == 1) epilogue256<SCONF_ACT_NONE, false, false, JH_, 5>(p, acc, cit, wr, wc, lane);    \
        else if constexpr (EK_ == 2) epilogue256<SCONF_ACT_NONE, true, false, JH_, 2, false, DEEPV>(p, acc, cit, wr, wc, lane);     \
        else if constexpr (EK_ == 3) epilogue256<SCONF_ACT_NONE, true, false, JH_, 3, false, DEEPV>(p, acc, cit, wr, wc, lane);     \
        else if constexpr (EK_ == 4) epilogue256<SCONF_ACT_GELU_DSAVE, false, false, JH_, 4>(p, acc, cit, wr, wc, lane); \
        else if constexpr (EK_ == 5) epilogue256<SCONF_ACT_MULAUX, false, false, JH_, 0, false, DEEPV>(p, acc, cit, wr, wc, lane);  \
        else if constexpr (EK_ == 7) epilogue256<SCONF_ACT_NONE, false, false, JH_, 0, true>(p, acc, cit, wr, wc, lane); \
        else if constexpr (EK_ == 8) epilogue256<SCONF_ACT_NONE, false, false, JH_, 1, true>(p, acc, cit, wr, wc, lane); \
        else if constexpr (EK_ == 9) epilogue256<SCONF_ACT_NONE, true, false, JH_, 11, false, DEEPV>(p, acc, cit, wr, wc, lane);    \
        else if constexpr (EK_ == 11) epilogue256<SCONF_ACT_NONE, false, false, JH_, 6>(p, acc, cit, wr, wc, lane);   \
        else if constexpr (EK_ == 12) epilogue256<SCONF_ACT_NONE, false, false, JH_, 7>(p, acc, cit, wr, wc, lane);   \
        else epilogue256<SCONF_ACT_SMAXBWD, false, false, JH_, 4, false, DEEPV>(p, acc, cit, wr, wc, lane);                         \
    } while (0)

// In-kernel time stamps (gfx950.h), DIAGNOSTIC build only (make EXTRA=-DSCONF_GEMM_STAMP; tools/gemm_stamp.py):
// per wave, cycle sums of the fragment reads, the LDS-DMA issue, the counted wait, the waits at the two barriers of a phase, the
// MFMA clusters and the epilogue.  Nothing of it exists in the product build.
#ifdef SCONF_GEMM_STAMP
__device__ unsigned long long g_gemm_stamps[256 * 8 * 8];
#define STAMP_OUT do { if ((threadIdx.x & 63) == 0 && blockIdx.x < 256) for (int i_ = 0; i_ < 8; ++i_) g_gemm_stamps[((long)blockIdx.x * 8 + (threadIdx.x >> 6)) * 8 + i_] = st_acc_[i_]; } while (0)
#else
#define STAMP_OUT
#endif
// leave the 4 youngest half-tiles in flight: 2 + 2 + 2 + JH DMA instructions per wave
constexpr std::true_type STEADY{};                 // tags of the two K-tile forms (ktile in the kernels)
constexpr std::false_type TAIL{};
template <int JH> __device__ __forceinline__ void wait_window(bool streaming) {
    if (!streaming) wait_vm<0>();
    else if (JH == 2) wait_vm<8>();
    else wait_vm<7>();
}

template <bool KS, int EK = -1, bool FAR = false>
__global__ __launch_bounds__(512) void gemm256_kernel(const GemmParams p) {
    constexpr int JH = 2, TN = 256;
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [2][A0 | A1 | B0 | B1], 128 KiB: the ONLY LDS object
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;
    Sched sc;
    sc.tn = TN; sc.tiles_n = p.N / TN; sc.tiles_m = p.M / TM; sc.ntiles = sc.tiles_m * sc.tiles_n; sc.total = sc.ntiles * p.splits; sc.gm = sc.tiles_n >= 8 ? 2 * GM2 : GM2;
    if ((int)blockIdx.x >= sc.total) return;

    const int ekind = __builtin_amdgcn_readfirstlane(epilogue_kind(p));
    // LDS-DMA prefetch (dma_voff above): per lane one offset per operand; descriptor, steps and LDS destination are scalar
    const bool rotb = !KS && p.rot_cos != nullptr;
    const unsigned va = dma_voff<KS, false, JH>(p.lda, tid), vb = dma_voff<KS, true, JH>(p.ldb, tid, rotb);
    DmaSteps<KS, false, JH> sa; DmaSteps<KS, true, JH> sb; sa.set(p.lda); sb.set(p.ldb, rotb);
    const unsigned ldsw = lds_addr(smem) + wave * 1024;
    DmaGeom<KS> geo; geo.set(p, ldsw);
    // one half-tile through the cursor's descriptor; the image offset is added to the wave's slot as a literal at the issue (tie_s: else
    // the compiler hoists one sum per image).  steady (the K-tiles of the steady loop below): the cursor is known valid - no test.
    auto issue_a = [&](const Cursor<KS, FAR>& c, int h, auto steady) __attribute__((always_inline)) {
        if constexpr (decltype(steady)::value) dma_pieces_s<2, 8192>(c.da, va, c.oa + h * sa.half(), sa.piece, tie_s(c.lds) + h * HT);
        else if (c.valid) dma_pieces<2, 8192>(c.da, va, c.oa + h * sa.half(), sa.piece, tie_s(c.lds) + h * HT);
    };
    auto issue_b = [&](const Cursor<KS, FAR>& c, int h, auto steady) __attribute__((always_inline)) {
        if constexpr (decltype(steady)::value) dma_pieces_s<2, 8192>(c.db, vb, c.offb() + h * sb.half(), sb.piece, tie_s(c.lds) + (2 + h) * HT);
        else if (c.valid) dma_pieces<2, 8192>(c.db, vb, c.offb() + h * sb.half(), sb.piece, tie_s(c.lds) + (2 + h) * HT);
    };

    f32x4 acc[2][4][2 + JH];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2 + JH; ++j) acc[h][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    Cursor<KS, FAR> pc;                               // prefetch cursor
    pc.v = blockIdx.x; pc.kt = 0; pc.lds = ldsw; pc.valid = 1; pc.it = item_coords(p, sc, pc.v); pc.seek(p, geo);
    int cv = pc.v; Item cit = pc.it;                  // compute position
    // prologue: K-tile 0 entirely, A0/B0 of K-tile 1 (the "phases -6 .. -1" of the schedule)
    issue_a(pc, 0, TAIL); issue_b(pc, 0, TAIL); issue_b(pc, 1, TAIL); issue_a(pc, 1, TAIL);
    pc.advance(p, sc, geo);
    issue_a(pc, 0, TAIL); issue_b(pc, 0, TAIL);
    if (pc.valid) wait_window<JH>(true);             // A0, B0 of K-tile 0 have landed
    else wait_vm<4>();
    __builtin_amdgcn_s_barrier();

    int cur = 0;
    bf16x8 fa[4][2], blo[2][2], bhi[JH][2];
    STAMP_DECL(8)
    while (true) {
        if (wr) __builtin_amdgcn_s_barrier();         // stagger the second wave row by one barrier
        // One K-tile.  steady: every issue of it is known valid and its advance stays inside the cursor's item (Cursor::step) - no
        // validity test, no drain, no item crossing; otherwise the general form with all of them.
        auto ktile = [&](auto steady, const bool last) __attribute__((always_inline)) {
            constexpr bool ST = decltype(steady)::value;
            const char* buf = smem + cur * BUF;
            // ---- q0: B-lo, A-lo -> acc[0][.][0..1] ---------------------------------------------------------------
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if constexpr (KS) frag_pair_ks(buf + 2 * HT, 32 * wc + 16 * j + 4 * (lane & 3), lane, blo[j][0], blo[j][1]);
                else {
#pragma unroll
                    for (int kk = 0; kk < 2; ++kk) blo[j][kk] = frag_b<KS, false>(buf + 2 * HT, wc, j, kk, lane);
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if constexpr (KS) frag_pair_ks(buf, 64 * wr + 16 * i + 4 * (lane & 3), lane, fa[i][0], fa[i][1]);
                else {
#pragma unroll
                    for (int kk = 0; kk < 2; ++kk) fa[i][kk] = frag_a<KS>(buf, wr, i, kk, lane);
                }
            }
            STAMP(6);
            issue_b(pc, 1, steady);
            STAMP(7);
            wait_window<JH>(ST || pc.valid);
            STAMP(0);
            __builtin_amdgcn_s_barrier();
            STAMP(1);
            if constexpr (KS) {
                wait_lgkm0();
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
                    for (int j = 0; j < 2; ++j) tie(blo[j][kk]);
#pragma unroll
                    for (int i = 0; i < 4; ++i) tie(fa[i][kk]);
                }
            }
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[0][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(blo[j][kk], fa[i][kk], acc[0][i][j], 0, 0, 0);
            __builtin_amdgcn_s_setprio(0);
            STAMP(2);
            __builtin_amdgcn_s_barrier();
            STAMP(3);
            // ---- q1: B-hi -> acc[0][.][2..3] ---------------------------------------------------------------------
#pragma unroll
            for (int j = 0; j < JH; ++j) {
                if constexpr (KS) frag_pair_ks(buf + 3 * HT, 32 * wc + 16 * j + 4 * (lane & 3), lane, bhi[j][0], bhi[j][1]);
                else {
#pragma unroll
                    for (int kk = 0; kk < 2; ++kk) bhi[j][kk] = frag_b<KS, false>(buf + 3 * HT, wc, j, kk, lane);
                }
            }
            STAMP(6);
            issue_a(pc, 1, steady);
            STAMP(7);
            wait_window<JH>(ST || pc.valid);
            STAMP(0);
            __builtin_amdgcn_s_barrier();
            STAMP(1);
            if constexpr (KS) {
                wait_lgkm0();
#pragma unroll
                for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                    for (int j = 0; j < JH; ++j) tie(bhi[j][kk]);
            }
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < JH; ++j)
                        acc[0][i][2 + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bhi[j][kk], fa[i][kk], acc[0][i][2 + j], 0, 0, 0);
            __builtin_amdgcn_s_setprio(0);
            STAMP(2);
            __builtin_amdgcn_s_barrier();
            STAMP(3);
            // ---- q2: A-hi -> acc[1][.][2..3] ---------------------------------------------------------------------
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if constexpr (KS) frag_pair_ks(buf + HT, 64 * wr + 16 * i + 4 * (lane & 3), lane, fa[i][0], fa[i][1]);
                else {
#pragma unroll
                    for (int kk = 0; kk < 2; ++kk) fa[i][kk] = frag_a<KS>(buf + HT, wr, i, kk, lane);
                }
            }
            if constexpr (ST) pc.step(geo); else pc.advance(p, sc, geo);
            STAMP(6);
            issue_a(pc, 0, steady);
            STAMP(7);
            wait_window<JH>(ST || pc.valid);
            STAMP(0);
            __builtin_amdgcn_s_barrier();
            STAMP(1);
            if constexpr (KS) {
                wait_lgkm0();
#pragma unroll
                for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                    for (int i = 0; i < 4; ++i) tie(fa[i][kk]);
            }
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < JH; ++j)
                        acc[1][i][2 + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bhi[j][kk], fa[i][kk], acc[1][i][2 + j], 0, 0, 0);
            __builtin_amdgcn_s_setprio(0);
            STAMP(2);
            __builtin_amdgcn_s_barrier();
            STAMP(3);
            // ---- q3: (B-lo still in registers) -> acc[1][.][0..1] ------------------------------------------------
            STAMP(6);
            issue_b(pc, 0, steady);
            STAMP(7);
            wait_window<JH>(ST || pc.valid);
            STAMP(0);
            __builtin_amdgcn_s_barrier();
            STAMP(1);
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[1][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(blo[j][kk], fa[i][kk], acc[1][i][j], 0, 0, 0);
            __builtin_amdgcn_s_setprio(0);
            STAMP(2);
            if (!(wr && last)) __builtin_amdgcn_s_barrier();   // the lagging row goes straight into its epilogue
            STAMP(3);
            cur ^= 1;
        };
        // The stream of this item's K-tiles: runs of steady K-tiles - as many as the cursor, two K-tiles ahead, has left in ITS item -
        // each followed by one general K-tile, in which the cursor crosses into its next item or runs out (far launches: all general).
        for (int kt = 0; kt < cit.nkt;) {
            const int run = min(cit.nkt - kt, pc.run());
            pc.kt += run;
            for (const int kend = kt + run; kt < kend; ++kt) ktile(STEADY, kt == cit.nkt - 1);
            if (kt < cit.nkt) { ktile(TAIL, kt == cit.nkt - 1); ++kt; }
        }
        // ---- epilogue: both wave rows concurrently; one specialised, contiguous code path per (activation, residual) ------
        if constexpr (KS) epilogue256<SCONF_ACT_NONE, false, true, JH>(p, acc, cit, wr, wc, lane);
        else if constexpr (EK >= 0) EPILOGUE_ONE(EK, JH);
        else EPILOGUE_NT(JH);
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2 + JH; ++j) acc[h][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        STAMP(4);                                    // epilogue (+ accumulator clears)
        __builtin_amdgcn_s_barrier();                 // re-align the two wave rows
        STAMP(5);
        cv += gridDim.x;
        if (cv >= sc.total) break;
        cit = item_coords(p, sc, cv);
    }
    wait_vm<0>();
    STAMP_OUT;
}

// ---- 256x192 tile, NT, THREE phases per K-tile -------------------------------------------------------------------------
// The 4-phase schedule above on a 192-wide tile (retired, DESIGN) had MFMA clusters of 16 / 8 / 8 / 16 (the hi column half is
// one 16-wide tile per wave), so in the two short phases the other wave row's load section outlasted the MFMAs.  With both A
// quadrants resident (32 more VGPRs; the 192-wide tile has 32 fewer accumulators) the K-tile folds into three 16-MFMA phases:
//   P0  read B-lo, A-lo     issue A1, B1 of K-tile s+1    MFMA  A-lo x B-lo
//   P1  read B-hi, A-hi     -                             MFMA  A-lo x B-hi, A-hi x B-hi
//   P2  -                   issue A0, B0 of K-tile s+2    MFMA  A-hi x B-lo
// WAR: A0/B0 are read in P0 and restaged in P2 of the same K-tile, A1/B1 are read in P1 and restaged in P0 of the next one -
// two phases after the read, as above.  RAW: 7 DMA instructions per wave and K-tile (2 + 2 + 2 + 1); the wait at the end of
// a phase leaves the 7 youngest in flight, which retires A0/B0(s+2) at the end of P2(s+1) and A1/B1(s+2) at the end of
// P0(s+2) - each one phase (and one barrier, two for the lagging wave row's partner) before its first read.
template <int EK = -1>
__global__ __launch_bounds__(512) void gemm192_kernel(const GemmParams p) {
    constexpr int JH = 1, WC = 48, TN = 192;
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [2][A0 | A1 | B0 | B1], the ONLY LDS object
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;
    Sched sc;
    sc.tn = TN; sc.tiles_n = p.N / TN; sc.tiles_m = p.M / TM; sc.ntiles = sc.tiles_m * sc.tiles_n; sc.total = sc.ntiles * p.splits; sc.gm = sc.tiles_n >= 8 ? 2 * GM2 : GM2;
    if ((int)blockIdx.x >= sc.total) return;

    const int ekind = __builtin_amdgcn_readfirstlane(epilogue_kind(p));
    constexpr bool KS = false;
    const unsigned va = dma_voff<KS, false, JH>(p.lda, tid), vb = dma_voff<KS, true, JH>(p.ldb, tid);
    const unsigned vb1 = dma_voff<KS, true, JH>(p.ldb, tid, false, true);          // the 64-row B1 image: own row map and swizzle
    DmaSteps<KS, false, JH> sa; DmaSteps<KS, true, JH> sb; sa.set(p.lda); sb.set(p.ldb);
    const unsigned ldsw = lds_addr(smem) + wave * 1024;
    DmaGeom<KS> geo; geo.set(p, ldsw);
    // one half-tile through the cursor's descriptor (gemm256_kernel has the notes); B1 is a single piece with its own per-lane offset
    auto issue_a = [&](const Cursor<KS, false>& c, int h, auto steady) __attribute__((always_inline)) {
        if constexpr (decltype(steady)::value) dma_pieces_s<2, 8192>(c.da, va, c.oa + h * sa.half(), sa.piece, tie_s(c.lds) + h * HT);
        else if (c.valid) dma_pieces<2, 8192>(c.da, va, c.oa + h * sa.half(), sa.piece, tie_s(c.lds) + h * HT);
    };
    auto issue_b = [&](const Cursor<KS, false>& c, int h, auto steady) __attribute__((always_inline)) {
        if constexpr (decltype(steady)::value) {
            if (h == 0) dma_pieces_s<2, 8192>(c.db, vb, c.oa, sb.piece, tie_s(c.lds) + 2 * HT);
            else        dma_piece_s(c.db, vb1, c.oa, tie_s(c.lds) + 3 * HT);
        } else if (c.valid) {
            if (h == 0) dma_pieces<2, 8192>(c.db, vb, c.oa, sb.piece, tie_s(c.lds) + 2 * HT);
            else        dma_piece(c.db, vb1, c.oa, tie_s(c.lds) + 3 * HT);
        }
    };

    f32x4 acc[2][4][3];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) acc[h][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    Cursor<KS, false> pc;                             // prefetch cursor: the K-tile whose A0/B0 were issued last
    pc.v = blockIdx.x; pc.kt = 0; pc.lds = ldsw; pc.valid = 1; pc.it = item_coords(p, sc, pc.v); pc.seek(p, geo);
    int cv = pc.v; Item cit = pc.it;
    // prologue: K-tile 0 entirely, A0/B0 of K-tile 1
    issue_a(pc, 0, TAIL); issue_b(pc, 0, TAIL); issue_a(pc, 1, TAIL); issue_b(pc, 1, TAIL);
    pc.advance(p, sc, geo);
    issue_a(pc, 0, TAIL); issue_b(pc, 0, TAIL);
    if (pc.valid) wait_vm<7>(); else wait_vm<3>();           // A0, B0 of K-tile 0 have landed
    __builtin_amdgcn_s_barrier();

    int cur = 0;
    bf16x8 flo[4][2], fhi[4][2], blo[2][2], bhi[2];
    while (true) {
        if (wr) __builtin_amdgcn_s_barrier();         // stagger the second wave row by one barrier
        // One K-tile.  steady: every issue of it is known valid and its advance stays inside the cursor's item (Cursor::step) - no
        // validity test, no drain, no item crossing; otherwise the general form with all of them.
        auto ktile = [&](auto steady, const bool last) __attribute__((always_inline)) {
            constexpr bool ST = decltype(steady)::value;
            const char* buf = smem + cur * BUF;
            // ---- P0 ------------------------------------------------------------------------------------------------
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) blo[j][kk] = frag_b<false, false>(buf + 2 * HT, wc, j, kk, lane);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) flo[i][kk] = frag_a<false>(buf, wr, i, kk, lane);
            issue_a(pc, 1, steady); issue_b(pc, 1, steady);             // pc = K-tile s+1
            wait_window<JH>(ST || pc.valid);
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[0][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(blo[j][kk], flo[i][kk], acc[0][i][j], 0, 0, 0);
            __builtin_amdgcn_s_setprio(0);
            __builtin_amdgcn_s_barrier();
            // ---- P1 ------------------------------------------------------------------------------------------------
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) bhi[kk] = frag_b<false, true>(buf + 3 * HT, wc, 0, kk, lane);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) fhi[i][kk] = frag_a<false>(buf + HT, wr, i, kk, lane);
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    acc[0][i][2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bhi[kk], flo[i][kk], acc[0][i][2], 0, 0, 0);
                    acc[1][i][2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bhi[kk], fhi[i][kk], acc[1][i][2], 0, 0, 0);
                }
            __builtin_amdgcn_s_setprio(0);
            __builtin_amdgcn_s_barrier();
            // ---- P2 ------------------------------------------------------------------------------------------------
            if constexpr (ST) pc.step(geo); else pc.advance(p, sc, geo);   // pc = K-tile s+2
            issue_a(pc, 0, steady); issue_b(pc, 0, steady);
            wait_window<JH>(ST || pc.valid);
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[1][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(blo[j][kk], fhi[i][kk], acc[1][i][j], 0, 0, 0);
            __builtin_amdgcn_s_setprio(0);
            if (!(wr && last)) __builtin_amdgcn_s_barrier();   // the lagging row goes straight into its epilogue
            cur ^= 1;
        };
        // The stream of this item's K-tiles: runs of steady K-tiles - as many as the cursor, two K-tiles ahead, has left in ITS item -
        // each followed by one general K-tile, in which the cursor crosses into its next item or runs out (far launches: all general).
        for (int kt = 0; kt < cit.nkt;) {
            const int run = min(cit.nkt - kt, pc.run());
            pc.kt += run;
            for (const int kend = kt + run; kt < kend; ++kt) ktile(STEADY, kt == cit.nkt - 1);
            if (kt < cit.nkt) { ktile(TAIL, kt == cit.nkt - 1); ++kt; }
        }
        if constexpr (EK >= 0) EPILOGUE_ONE(EK, JH);
        else EPILOGUE_NT(JH);
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) acc[h][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        __builtin_amdgcn_s_barrier();                 // re-align the two wave rows
        cv += gridDim.x;
        if (cv >= sc.total) break;
        cit = item_coords(p, sc, cv);
    }
    wait_vm<0>();
}

}  // namespace

// Tile width for the NT layout: fewest "rounds x width" over the CUs (ties -> the wider tile); 0 = not eligible.
static int pick_width(const GemmParams& p, int layout, int cus) {
    if (p.M % TM || p.K % TK || p.k_per_split % TK) return 0;                 // whole tiles only: the kernels floor M / TM and K / TK
    if (p.rot_cos) return (layout == 0 && p.N % 256 == 0) ? 256 : 0;          // the rotary epilogue exists for the 256-wide tile
    long best = 0; int bw = 0;
    for (int w : {256, 192}) {
        if (p.N % w || (w == 192 && layout != 0)) continue;
        const long items = (long)(p.M / TM) * (p.N / w) * p.splits;
        const long cost = ((items + cus - 1) / cus) * w * (w == 192 ? 9 : 8);   // the 192-wide tile runs ~12 % below the 256 one per flop
        if (!bw || cost < best) { best = cost; bw = w; }
    }
    return bw;
}

// K-strided launches whose per-item offsets do not fit the 32-bit offset fields of the LDS-DMA (Cursor): the last K-tile of an item
// starts (k - 64) ld elements from the item's corner, its second piece 32 ld further, and a lane's own offset is at most 63 ld + 256 -
// (k + 32) ld elements and 1 KiB bound the sum.  (K-contiguous items span 2 K bytes, far below the limit that fits32 below sets.)
static bool far_launch(const GemmParams& p) {
    return ((long)p.k_per_split + 32) * std::max(p.lda, p.ldb) * 2 + 1024 > 0xffffffffL;
}

bool sconf_gemm256_eligible(const GemmParams& p, int layout) {
    if (layout != 0 && layout != 2) return false;
    const bool ks = layout == 2;
    // specialised epilogues: NT {plain, +residual, GELU_DSAVE, MULAUX} (bias / pre-save / f32 output in any of them); TN plain
    if (ks ? (p.act != SCONF_ACT_NONE || p.resid || p.pre)
           : !(p.act == SCONF_ACT_NONE || ((p.act == SCONF_ACT_GELU_DSAVE || p.act == SCONF_ACT_MULAUX) && !p.resid) ||
               (p.act == SCONF_ACT_SMAXBWD && !p.resid && !p.bias && !p.out_f32 && !p.pre && p.splits == 1))) return false;
    // The 32-bit offset fields of the LDS-DMA (per-lane voffset + scalar soffset, against a descriptor that the kernel bases at
    // the item's corner of the operand with 64-bit arithmetic): the farthest 16 bytes of one K-tile's pair of half-tiles end
    // (255 ld + 64) * 2 bytes from the K-tile's corner for a K-contiguous operand (256 rows x 64 k) and (63 ld + 256) * 2 for a
    // K-strided one (64 k-rows x 256), and num_records is at most 2^32 - 1.  An item's K-tiles add 2 K bytes at most to the former
    // (counted below) and are far_launch's business for the latter.  The operand's size does not enter: operands beyond 4 GiB and
    // K-strided items whose k-range times ld passes 4 GiB stay on this kernel.
    auto fits32 = [&](long ld) { return (ks ? 63 * ld + 256 : 255 * ld + 64 + p.K) * 2 <= 0xffffffffL; };
    if (!fits32(p.lda) || !fits32(p.ldb)) return false;
    const int cus = num_cus();
    const int w = pick_width(p, layout, cus);
    if (!w || (p.act == SCONF_ACT_SMAXBWD && w != 256)) return false;
    // one workgroup per CU: below ~3/4 of a round the 128x128 kernel (2 per CU, 4x the tiles) fills the chip better
    return (long)(p.M / TM) * (p.N / w) * p.splits * 4 >= 3L * cus;
}

int sconf_gemm256_width(const GemmParams& p, int layout) { return pick_width(p, layout, num_cus()); }

int sconf_gemm256_launch(const GemmParams& p, int layout, hipStream_t stream) {
    static bool attr_set = false;
    const size_t shmem = 2 * BUF;
    lds_limit_once(attr_set, {(const void*)gemm256_kernel<false>, (const void*)gemm256_kernel<true>, (const void*)gemm256_kernel<true, -1, true>,
                             (const void*)gemm256_kernel<false, 0>, (const void*)gemm256_kernel<false, 1>, (const void*)gemm256_kernel<false, 2>,
                             (const void*)gemm256_kernel<false, 3>, (const void*)gemm256_kernel<false, 4>, (const void*)gemm256_kernel<false, 5>,
                             (const void*)gemm256_kernel<false, 7>, (const void*)gemm256_kernel<false, 8>, (const void*)gemm256_kernel<false, 9>,
                             (const void*)gemm256_kernel<false, 10>, (const void*)gemm256_kernel<false, 11>, (const void*)gemm256_kernel<false, 12>,
                             (const void*)gemm192_kernel<11>, (const void*)gemm192_kernel<12>, (const void*)gemm192_kernel<-1>, (const void*)gemm192_kernel<0>,
                             (const void*)gemm192_kernel<1>, (const void*)gemm192_kernel<2>, (const void*)gemm192_kernel<3>, (const void*)gemm192_kernel<4>,
                             (const void*)gemm192_kernel<5>, (const void*)gemm192_kernel<9>}, shmem);
    const int cus = num_cus();
    const int w = pick_width(p, layout, cus);
    const int total = (p.M / TM) * (p.N / w) * p.splits;
    dim3 grid(std::min(total, cus)), block(512);
    // NT: one kernel instantiation per specialised epilogue kind; the kernel that switches (EK = -1) takes kind 6
    const int ek = layout == 2 ? -1 : epilogue_kind(p);
#define L256(EK_) hipLaunchKernelGGL((gemm256_kernel<false, EK_>), grid, block, shmem, stream, p)
#define L192(EK_) hipLaunchKernelGGL(gemm192_kernel<EK_>, grid, block, shmem, stream, p)
    if (layout == 2) {
        if (far_launch(p)) hipLaunchKernelGGL((gemm256_kernel<true, -1, true>), grid, block, shmem, stream, p);
        else               hipLaunchKernelGGL((gemm256_kernel<true>), grid, block, shmem, stream, p);
    }
    else if (w == 256) {
        switch (ek) {
            case 0: L256(0); break; case 1: L256(1); break; case 2: L256(2); break; case 3: L256(3); break; case 4: L256(4); break;
            case 5: L256(5); break; case 7: L256(7); break; case 8: L256(8); break; case 9: L256(9); break; case 10: L256(10); break;
            case 11: L256(11); break; case 12: L256(12); break;
            default: L256(-1);
        }
    } else {
        switch (ek) {
            case 0: L192(0); break; case 1: L192(1); break; case 2: L192(2); break; case 3: L192(3); break; case 4: L192(4); break;
            case 5: L192(5); break; case 9: L192(9); break; case 11: L192(11); break; case 12: L192(12); break;
            default: L192(-1);
        }
    }
#undef L256
#undef L192
    SCONF_LAUNCH_OK("sconf_gemm_bf16 (256-row tile)");
#ifdef SCONF_GEMM_STAMP
    if (getenv("SCONF_GEMM_STAMP_PRINT") && (layout == 2 || w == 256)) {
        (void)hipStreamSynchronize(stream);
        static unsigned long long hb[256 * 8 * 8];
        (void)hipMemcpyFromSymbol(hb, HIP_SYMBOL(g_gemm_stamps), sizeof(hb));
        const int nwg = std::min(total, 256);
        const double ktiles = (double)total / nwg * (p.k_per_split / TK);           // K-tiles per workgroup
        static const char* nm[8] = {"vmcnt wait", "barrier 1", "MFMA cluster", "barrier 2", "epilogue", "re-align", "frag reads", "DMA issue"};
        for (int g = 0; g < 2; ++g) {
            double sums[8] = {}, tot = 0;
            for (int wg = 0; wg < nwg; ++wg) for (int wv = 4 * g; wv < 4 * g + 4; ++wv) for (int i = 0; i < 8; ++i) sums[i] += (double)hb[(wg * 8 + wv) * 8 + i];
            for (int i = 0; i < 8; ++i) tot += sums[i];
            fprintf(stderr, "[gemm256 %s M=%d N=%d K=%d stamps] wave row %d: cycles per K-tile %.0f:", layout == 2 ? "TN" : "NT", p.M, p.N, p.K, g, tot / (nwg * 4.0 * ktiles));
            for (int i = 0; i < 8; ++i) fprintf(stderr, "  %s %.0f (%.1f%%)", nm[i], sums[i] / (nwg * 4.0 * ktiles), 100.0 * sums[i] / tot);
            fprintf(stderr, "\n");
        }
    }
#endif
    return 0;
}
