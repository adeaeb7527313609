// Edit counts (errors, substitutions, deletions, insertions) of ragged pairs of id sequences: the scoring behind
// word_error_rate_detail (lcasr/eval/wer.py:5-73, which sits on jiwer) and a token error rate straight from sconf_ctc_collapse.
//
// The counts need no alignment memory.  Over the packed key  cost * 2^32 + substitutions  the Levenshtein recurrence is one
// min-plus DP: a diagonal step adds 0 on a match and 2^32 + 1 on a mismatch, a vertical or horizontal step adds 2^32, and the
// plain u64 minimum of the three candidates is the lexicographic minimum of (cost, substitutions).  The final key gives the
// distance and the substitutions of the optimal alignment with the fewest of them; every alignment has ins - del = m - n and
// sub + del + ins = cost, which fixes the other two.
//
// Geometry: one workgroup of ED_WAVES waves per pair.  DP rows are hypothesis ids, DP columns reference ids.  A lane keeps
// ED_CPL consecutive columns of the previous row in registers, a wave the ED_STRIP = 64 * ED_CPL columns next to each other, the
// workgroup ED_PASS columns; a wider reference takes several passes, with the pass's last column (one key per row) parked in
// the workspace and read back as the next pass's left boundary.  Rows stream past the lanes in skew: at step s lane t is on row
// s - t and hands the key of its last column to lane t + 1 by __shfl_up.  Rows are cut into blocks of ED_ROWS: at macro-step
// k wave w works on row block k - w, reads its left boundary (the last column of wave w - 1 for that block) from LDS and leaves
// its own last column there for wave w + 1.  Waves meet at one __syncthreads() per macro-step: no flags, no spinning.
#include "common.h"

namespace {

typedef unsigned long long u64;
constexpr int ED_CPL = 8;                          // reference columns per lane
constexpr int ED_WAVES = 4;
constexpr int ED_STRIP = 64 * ED_CPL;              // columns per wave
constexpr int ED_PASS = ED_WAVES * ED_STRIP;       // columns per pass of the workgroup
constexpr int ED_ROWS = 256;                       // rows between barriers
constexpr int ED_THREADS = 64 * ED_WAVES;
constexpr int ED_HRING = 8;                        // staged hypothesis blocks: ED_WAVES in use + the one being fetched
static_assert(ED_ROWS == ED_THREADS, "one thread stages one row of a block");
static_assert(ED_HRING > ED_WAVES && (ED_HRING & (ED_HRING - 1)) == 0, "ring must hold the blocks in flight");
constexpr u64 ED_STEP = 1ull << 32, ED_SUB = ED_STEP + 1;

__device__ __forceinline__ u64 shfl_up1(u64 v) {
    unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
    lo = __shfl_up(lo, 1, 64); hi = __shfl_up(hi, 1, 64);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 min64(u64 a, u64 b) { return a < b ? a : b; }

__device__ __forceinline__ void write_counts(long long* o, long long cost, long long sub, long long m, long long n) {
    const long long del = (cost - sub - (m - n)) / 2;
    o[0] = cost; o[1] = sub; o[2] = del; o[3] = del + m - n;
}

__global__ __launch_bounds__(ED_THREADS) void edit_counts_kernel(const int* __restrict__ hyp, const long long* __restrict__ hyp_off,
                                                                 const int* __restrict__ ref, const long long* __restrict__ ref_off,
                                                                 long long* __restrict__ out, u64* ws, long long ws_keys) {
    __shared__ int hs[ED_HRING][ED_ROWS];                  // hypothesis ids of the row blocks in flight
    __shared__ u64 bin0[2][ED_ROWS];                       // left boundary of wave 0: column 0, or the parked column of the last pass
    __shared__ u64 bnd[ED_WAVES - 1][2][ED_ROWS];          // last column of wave w for one row block, read by wave w + 1 a macro-step later
    const long long p = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long long h0 = hyp_off[p], m = hyp_off[p + 1] - h0, r0 = ref_off[p], n = ref_off[p + 1] - r0;
    long long* o = out + p * 4;
    if (m <= 0 || n <= 0) {                                 // an empty side: all insertions or all deletions
        if (tid == 0) write_counts(o, m > n ? m : (n > 0 ? n : 0), 0, m > 0 ? m : 0, n > 0 ? n : 0);
        return;
    }
    const long long slot = (h0 - hyp_off[0]) + p;           // pair p parks its column behind those of the pairs before it
    if (n > ED_PASS && (ws == nullptr || slot + m + 1 > ws_keys)) {
        if (tid == 0) { o[0] = -1; o[1] = -1; o[2] = -1; o[3] = -1; }      // workspace too small: reported, nothing overrun
        return;
    }
    u64* col = ws + slot;                                   // col[i - 1] = D[i][first column of the pass]; touched only when n > ED_PASS
    const long long nblocks = (m + ED_ROWS - 1) / ED_ROWS;

    for (long long c0 = 0; c0 < n; c0 += ED_PASS) {
        const bool more = c0 + ED_PASS < n;
        const long long strip0 = c0 + (long long)w * ED_STRIP;             // DP column left of this wave's strip
        const bool live = strip0 < n;                                       // wave-uniform; strips right of the reference idle
        const long long lc = strip0 + lane * ED_CPL;                        // DP column left of this lane's run
        int rf[ED_CPL]; u64 up[ED_CPL];
#pragma unroll
        for (int c = 0; c < ED_CPL; ++c) {
            const long long j = lc + c + 1;
            rf[c] = j <= n ? ref[r0 + j - 1] : 0;                           // columns past n compute values nobody reads
            up[c] = (u64)j << 32;                                           // row 0: j deletions
        }
        u64 dl = (u64)lc << 32, last = 0;

        auto stage = [&](long long b) {                                     // block b: ids and wave 0's boundary, one row per thread
            const long long i = b * ED_ROWS + tid + 1;
            if (i <= m) {
                hs[b & (ED_HRING - 1)][tid] = hyp[h0 + i - 1];
                bin0[b & 1][tid] = c0 == 0 ? (u64)i << 32 : col[i - 1];
            }
        };
        stage(0);
        __syncthreads();
        for (long long k = 0; k < nblocks + ED_WAVES - 1; ++k) {
            if (k + 1 < nblocks) stage(k + 1);
            const long long b = k - w;
            if (live && b >= 0 && b < nblocks) {
                const long long left_rows = m - b * ED_ROWS;
                const int rows = left_rows < ED_ROWS ? (int)left_rows : ED_ROWS;
                const int* hb = hs[b & (ED_HRING - 1)];
                const u64* in = w == 0 ? bin0[b & 1] : bnd[w - 1][b & 1];
                u64* ob = bnd[w < ED_WAVES - 1 ? w : 0][b & 1];
                for (int s = 0; s < rows + 63; ++s) {
                    u64 left_in = shfl_up1(last);                           // lane t - 1 finished this row one step ago
                    const int r = s - lane;
                    if ((unsigned)r < (unsigned)rows) {
                        if (lane == 0) left_in = in[r];
                        const int h = hb[r];
                        u64 d = dl, left = left_in;
#pragma unroll
                        for (int c = 0; c < ED_CPL; ++c) {
                            const u64 t = min64(d + (h == rf[c] ? 0ull : ED_SUB), up[c] + ED_STEP);
                            const u64 v = min64(t, left + ED_STEP);
                            d = up[c]; up[c] = v; left = v;
                        }
                        dl = left_in; last = left;
                        if (lane == 63) {
                            if (w < ED_WAVES - 1) ob[r] = left;
                            else if (more) col[b * ED_ROWS + r] = left;
                        }
                    }
                }
            }
            __syncthreads();
        }
        if (!more && live) {
            const long long j = n - lc;                                      // this lane holds column n as its j-th
#pragma unroll
            for (int c = 0; c < ED_CPL; ++c)
                if (j == c + 1) write_counts(o, (long long)(up[c] >> 32), (long long)(up[c] & 0xffffffffull), m, n);
        }
    }
}

}  // namespace

// Launch geometry (bookkeeping for tests and benchmarks, in the manner of sconf_convmod_tile_frames).
SCONF_API int sconf_edit_strip_cols(void) { return ED_STRIP; }
SCONF_API int sconf_edit_pass_cols(void) { return ED_PASS; }
SCONF_API int sconf_edit_block_rows(void) { return ED_ROWS; }

// Bytes that always suffice for P pairs with at most max_hyp / max_ref ids a side; 0 while no reference needs a second pass.
SCONF_API int64_t sconf_edit_counts_workspace(int64_t P, int64_t max_hyp, int64_t max_ref) {
    if (P < 0 || max_hyp < 0 || max_ref < 0 || max_hyp > (1ll << 30) || max_ref > (1ll << 30)) return -1;
    if (P == 0 || max_ref <= ED_PASS) return 0;
    return P * (max_hyp + 1) * (int64_t)sizeof(u64);
}

SCONF_API int sconf_edit_counts(const int32_t* hyp, const int64_t* hyp_off, const int32_t* ref, const int64_t* ref_off, int64_t P,
                                int64_t* out, void* ws, int64_t ws_bytes, hipStream_t stream) {
    SCONF_REQUIRE(P >= 0 && P < (1ll << 31), "sconf_edit_counts: P=%ld out of range", (long)P);
    if (P == 0) return 0;
    SCONF_REQUIRE(hyp_off && ref_off && out, "sconf_edit_counts: hyp_off, ref_off and out must not be null");
    SCONF_REQUIRE(ws_bytes >= 0 && (ws || ws_bytes == 0), "sconf_edit_counts: workspace of %ld bytes at a null pointer", (long)ws_bytes);
    SCONF_REQUIRE(((uintptr_t)ws & 7) == 0, "sconf_edit_counts: workspace must be 8-byte aligned");
    hipLaunchKernelGGL(edit_counts_kernel, dim3((unsigned)P), dim3(ED_THREADS), 0, stream, (const int*)hyp, (const long long*)hyp_off,
                       (const int*)ref, (const long long*)ref_off, (long long*)out, (u64*)ws, (long long)(ws_bytes / 8));
    SCONF_LAUNCH_OK("sconf_edit_counts");
    return 0;
}
