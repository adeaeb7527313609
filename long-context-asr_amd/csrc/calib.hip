// Calibration unit (include/sconf_calib.h): the edit alignment of ragged pairs of id sequences - which hypothesis ids are hits,
// substitutions and insertions, which reference ids are deleted - and the frame confidences of confid.hip at K softmax temperatures
// from one pass over the rows.
//
// The alignment's forward pass is the min-plus DP of editdist.hip over the packed key  cost * 2^32 + substitutions, in the same
// geometry (one workgroup per pair, AL_CPL columns per lane, rows in skew through the lanes, row blocks handed from wave to wave
// through LDS, one barrier per macro-step, the last column of a pass parked in the workspace), restated here because it also
// stores, per cell, which of the three candidates gave the minimum.  A lane packs the 2-bit directions of its AL_CPL columns of one
// row into one 16-bit word and stores it at [tile][step][lane], so a wave's store is one 128-byte line and no two lanes share a
// word.  The backtrace follows in the same kernel: all lanes copy the tile under the path into LDS, one lane walks it to the tile's
// edge.  A path crosses at most ceil(H / AL_ROWS) + ceil(R / AL_STRIP) tiles and takes H + R dependent LDS reads in all.
//
// Built WITHOUT -ffast-math (see the Makefile), as confid.hip is: the sweep shares confid_measure.h with it and its column at
// temperature 1 must give sconf_confid_frames' bits.
#include "common.h"
#include "../../include/sconf_confid.h"
#include "../../include/sconf_calib.h"
#include "confid_measure.h"

namespace {

// ---- the alignment ------------------------------------------------------------------------------------------------------------------
typedef unsigned long long u64;
constexpr int AL_CPL = 8;                          // reference columns per lane = cells per stored word
constexpr int AL_WAVES = 4;
constexpr int AL_STRIP = 64 * AL_CPL;              // columns per wave: a tile's width
constexpr int AL_PASS = AL_WAVES * AL_STRIP;       // columns per pass of the workgroup
constexpr int AL_ROWS = 256;                       // rows between barriers: a tile's height
constexpr int AL_THREADS = 64 * AL_WAVES;
constexpr int AL_HRING = 8;                        // staged hypothesis blocks: AL_WAVES in use + the one being fetched
constexpr int AL_STEPS = AL_ROWS + 63;             // skewed steps of one tile
constexpr int AL_TILE_WORDS = AL_STEPS * 64;       // 16-bit words of one tile
constexpr int AL_TILE_BYTES = AL_TILE_WORDS * 2;
constexpr int AL_MAX_LEN = 65535;
static_assert(AL_ROWS == AL_THREADS, "one thread stages one row of a block");
static_assert(AL_HRING > AL_WAVES && (AL_HRING & (AL_HRING - 1)) == 0, "ring must hold the blocks in flight");
static_assert(2 * AL_CPL == 16 && AL_TILE_BYTES % 16 == 0, "a lane's directions of one row fill one 16-bit word; tiles are copied in 16-byte pieces");
constexpr u64 AL_STEP = 1ull << 32, AL_SUB = AL_STEP + 1;
enum { DIR_DIAG = 0, DIR_UP = 1, DIR_LEFT = 2 };

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

__host__ __device__ inline long long parked_bytes(long long H, long long R) { return R > AL_PASS ? ((H + 1) * 8 + 15) / 16 * 16 : 0; }
__host__ __device__ inline long long pair_bytes(long long H, long long R) {
    if (H <= 0 || R <= 0) return 0;
    return parked_bytes(H, R) + ((H + AL_ROWS - 1) / AL_ROWS) * ((R + AL_STRIP - 1) / AL_STRIP) * AL_TILE_BYTES;
}

__global__ __launch_bounds__(AL_THREADS) void edit_align_kernel(const int* __restrict__ hyp, const long long* __restrict__ hyp_off,
                                                                const int* __restrict__ ref, const long long* __restrict__ ref_off,
                                                                int* __restrict__ hyp_to_ref, int* __restrict__ ref_to_hyp,
                                                                long long* __restrict__ out, unsigned char* ws, const long long* __restrict__ ws_off) {
    __shared__ int hs[AL_HRING][AL_ROWS];                  // hypothesis ids of the row blocks in flight
    __shared__ u64 bin0[2][AL_ROWS];                       // left boundary of wave 0: column 0, or the parked column of the last pass
    __shared__ u64 bnd[AL_WAVES - 1][2][AL_ROWS];          // last column of wave w for one row block, read by wave w + 1 a macro-step later
    __shared__ __attribute__((aligned(16))) unsigned short tile[AL_TILE_WORDS];      // the backtrace's tile
    const long long p = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long long h0 = hyp_off[p], m = hyp_off[p + 1] - h0, r0 = ref_off[p], n = ref_off[p + 1] - r0;
    int* hm = hyp_to_ref + h0;
    int* rm = ref_to_hyp + r0;
    long long* o = out + p * 4;
    const long long w0 = ws_off[p], need = pair_bytes(m, n);
    const bool refused = m > AL_MAX_LEN || n > AL_MAX_LEN ||
                         (need > 0 && (ws == nullptr || ws_off[p + 1] - w0 < need || w0 < 0 || (((uintptr_t)ws + (uintptr_t)w0) & 15) != 0));
    if (refused || m <= 0 || n <= 0) {                     // refused, or an empty side: all insertions or all deletions
        for (long long i = tid; i < m; i += AL_THREADS) hm[i] = -1;
        for (long long j = tid; j < n; j += AL_THREADS) rm[j] = -1;
        if (tid == 0) {
            if (refused) { o[0] = -1; o[1] = -1; o[2] = -1; o[3] = -1; }
            else write_counts(o, m > n ? m : (n > 0 ? n : 0), 0, m > 0 ? m : 0, n > 0 ? n : 0);
        }
        return;
    }
    u64* col = reinterpret_cast<u64*>(ws + w0);            // col[i - 1] = D[i][first column of the pass]; touched only when n > AL_PASS
    unsigned short* tiles = reinterpret_cast<unsigned short*>(ws + w0 + parked_bytes(m, n));
    const long long nblocks = (m + AL_ROWS - 1) / AL_ROWS, nstrips = (n + AL_STRIP - 1) / AL_STRIP;

    for (long long c0 = 0; c0 < n; c0 += AL_PASS) {
        const bool more = c0 + AL_PASS < n;
        const long long strip0 = c0 + (long long)w * AL_STRIP;             // DP column left of this wave's strip
        const bool live = strip0 < n;                                       // wave-uniform; strips right of the reference idle
        const long long gs = strip0 / AL_STRIP;                             // this wave's strip among the pair's (< nstrips where live)
        const long long lc = strip0 + lane * AL_CPL;                        // DP column left of this lane's run
        int rf[AL_CPL]; u64 up[AL_CPL];
#pragma unroll
        for (int c = 0; c < AL_CPL; ++c) {
            const long long j = lc + c + 1;
            rf[c] = j <= n ? ref[r0 + j - 1] : 0;                           // columns past n compute values nobody reads
            up[c] = (u64)j << 32;                                           // row 0: j deletions
        }
        u64 dl = (u64)lc << 32, last = 0;

        auto stage = [&](long long b) {                                     // block b: ids and wave 0's boundary, one row per thread
            const long long i = b * AL_ROWS + tid + 1;
            if (i <= m) {
                hs[b & (AL_HRING - 1)][tid] = hyp[h0 + i - 1];
                bin0[b & 1][tid] = c0 == 0 ? (u64)i << 32 : col[i - 1];
            }
        };
        stage(0);
        __syncthreads();
        for (long long k = 0; k < nblocks + AL_WAVES - 1; ++k) {
            if (k + 1 < nblocks) stage(k + 1);
            const long long b = k - w;
            if (live && b >= 0 && b < nblocks) {
                const long long left_rows = m - b * AL_ROWS;
                const int rows = left_rows < AL_ROWS ? (int)left_rows : AL_ROWS;
                const int* hb = hs[b & (AL_HRING - 1)];
                const u64* in = w == 0 ? bin0[b & 1] : bnd[w - 1][b & 1];
                u64* ob = bnd[w < AL_WAVES - 1 ? w : 0][b & 1];
                unsigned short* tp = tiles + (b * nstrips + gs) * AL_TILE_WORDS + lane;
                for (int s = 0; s < rows + 63; ++s) {
                    u64 left_in = shfl_up1(last);                           // lane t - 1 finished this row one step ago
                    const int r = s - lane;
                    if ((unsigned)r < (unsigned)rows) {
                        if (lane == 0) left_in = in[r];
                        const int h = hb[r];
                        u64 d = dl, left = left_in;
                        unsigned bits = 0;
#pragma unroll
                        for (int c = 0; c < AL_CPL; ++c) {
                            const u64 cd = d + (h == rf[c] ? 0ull : AL_SUB), cu = up[c] + AL_STEP, cl = left + AL_STEP;
                            const u64 v = min64(min64(cd, cu), cl);
                            bits |= (cd == v ? (unsigned)DIR_DIAG : cu == v ? (unsigned)DIR_UP : (unsigned)DIR_LEFT) << (2 * c);     // the first that reproduces v
                            d = up[c]; up[c] = v; left = v;
                        }
                        tp[s * 64] = (unsigned short)bits;                  // s = r + lane <= AL_STEPS - 1
                        dl = left_in; last = left;
                        if (lane == 63) {
                            if (w < AL_WAVES - 1) ob[r] = left;
                            else if (more) col[b * AL_ROWS + r] = left;
                        }
                    }
                }
            }
            __syncthreads();
        }
        if (!more && live) {
            const long long j = n - lc;                                      // this lane holds column n as its j-th
#pragma unroll
            for (int c = 0; c < AL_CPL; ++c)
                if (j == c + 1) write_counts(o, (long long)(up[c] >> 32), (long long)(up[c] & 0xffffffffull), m, n);
        }
    }

    // the backtrace: (i, j) from (m, n) until a side is used up, a tile at a time
    // Every thread walks the same path out of the tile in LDS (all lanes read one word: a broadcast) and keeps (i, j) in its own
    // registers, made wave-uniform after each tile; thread 0 alone writes the maps.  No state is handed from thread to thread, so
    // both barriers stand in control flow that is uniform for the compiler too.
    int i = (int)m, j = (int)n;                                              // (m, n come from scalar loads: uniform)
    while (i > 0 && j > 0) {
        const int b = (i - 1) / AL_ROWS, gs = (j - 1) / AL_STRIP;
        const long long left_rows = m - (long long)b * AL_ROWS;
        const int pieces = ((left_rows < AL_ROWS ? (int)left_rows : AL_ROWS) + 63) * (64 * 2 / 16);      // the steps the block has, in 16-byte pieces
        const uint4* src = reinterpret_cast<const uint4*>(tiles + ((long long)b * nstrips + gs) * AL_TILE_WORDS);
        __syncthreads();                                                     // the directions are stored / the tile before is walked by all
        for (int k = tid; k < pieces; k += AL_THREADS) reinterpret_cast<uint4*>(tile)[k] = src[k];
        __syncthreads();
        while (i > 0 && j > 0 && (i - 1) / AL_ROWS == b && (j - 1) / AL_STRIP == gs) {
            const int r = (i - 1) % AL_ROWS, q = (j - 1) % AL_STRIP, t = q / AL_CPL, c = q % AL_CPL;
            const int dir = (tile[(r + t) * 64 + t] >> (2 * c)) & 3;
            if (dir == DIR_DIAG) {
                if (tid == 0) { hm[i - 1] = j - 1; rm[j - 1] = i - 1; }
                --i; --j;
            } else if (dir == DIR_UP) {
                if (tid == 0) hm[i - 1] = -1;
                --i;
            } else {
                if (tid == 0) rm[j - 1] = -1;
                --j;
            }
        }
        i = __builtin_amdgcn_readfirstlane(i); j = __builtin_amdgcn_readfirstlane(j);
    }
    for (int k = tid; k < i; k += AL_THREADS) hm[k] = -1;                    // j == 0: up to the corner
    for (int k = tid; k < j; k += AL_THREADS) rm[k] = -1;                    // i == 0: left to the corner
}

// ---- the sweep ----------------------------------------------------------------------------------------------------------------------
constexpr int MAX_TEMPS = 16;

// the three sums of one element d = x - m <= 0 (or -inf) at the exponent scale c = fl(inv_temp * log2 e): add<METHOD> of
// confid_measure.h with its constant replaced; the entropy's sum is scaled by inv_temp once per row
template <int METHOD> __device__ __forceinline__ void add_t(Sums& s, float d, float alpha, float c) {
    const float e = __builtin_amdgcn_exp2f(d * c);
    s.z += e;
    if (METHOD == SCONF_CONFID_SHANNON) s.t += e > 0.f ? e * d : 0.f;
    if (METHOD == SCONF_CONFID_TSALLIS || METHOD == SCONF_CONFID_RENYI) s.a += __builtin_amdgcn_exp2f((alpha * d) * c);
}
__device__ __forceinline__ bool temp_ok(float it) { return it > 0.f && it < INFINITY; }

// frames_group_kernel of confid.hip with the sums repeated per temperature over the row in registers
template <int METHOD, int G, int NQ>
__global__ __launch_bounds__(BLOCK) void sweep_group_kernel(const float* __restrict__ x, long M, int C, long stride, int vec, Measure q,
                                                            const float* __restrict__ inv_temps, int K, int* __restrict__ idx, float* __restrict__ conf) {
    const int g = threadIdx.x & (G - 1);
    long row = (long)blockIdx.x * (BLOCK / G) + threadIdx.x / G;
    const bool live = row < M;
    if (!live) row = M - 1;                                                // a group behind the last row repeats it and stores nothing
    const float* xr = x + row * stride;
    float v[NQ][4];
    Best b{-INFINITY, NO_INDEX};
    bool bad = false;
#pragma unroll
    for (int j = 0; j < NQ; ++j) load_quad(xr, (g + G * j) * 4, C, vec, v[j]);
#pragma unroll
    for (int j = 0; j < NQ; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) { bad |= v[j][e] != v[j][e]; take(b, v[j][e], (g + G * j) * 4 + e); }
    b = group_best<G>(b);
    bad = group_any<G>(bad) || !(fabsf(b.v) < INFINITY);
    if (g == 0 && live) idx[row] = bad ? -1 : b.i;
    for (int k = 0; k < K; ++k) {
        const float it = inv_temps[k], c = it * 1.4426950408889634f;
        Sums s{0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < NQ; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) add_t<METHOD>(s, v[j][e] - b.v, q.alpha, c);
        s.z = group_sum<G>(s.z);
        if (METHOD == SCONF_CONFID_SHANNON) s.t = group_sum<G>(s.t) * it;
        if (METHOD == SCONF_CONFID_TSALLIS || METHOD == SCONF_CONFID_RENYI) s.a = group_sum<G>(s.a);
        if (g == 0 && live) conf[(long)k * M + row] = bad || !temp_ok(it) ? __builtin_nanf("") : confidence<METHOD>(s, q);
    }
}

// frames_block_kernel of confid.hip likewise.  REG: the row stays in the registers of the workgroup; otherwise every temperature
// reads the row again, out of the cache.
template <int METHOD, bool REG>
__global__ __launch_bounds__(BLOCK) void sweep_block_kernel(const float* __restrict__ x, long M, int C, long stride, int vec, Measure q,
                                                            const float* __restrict__ inv_temps, int K, int* __restrict__ idx, float* __restrict__ conf) {
    __shared__ float shv[BLOCK / 64][4];
    __shared__ int shi[BLOCK / 64][2];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long row = blockIdx.x;
    const float* xr = x + row * stride;
    const int nq = (C + 3) / 4;
    float keep[REG ? QUADS : 1][4];
    Best b{-INFINITY, NO_INDEX};
    bool bad = false;
    if (REG) {
#pragma unroll
        for (int j = 0; j < QUADS; ++j) load_quad(xr, (threadIdx.x + BLOCK * j) * 4, C, vec, keep[REG ? j : 0]);
#pragma unroll
        for (int j = 0; j < QUADS; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float t = keep[REG ? j : 0][e]; bad |= t != t; take(b, t, (threadIdx.x + BLOCK * j) * 4 + e); }
    } else {
        for (int k = threadIdx.x; k < nq; k += BLOCK) {
            float v[4];
            load_quad(xr, k * 4, C, vec, v);
#pragma unroll
            for (int e = 0; e < 4; ++e) { bad |= v[e] != v[e]; take(b, v[e], k * 4 + e); }
        }
    }
    b = wave_best(b);
    bad = __any(bad);
    if (lane == 0) { shv[wv][0] = b.v; shi[wv][0] = b.i; shi[wv][1] = bad; }
    __syncthreads();
    b = Best{shv[0][0], shi[0][0]}; bad = shi[0][1];
#pragma unroll
    for (int w = 1; w < BLOCK / 64; ++w) { take(b, shv[w][0], shi[w][0]); bad |= shi[w][1] != 0; }
    bad = bad || !(fabsf(b.v) < INFINITY);
    if (bad) {                                                             // the same for every thread of the workgroup
        if (threadIdx.x == 0) idx[row] = -1;
        if (threadIdx.x < K) conf[(long)threadIdx.x * M + row] = __builtin_nanf("");
        return;
    }
    if (threadIdx.x == 0) idx[row] = b.i;
    for (int k = 0; k < K; ++k) {
        const float it = inv_temps[k], c = it * 1.4426950408889634f;
        Sums s{0.f, 0.f, 0.f};
        if (REG) {
#pragma unroll
            for (int j = 0; j < QUADS; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) add_t<METHOD>(s, keep[REG ? j : 0][e] - b.v, q.alpha, c);
        } else {
            for (int u = threadIdx.x; u < nq; u += BLOCK) {
                float v[4];
                load_quad(xr, u * 4, C, vec, v);
#pragma unroll
                for (int e = 0; e < 4; ++e) add_t<METHOD>(s, v[e] - b.v, q.alpha, c);
            }
        }
        s.z = wave_sum(s.z); s.t = wave_sum(s.t); s.a = wave_sum(s.a);
        __syncthreads();                                                   // the sums of the temperature before have been read
        if (lane == 0) { shv[wv][1] = s.z; shv[wv][2] = s.t; shv[wv][3] = s.a; }
        __syncthreads();
        if (threadIdx.x == 0) {
            Sums r{0.f, 0.f, 0.f};
#pragma unroll
            for (int w = 0; w < BLOCK / 64; ++w) { r.z += shv[w][1]; r.t += shv[w][2]; r.a += shv[w][3]; }
            r.t *= it;
            conf[(long)k * M + row] = temp_ok(it) ? confidence<METHOD>(r, q) : __builtin_nanf("");
        }
    }
}

struct SweepArgs { const float* x; long M; int C; long stride; int vec; Measure q; const float* inv_temps; int K; int* idx; float* conf; hipStream_t st; };

template <int METHOD, int G, int NQ> void sweep_group(const SweepArgs& a) {
    hipLaunchKernelGGL((sweep_group_kernel<METHOD, G, NQ>), dim3((unsigned)cdiv(a.M, BLOCK / G)), dim3(BLOCK), 0, a.st, a.x, a.M, a.C, a.stride, a.vec,
                       a.q, a.inv_temps, a.K, a.idx, a.conf);
}
template <int METHOD, bool REG> void sweep_block(const SweepArgs& a) {
    hipLaunchKernelGGL((sweep_block_kernel<METHOD, REG>), dim3((unsigned)a.M), dim3(BLOCK), 0, a.st, a.x, a.M, a.C, a.stride, a.vec, a.q, a.inv_temps,
                       a.K, a.idx, a.conf);
}
// the row geometries of sconf_confid_frames, class count for class count
template <int METHOD> void launch_sweep(const SweepArgs& a) {
    const int C = a.C;
    if (C <= 64) sweep_group<METHOD, 16, 1>(a);
    else if (C <= 128) sweep_group<METHOD, 16, 2>(a);
    else if (C <= 192) sweep_group<METHOD, 16, 3>(a);
    else if (C <= 256) sweep_group<METHOD, 16, 4>(a);
    else if (C <= 512) sweep_group<METHOD, 64, 2>(a);
    else if (C <= ROW_CAPACITY) sweep_group<METHOD, 64, QUADS>(a);
    else if (C <= BLOCK_CAPACITY) sweep_block<METHOD, true>(a);
    else sweep_block<METHOD, false>(a);
}

}  // namespace

SCONF_API int sconf_edit_align_strip_cols(void) { return AL_STRIP; }
SCONF_API int sconf_edit_align_pass_cols(void) { return AL_PASS; }
SCONF_API int sconf_edit_align_block_rows(void) { return AL_ROWS; }
SCONF_API int sconf_edit_align_cells_per_word(void) { return AL_CPL; }
SCONF_API int sconf_edit_align_tile_bytes(void) { return AL_TILE_BYTES; }
SCONF_API int sconf_edit_align_max_len(void) { return AL_MAX_LEN; }

SCONF_API int64_t sconf_edit_align_pair_bytes(int64_t H, int64_t R) {
    if (H < 0 || R < 0 || H > AL_MAX_LEN || R > AL_MAX_LEN) return -1;
    return pair_bytes(H, R);
}

SCONF_API int sconf_edit_align(const int32_t* hyp, const int64_t* hyp_off, const int32_t* ref, const int64_t* ref_off, int64_t P,
                               int32_t* hyp_to_ref, int32_t* ref_to_hyp, int64_t* counts, void* ws, const int64_t* ws_off, hipStream_t stream) {
    SCONF_REQUIRE(P >= 0 && P < (1ll << 31), "sconf_edit_align: P=%ld out of range", (long)P);
    if (P == 0) return 0;
    SCONF_REQUIRE(hyp_off && ref_off && ws_off && counts, "sconf_edit_align: hyp_off, ref_off, ws_off and counts must not be null");
    SCONF_REQUIRE(((uintptr_t)ws & 15) == 0, "sconf_edit_align: workspace must be 16-byte aligned");
    hipLaunchKernelGGL(edit_align_kernel, dim3((unsigned)P), dim3(AL_THREADS), 0, stream, (const int*)hyp, (const long long*)hyp_off,
                       (const int*)ref, (const long long*)ref_off, (int*)hyp_to_ref, (int*)ref_to_hyp, (long long*)counts, (unsigned char*)ws,
                       (const long long*)ws_off);
    SCONF_LAUNCH_OK("sconf_edit_align");
    return 0;
}

SCONF_API int sconf_calib_max_temps(void) { return MAX_TEMPS; }

SCONF_API int sconf_calib_frames_sweep(const float* x, int64_t M, int64_t classes, int64_t row_stride, int method, int norm, float alpha,
                                       const float* inv_temps, int64_t K, int32_t* idx, float* conf, hipStream_t stream) {
    SCONF_REQUIRE(M >= 0 && M < (1L << 31), "sconf_calib_frames_sweep: M=%ld must be in 0 .. 2^31 - 1", (long)M);
    SCONF_REQUIRE(classes >= 2 && classes < (1L << 30), "sconf_calib_frames_sweep: classes=%ld must be at least 2 (and below 2^30)", (long)classes);
    SCONF_REQUIRE(row_stride >= classes, "sconf_calib_frames_sweep: row stride %ld is below classes=%ld", (long)row_stride, (long)classes);
    SCONF_REQUIRE(row_stride <= (1L << 62) / (M > 0 ? M : 1), "sconf_calib_frames_sweep: M * row_stride must be below 2^62");
    SCONF_REQUIRE(K >= 1 && K <= MAX_TEMPS, "sconf_calib_frames_sweep: K=%ld temperatures; 1 .. %d", (long)K, MAX_TEMPS);
    SCONF_REQUIRE(method >= SCONF_CONFID_MAX_PROB && method <= SCONF_CONFID_RENYI, "sconf_calib_frames_sweep: unknown method %d", method);
    SCONF_REQUIRE(norm == SCONF_CONFID_LIN || norm == SCONF_CONFID_EXP, "sconf_calib_frames_sweep: unknown norm %d", norm);
    SCONF_REQUIRE(!(method == SCONF_CONFID_MAX_PROB && norm == SCONF_CONFID_EXP),
                  "sconf_calib_frames_sweep: max_prob has no exp normalisation: norm must be lin");
    const bool with_alpha = method == SCONF_CONFID_TSALLIS || method == SCONF_CONFID_RENYI;
    if (with_alpha && alpha == 1.f) method = SCONF_CONFID_SHANNON;                // the limit of both, taken here: no 1 / (alpha - 1)
    else SCONF_REQUIRE(!with_alpha || alpha_ok(alpha), "sconf_calib_frames_sweep: alpha=%g must be in (0, 1), 1 or (1, 4]", (double)alpha);
    SCONF_REQUIRE(x && inv_temps && idx && conf, "sconf_calib_frames_sweep: null x, inv_temps, idx or conf");
    if (M == 0) return 0;
    const int vec = ((uintptr_t)x % 16 == 0) && row_stride % 4 == 0;
    const SweepArgs a{x, (long)M, (int)classes, (long)row_stride, vec, measure_of(method, norm, alpha, classes), inv_temps, (int)K, idx, conf, stream};
    switch (method) {
        case SCONF_CONFID_MAX_PROB: launch_sweep<SCONF_CONFID_MAX_PROB>(a); break;
        case SCONF_CONFID_SHANNON: launch_sweep<SCONF_CONFID_SHANNON>(a); break;
        case SCONF_CONFID_TSALLIS: launch_sweep<SCONF_CONFID_TSALLIS>(a); break;
        default: launch_sweep<SCONF_CONFID_RENYI>(a); break;
    }
    SCONF_LAUNCH_OK("sconf_calib_frames_sweep");
    return 0;
}
