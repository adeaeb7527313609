// CTC keyword search (include/sconf_kws.h): a list of keywords and the log-scores of a recording become timed, scored hits.
//
// Two kernels.  kws_gather_kernel is the only pass over x (B, N, C): per frame the row maximum over `classes` columns, then
// llr = x - max of the U columns the keyword set uses, into a compact (B, N, Upad) table in the workspace.  Row geometries as
// confid.hip: 16 lanes per row up to 256 classes, a wave per row up to 1024, a workgroup per row above, 16-byte loads where the row
// allows them.  kws_walk_kernel gives one wave to 64 lanes of the keyword image and one sample: lane = one lattice state of one
// keyword, the neighbours' (score, start) by a one-lane DPP shift taken once and twice, masked by the image's flags, the lane's llr of the next PREFETCH
// frames held in registers (the addresses depend on no state), the non-maximum suppression of a keyword in the registers of its
// LAST lane, which alone writes that keyword's slots.  No LDS, no barrier, no atomics.
//
// Built WITHOUT -ffast-math (see the Makefile): -inf is a value here, v != v is the NaN test, and every comparison keeps its meaning.
// The arithmetic is one f32 subtraction and one f32 addition per step, so there is nothing to contract.
#include "common.h"
#include "../../include/sconf_kws.h"

namespace {

constexpr int MAX_LABELS = 32;                 // 2 * 32 - 1 = 63 states: one wave
constexpr int PREFETCH = 8;                    // frames of llr a lane holds ahead
constexpr int MAX_HITS = 1024;
constexpr int BLOCK = 256;
constexpr int WAVES = BLOCK / 64;              // image waves per workgroup of the walk
constexpr long MAX_COLUMNS = 1L << 20;

__device__ __forceinline__ void load_quad(const float* __restrict__ xr, int c, int classes, int vec, float (&v)[4]) {
    if (vec && c + 4 <= classes) load4(xr + c, v);
    else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = c + e < classes ? xr[c + e] : -INFINITY;
    }
}

// the compact row of one frame: thread `me` of `team` takes the quads me, me + team, ...  Column j of the table is llr of the class
// columns[j] (-1: the blank of the call; anything else clamped into the classes); the columns behind U hold -inf.
__device__ __forceinline__ void write_row(const float* __restrict__ xr, float m, bool bad, const int* __restrict__ columns, int U, int Upad,
                                          int classes, int blank, float* __restrict__ out, int vst, int me, int team) {
    for (int q = me; q < Upad / 4; q += team) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = q * 4 + e;
            const int c0 = columns[min(j, U - 1)];
            const int c = c0 < 0 ? blank : min(c0, classes - 1);
            const float d = (xr[c] - m) + 0.f;                             // (+ 0: a -0, from a row whose maximum is both +0 and -0, becomes +0)
            v[e] = (j < U && !bad) ? d : -INFINITY;
        }
        if (vst) store4(out + q * 4, v);
        else {
#pragma unroll
            for (int e = 0; e < 4; ++e) out[q * 4 + e] = v[e];
        }
    }
}

// A row in the registers of GL lanes (16: four rows per wave; 64: one row per wave); lane g holds the quads g, g + GL, ...
template <int GL, int NQ>
__global__ __launch_bounds__(BLOCK) void kws_gather_kernel(const float* __restrict__ x, long M, int classes, long stride, int vec,
                                                           const int* __restrict__ columns, int U, int Upad, int blank,
                                                           float* __restrict__ tab, int vst) {
    const int g = threadIdx.x & (GL - 1);
    long row = (long)blockIdx.x * (BLOCK / GL) + threadIdx.x / GL;
    const bool live = row < M;
    if (!live) row = M - 1;                                                // a group behind the last row repeats it and stores nothing
    const float* xr = x + row * stride;
    float v[NQ][4];
#pragma unroll
    for (int j = 0; j < NQ; ++j) load_quad(xr, (g + GL * j) * 4, classes, vec, v[j]);
    float m = -INFINITY;
    int bad = 0;
#pragma unroll
    for (int j = 0; j < NQ; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) { bad |= v[j][e] != v[j][e]; m = fmaxf(m, v[j][e]); }
#pragma unroll
    for (int o = GL / 2; o > 0; o >>= 1) { m = fmaxf(m, __shfl_xor(m, o, 64)); bad |= __shfl_xor(bad, o, 64); }
    const bool dead = bad || !(fabsf(m) < INFINITY);                       // a NaN, a +inf, or nothing finite
    if (live) write_row(xr, m, dead, columns, U, Upad, classes, blank, tab + row * Upad, vst, g, GL);
}

// A row above the wave's capacity: one workgroup per row, thread t takes the quads t, t + 256, ...
__global__ __launch_bounds__(BLOCK) void kws_gather_block_kernel(const float* __restrict__ x, int classes, long stride, int vec,
                                                                 const int* __restrict__ columns, int U, int Upad, int blank,
                                                                 float* __restrict__ tab, int vst) {
    __shared__ float shm[WAVES];
    __shared__ int shb[WAVES];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long row = blockIdx.x;
    const float* xr = x + row * stride;
    const int nq = (classes + 3) / 4;
    float m = -INFINITY;
    int bad = 0;
    for (int k = threadIdx.x; k < nq; k += BLOCK) {
        float v[4];
        load_quad(xr, k * 4, classes, vec, v);
#pragma unroll
        for (int e = 0; e < 4; ++e) { bad |= v[e] != v[e]; m = fmaxf(m, v[e]); }
    }
    m = wave_max(m);
    bad = __any(bad);
    if (lane == 0) { shm[wv] = m; shb[wv] = bad; }
    __syncthreads();
    m = shm[0]; bad = shb[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) { m = fmaxf(m, shm[w]); bad |= shb[w]; }
    const bool dead = bad || !(fabsf(m) < INFINITY);
    write_row(xr, m, dead, columns, U, Upad, classes, blank, tab + row * Upad, vst, threadIdx.x, BLOCK);
}

// A pair (v, b) as ONE unsigned 64-bit key whose order is the pair order (larger v, then smaller b).  Every score here is -inf, a
// negative number or +0 (an llr is x - max <= 0 and the table holds no -0, see write_row; sums of such are such), and among those a
// larger value has SMALLER bits, so ~bits(v) rises with v; ~b rises as b falls.  One 64-bit compare and two selects per candidate
// instead of three compares, their combination and two selects; the bits of v come back out of the key unchanged.
__device__ __forceinline__ unsigned long long key_of(unsigned hi, unsigned lo) { return ((unsigned long long)hi << 32) | lo; }
__device__ __forceinline__ void take(unsigned long long& best, unsigned long long cand, bool allowed) {
    best = (allowed & (cand > best)) ? cand : best;
}

// The value of the lane below (wave_shr:1 as a DPP modifier: a register move, where __shfl_up goes through the LDS crossbar); lane 0
// keeps its own, as __shfl_up does.  Applied twice it gives the lane two below; there the lanes 0 AND 1 differ from __shfl_up(., 2),
// which no SKIP lane of a valid image sits on (a SKIP lane is state 2 or more of its keyword).
__device__ __forceinline__ unsigned lane_below(unsigned x) { return (unsigned)__builtin_amdgcn_update_dpp((int)x, (int)x, 0x138, 0xf, 0xf, false); }

__global__ __launch_bounds__(BLOCK) void kws_walk_kernel(const float* __restrict__ tab, const int* __restrict__ image,
                                                         const int* __restrict__ in_len, int* __restrict__ hit_frames,
                                                         float* __restrict__ hit_score, int* __restrict__ hit_count, int n_waves, int U,
                                                         int Upad, int K, int cap, int N) {
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (w >= n_waves) return;                                              // (the whole wave alike)
    const int b = blockIdx.y;
    const int* rec = image + ((long)w * 64 + lane) * 4;
    const int u0 = rec[0];
    const bool idle = u0 < 0;
    const int u = min(max(u0, 0), U - 1);                                  // every index of the image is clamped to the call's sizes
    const int flags = idle ? 0 : rec[1];
    const bool first = flags & SCONF_KWS_FIRST, skip = flags & SCONF_KWS_SKIP, last = flags & SCONF_KWS_LAST;
    const int k = min(max(rec[2], 0), K - 1);
    const float thr = __int_as_float(rec[3]);
    const int T = min(max(len_of(in_len, b, N), 0), N);
    const float* col = tab + (long)b * N * Upad + u;
    const long slot0 = ((long)b * K + k) * cap;

    unsigned hi = ~__float_as_uint(-INFINITY), lo = ~0u;                   // the lane's state (v, b) = (-inf, 0) as its key's two halves
    bool have = false;                                                     // a LAST lane's suppression state
    float cE = -INFINITY;
    int cs = -1, ce = -1, count = 0;

    float cur[PREFETCH], nxt[PREFETCH];
    if (T > 0) {
#pragma unroll
        for (int g = 0; g < PREFETCH; ++g) cur[g] = col[(long)min(g, T - 1) * Upad];
    }
    for (int t0 = 0; t0 < T; t0 += PREFETCH) {
#pragma unroll
        for (int g = 0; g < PREFETCH; ++g) nxt[g] = col[(long)min(t0 + PREFETCH + g, T - 1) * Upad];     // clamped, outside every branch
#pragma unroll
        for (int g = 0; g < PREFETCH; ++g) {
            const int t = t0 + g;
            if (t < T) {                                                   // (the whole wave alike)
                const float e = idle ? -INFINITY : cur[g];
                const unsigned h1 = lane_below(hi), l1 = lane_below(lo), h2 = lane_below(h1), l2 = lane_below(l1);
                unsigned long long best = key_of(hi, lo);
                take(best, key_of(h1, l1), !first);
                take(best, key_of(h2, l2), skip);
                take(best, key_of(~0u, ~(unsigned)t), first);               // the fresh start (+0, t)
                const float v = e + __uint_as_float(~(unsigned)(best >> 32));
                hi = ~__float_as_uint(v);
                lo = (unsigned)best;
                if (last && v > -INFINITY && v >= thr) {                   // a candidate (E, s, e) = (v, st, t + 1)
                    const int st = (int)~lo;
                    if (have && st >= ce) {                                // it begins behind cur: cur is a hit
                        if (count < cap) {
                            hit_frames[(slot0 + count) * 2] = cs; hit_frames[(slot0 + count) * 2 + 1] = ce;
                            hit_score[slot0 + count] = cE;
                        }
                        ++count;
                        have = false;
                    }
                    if (!have || v > cE) { have = true; cE = v; cs = st; ce = t + 1; }
                }
            }
        }
#pragma unroll
        for (int g = 0; g < PREFETCH; ++g) cur[g] = nxt[g];
    }
    if (last) {
        if (have) {
            if (count < cap) {
                hit_frames[(slot0 + count) * 2] = cs; hit_frames[(slot0 + count) * 2 + 1] = ce;
                hit_score[slot0 + count] = cE;
            }
            ++count;
        }
        for (int i = count; i < cap; ++i) { hit_frames[(slot0 + i) * 2] = -1; hit_frames[(slot0 + i) * 2 + 1] = -1; hit_score[slot0 + i] = -INFINITY; }
        hit_count[(long)b * K + k] = count;
    }
}

template <int GL, int NQ>
void launch_group(const float* x, long M, int classes, long stride, int vec, const int* columns, int U, int Upad, int blank, float* tab,
                  int vst, hipStream_t st) {
    hipLaunchKernelGGL((kws_gather_kernel<GL, NQ>), dim3((unsigned)cdiv(M, BLOCK / GL)), dim3(BLOCK), 0, st, x, M, classes, stride, vec, columns, U,
                       Upad, blank, tab, vst);
}

}  // namespace

SCONF_API int sconf_kws_max_labels(void) { return MAX_LABELS; }
SCONF_API int sconf_kws_prefetch(void) { return PREFETCH; }
SCONF_API int sconf_kws_max_hits(void) { return MAX_HITS; }

SCONF_API int64_t sconf_kws_workspace(int64_t B, int64_t N, int64_t U) {
    if (B < 1 || B > 65535 || N < 1 || N >= (1L << 31) || B * N >= (1L << 31) - 2 * PREFETCH || U < 1 || U > MAX_COLUMNS) return -1;
    return round256(4 * B * N * ((U + 3) / 4 * 4));
}

SCONF_API int sconf_kws_search(const float* x, const int32_t* input_lengths, const int32_t* image, int64_t n_waves, int64_t U, int64_t K,
                               int32_t* hit_frames, float* hit_score, int32_t* hit_count, int64_t cap, void* workspace, int64_t workspace_bytes,
                               int64_t B, int64_t N, int64_t C, int64_t classes, int blank, sconf_stream_t stream) {
    SCONF_REQUIRE(x && image && hit_frames && hit_score && hit_count && workspace, "sconf_kws_search: null pointer");
    SCONF_REQUIRE(B >= 1 && N >= 1 && K >= 1 && K <= 0x7fffffff, "sconf_kws_search: bad sizes B = %ld, N = %ld, K = %ld: each at least 1", (long)B,
                  (long)N, (long)K);
    SCONF_REQUIRE(C >= 1 && C < (1L << 30) && classes >= 1 && classes <= C, "sconf_kws_search: classes = %ld for rows of %ld: 1 .. C", (long)classes, (long)C);
    SCONF_REQUIRE(blank >= 0 && blank < classes, "sconf_kws_search: blank %d out of range [0, %ld)", blank, (long)classes);
    SCONF_REQUIRE(cap >= 1 && cap <= MAX_HITS, "sconf_kws_search: cap %ld: 1 .. %d", (long)cap, MAX_HITS);
    SCONF_REQUIRE(n_waves >= 1 && n_waves <= 0x7fffff && U >= 1, "sconf_kws_search: an image of %ld waves and %ld columns: each at least 1", (long)n_waves, (long)U);
    const int64_t need = sconf_kws_workspace(B, N, U);
    SCONF_REQUIRE(need > 0, "sconf_kws_search: bad sizes B = %ld, N = %ld, U = %ld (B <= 65535, B N < 2^31, U <= 2^20)", (long)B, (long)N, (long)U);
    SCONF_REQUIRE(workspace_bytes >= need, "sconf_kws_search: workspace of %ld bytes, %ld needed", (long)workspace_bytes, (long)need);
    const long M = B * N;
    const int Upad = (int)((U + 3) / 4 * 4), cl = (int)classes, u = (int)U;
    const int* columns = image + n_waves * 256;
    float* tab = (float*)workspace;
    const int vec = ((uintptr_t)x % 16 == 0) && C % 4 == 0, vst = (uintptr_t)workspace % 16 == 0;
    if (cl <= 64) launch_group<16, 1>(x, M, cl, C, vec, columns, u, Upad, blank, tab, vst, stream);
    else if (cl <= 128) launch_group<16, 2>(x, M, cl, C, vec, columns, u, Upad, blank, tab, vst, stream);
    else if (cl <= 192) launch_group<16, 3>(x, M, cl, C, vec, columns, u, Upad, blank, tab, vst, stream);
    else if (cl <= 256) launch_group<16, 4>(x, M, cl, C, vec, columns, u, Upad, blank, tab, vst, stream);
    else if (cl <= 512) launch_group<64, 2>(x, M, cl, C, vec, columns, u, Upad, blank, tab, vst, stream);
    else if (cl <= 1024) launch_group<64, 4>(x, M, cl, C, vec, columns, u, Upad, blank, tab, vst, stream);
    else hipLaunchKernelGGL(kws_gather_block_kernel, dim3((unsigned)M), dim3(BLOCK), 0, stream, x, cl, (long)C, vec, columns, u, Upad, blank, tab, vst);
    hipLaunchKernelGGL(kws_walk_kernel, dim3((unsigned)cdiv(n_waves, WAVES), (unsigned)B), dim3(BLOCK), 0, stream, tab, image, input_lengths, hit_frames,
                       hit_score, hit_count, (int)n_waves, u, Upad, (int)K, (int)cap, (int)N);
    SCONF_LAUNCH_OK("sconf_kws_search");
    return 0;
}
