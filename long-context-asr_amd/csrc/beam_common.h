// What csrc/beam.hip (the LM-free search) and csrc/beam_lm.hip (the search with an n-gram LM fused in) share: limits and size helpers,
// the f64 log-sum-exp, the prefix hash and the compaction kernel.  An internal header: everything sits in an anonymous namespace, so
// each of the two files instantiates its own copy (the kernels have internal linkage) and both are compiled without -ffast-math.
#pragma once
#include "common.h"
#include <algorithm>
#include <climits>
#include <cmath>

namespace {

constexpr int MAX_W = 128;                      // beams
constexpr int MAX_K = 16;                       // kept tokens per frame
constexpr int G = 16;                           // frames per record chunk
constexpr int RANK_MAX = 128;                   // a frame of at most this many candidates is ranked by counting, a larger one is sorted
constexpr int NPF = (G * (2 + 2 * MAX_K) + 63) / 64;   // prefetch registers per thread at the smallest workgroup (64 threads)
constexpr unsigned long long H0 = 0x9E3779B97F4A7C15ull;

inline int pow2ceil(long n) { int p = 2; while (p < n) p <<= 1; return p; }
inline int search_threads(long W, long K) { return std::min(std::max(pow2ceil(W * (K + 1)) / 2, 64), 1024); }
inline bool sizes_ok(int64_t W, int64_t K) { return W >= 1 && W <= MAX_W && K >= 1 && K <= MAX_K; }

struct Fin { int node, len; double score; };

__device__ __forceinline__ double lse2(double a, double b) {
    const double m = fmax(a, b);
    if (!(m > -(double)INFINITY)) return m;             // both -inf: neutral
    return m + log1p(exp(-fabs(a - b)));
}

__device__ __forceinline__ unsigned long long extend_hash(unsigned long long h, int c) {     // splitmix64 finaliser over (h, c)
    unsigned long long z = (h ^ (unsigned long long)(unsigned)c) + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// (v, i) before (w, j) in the order "larger value first, lower index on ties"
__device__ __forceinline__ bool before(float v, int i, float w, int j) { return v > w || (v == w && i < j); }

// Block-wide arg-max in that order over 256 threads; every thread gets the result.  sh_v / sh_i: 4 entries each.
__device__ __forceinline__ void block_argmax(float& v, int& i, float* sh_v, int* sh_i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float w = __shfl_xor(v, o, 64);
        const int j = __shfl_xor(i, o, 64);
        if (before(w, j, v, i)) { v = w; i = j; }
    }
    __syncthreads();                                    // the previous use of sh_v / sh_i is over
    if ((threadIdx.x & 63) == 0) { sh_v[threadIdx.x >> 6] = v; sh_i[threadIdx.x >> 6] = i; }
    __syncthreads();
    v = sh_v[0]; i = sh_i[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) if (before(sh_v[w], sh_i[w], v, i)) { v = sh_v[w]; i = sh_i[w]; }
}

// One workgroup per (sample, frame) row.  Dynamic LDS: the row [C], then 4 + 4 + 4 + 4 MAX_K + 4 MAX_K words of scratch.
__global__ __launch_bounds__(256) void beam_compact_kernel(const float* __restrict__ lp, const int* __restrict__ in_len,
                                                           int* __restrict__ rec, int B, int N, int C, int blank, float thr, int Kmax) {
    extern __shared__ float row[];                      // [C]
    float* sh_v = row + C;                              // [4]
    int* sh_i = reinterpret_cast<int*>(sh_v + 4);       // [4]
    int* cnt_w = sh_i + 4;                              // [4]
    int* st_c = cnt_w + 4;                              // [4][MAX_K]
    float* st_v = reinterpret_cast<float*>(st_c + 4 * MAX_K);   // [4][MAX_K]
    const int RS = 2 + 2 * Kmax;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int seg = ((C + 3) / 4 + 63) / 64 * 64;       // classes per wave in the ordered pass, whole rounds of 64
    for (long bt = blockIdx.x; bt < (long)B * N; bt += gridDim.x) {
        const int t = (int)(bt % N), b = (int)(bt / N);
        const int T = len_of(in_len, b, N);
        if (T > N || t >= T) continue;                  // (uniform over the workgroup; a poisoned sample's rows are never read)
        __syncthreads();                                // the previous row is done with
        const float* src = lp + bt * C;
        float bv = -INFINITY;
        int bi = INT_MAX, q = 0;
        for (int c = tid * 4; c < C; c += 1024) {
            const float4 x = *reinterpret_cast<const float4*>(src + c);
            *reinterpret_cast<float4*>(row + c) = x;
            const float xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (before(xs[e], c + e, bv, bi)) { bv = xs[e]; bi = c + e; }
                q += (c + e != blank) & (xs[e] >= thr);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
        block_argmax(bv, bi, sh_v, sh_i);               // (its barriers also publish the row)
        if (lane == 0) cnt_w[wave] = q;
        __syncthreads();
        const int amax = bi == INT_MAX ? 0 : bi;        // (only a row of NaN has no arg-max)
        const bool extra = amax != blank && !(row[amax] >= thr);          // the arg-max alone, below the threshold
        const int Q = cnt_w[0] + cnt_w[1] + cnt_w[2] + cnt_w[3] + (extra ? 1 : 0);
        float pv = -INFINITY;                           // keep what is not behind (pv, pc); everything that qualifies if Q <= Kmax
        int pc = INT_MAX;
        if (Q > Kmax) {                                 // (uniform) then every qualifying class is >= thr: the arg-max is one of them
            float cv = INFINITY;
            int cc = -1;
            for (int s = 0; s < Kmax; ++s) {            // the next entry in the order after (cv, cc)
                float v = -INFINITY;
                int i = INT_MAX;
                for (int c = tid; c < C; c += 256) {
                    const float x = row[c];
                    if (c != blank && x >= thr && before(cv, cc, x, c) && before(x, c, v, i)) { v = x; i = c; }
                }
                block_argmax(v, i, sh_v, sh_i);
                if (i == INT_MAX) break;
                cv = v; cc = i;
            }
            pv = cv; pc = cc;
        }
        __syncthreads();
        // ordered pass: wave w scans classes [w seg, (w + 1) seg) 64 at a time and stages its kept entries in class order
        int mine = 0;
        for (int c0 = wave * seg; c0 < min(C, (wave + 1) * seg); c0 += 64) {
            const int c = c0 + lane;
            bool keep = false;
            float x = 0.f;
            if (c < C && c != blank) {
                x = row[c];
                keep = (x >= thr || (extra && c == amax)) && !before(pv, pc, x, c);
            }
            const unsigned long long m = __ballot(keep);
            const int at = mine + __popcll(m & ((1ull << lane) - 1));
            if (keep && at < MAX_K) { st_c[wave * MAX_K + at] = c; st_v[wave * MAX_K + at] = x; }
            mine += __popcll(m);
        }
        if (lane == 0) cnt_w[wave] = min(mine, MAX_K);
        __syncthreads();
        const int total = min(cnt_w[0] + cnt_w[1] + cnt_w[2] + cnt_w[3], Kmax);
        int* out = rec + bt * RS;
        if (tid == 0) { out[0] = __float_as_int(row[blank]); out[1] = total; }
        if (tid < total) {
            int w = 0, k = tid;
            while (k >= cnt_w[w]) { k -= cnt_w[w]; ++w; }
            out[2 + 2 * tid] = st_c[w * MAX_K + k];
            out[3 + 2 * tid] = __float_as_int(st_v[w * MAX_K + k]);
        }
    }
}

}  // namespace
