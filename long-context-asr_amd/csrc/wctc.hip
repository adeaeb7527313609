// Wild-card CTC loss (W-CTC) forward + backward: include/sconf_wctc.h has the function, the gradient and the departures from the
// reference's lcasr/losses/wctc.py.  Batch-major (B,N,C) f32 log-probs, as the CTC kernels (ctc.hip) whose state discipline this
// file keeps: f64 recursion state (log2 units) in LDS, the transcendental part in f32, one barrier per frame, emissions gathered once
// into contiguous rows and prefetched into registers a group of frames ahead.  What it does NOT keep is the stored form of the a
// rows, f32 relative to an f64 offset per frame.  Every state of a CTC row has consumed the same t emissions, so a CTC row lies within
// hundreds of its maximum where the posterior lives.  The wild-card feeds mass 1 into states 0 and 1 at EVERY frame: a W-CTC row
// runs from O(1) at its first states down to the product of s / 2 label probabilities at state s, at every frame, and the
// posterior lives all along that slope.  Relative to any per-frame scalar the deep states sit thousands below: an f32 there has an
// ulp of 2.4e-4 .. 4.9e-4, and the gradient error measured with ctc.hip's stored form was 1.0e-4 of the maximum at 1025 states,
// 1.1e-4 at 300 labels x 144 classes of weak emissions and 3.4e-4 at 4097 states (the tests allow 2e-4).  So the a rows are stored
// as they are in LDS: f64, log2 units, no offsets (16 instead of 12 bytes of workspace per state and frame).
//
// What differs from CTC and shapes the kernels:
//   * w_t = df/de_t depends on EVERY e_t, so the b lattice cannot run beside the a lattice.  The forward launch runs a over time,
//     writes e_t per frame, then reduces over t (f64, fixed order) and writes w_t; the backward launch runs b.
//   * The wild-card is a source of mass 1 into states 0 and 1 at every frame; the gradient has the matching sink w_t / E_t into
//     states 2L-1 and 2L at every frame.  In MIRRORED coordinates (b walks the reversed lattice backwards in time) both are one
//     fourth term of the log-sum-exp of states 0 and 1, so one kernel body serves both directions.
//   * In soft mode w_t is negative wherever e_t < f - 1, so b is signed.  The backward carries w = w+ - w- as TWO non-negative
//     lattices (template parameter K) through the same pass; they meet once per state and frame, in the product a (b+ - b-).
//   * b is not stored: the backward reads the stored a row of its frame and stores the product a_t(s) b_t(s) (linear, f32, signed),
//     which the per-frame gradient kernel sums by class in a fixed order.
#include "common.h"
#include "../../include/sconf_wctc.h"
#include <algorithm>

namespace {

constexpr int MAX_LABELS = 2552;                        // 2 lattices x 2 rows x (2 * 2552 + 1 + 5 + 2) f64 = 163 584 bytes <= 160 KB
constexpr double NEG_BIG = -1e300;                      // "unreachable", finite: absorbs what is added to it, (float)NEG_BIG = -inf
constexpr double DEAD = -1e290;                         // anything below is unreachable
constexpr double LOG2E_D = 1.4426950408889634, LN2_D = 0.6931471805599453;

__device__ __forceinline__ double max_f64(double a, double b) {          // fmax() canonicalises its inputs first (3 instructions)
    double r; asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r;
}
// log2(2^a + 2^b + 2^c + 2^d): maximum and differences in f64, the transcendental part in f32 (~1e-7 absolute whatever the magnitude)
__device__ __forceinline__ double lse4_log2(double a, double b, double c, double d) {
    const double m = max_f64(max_f64(a, b), max_f64(c, d));
    const float s = (__builtin_amdgcn_exp2f((float)(a - m)) + __builtin_amdgcn_exp2f((float)(b - m))) +
                    (__builtin_amdgcn_exp2f((float)(c - m)) + __builtin_amdgcn_exp2f((float)(d - m)));
    return m + (double)__builtin_amdgcn_logf(s);
}

// The parts of the workspace (include/sconf_wctc.h), each on a 256-byte boundary.
struct Parts { float *lpg, *prod; double *alpha, *e, *w, *sink, *f; int64_t bytes; };
static Parts carve(void* ws, int64_t B, int64_t N, int64_t Lmax, int K) {
    char* p = (char*)ws;
    int64_t o = 0;
    auto take = [&](int64_t n) { char* r = p + o; o += round256(n); return r; };
    Parts q;
    q.lpg = (float*)take(B * N * Lmax * 4); q.alpha = (double*)take(B * N * Lmax * 8); q.prod = (float*)take(B * N * Lmax * 4);
    q.e = (double*)take(B * N * 8); q.w = (double*)take(B * N * 8);
    q.sink = (double*)take((int64_t)K * B * N * 8); q.f = (double*)take(B * 8);
    q.bytes = o;
    return q;
}

// One workgroup per (sample, frame): the frame's log-prob row is streamed into LDS with 16-byte loads and the 2S+1 lattice emissions
// are gathered from there (ctc_gather_kernel's scheme).  Frames >= input_length and states >= 2 target_length + 1 get 0.
__global__ __launch_bounds__(256) void wctc_gather_kernel(const float* __restrict__ lp, const int* __restrict__ targets, const int* __restrict__ in_len,
                                                          const int* __restrict__ tg_len, float* __restrict__ lpg,
                                                          int B, int N, int C, int Smax, int Lmax, int blank) {
    extern __shared__ float row[];                      // [C]
    for (long bt = blockIdx.x; bt < (long)B * N; bt += gridDim.x) {
        const int t = (int)(bt % N), b = (int)(bt / N);
        float* out = lpg + bt * Lmax;
        const int L = 2 * min(max(tg_len[b], 0), Smax) + 1;
        if (t >= in_len[b]) {
            for (int s = threadIdx.x; s < Lmax; s += 256) out[s] = 0.f;
            continue;
        }
        __syncthreads();                                // the previous row's gathers are done
        const float* src = lp + bt * C;
        for (int c = threadIdx.x * 4; c < C; c += 1024) *reinterpret_cast<float4*>(row + c) = *reinterpret_cast<const float4*>(src + c);
        __syncthreads();
        for (int s = threadIdx.x; s < Lmax; s += 256) {
            float v = 0.f;
            if (s < L) {
                int lab = (s & 1) ? targets[(long)b * Smax + (s >> 1)] : blank;
                lab = min(max(lab, 0), C - 1);          // an out-of-range label poisons the sample (lattice kernel); never index with it
                v = row[lab];
            }
            out[s] = v;
        }
    }
}

// Fixed-order reductions over the workgroup through `red` (blockDim.x doubles): a tree whose shape depends on blockDim.x only.
template <typename OP> __device__ __forceinline__ double block_reduce_f64(double v, double* red, OP op) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int o = blockDim.x >> 1; o > 0; o >>= 1) {
        if (tid < o) red[tid] = op(red[tid], red[tid + o]);
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// One workgroup per sample.  BWD = false: the a lattice forwards in time, e_t per frame, then f and w_t.  BWD = true: K lattices b
// (K = 2: of w+ and of w-) backwards in time on the mirrored lattice, and the products a_t(s) (b+_t(s) - b-_t(s)).
// MAXS = lattice states per thread (adjacent, in mirrored coordinates sp: their MAXS + 2 inputs are one contiguous LDS read).
// What the LDS rows hold: forwards log2 a_t(sp); backwards g_t(sp) = p_t(ext) b_t(sp), so that the step has the same shape both ways:
//     v = lse( prev[sp], prev[sp-1], [skip] prev[sp-2], [sp <= 1] x_t ),    x_t = 0 (the wild-card) | log2(w_t / E_t) (the sink)
//     forwards  cur[sp] = v + emission;                     stored: cur, f64 (the head of this file says why not f32)
//     backwards b = v; cur[sp] = v + emission;              stored: 2^(a + b+) - 2^(a + b-) as f32, the sums in f64
template <int MAXS, bool BWD, int K>
__global__ __launch_bounds__(1024) void wctc_lattice_kernel(const float* __restrict__ lpg, const int* __restrict__ targets,
                                                            const int* __restrict__ in_len, const int* __restrict__ tg_len,
                                                            double* __restrict__ alpha, float* __restrict__ prod,
                                                            double* __restrict__ ev, double* __restrict__ wv, double* __restrict__ sink,
                                                            double* __restrict__ fv, float* __restrict__ nll,
                                                            int B, int N, int C, int Smax, int Lmax, int mode) {
    extern __shared__ double lat[];                     // [K][2][W]
    const int b = blockIdx.x;
    const int T = in_len[b], S = tg_len[b], L = 2 * S + 1;
    const int nt = blockDim.x, tid = threadIdx.x;
    const int W = Lmax + MAXS + 2;                      // two guard cells in front, MAXS cells of slack behind
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long bN = (long)b * N;
    if constexpr (BWD) {
        const double f = fv[b];
        if (!(f > -INFINITY && f < INFINITY)) return;  // infeasible (-inf) or poisoned (NaN): the gradient kernel reads no product
    } else {
        if (T <= 0) { if (tid == 0) { nll[b] = INFINITY; fv[b] = -INFINITY; } return; }
        // What the host-side checks refuse when the lengths live on the host: the sample is poisoned and nothing is indexed with the bad value.
        int bad = (T > N) | (S < 1) | (S > Smax);
        if (!bad) for (int i = tid; i < S; i += nt) { const int lab = targets[(long)b * Smax + i]; bad |= (lab < 0) | (lab >= C); }
        if (__syncthreads_or(bad)) { if (tid == 0) { nll[b] = NAN; fv[b] = NAN; } return; }
    }

    const int sp0 = tid * MAXS, cnt = min(max(L - sp0, 0), MAXS);
    bool skip_ok[MAXS];
#pragma unroll
    for (int k = 0; k < MAXS; ++k) {
        const int sp = sp0 + k;
        skip_ok[k] = false;
        if (sp < L && sp >= 2) {
            const int s = BWD ? L - 1 - sp : sp;
            if (s & 1) {
                const int s2 = BWD ? s + 2 : s - 2;
                skip_ok[k] = targets[(long)b * Smax + (s >> 1)] != targets[(long)b * Smax + (s2 >> 1)];
            }
        }
    }
    for (int i = tid; i < K * 2 * W; i += nt) lat[i] = NEG_BIG;          // a_{-1} = 0, b_T = 0: the wild-card / the sinks supply all mass
    __syncthreads();

    const float* lg = lpg + bN * Lmax;
    double* arow = alpha + bN * Lmax;
    float* prow = prod + bN * Lmax;
    // Frames are prefetched in groups of G: unconditional loads from clamped (always valid) addresses, so none is waited for inside a branch.
    constexpr int G = MAXS <= 2 ? 4 : (MAXS <= 4 ? 2 : 1);
    struct Group { float em[G][MAXS]; double al[BWD ? G : 1][BWD ? MAXS : 1]; double x[BWD ? K : 1][BWD ? G : 1]; };
    Group pf, nx;
    auto load_group = [&](Group& dst, int i0) {
#pragma unroll
        for (int j = 0; j < G; ++j) {
            const int i = min(i0 + j, T - 1);
            const int t = BWD ? T - 1 - i : i;
#pragma unroll
            for (int k = 0; k < MAXS; ++k) {
                const int sp = min(sp0 + k, L - 1);
                const int s = BWD ? L - 1 - sp : sp;
                dst.em[j][k] = lg[(long)t * Lmax + s];
                if constexpr (BWD) dst.al[j][k] = arow[(long)t * Lmax + s];
            }
            if constexpr (BWD) {
#pragma unroll
                for (int q = 0; q < K; ++q) dst.x[q][j] = sink[(long)q * B * N + bN + t];
            }
        }
    };
    load_group(pf, 0);
    const int w0 = wave * 64 * MAXS;                     // the wave's first state
    for (int i0 = 0; i0 < T; i0 += G) {
        load_group(nx, i0 + G);                          // prefetch the next G frames
#pragma unroll
        for (int j = 0; j < G; ++j) {
            const int i = i0 + j;
            if (i < T) {                                  // uniform across the workgroup
                const int t = BWD ? T - 1 - i : i;
                double* orow_a = arow + (long)t * Lmax;
                float* orow = prow + (long)t * Lmax;
                if (w0 <= 2 * i + 1) {                    // wave-uniform: mass has come i frames from states 0 and 1
                    if (cnt > 0) {
                        double bsum[K][MAXS];
#pragma unroll
                        for (int q = 0; q < K; ++q) {
                            double* cur = lat + (size_t)(q * 2 + (i & 1)) * W + 2;
                            const double* prev = lat + (size_t)(q * 2 + ((i & 1) ^ 1)) * W + 2;
                            const double x = BWD ? pf.x[BWD ? q : 0][BWD ? j : 0] : 0.0;
                            double pv[MAXS + 2];
#pragma unroll
                            for (int r = 0; r < MAXS + 2; ++r) pv[r] = prev[sp0 - 2 + r];
#pragma unroll
                            for (int k = 0; k < MAXS; ++k) {
                                const double v = lse4_log2(pv[k + 2], pv[k + 1], skip_ok[k] ? pv[k] : NEG_BIG, sp0 + k < 2 ? x : NEG_BIG);
                                const double nv = __builtin_fma((double)fmaxf(pf.em[j][k], -1e30f), LOG2E_D, v);   // an emission of -inf stays finite
                                bsum[q][k] = v;
                                if (k < cnt) cur[sp0 + k] = nv;
                                if constexpr (!BWD) { if (k < cnt) orow_a[sp0 + k] = nv; }
                            }
                        }
                        if constexpr (BWD) {
#pragma unroll
                            for (int k = 0; k < MAXS; ++k) {
                                const double a2 = pf.al[j][k];                                             // log2 a_t(s): the large parts meet in f64
                                float o = __builtin_amdgcn_exp2f((float)(a2 + bsum[0][k]));
                                if constexpr (K == 2) o -= __builtin_amdgcn_exp2f((float)(a2 + bsum[1][k]));
                                if (k < cnt) orow[L - 1 - sp0 - k] = o;
                            }
                        }
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < MAXS; ++k)
                        if (k < cnt) {
#pragma unroll
                            for (int q = 0; q < K; ++q) lat[(size_t)(q * 2 + (i & 1)) * W + 2 + sp0 + k] = NEG_BIG;
                            if (BWD) orow[L - 1 - sp0 - k] = 0.f; else orow_a[sp0 + k] = NEG_BIG;
                        }
                }
                wait_lgkm0_barrier();
                if (!BWD && tid == nt - 1) {              // e_t from the row just published (not written again before the barrier of frame i + 1)
                    const double* cur = lat + (size_t)(i & 1) * W + 2;
                    const double e2 = lse4_log2(cur[L - 1], cur[L - 2], NEG_BIG, NEG_BIG);
                    ev[bN + t] = e2 < DEAD ? -(double)INFINITY : e2 * LN2_D;
                }
            }
        }
        pf = nx;
    }
    if constexpr (!BWD) {
        // The reduction over time: every thread takes the frames tid, tid + nt, .. in order, the workgroup a fixed tree.  f64 throughout.
        __shared__ double red[1024];
        __threadfence_block();
        __syncthreads();                                  // every e_t is visible to the workgroup
        const double* e = ev + bN;
        double mx = -INFINITY;
        for (int t = tid; t < T; t += nt) mx = fmax(mx, e[t]);
        const double M = block_reduce_f64(mx, red, [](double a, double c) { return fmax(a, c); });
        if (!(M > -INFINITY)) {                           // no frame reaches the last label: infeasible
            if (tid == 0) { nll[b] = INFINITY; fv[b] = -INFINITY; }
            return;
        }
        double z = 0.0;
        for (int t = tid; t < T; t += nt) if (e[t] > -INFINITY) z += exp(e[t] - M);
        const double lse = M + log(block_reduce_f64(z, red, [](double a, double c) { return a + c; }));
        double f = lse;
        int first = 0;
        if (mode == SCONF_WCTC_MAX_PROB) {
            double tm = 4e9;
            for (int t = tid; t < T; t += nt) if (e[t] == M) { tm = (double)t; break; }
            first = (int)block_reduce_f64(tm, red, [](double a, double c) { return fmin(a, c); });
            f = M;
        } else if (mode == SCONF_WCTC_SOFT) {
            double acc = 0.0;
            for (int t = tid; t < T; t += nt) if (e[t] > -INFINITY) acc += exp(e[t] - lse) * e[t];
            f = block_reduce_f64(acc, red, [](double a, double c) { return a + c; });
        }
        for (int t = tid; t < T; t += nt) {
            double w = 0.0;
            if (e[t] > -INFINITY) {
                if (mode == SCONF_WCTC_MAX_PROB) w = t == first ? 1.0 : 0.0;
                else { w = exp(e[t] - lse); if (mode == SCONF_WCTC_SOFT) w *= 1.0 + e[t] - f; }
            }
            wv[bN + t] = w;
            const double l2 = w != 0.0 ? log2(fabs(w)) - e[t] * LOG2E_D : NEG_BIG;              // log2(|w_t| / E_t)
            sink[bN + t] = w > 0.0 ? l2 : NEG_BIG;
            if (mode == SCONF_WCTC_SOFT) sink[(long)B * N + bN + t] = w < 0.0 ? l2 : NEG_BIG;
        }
        if (tid == 0) { nll[b] = (float)-f; fv[b] = f; }
    }
}

// One workgroup per (b, t) row: grad[c] = -g * sum of the products of the states whose label is c.  Every sum in a fixed order
// (ctc_grad_logits_kernel's scheme): the blank states, half of them and one address, are summed in registers, then per wave; the
// label products of a chunk are staged in LDS with their labels, and wave w adds those whose label is w mod 4, so all states of
// one label are added by one wave, in state order.
__global__ __launch_bounds__(256) void wctc_grad_kernel(const float* __restrict__ prod, const double* __restrict__ fv, const int* __restrict__ targets,
                                                        const int* __restrict__ in_len, const int* __restrict__ tg_len,
                                                        const float* __restrict__ grad_out, float* __restrict__ grad,
                                                        int B, int N, int C, int Smax, int Lmax, int blank) {
    extern __shared__ float occ[];                      // [C]
    __shared__ float wpart[4];
    constexpr int LCH = 1024;                           // label states staged per chunk
    __shared__ int stg_lab[LCH];
    __shared__ float stg_occ[LCH];
    const long bt = blockIdx.x;
    const int b = (int)(bt / N), t = (int)(bt % N);
    float* gr = grad + bt * C;
    const double f = fv[b];
    const bool pad = t >= in_len[b] || f == -(double)INFINITY, bad = f != f;      // uniform over the workgroup
    if (pad || bad) {                                   // past the sample's length or infeasible: zeros; poisoned: NaN rows
        const float z = pad ? 0.f : NAN;
        for (int c = threadIdx.x * 4; c < C; c += 1024) { float v[4] = {z, z, z, z}; store4(gr + c, v); }
        return;
    }
    for (int c = threadIdx.x; c < C; c += 256) occ[c] = 0.f;
    __syncthreads();
    const int S_ = tg_len[b];
    const float* pr = prod + bt * Lmax;
    const int wvi = threadIdx.x >> 6, ln = threadIdx.x & 63;
    float blk = 0.f;
    for (int k = threadIdx.x; k <= S_; k += 256) blk += pr[2 * k];                 // blank states s = 2k
    for (int k0 = 0; k0 < S_; k0 += LCH) {                                       // label states s = 2k + 1, LCH at a time
        const int n = min(LCH, S_ - k0);
        for (int j = threadIdx.x; j < n; j += 256) { stg_lab[j] = targets[(long)b * Smax + k0 + j]; stg_occ[j] = pr[2 * (k0 + j) + 1]; }
        __syncthreads();
        for (int j = ln; j < n; j += 64) {
            const int lab = stg_lab[j];
            if ((lab & 3) == wvi) atomicAdd(&occ[lab], stg_occ[j]);
        }
        if (k0 + LCH < S_) __syncthreads();                                      // (uniform) the next chunk overwrites the staging
    }
    blk = wave_sum(blk);
    if (ln == 0) wpart[wvi] = blk;
    __syncthreads();                                    // occ and the per-wave sums are complete
    const float oblank = ((wpart[0] + wpart[1]) + wpart[2]) + wpart[3];           // added to occ[blank] on use
    const float g = grad_out ? grad_out[b] : 1.f;
    for (int c = threadIdx.x * 4; c < C; c += 1024) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = -g * (c + e == blank ? occ[c + e] + oblank : occ[c + e]);
        store4(gr + c, v);
    }
}

struct Geo { int nt, spt; size_t lds; };
static Geo geometry(int Lmax, int K) {
    Geo g;
    g.nt = Lmax <= 256 ? 256 : (Lmax <= 512 ? 512 : 1024);          // the serial step costs a barrier + the slowest thread: few states each
    g.spt = cdiv(Lmax, g.nt);
    g.lds = (size_t)K * 2 * (Lmax + g.spt + 2) * 8;
    return g;
}

static int check_common(const char* who, const void* targets, const void* il, const void* tl, const void* ws, int64_t ws_bytes,
                        int64_t B, int64_t N, int64_t C, int64_t Smax, int blank, int mode) {
    SCONF_REQUIRE(mode == SCONF_WCTC_SOFT || mode == SCONF_WCTC_MAX_PROB || mode == SCONF_WCTC_SUM_PROB, "%s: bad mode %d", who, mode);
    SCONF_REQUIRE(B >= 1 && N >= 1 && B * N < (1L << 31), "%s: B = %ld, N = %ld: both must be at least 1 and B * N below 2^31", who, (long)B, (long)N);
    SCONF_REQUIRE(C >= 4 && C % 4 == 0 && C <= 16384, "%s: C must be a multiple of 4 and at most 16384 (%ld classes)", who, (long)C);
    SCONF_REQUIRE(Smax >= 1 && Smax <= MAX_LABELS, "%s: Smax = %ld: 1 .. %d labels are supported", who, (long)Smax, MAX_LABELS);
    SCONF_REQUIRE(blank >= 0 && blank < C, "%s: blank %d out of range", who, blank);
    SCONF_REQUIRE(targets && il && tl && ws, "%s: null pointer (targets, input_lengths, target_lengths and workspace are required)", who);
    const int64_t need = sconf_wctc_workspace(B, N, Smax, mode);
    SCONF_REQUIRE(ws_bytes >= need, "%s: workspace of %ld bytes, %ld are needed", who, (long)ws_bytes, (long)need);
    return 0;
}

}  // namespace

SCONF_API int sconf_wctc_max_labels(void) { return MAX_LABELS; }

SCONF_API int64_t sconf_wctc_workspace(int64_t B, int64_t N, int64_t Smax, int mode) {
    if (B < 1 || N < 1 || B * N >= (1L << 31) || Smax < 1 || Smax > MAX_LABELS || mode < SCONF_WCTC_SOFT || mode > SCONF_WCTC_SUM_PROB) return -1;
    return carve(nullptr, B, N, 2 * Smax + 1, mode == SCONF_WCTC_SOFT ? 2 : 1).bytes;
}

#define WCTC_LAUNCH(MS, BWD, K) do { \
        if (geo.lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)wctc_lattice_kernel<MS, BWD, K>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)geo.lds); \
        hipLaunchKernelGGL((wctc_lattice_kernel<MS, BWD, K>), dim3((unsigned)B), dim3(geo.nt), geo.lds, stream, p.lpg, targets, input_lengths, \
                           target_lengths, p.alpha, p.prod, p.e, p.w, p.sink, p.f, nll, (int)B, (int)N, (int)C, (int)Smax, Lmax, mode); } while (0)
#define WCTC_BY_SPT(BWD, K) do { switch (geo.spt) { case 1: WCTC_LAUNCH(1, BWD, K); break; case 2: WCTC_LAUNCH(2, BWD, K); break; \
        case 3: WCTC_LAUNCH(3, BWD, K); break; case 4: WCTC_LAUNCH(4, BWD, K); break; default: WCTC_LAUNCH(5, BWD, K); } } while (0)

SCONF_API int sconf_wctc_fwd(const float* log_probs, const int32_t* targets, const int32_t* input_lengths, const int32_t* target_lengths,
                             float* nll, void* workspace, int64_t workspace_bytes, int64_t B, int64_t N, int64_t C, int64_t Smax, int blank,
                             int mode, hipStream_t stream) {
    if (check_common("sconf_wctc_fwd", targets, input_lengths, target_lengths, workspace, workspace_bytes, B, N, C, Smax, blank, mode)) return 1;
    SCONF_REQUIRE(log_probs && nll, "sconf_wctc_fwd: null pointer (log_probs and nll are required)");
    const int Lmax = (int)(2 * Smax + 1);
    const int K = mode == SCONF_WCTC_SOFT ? 2 : 1;
    const Parts p = carve(workspace, B, N, Lmax, K);
    hipLaunchKernelGGL(wctc_gather_kernel, dim3((unsigned)std::min<long>(B * N, 65536)), dim3(256), (size_t)C * 4, stream, log_probs, targets,
                       input_lengths, target_lengths, p.lpg, (int)B, (int)N, (int)C, (int)Smax, Lmax, blank);
    const Geo geo = geometry(Lmax, 1);
    SCONF_REQUIRE(geo.spt <= 5, "sconf_wctc_fwd: target too long (%ld labels)", (long)Smax);
    WCTC_BY_SPT(false, 1);
    SCONF_LAUNCH_OK("sconf_wctc_fwd");
    return 0;
}

SCONF_API int sconf_wctc_bwd(const int32_t* targets, const int32_t* input_lengths, const int32_t* target_lengths, const float* grad_out,
                             float* grad, void* workspace, int64_t workspace_bytes, int64_t B, int64_t N, int64_t C, int64_t Smax, int blank,
                             int mode, hipStream_t stream) {
    if (check_common("sconf_wctc_bwd", targets, input_lengths, target_lengths, workspace, workspace_bytes, B, N, C, Smax, blank, mode)) return 1;
    SCONF_REQUIRE(grad, "sconf_wctc_bwd: null pointer (grad is required)");
    const int Lmax = (int)(2 * Smax + 1);
    const int K = mode == SCONF_WCTC_SOFT ? 2 : 1;
    const Parts p = carve(workspace, B, N, Lmax, K);
    float* nll = nullptr;
    const Geo geo = geometry(Lmax, K);
    SCONF_REQUIRE(geo.spt <= 5 && geo.lds <= 160 * 1024, "sconf_wctc_bwd: target too long (%ld labels)", (long)Smax);
    if (K == 2) WCTC_BY_SPT(true, 2); else WCTC_BY_SPT(true, 1);
    hipLaunchKernelGGL(wctc_grad_kernel, dim3((unsigned)(B * N)), dim3(256), (size_t)C * 4, stream, p.prod, p.f, targets, input_lengths,
                       target_lengths, grad_out, grad, (int)B, (int)N, (int)C, (int)Smax, Lmax, blank);
    SCONF_LAUNCH_OK("sconf_wctc_bwd");
    return 0;
}
