// Posterior unit (include/sconf_post.h): the CTC likelihood of every string at edit distance 1 from a hypothesis y, as log-likelihood
// ratios against y, and the slot and gap posteriors on top of them.
//
// Three kernels.  post_lattice_kernel stores the forward rows alpha and the backward rows betahat of y in f64: one workgroup per
// (sample, direction), the row double-buffered in LDS, one barrier per frame, the next frame's emissions gathered into registers
// while the current one is computed.  post_neighbours_kernel is the hot one: a neighbour shares y's rows in front of and behind its
// edit, so it costs one serial chain over a single bridge state; a lane runs the chain of one (slot or gap, class), a wave 64
// consecutive classes of one slot, so the frame's scores are one coalesced segment and the lattice values of the step are
// wave-uniform loads.  post_slots_kernel reduces every row of the two outputs to a posterior and its best alternative.
//
// All recursions keep their state in f64 in LOG2 units, the transcendental part of a log-sum-exp in f32 on v_exp_f32 / v_log_f32
// as ctc.hip does; unlike there "unreachable" is a true -inf, which the outputs report.  Built WITHOUT -ffast-math (see the
// Makefile): -inf is a value here, and v != v and v - v == 0 are tests.
#include "common.h"
#include "../../include/sconf_post.h"

namespace {

constexpr double LOG2E_D = 1.4426950408889634, LN2_D = 0.6931471805599453;
constexpr int MAX_LABELS = 4095;                           // 2 rows of 2 * 4095 + 1 + 4 doubles: 131120 bytes of LDS
constexpr double STEP_ERROR = 6.0 / 8388608.0;             // 6 * 2^-23 nats per frame: the header's NUMERICS
constexpr int LAT_PAD = 2;                                 // states of -inf in front of and behind a row in LDS: s - 2 .. s + 2 need no test

__device__ __forceinline__ double neg_inf() { return -__builtin_huge_val(); }

// log2(2^a + 2^b (+ 2^c)).  The maximum and the differences in f64, the rest in f32; the largest term is exactly 1.  All arguments
// -inf: the differences are taken against 0 instead, every exponential is 0 and log2(0) = -inf is the result, without a branch.
__device__ __forceinline__ double lse2(double a, double b) {
    const double m = fmax(a, b), lo = fmin(a, b), d = m == neg_inf() ? 0.0 : m;
    const float s = __builtin_amdgcn_exp2f((float)(m - d)) + __builtin_amdgcn_exp2f((float)(lo - d));
    return d + (double)__builtin_amdgcn_logf(s);
}
__device__ __forceinline__ double lse3(double a, double b, double c) {
    const double m = fmax(a, fmax(b, c)), d = m == neg_inf() ? 0.0 : m;
    const float s = __builtin_amdgcn_exp2f((float)(a - d)) + __builtin_amdgcn_exp2f((float)(b - d)) + __builtin_amdgcn_exp2f((float)(c - d));
    return d + (double)__builtin_amdgcn_logf(s);
}
__device__ __forceinline__ bool finite_f64(double v) { return v - v == 0.0; }
__device__ __forceinline__ bool sizes_ok(int T, int L, int N, int Smax) { return T >= 0 && T <= N && L >= 0 && L <= Smax; }

// ---- the rows -----------------------------------------------------------------------------------------------------------------------
// Workspace: alpha at [(b N + t) W + s], betahat at [((B + b) N + t) W + s], W = 2 Smax + 1.  Thread `tid` owns the states
// tid + k * blockDim.x, k < MAXS.
template <int MAXS>
__global__ __launch_bounds__(1024) void post_lattice_kernel(const float* __restrict__ lp, const int* __restrict__ targets,
                                                            const int* __restrict__ in_len, const int* __restrict__ tg_len, int N, int C,
                                                            long stride, int Smax, int blank, double* __restrict__ ws,
                                                            double* __restrict__ loglik) {
    extern __shared__ double lat[];                        // [2][LAT_PAD + W + LAT_PAD]
    const int b = blockIdx.x >> 1, dir = blockIdx.x & 1, B = gridDim.x >> 1, tid = threadIdx.x, nt = blockDim.x;
    const int W = 2 * Smax + 1, RW = W + 2 * LAT_PAD;
    const int T = in_len[b], L = tg_len[b];
    const bool sized = sizes_ok(T, L, N, Smax);
    const int* y = targets + (long)b * Smax;
    const float* x = lp + (long)b * N * stride;
    if (dir == 0) {                                        // the forward workgroup decides whether the sample is poisoned, and says so
        int bad = !sized;
        if (sized) {
            for (int i = tid; i < L; i += nt) { const int v = y[i]; bad |= (v < 0) | (v >= C) | (v == blank); }
            for (long i = tid; i < (long)T * C; i += nt) {
                const long t = i / C;
                const float v = x[t * stride + (i - t * C)];
                bad |= (v != v) | (v == INFINITY);
            }
        }
        bad = __syncthreads_or(bad);
        if (bad || T == 0) {
            if (tid == 0) loglik[b] = bad ? __builtin_nan("") : (L == 0 ? 0.0 : neg_inf());
            return;
        }
    } else if (!sized || T == 0) {
        return;                                            // (labels are clamped below: a poisoned sample's rows are computed and never read)
    }
    const int S = 2 * L + 1;
    for (int i = tid; i < 2 * RW; i += nt) lat[i] = neg_inf();
    int lab[MAXS];
    bool skip[MAXS];
#pragma unroll
    for (int k = 0; k < MAXS; ++k) {
        const int s = tid + k * nt, i = s >> 1;
        lab[k] = blank; skip[k] = false;
        if (s < S && (s & 1)) {
            lab[k] = min(max(y[i], 0), C - 1);
            skip[k] = dir == 0 ? (i >= 1 && y[i] != y[i - 1]) : (i + 1 < L && y[i] != y[i + 1]);
        }
    }
    double* out = ws + ((long)dir * B + b) * N * W;
    const int step = dir == 0 ? -1 : 1;                    // where the states a state is reached from lie
    float e[MAXS];
    {
        const float* xr = x + (long)(dir == 0 ? 0 : T - 1) * stride;
#pragma unroll
        for (int k = 0; k < MAXS; ++k) e[k] = xr[lab[k]];
    }
    __syncthreads();
    for (int f = 0; f < T; ++f) {
        const int t = dir == 0 ? f : T - 1 - f;
        const double* prev = lat + ((f + 1) & 1) * RW + LAT_PAD;
        double* cur = lat + (f & 1) * RW + LAT_PAD;
        float en[MAXS];
        if (f + 1 < T) {                                   // the next frame's emissions, in flight under this frame's arithmetic
            const float* xr = x + (long)(t - step) * stride;
#pragma unroll
            for (int k = 0; k < MAXS; ++k) en[k] = xr[lab[k]];
        }
#pragma unroll
        for (int k = 0; k < MAXS; ++k) {
            const int s = tid + k * nt;
            if (s < S) {
                double v;
                if (f == 0) v = (dir == 0 ? s <= 1 : s >= S - 2) ? 0.0 : neg_inf();
                else v = lse3(prev[s], prev[s + step], skip[k] ? prev[s + 2 * step] : neg_inf());
                v += (double)e[k] * LOG2E_D;
                cur[s] = v;
                out[(long)t * W + s] = v;
            }
        }
        if (f + 1 < T) {
#pragma unroll
            for (int k = 0; k < MAXS; ++k) e[k] = en[k];
        }
        __syncthreads();
    }
    if (dir == 0 && tid == 0) {
        const double* last = lat + ((T - 1) & 1) * RW + LAT_PAD;
        loglik[b] = lse2(last[S - 1], last[S - 2]) * LN2_D;                  // (S == 1: last[-1] is the pad, -inf)
    }
}

// ---- the neighbours -----------------------------------------------------------------------------------------------------------------
constexpr int NB_WAVES = 4;

__device__ __forceinline__ double wave_lse(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = lse2(v, __shfl_xor(v, o, 64));
    return v;
}

// Task = (row, chunk of 64 classes); rows 0 .. Smax - 1 are the slots, Smax .. 2 Smax the gaps.  One wave per task.
__global__ __launch_bounds__(64 * NB_WAVES) void post_neighbours_kernel(const float* __restrict__ lp, const int* __restrict__ targets,
                                                                        const int* __restrict__ in_len, const int* __restrict__ tg_len,
                                                                        int B, int N, int C, long stride, int Smax, int blank, int chunks,
                                                                        const double* __restrict__ ws, const double* __restrict__ loglik,
                                                                        float* __restrict__ sub, float* __restrict__ ins) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const long task = (long)blockIdx.x * NB_WAVES + (threadIdx.x >> 6);
    if (task >= (long)(2 * Smax + 1) * chunks) return;     // (wave-uniform, as everything below but c and what hangs on it)
    const int r = (int)(task / chunks), chunk = (int)(task - (long)r * chunks);
    const int c = chunk * 64 + lane;
    const bool is_sub = r < Smax;
    const int idx = is_sub ? r : r - Smax;
    float* outp = is_sub ? sub + ((long)b * Smax + idx) * C : ins + ((long)b * (Smax + 1) + idx) * C;
    const int T = in_len[b], L = tg_len[b];
    const double ll = loglik[b];
    if (!finite_f64(ll) || !sizes_ok(T, L, N, Smax) || (is_sub ? idx >= L : idx > L)) {
        if (c < C) outp[c] = __builtin_nanf("");
        return;
    }
    const int W = 2 * Smax + 1;
    const int* y = targets + (long)b * Smax;
    const double* A = ws + (long)b * N * W;                // alpha rows
    const double* G = ws + ((long)B + b) * N * W;          // betahat rows
    const float* x = lp + (long)b * N * stride;
    const int cc = c < C ? c : C - 1;                      // lanes behind the last class repeat it and store nothing

    const int p = 2 * idx, q = is_sub ? p + 2 : p;
    const bool has_prev = idx > 0, has_next = is_sub ? idx + 1 < L : idx < L, last = !has_next;
    const int prev = has_prev ? y[idx - 1] : -1, next = has_next ? y[is_sub ? idx + 1 : idx] : -1;
    const bool use_prev = has_prev && cc != prev, use_next = has_next && cc != next;
    // a_t is -inf while t < p / 2 (alpha_{t-1}(p - 1) is), and betahat_{t+1}(q + 1) is -inf once fewer than L - 1 - q / 2 frames
    // follow frame t + 1: the chain runs over the frames between.  `last` has no such end: its term is a_{T-1} itself.
    // A wave whose only class is the blank (the last chunk where blank == C - 1 == 64 k) has no chain to run: the blank column is
    // the deletion in a slot and 0 in a gap.
    const bool no_chain = chunk * 64 == blank && blank + 1 == C;
    const int t0 = idx, t1 = no_chain ? idx - 1 : last ? T - 1 : T - 2 - (L - 1 - q / 2);
    double a = neg_inf(), R = neg_inf();
    float xt = t0 <= t1 ? x[(long)t0 * stride + cc] : 0.f;
    for (int t = t0; t <= t1; ++t) {
        const float xn = t < t1 ? x[(long)(t + 1) * stride + cc] : 0.f;     // the next frame's score, in flight under this step
        if (t == 0) a = 0.0;                               // t0 == 0: p == 0, the string may begin with c
        else {
            const double* At = A + (long)(t - 1) * W + p;
            a = lse3(a, At[0], use_prev ? At[-1] : neg_inf());
        }
        a += (double)xt * LOG2E_D;
        if (t < T - 1) {
            const double* Gt = G + (long)(t + 1) * W + q;
            R = lse2(R, a + (use_next ? lse2(Gt[0], Gt[1]) : Gt[0]));
        } else {
            R = lse2(R, a);                                // t == T - 1 is reached only where `last`
        }
        xt = xn;
    }
    if (is_sub && blank / 64 == chunk) {                   // the deletion of y_idx, summed over the frames by the lanes of this wave
        double D;
        if (idx == L - 1) {
            const double* At = A + (long)(T - 1) * W + p;
            D = lse2(At[0], has_prev ? At[-1] : neg_inf());
        } else {
            const bool hop = has_prev && prev != next;     // y_{i-1} straight to y_{i+1}
            D = neg_inf();
            for (int t = lane; t < T - 1; t += 64) {
                const double* At = A + (long)t * W + p;
                D = lse2(D, lse2(At[0], hop ? At[-1] : neg_inf()) + G[(long)(t + 1) * W + p + 3]);
            }
            if (idx == 0 && lane == 0) D = lse2(D, G[3]);  // the shortened string begins with y_1 at frame 0
            D = wave_lse(D);
        }
        if (cc == blank) R = D;
    }
    float llr = (float)((R - ll * LOG2E_D) * LN2_D);
    if (!is_sub && cc == blank) llr = 0.f;                 // nothing inserted: exactly 0
    if (c < C) outp[c] = llr;
}

// ---- the summary --------------------------------------------------------------------------------------------------------------------
struct Best { float v; int i; };
__device__ __forceinline__ void take(Best& b, float v, int i) { if (v > b.v || (v == b.v && i < b.i)) { b.v = v; b.i = i; } }

__global__ __launch_bounds__(256) void post_slots_kernel(const float* __restrict__ sub, const float* __restrict__ ins,
                                                         const int* __restrict__ targets, long rows, int C, int Smax, int blank,
                                                         float* __restrict__ post, int* __restrict__ alt, float* __restrict__ alt_post,
                                                         float* __restrict__ gap_post, int* __restrict__ gap_alt,
                                                         float* __restrict__ gap_alt_post) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int W = 2 * Smax + 1;
    const long b = row / W;
    const int r = (int)(row - b * W);
    const bool is_sub = r < Smax;
    const long o = is_sub ? b * Smax + r : b * (Smax + 1) + (r - Smax);
    const float* v = (is_sub ? sub : ins) + o * C;
    const int own = is_sub ? targets[o] : blank;
    Best best{-INFINITY, 0x7fffffff};
    float m = -INFINITY, own_v = -INFINITY;
    bool bad = false, have = false;
    for (int c = lane; c < C; c += 64) {
        const float t = v[c];
        bad |= t != t;
        m = fmaxf(m, t);
        if (c == own) { own_v = t; have = true; }
        else take(best, t, c);
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        m = fmaxf(m, __shfl_xor(m, s, 64));
        own_v = fmaxf(own_v, __shfl_xor(own_v, s, 64));
        take(best, __shfl_xor(best.v, s, 64), __shfl_xor(best.i, s, 64));
    }
    bad = __any(bad) || !__any(have) || !(fabsf(m) < INFINITY);
    double z = 0.0;
    if (!bad)
        for (int c = lane; c < C; c += 64) z += exp((double)v[c] - (double)m);
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) z += __shfl_xor(z, s, 64);
    if (lane == 0) {
        float* pp = is_sub ? post : gap_post;
        int* pa = is_sub ? alt : gap_alt;
        float* pq = is_sub ? alt_post : gap_alt_post;
        pp[o] = bad ? __builtin_nanf("") : (float)(exp((double)own_v - (double)m) / z);
        pa[o] = bad ? -1 : best.i;
        pq[o] = bad ? __builtin_nanf("") : (float)(exp((double)best.v - (double)m) / z);
    }
}

int64_t workspace_bytes_of(int64_t B, int64_t N, int64_t Smax) {
    if (B < 0 || N < 0 || Smax < 0 || Smax > MAX_LABELS || B >= (1ll << 31) || N >= (1ll << 31)) return -1;
    const int64_t W = 2 * Smax + 1;
    if (B * N > (1ll << 62) / (16 * W)) return -1;
    return 16 * B * N * W;
}

int check_common(const char* who, const float* log_probs, const int32_t* targets, const int32_t* input_lengths,
                 const int32_t* target_lengths, int64_t B, int64_t N, int64_t C, int64_t row_stride, int64_t Smax, int blank,
                 const void* workspace, int64_t workspace_bytes, const double* loglik) {
    SCONF_REQUIRE(B >= 0 && B < (1ll << 31) && N >= 0 && N < (1ll << 31), "%s: B=%ld, N=%ld out of range", who, (long)B, (long)N);
    SCONF_REQUIRE(Smax >= 0 && Smax <= MAX_LABELS, "%s: Smax=%ld labels; 0 .. %d", who, (long)Smax, MAX_LABELS);
    SCONF_REQUIRE(C >= 2 && C < (1ll << 30), "%s: C=%ld classes must be at least 2 (and below 2^30)", who, (long)C);
    SCONF_REQUIRE(blank >= 0 && blank < C, "%s: blank %d is outside 0 .. %ld", who, blank, (long)C - 1);
    SCONF_REQUIRE(row_stride >= C, "%s: row stride %ld is below C=%ld", who, (long)row_stride, (long)C);
    SCONF_REQUIRE(row_stride <= (1ll << 62) / ((B > 0 ? B : 1) * (N > 0 ? N : 1)), "%s: B * N * row_stride must be below 2^62", who);
    if (B == 0) return 0;
    SCONF_REQUIRE((log_probs || N == 0) && (targets || Smax == 0) && input_lengths && target_lengths && loglik,
                  "%s: null log_probs, targets, input_lengths, target_lengths or loglik", who);
    const int64_t need = workspace_bytes_of(B, N, Smax);
    SCONF_REQUIRE(need >= 0, "%s: the workspace of B=%ld, N=%ld, Smax=%ld overflows", who, (long)B, (long)N, (long)Smax);
    SCONF_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), "%s: workspace of %ld bytes, %ld needed", who, (long)workspace_bytes, (long)need);
    SCONF_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s: workspace must be 16-byte aligned", who);
    return 0;
}

}  // namespace

SCONF_API int sconf_post_max_labels(void) { return MAX_LABELS; }
SCONF_API int64_t sconf_post_workspace(int64_t B, int64_t N, int64_t Smax) { return workspace_bytes_of(B, N, Smax); }
SCONF_API int sconf_post_step_error(double* nats) {
    SCONF_REQUIRE(nats != nullptr, "sconf_post_step_error: null nats");
    *nats = STEP_ERROR;
    return 0;
}

SCONF_API int sconf_post_lattice(const float* log_probs, const int32_t* targets, const int32_t* input_lengths, const int32_t* target_lengths,
                                 int64_t B, int64_t N, int64_t C, int64_t row_stride, int64_t Smax, int blank, void* workspace,
                                 int64_t workspace_bytes, double* loglik, hipStream_t stream) {
    if (check_common("sconf_post_lattice", log_probs, targets, input_lengths, target_lengths, B, N, C, row_stride, Smax, blank, workspace,
                     workspace_bytes, loglik)) return 1;
    if (B == 0) return 0;
    const int W = (int)(2 * Smax + 1);
    const int nt = std::min(1024, std::max(64, cdiv(cdiv(W, 4), 64) * 64));          // four states a thread up to 4096 states, then eight
    const int spt = cdiv(W, nt);
    const size_t sh = (size_t)2 * (W + 2 * LAT_PAD) * sizeof(double);
#define POST_LATTICE(MS) do { \
        if (sh > 48 * 1024) (void)hipFuncSetAttribute((const void*)post_lattice_kernel<MS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh); \
        hipLaunchKernelGGL((post_lattice_kernel<MS>), dim3((unsigned)(2 * B)), dim3(nt), sh, stream, log_probs, (const int*)targets, \
                           (const int*)input_lengths, (const int*)target_lengths, (int)N, (int)C, (long)row_stride, (int)Smax, blank, \
                           (double*)workspace, loglik); } while (0)
    if (spt <= 1) POST_LATTICE(1); else if (spt <= 2) POST_LATTICE(2); else if (spt <= 4) POST_LATTICE(4); else POST_LATTICE(8);
#undef POST_LATTICE
    SCONF_LAUNCH_OK("sconf_post_lattice");
    return 0;
}

SCONF_API int sconf_post_neighbours(const float* log_probs, const int32_t* targets, const int32_t* input_lengths,
                                    const int32_t* target_lengths, int64_t B, int64_t N, int64_t C, int64_t row_stride, int64_t Smax,
                                    int blank, const void* workspace, int64_t workspace_bytes, const double* loglik, float* sub_llr,
                                    float* ins_llr, hipStream_t stream) {
    if (check_common("sconf_post_neighbours", log_probs, targets, input_lengths, target_lengths, B, N, C, row_stride, Smax, blank, workspace,
                     workspace_bytes, loglik)) return 1;
    SCONF_REQUIRE(B <= 65535, "sconf_post_neighbours: B=%ld samples; at most 65535 a call", (long)B);
    if (B == 0) return 0;
    SCONF_REQUIRE((sub_llr || Smax == 0) && ins_llr, "sconf_post_neighbours: null sub_llr or ins_llr");
    const int chunks = cdiv(C, 64);
    const long tasks = (long)(2 * Smax + 1) * chunks;
    SCONF_REQUIRE((tasks + NB_WAVES - 1) / NB_WAVES < (1ll << 31), "sconf_post_neighbours: (2 Smax + 1) * ceil(C / 64) waves are too many");
    hipLaunchKernelGGL(post_neighbours_kernel, dim3((unsigned)((tasks + NB_WAVES - 1) / NB_WAVES), (unsigned)B), dim3(64 * NB_WAVES), 0, stream, log_probs,
                       (const int*)targets, (const int*)input_lengths, (const int*)target_lengths, (int)B, (int)N, (int)C, (long)row_stride,
                       (int)Smax, blank, chunks, (const double*)workspace, loglik, sub_llr, ins_llr);
    SCONF_LAUNCH_OK("sconf_post_neighbours");
    return 0;
}

SCONF_API int sconf_post_slots(const float* sub_llr, const float* ins_llr, const int32_t* targets, int64_t B, int64_t C, int64_t Smax, int blank,
                               float* post, int32_t* alt, float* alt_post, float* gap_post, int32_t* gap_alt, float* gap_alt_post,
                               hipStream_t stream) {
    SCONF_REQUIRE(B >= 0 && B < (1ll << 31), "sconf_post_slots: B=%ld out of range", (long)B);
    SCONF_REQUIRE(Smax >= 0 && Smax <= MAX_LABELS, "sconf_post_slots: Smax=%ld labels; 0 .. %d", (long)Smax, MAX_LABELS);
    SCONF_REQUIRE(C >= 2 && C < (1ll << 30), "sconf_post_slots: C=%ld classes must be at least 2 (and below 2^30)", (long)C);
    SCONF_REQUIRE(blank >= 0 && blank < C, "sconf_post_slots: blank %d is outside 0 .. %ld", blank, (long)C - 1);
    if (B == 0) return 0;
    SCONF_REQUIRE(ins_llr && gap_post && gap_alt && gap_alt_post, "sconf_post_slots: null ins_llr, gap_post, gap_alt or gap_alt_post");
    SCONF_REQUIRE(Smax == 0 || (sub_llr && targets && post && alt && alt_post), "sconf_post_slots: null sub_llr, targets, post, alt or alt_post");
    const long rows = (long)B * (2 * Smax + 1);
    SCONF_REQUIRE((rows + 3) / 4 < (1ll << 31), "sconf_post_slots: B * (2 Smax + 1) rows are too many");
    hipLaunchKernelGGL(post_slots_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, sub_llr, ins_llr, (const int*)targets, rows, (int)C,
                       (int)Smax, blank, post, (int*)alt, alt_post, gap_post, (int*)gap_alt, gap_alt_post);
    SCONF_LAUNCH_OK("sconf_post_slots");
    return 0;
}
