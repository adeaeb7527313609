// Confidence scores (include/sconf_confid.h): a confidence and the argmax of every frame in one pass over the log-scores, the greedy
// CTC collapse of the argmax vector with the frames of every label, and the aggregation of spans of frames (or tokens) to one
// value each.  What NeMo's ConfidenceConfig computes on the host, without a host read.
//
// Built WITHOUT -ffast-math (see the Makefile): the sums keep their written order, the per-row logf and expf are the HIP math
// library's, and v != v must stay a NaN test.
#include "common.h"
#include "../../include/sconf_confid.h"
#include "confid_measure.h"

namespace {

constexpr int SCAN_PER_THREAD = 4;
constexpr int SCAN_CHUNK = BLOCK * SCAN_PER_THREAD;

// A row in the registers of G lanes (16: four rows per wave, for the short rows of a 129- or 144-class model, so that a wave has
// several 16-byte loads per lane in flight; 64: one row per wave).  Lane g of the group holds the quads g, g + G, ... of four
// neighbouring elements, so that the 16-byte path and the element path sum in one order.
template <int METHOD, int G, int NQ>
__global__ __launch_bounds__(BLOCK) void frames_group_kernel(const float* __restrict__ x, long M, int C, long stride, int vec, Measure q,
                                                             int* __restrict__ idx, float* __restrict__ conf) {
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
    Sums s{0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NQ; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) add<METHOD>(s, v[j][e] - b.v, q.alpha);
    s.z = group_sum<G>(s.z);
    if (METHOD == SCONF_CONFID_SHANNON) s.t = group_sum<G>(s.t);
    if (METHOD == SCONF_CONFID_TSALLIS || METHOD == SCONF_CONFID_RENYI) s.a = group_sum<G>(s.a);
    if (g == 0 && live) {
        idx[row] = bad ? -1 : b.i;
        conf[row] = bad ? __builtin_nanf("") : confidence<METHOD>(s, q);
    }
}

// A row above the wave's capacity: one workgroup per row; thread t holds the quads t, t + 256, ...  REG: the row stays in the
// registers of the workgroup (up to BLOCK_CAPACITY classes).  Otherwise two passes (maximum, then the sums), the second of which
// finds the row in the cache.  The four waves' results are combined in wave order.
template <int METHOD, bool REG>
__global__ __launch_bounds__(BLOCK) void frames_block_kernel(const float* __restrict__ x, int C, long stride, int vec, Measure q,
                                                             int* __restrict__ idx, float* __restrict__ conf) {
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
        if (threadIdx.x == 0) { idx[row] = -1; conf[row] = __builtin_nanf(""); }
        return;
    }
    Sums s{0.f, 0.f, 0.f};
    if (REG) {
#pragma unroll
        for (int j = 0; j < QUADS; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) add<METHOD>(s, keep[REG ? j : 0][e] - b.v, q.alpha);
    } else {
        for (int k = threadIdx.x; k < nq; k += BLOCK) {
            float v[4];
            load_quad(xr, k * 4, C, vec, v);
#pragma unroll
            for (int e = 0; e < 4; ++e) add<METHOD>(s, v[e] - b.v, q.alpha);
        }
    }
    s.z = wave_sum(s.z); s.t = wave_sum(s.t); s.a = wave_sum(s.a);
    if (lane == 0) { shv[wv][1] = s.z; shv[wv][2] = s.t; shv[wv][3] = s.a; }
    __syncthreads();
    if (threadIdx.x == 0) {
        Sums r{0.f, 0.f, 0.f};
#pragma unroll
        for (int w = 0; w < BLOCK / 64; ++w) { r.z += shv[w][1]; r.t += shv[w][2]; r.a += shv[w][3]; }
        idx[row] = b.i; conf[row] = confidence<METHOD>(r, q);
    }
}

// One workgroup per sequence.  Thread t of a step looks at the frames base + 4 t .. base + 4 t + 3; an inclusive scan of the
// "opens a label" flags over the workgroup, on top of the count carried from the steps before, numbers the labels.  The frame
// before and the frame after a frame are read from memory, so a run that straddles two steps needs nothing but the count.
__global__ __launch_bounds__(BLOCK) void runs_kernel(const int* __restrict__ idx, const int* __restrict__ lengths, int N, int blank,
                                                     int* __restrict__ targets, int* __restrict__ spans, int* __restrict__ target_lengths,
                                                     int S_cap) {
    __shared__ int wave_total[BLOCK / 64];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int* row = idx + (long)b * N;
    int* tg = targets + (long)b * S_cap;
    int* sp = spans + (long)b * S_cap * 3;
    const int len = min(max(len_of(lengths, b, N), 0), N);
    int carry = 0;
    for (int base = 0; base < len; base += SCAN_CHUNK) {
        const int t0 = base + threadIdx.x * SCAN_PER_THREAD;
        int cur[SCAN_PER_THREAD + 2];                                      // the frame before, the four frames, the frame after
#pragma unroll
        for (int e = 0; e < SCAN_PER_THREAD + 2; ++e) {
            const int t = t0 - 1 + e;
            cur[e] = t >= 0 && t < len ? row[t] : -1;                      // -1: no label and equal to no label
        }
        int opens[SCAN_PER_THREAD], mine = 0;
#pragma unroll
        for (int e = 0; e < SCAN_PER_THREAD; ++e) {
            const int c = cur[e + 1];
            opens[e] = c >= 0 && c != blank && c != cur[e];
            mine += opens[e];
        }
        int incl = mine;                                                   // inclusive scan over the wave, then over the waves
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int up = __shfl_up(incl, o, 64); if (lane >= o) incl += up; }
        __syncthreads();                                                   // the totals of the step before have been read
        if (lane == 63) wave_total[wv] = incl;
        __syncthreads();
        int before = carry, total = carry;
#pragma unroll
        for (int w = 0; w < BLOCK / 64; ++w) { if (w < wv) before += wave_total[w]; total += wave_total[w]; }
        int k = before + incl - mine;                                      // labels opened before this thread's frames
#pragma unroll
        for (int e = 0; e < SCAN_PER_THREAD; ++e) {
            const int t = t0 + e, c = cur[e + 1];
            if (opens[e]) {
                if (k < S_cap) { tg[k] = c; sp[3 * k] = t; }
                if (k >= 1 && k - 1 < S_cap) sp[3 * (k - 1) + 2] = t;
                ++k;
            }
            if (c >= 0 && c != blank && c != cur[e + 2] && k >= 1 && k - 1 < S_cap) sp[3 * (k - 1) + 1] = t + 1;     // the run of label k - 1 ends
        }
        carry = total;
    }
    if (carry >= 1 && carry - 1 < S_cap && threadIdx.x == 0) sp[3 * (carry - 1) + 2] = len;
    for (int k = min(carry, S_cap) + threadIdx.x; k < S_cap; k += BLOCK) { tg[k] = 0; sp[3 * k] = 0; sp[3 * k + 1] = 0; sp[3 * k + 2] = 0; }
    if (threadIdx.x == 0) target_lengths[b] = carry > S_cap ? -1 : carry;
}

// One wave per span.  Two accumulators side by side - over the frames that are kept and over all frames - so that the fallback of a
// span with nothing but blanks costs no second pass.
template <int AGG> __device__ __forceinline__ float agg_unit() {
    return AGG == SCONF_CONFID_MIN ? INFINITY : AGG == SCONF_CONFID_MAX ? -INFINITY : AGG == SCONF_CONFID_PROD ? 1.f : 0.f;
}
template <int AGG> __device__ __forceinline__ float agg2(float a, float v) {
    return AGG == SCONF_CONFID_MIN ? fminf(a, v) : AGG == SCONF_CONFID_MAX ? fmaxf(a, v) : AGG == SCONF_CONFID_PROD ? a * v : a + v;
}
template <int AGG> __device__ __forceinline__ float wave_agg(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = agg2<AGG>(v, __shfl_xor(v, o, 64));
    return v;
}

template <int AGG>
__global__ __launch_bounds__(BLOCK) void aggregate_kernel(const float* __restrict__ values, const int* __restrict__ idx, int blank, int M,
                                                          const int* __restrict__ spans, long S, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long s = (long)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
    if (s >= S) return;
    const int a = spans[2 * s], b = spans[2 * s + 1];
    if (a < 0 || b > M || a >= b) {                                        // empty, or refused: nothing of values is read
        if (lane == 0) out[s] = __builtin_nanf("");
        return;
    }
    float kept = agg_unit<AGG>(), all = agg_unit<AGG>();
    int n_kept = 0, n_all = 0;
    bool nan_kept = false, nan_all = false;
    for (int t = a + lane; t < b; t += 64) {
        const float v = values[t];
        const bool nan = v != v;
        int keep = 1;
        if (idx) { const int c = idx[t]; keep = c >= 0 && c != blank; }
        all = agg2<AGG>(all, v); ++n_all; nan_all |= nan;
        if (keep) { kept = agg2<AGG>(kept, v); ++n_kept; nan_kept |= nan; }
    }
    kept = wave_agg<AGG>(kept); all = wave_agg<AGG>(all);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { n_kept += __shfl_xor(n_kept, o, 64); n_all += __shfl_xor(n_all, o, 64); }
    nan_kept = __any(nan_kept); nan_all = __any(nan_all);
    if (lane == 0) {
        const bool use_all = n_kept == 0;
        float r = use_all ? all : kept;
        if (AGG == SCONF_CONFID_MEAN) r /= (float)(use_all ? n_all : n_kept);
        out[s] = (use_all ? nan_all : nan_kept) ? __builtin_nanf("") : r;
    }
}

template <int METHOD, int G, int NQ>
void launch_group(const float* x, long M, int C, long stride, int vec, const Measure& q, int* idx, float* conf, hipStream_t st) {
    hipLaunchKernelGGL((frames_group_kernel<METHOD, G, NQ>), dim3((unsigned)cdiv(M, BLOCK / G)), dim3(BLOCK), 0, st, x, M, C, stride, vec, q, idx, conf);
}

template <int METHOD>
void launch_frames(const float* x, long M, int C, long stride, int vec, const Measure& q, int* idx, float* conf, hipStream_t st) {
    if (C <= 64) launch_group<METHOD, 16, 1>(x, M, C, stride, vec, q, idx, conf, st);
    else if (C <= 128) launch_group<METHOD, 16, 2>(x, M, C, stride, vec, q, idx, conf, st);
    else if (C <= 192) launch_group<METHOD, 16, 3>(x, M, C, stride, vec, q, idx, conf, st);
    else if (C <= 256) launch_group<METHOD, 16, 4>(x, M, C, stride, vec, q, idx, conf, st);
    else if (C <= 512) launch_group<METHOD, 64, 2>(x, M, C, stride, vec, q, idx, conf, st);
    else if (C <= ROW_CAPACITY) launch_group<METHOD, 64, QUADS>(x, M, C, stride, vec, q, idx, conf, st);
    else if (C <= BLOCK_CAPACITY) hipLaunchKernelGGL((frames_block_kernel<METHOD, true>), dim3((unsigned)M), dim3(BLOCK), 0, st, x, C, stride, vec, q, idx, conf);
    else hipLaunchKernelGGL((frames_block_kernel<METHOD, false>), dim3((unsigned)M), dim3(BLOCK), 0, st, x, C, stride, vec, q, idx, conf);
}

}  // namespace

SCONF_API int sconf_confid_row_capacity(void) { return ROW_CAPACITY; }
SCONF_API int sconf_confid_block_capacity(void) { return BLOCK_CAPACITY; }
SCONF_API int sconf_confid_scan_chunk(void) { return SCAN_CHUNK; }

SCONF_API int sconf_confid_frames(const float* x, int64_t M, int64_t classes, int64_t row_stride, int method, int norm, float alpha,
                                  int32_t* idx, float* conf, hipStream_t stream) {
    SCONF_REQUIRE(M >= 0 && M < (1L << 31), "sconf_confid_frames: M=%ld must be in 0 .. 2^31 - 1", (long)M);
    SCONF_REQUIRE(classes >= 2 && classes < (1L << 30), "sconf_confid_frames: classes=%ld must be at least 2 (and below 2^30)", (long)classes);
    SCONF_REQUIRE(row_stride >= classes, "sconf_confid_frames: row stride %ld is below classes=%ld", (long)row_stride, (long)classes);
    SCONF_REQUIRE(row_stride <= (1L << 62) / (M > 0 ? M : 1), "sconf_confid_frames: M * row_stride must be below 2^62");
    SCONF_REQUIRE(method >= SCONF_CONFID_MAX_PROB && method <= SCONF_CONFID_RENYI, "sconf_confid_frames: unknown method %d", method);
    SCONF_REQUIRE(norm == SCONF_CONFID_LIN || norm == SCONF_CONFID_EXP, "sconf_confid_frames: unknown norm %d", norm);
    SCONF_REQUIRE(!(method == SCONF_CONFID_MAX_PROB && norm == SCONF_CONFID_EXP),
                  "sconf_confid_frames: max_prob has no exp normalisation: norm must be lin");
    const bool with_alpha = method == SCONF_CONFID_TSALLIS || method == SCONF_CONFID_RENYI;
    if (with_alpha && alpha == 1.f) method = SCONF_CONFID_SHANNON;                // the limit of both, taken here: no 1 / (alpha - 1)
    else SCONF_REQUIRE(!with_alpha || alpha_ok(alpha), "sconf_confid_frames: alpha=%g must be in (0, 1), 1 or (1, 4]", (double)alpha);
    SCONF_REQUIRE(x && idx && conf, "sconf_confid_frames: null x, idx or conf");
    if (M == 0) return 0;
    const Measure q = measure_of(method, norm, alpha, classes);
    const int vec = ((uintptr_t)x % 16 == 0) && row_stride % 4 == 0;
    switch (method) {
        case SCONF_CONFID_MAX_PROB: launch_frames<SCONF_CONFID_MAX_PROB>(x, M, (int)classes, row_stride, vec, q, idx, conf, stream); break;
        case SCONF_CONFID_SHANNON: launch_frames<SCONF_CONFID_SHANNON>(x, M, (int)classes, row_stride, vec, q, idx, conf, stream); break;
        case SCONF_CONFID_TSALLIS: launch_frames<SCONF_CONFID_TSALLIS>(x, M, (int)classes, row_stride, vec, q, idx, conf, stream); break;
        default: launch_frames<SCONF_CONFID_RENYI>(x, M, (int)classes, row_stride, vec, q, idx, conf, stream); break;
    }
    SCONF_LAUNCH_OK("sconf_confid_frames");
    return 0;
}

SCONF_API int sconf_confid_runs(const int32_t* idx, const int32_t* lengths, int64_t B, int64_t N, int blank, int32_t* targets,
                                int32_t* spans, int32_t* target_lengths, int64_t S_cap, hipStream_t stream) {
    SCONF_REQUIRE(B >= 0 && B < (1L << 31), "sconf_confid_runs: B=%ld must be in 0 .. 2^31 - 1", (long)B);
    SCONF_REQUIRE(N >= 0 && N < (1L << 31) - SCAN_CHUNK, "sconf_confid_runs: N=%ld must be in 0 .. 2^31 - 1 - %d", (long)N, SCAN_CHUNK);
    SCONF_REQUIRE(S_cap >= 0 && S_cap < (1L << 31) / 3, "sconf_confid_runs: S_cap=%ld must be in 0 .. (2^31 - 1) / 3", (long)S_cap);
    SCONF_REQUIRE(target_lengths && (idx || N == 0) && ((targets && spans) || S_cap == 0), "sconf_confid_runs: null idx, targets, spans or target_lengths");
    if (B == 0) return 0;
    hipLaunchKernelGGL(runs_kernel, dim3((unsigned)B), dim3(BLOCK), 0, stream, idx, lengths, (int)N, blank, targets, spans, target_lengths, (int)S_cap);
    SCONF_LAUNCH_OK("sconf_confid_runs");
    return 0;
}

SCONF_API int sconf_confid_aggregate(const float* values, const int32_t* idx, int blank, int64_t M, const int32_t* spans, int64_t S,
                                     int aggregation, float* out, hipStream_t stream) {
    SCONF_REQUIRE(M >= 0 && M < (1L << 31) - 64, "sconf_confid_aggregate: M=%ld must be in 0 .. 2^31 - 65", (long)M);
    SCONF_REQUIRE(S >= 0 && S < (1L << 31), "sconf_confid_aggregate: S=%ld must be in 0 .. 2^31 - 1", (long)S);
    SCONF_REQUIRE(aggregation >= SCONF_CONFID_MEAN && aggregation <= SCONF_CONFID_PROD, "sconf_confid_aggregate: unknown aggregation %d", aggregation);
    SCONF_REQUIRE((values || M == 0) && ((spans && out) || S == 0), "sconf_confid_aggregate: null values, spans or out");
    if (S == 0) return 0;
    const dim3 grid((unsigned)cdiv(S, BLOCK / 64)), block(BLOCK);
    switch (aggregation) {
        case SCONF_CONFID_MEAN: hipLaunchKernelGGL(aggregate_kernel<SCONF_CONFID_MEAN>, grid, block, 0, stream, values, idx, blank, (int)M, spans, (long)S, out); break;
        case SCONF_CONFID_MIN: hipLaunchKernelGGL(aggregate_kernel<SCONF_CONFID_MIN>, grid, block, 0, stream, values, idx, blank, (int)M, spans, (long)S, out); break;
        case SCONF_CONFID_MAX: hipLaunchKernelGGL(aggregate_kernel<SCONF_CONFID_MAX>, grid, block, 0, stream, values, idx, blank, (int)M, spans, (long)S, out); break;
        default: hipLaunchKernelGGL(aggregate_kernel<SCONF_CONFID_PROD>, grid, block, 0, stream, values, idx, blank, (int)M, spans, (long)S, out); break;
    }
    SCONF_LAUNCH_OK("sconf_confid_aggregate");
    return 0;
}
