// What csrc/align.hip (one lattice per workgroup, up to 8191 labels), csrc/align_long.hip (the lattice cut into state slabs, up to
// 65535 labels) and csrc/seg.hip (either of them with a star label) share: the workspace pitches, the emission gather, the emission
// loads of the lattice step, the walk back, the two output kernels and their launches.  An internal header: everything sits in an
// anonymous namespace, so each of the files instantiates its own copy (the kernels have internal linkage).  All of it indexes the
// lattice by its GLOBAL state over the whole 2 Smax + 1, so none of it knows whether one workgroup or a chain of slab launches
// filled the back-pointers.
#pragma once
#include "common.h"
#include <algorithm>

namespace {

constexpr int WALK_K = 16;                      // frames per walk-back window
constexpr int WALK_CELLS = 32;                  // cells fetched per row: >= 2 WALK_K - 1

// compact emission row: labels [0, LP), the blank at LP, 3 floats of padding; LP leaves a whole thread's worth of labels behind Smax
inline int label_pitch(int64_t Smax) { return (int)((Smax + 7) / 8 * 8 + 8); }
// back-pointer row: a multiple of 48 bytes, so that the last busy thread's 12- or 16-byte store ends inside its own row
inline int bp_pitch(int64_t Smax) { return (int)((2 * Smax + 1 + 47) / 48 * 48); }
// frames per walk-back fetch; measurement: SCONF_ALIGN_WALK_WINDOW=1 walks one frame per fetch
inline int walk_window() {
    int K = WALK_K;
    if (const char* e = getenv("SCONF_ALIGN_WALK_WINDOW")) { const int v = atoi(e); if (v >= 1 && v <= WALK_K) K = v; }
    return K;
}

// One workgroup per (sample, frame) row: the frame's log-probs go to LDS with 16-byte loads, the S + 1 emissions are gathered from
// there (ctc_gather_kernel's scheme).  Frames at or past the sample's length are never read by the lattice and are not written.
// STAR (csrc/seg.hip): the label value C is the star, whose cell is `star_logp` at every frame; the row that is read stays C wide.
template <bool STAR>
__global__ __launch_bounds__(256) void align_gather_kernel(const float* __restrict__ lp, const int* __restrict__ targets,
                                                           const int* __restrict__ in_len, const int* __restrict__ tg_len,
                                                           float* __restrict__ em, int B, int N, int C, int Smax, int LP, int blank,
                                                           float star_logp) {
    extern __shared__ float row[];                      // [C]
    const int E = LP + 4;
    for (long bt = blockIdx.x; bt < (long)B * N; bt += gridDim.x) {
        const int t = (int)(bt % N), b = (int)(bt / N);
        if (t >= len_of(in_len, b, N)) continue;         // (uniform over the workgroup)
        const int S = min(max(len_of(tg_len, b, Smax), 0), Smax);
        __syncthreads();                                // the previous row's gathers are done
        const float* src = lp + bt * C;
        for (int c = threadIdx.x * 4; c < C; c += 1024) *reinterpret_cast<float4*>(row + c) = *reinterpret_cast<const float4*>(src + c);
        __syncthreads();
        float* out = em + bt * E;
        for (int j = threadIdx.x; j < E; j += 256) {
            float v = 0.f;
            if (j < S) {
                const int lab = targets[(long)b * Smax + j];
                v = row[min(max(lab, 0), C - 1)];       // an out-of-range label poisons the sample; never index with it
                if (STAR && lab == C) v = star_logp;
            }
            else if (j == LP) v = row[blank];
            out[j] = v;
        }
    }
}

template <int NL> __device__ __forceinline__ void load_labels(const float* p, float (&v)[NL]) {
    if constexpr (NL % 4 == 0) {
#pragma unroll
        for (int i = 0; i < NL; i += 4) { const float4 x = *reinterpret_cast<const float4*>(p + i); v[i] = x.x; v[i + 1] = x.y; v[i + 2] = x.z; v[i + 3] = x.w; }
    } else if constexpr (NL % 2 == 0) {
#pragma unroll
        for (int i = 0; i < NL; i += 2) { const float2 x = *reinterpret_cast<const float2*>(p + i); v[i] = x.x; v[i + 1] = x.y; }
    } else {
#pragma unroll
        for (int i = 0; i < NL; ++i) v[i] = p[i];
    }
}

// One wave per sample.  Also sets every span of the sample to (-1, -1); the frame kernel then writes those of the tokens on the path.
__global__ __launch_bounds__(64) void align_walk_kernel(const unsigned char* __restrict__ bp, const int* __restrict__ endst,
                                                        const int* __restrict__ in_len, int* __restrict__ path, int* __restrict__ spans,
                                                        int N, int Smax, int BPW, int K) {
    __shared__ unsigned char win[WALK_K][WALK_CELLS];
    __shared__ int st[WALK_K + 1];
    const int b = blockIdx.x, lane = threadIdx.x;
    for (int i = lane; i < 2 * Smax; i += 64) spans[(long)b * 2 * Smax + i] = -1;
    const int e = endst[b];
    if (e < 0) return;
    int t = len_of(in_len, b, N) - 1, s = e;            // (T is in 1..N: the lattice kernel has checked it)
    const unsigned char* base = bp + (long)b * N * BPW;
    const int r = lane >> 2, q = lane & 3;
    while (t >= 0) {
        const int kk = min(K, t + 1);
        if (r < kk) {                                     // row r of the window: frame t - r, cells s - 31 .. s
            const unsigned char* rowp = base + (long)(t - r) * BPW;
            unsigned char c[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) c[j] = rowp[max(s - (WALK_CELLS - 1) + q * 8 + j, 0)];
#pragma unroll
            for (int j = 0; j < 8; ++j) win[r][q * 8 + j] = c[j];
        }
        __syncthreads();
        if (lane == 0) {
            int cs = s;
            for (int k = 0; k < kk; ++k) {
                st[k] = cs;
                if (t - k > 0) cs = max(cs - min((int)(win[k][WALK_CELLS - 1 - (s - cs)] & 3), 2), 0);
            }
            st[WALK_K] = cs;
        }
        __syncthreads();
        if (lane < kk) path[(long)b * N + t - lane] = st[lane];
        s = st[WALK_K];
        t -= kk;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void align_frames_kernel(const int* __restrict__ targets, const int* __restrict__ endst,
                                                           const int* __restrict__ in_len, int* __restrict__ path, int* __restrict__ labels,
                                                           int* __restrict__ spans, int N, int Smax, int blank) {
    const int b = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
    if (t >= N) return;
    const long o = (long)b * N + t;
    if (endst[b] < 0) { path[o] = -1; labels[o] = -1; return; }
    const int T = len_of(in_len, b, N);
    if (t >= T) { path[o] = -1; labels[o] = -1; return; }
    const int s = path[o];
    if (s & 1) {
        const int j = s >> 1;
        labels[o] = targets[(long)b * Smax + j];
        if (t == 0 || path[o - 1] != s) spans[((long)b * Smax + j) * 2] = t;
        if (t == T - 1 || path[o + 1] != s) spans[((long)b * Smax + j) * 2 + 1] = t + 1;
    } else labels[o] = blank;
}

// STAR: a token whose label is C sums `star_logp` once per frame of its span instead of a log-prob.
template <bool STAR>
__global__ __launch_bounds__(256) void align_tokens_kernel(const float* __restrict__ lp, const int* __restrict__ targets,
                                                           const int* __restrict__ endst, const int* __restrict__ in_len,
                                                           const int* __restrict__ tg_len, int* __restrict__ spans, float* __restrict__ token_logp,
                                                           int N, int C, int Smax, float star_logp) {
    const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= Smax) return;
    const long o = (long)b * Smax + j;
    float sum = 0.f;
    if (endst[b] >= 0 && j < len_of(tg_len, b, Smax)) {
        const int lab = targets[o], f = spans[2 * o], l = min(spans[2 * o + 1], len_of(in_len, b, N));
        if (STAR && lab == C) { if (f >= 0) for (int t = f; t < l; ++t) sum += star_logp; }
        else if (f >= 0) for (int t = f; t < l; ++t) sum += lp[((long)b * N + t) * C + lab];  // (f < 0: only a path through non-finite log-probs skips a token)
    } else { spans[2 * o] = -1; spans[2 * o + 1] = -1; }
    token_logp[o] = sum;
}

// Steps 1 and 3 to 5 of a call as launches, the same for every lattice form.
template <bool STAR>
inline void launch_align_gather(const float* log_probs, const int* targets, const int* input_lengths, const int* target_lengths, float* em,
                                int64_t B, int64_t N, int64_t C, int64_t Smax, int LP, int blank, float star_logp, hipStream_t stream) {
    hipLaunchKernelGGL(align_gather_kernel<STAR>, dim3((unsigned)std::min<long>(B * N, 65536)), dim3(256), (size_t)C * 4, stream, log_probs, targets,
                       input_lengths, target_lengths, em, (int)B, (int)N, (int)C, (int)Smax, LP, blank, star_logp);
}

template <bool STAR>
inline void launch_align_outputs(const float* log_probs, const int* targets, const int* input_lengths, const int* target_lengths,
                                 const unsigned char* bp, const int* endst, int* path, int* labels, int* spans, float* token_logp, int64_t B,
                                 int64_t N, int64_t C, int64_t Smax, int BPW, int blank, float star_logp, hipStream_t stream) {
    hipLaunchKernelGGL(align_walk_kernel, dim3((unsigned)B), dim3(64), 0, stream, bp, endst, input_lengths, path, spans, (int)N, (int)Smax, BPW,
                       walk_window());
    hipLaunchKernelGGL(align_frames_kernel, dim3((unsigned)cdiv(N, 256), (unsigned)B), dim3(256), 0, stream, targets, endst, input_lengths,
                       path, labels, spans, (int)N, (int)Smax, blank);
    if (Smax > 0)
        hipLaunchKernelGGL(align_tokens_kernel<STAR>, dim3((unsigned)cdiv(Smax, 256), (unsigned)B), dim3(256), 0, stream, log_probs, targets, endst,
                           input_lengths, target_lengths, spans, token_logp, (int)N, (int)C, (int)Smax, star_logp);
}

}  // namespace
