// Test-time adaptation helpers (dynamic evaluation, lcasr/eval/dynamic_eval.py:11-142) and SpecAugment:
//   * band masking fused with the batch repeat + clone       (lcasr/utils/augmentation.py:75-100, dynamic_eval.py:84-86)
//   * deterministic mean of a spectrogram to a device scalar  (augmentation.py:73)
//   * greedy CTC pseudo-labels without leaving the device     (lcasr/decoding/greedy.py:19-21, dynamic_eval.py:92-93)
// All HBM-bound single-pass kernels.
#include "common.h"
#include <algorithm>

namespace {

constexpr int MASK_CHUNK = 4096;      // elements of one (b, f) row per workgroup: 4 x 16 B per thread

__device__ __forceinline__ bool in_any(const int* __restrict__ iv, int n, int v) {
    bool hit = false;
    for (int i = 0; i < n; ++i) hit |= v >= iv[2 * i] && v < iv[2 * i + 1];
    return hit;
}

// dst[b,f,t] = *mask_value where t is in one of row b's time intervals or f in one of its frequency intervals, else
// src[b,f,t] (src batch stride sb elements; 0 broadcasts one window to every copy).  grid = (B*F, ceil(T / MASK_CHUNK)).
// A row is moved in 16-byte accesses when its source and destination addresses are congruent modulo 16 (always so when
// T % 4 == 0): `head` scalar elements up to the first 16-byte boundary, float4 groups, scalar tail.  Chunk c > 0 starts at
// c * MASK_CHUNK + head so that no group straddles two workgroups.  Otherwise the row goes element by element.
__global__ __launch_bounds__(256) void spec_mask_kernel(const float* __restrict__ src, long sb, float* __restrict__ dst, int F, long T,
                                                        const int* __restrict__ t_iv, int n_t, const int* __restrict__ f_iv, int n_f,
                                                        const float* __restrict__ mask_value) {
    const long row = blockIdx.x;
    const long b = row / F;
    const int f = (int)(row - b * F);
    const float* s = src + b * sb + (long)f * T;
    float* d = dst + row * T;
    const float mv = *mask_value;
    const int* tv = t_iv + b * n_t * 2;
    const bool whole = in_any(f_iv + b * n_f * 2, n_f, f);       // the frequency bin is masked: no need to read the source
    const int as = (int)(((uintptr_t)s >> 2) & 3), ad = (int)(((uintptr_t)d >> 2) & 3);
    const bool vec = as == ad;
    const long head = vec ? ((4 - ad) & 3) : 0;
    const long c = blockIdx.y;
    const long lo = c == 0 ? 0 : c * MASK_CHUNK + head;
    const long hi = std::min<long>(T, (c + 1) * MASK_CHUNK + head);
    if (lo >= hi) return;
    long v0 = lo, v1 = lo;                                       // [v0, v1): the part moved as float4 groups
    if (vec) { v0 = std::min<long>(std::max<long>(lo, head), hi); v1 = v0 + (hi - v0) / 4 * 4; }
    for (long g = v0 + 4L * threadIdx.x; g < v1; g += 4 * 256) {
        float v[4];
        if (whole) { v[0] = v[1] = v[2] = v[3] = mv; }
        else {
            load4(s + g, v);
#pragma unroll
            for (int e = 0; e < 4; ++e) if (in_any(tv, n_t, (int)(g + e))) v[e] = mv;
        }
        store4(d + g, v);
    }
    // scalar parts: [lo, v0) (at most 3 elements, chunk 0 only) and [v1, hi) (at most 3 at the end of the row, or everything
    // when the row cannot be vectorised)
    for (long t = lo + threadIdx.x; t < v0; t += 256) d[t] = (whole || in_any(tv, n_t, (int)t)) ? mv : s[t];
    for (long t = v1 + threadIdx.x; t < hi; t += 256) d[t] = (whole || in_any(tv, n_t, (int)t)) ? mv : s[t];
}

constexpr int MEAN_BLOCKS = 1024;     // upper bound of stage-1 workgroups = partial sums

// Stage 1 of the mean: workgroup g adds its share in a fixed order (thread-strided f32 sums, wave tree, waves in order)
// and writes ONE f64 partial.  x is (B, R, T); with lengths only t < min(lengths[b], T) of every row counts (and is read).
__global__ __launch_bounds__(256) void mean_partial_kernel(const float* __restrict__ x, long B, long R, long T,
                                                           const int* __restrict__ lengths, double* __restrict__ partial) {
    __shared__ float sh[16];
    float a = 0.f;
    if (lengths == nullptr) {
        const long n = B * R * T;
        const bool vec = (((uintptr_t)x) & 15) == 0;
        const long n4 = vec ? n / 4 : 0;
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
            float v[4]; load4(x + 4 * i, v);
            a += (v[0] + v[1]) + (v[2] + v[3]);
        }
        for (long i = 4 * n4 + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) a += x[i];
    } else {
        for (long row = blockIdx.x; row < B * R; row += gridDim.x) {
            const long L = std::min<long>(std::max(lengths[row / R], 0), T);
            const float* xr = x + row * T;
            for (long t = threadIdx.x; t < L; t += 256) a += xr[t];
        }
    }
    const float tot = block_sum(a, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = (double)tot;
}

// Stage 2: one wave.  Lane l adds its ceil(np / 64) consecutive partials in index order, the 64 lane sums go through the fixed
// xor tree; the element count comes from the lengths, if given, in the same way.
__global__ __launch_bounds__(64) void mean_finish_kernel(const double* __restrict__ partial, int np, long B, long R, long T,
                                                         const int* __restrict__ lengths, float* __restrict__ out) {
    const int lane = threadIdx.x;
    const int per = (np + 63) / 64;
    double s = 0.0;
    for (int i = lane * per; i < min((lane + 1) * per, np); ++i) s += partial[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    long long cnt = (long long)B * R * T;
    if (lengths != nullptr) {
        cnt = 0;
        for (long b = lane; b < B; b += 64) cnt += R * std::min<long>(std::max(lengths[b], 0), T);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    }
    if (lane == 0) *out = (float)(s / (double)cnt);             // 0 / 0 = NaN, torch's mean of an empty selection
}

// One wave per sequence over its frame arg-maxes, 64 frames per tile: lane l keeps frame base + l when it lies below the
// sequence length, differs from its predecessor (the previous tile's last frame for lane 0) and is not blank; the kept
// frames are compacted with a ballot and a prefix popcount, the running offset carries from tile to tile.  More labels than
// S_cap: nothing is written past the buffer and target_lengths[b] = -1.
__global__ __launch_bounds__(64) void collapse_compact_kernel(const int* __restrict__ idx, long N, const int* __restrict__ lengths,
                                                              int blank, int* __restrict__ targets, long S_cap,
                                                              int* __restrict__ target_lengths) {
    const long b = blockIdx.x;
    const int lane = threadIdx.x;
    const long L = lengths ? std::min<long>(std::max(lengths[b], 0), N) : N;
    const int* ib = idx + b * N;
    int* tb = targets + b * S_cap;
    long off = 0;
    int carry = -1;                                             // no predecessor: every label differs from it
    for (long base = 0; base < L; base += 256) {                // 4 tiles per trip: their loads are in flight together
        int c4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { const long n = base + 64 * j + lane; c4[j] = n < L ? ib[n] : -1; }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int cur = c4[j];                              // -1 beyond the sequence: never kept, never a predecessor of a kept frame
            int prev = __shfl_up(cur, 1, 64);
            if (lane == 0) prev = carry;
            const bool keep = cur >= 0 && cur != prev && cur != blank;
            const unsigned long long m = __ballot(keep);
            const long pos = off + __popcll(m & ((1ull << lane) - 1ull));
            if (keep && pos < S_cap) tb[pos] = cur;
            off += __popcll(m);
            carry = __shfl(cur, 63, 64);
        }
    }
    if (lane == 0) target_lengths[b] = off > S_cap ? -1 : (int)off;
}

}  // namespace

// dst (B,F,T) = src (Bs,F,T; batch stride src_batch_stride elements, 0 = broadcast) with the union of row b's time intervals
// t_iv (B,n_t,2) and frequency intervals f_iv (B,n_f,2), half-open [start, end), filled with *mask_value (device f32).
// Replaces SpecAugment.forward's masked_fill sequence (lcasr/utils/augmentation.py:83-98) and, with stride 0, the
// repeat + clone in front of it (lcasr/eval/dynamic_eval.py:84-86).
SCONF_API int sconf_spec_mask(const float* src, int64_t src_batch_stride, float* dst, int64_t B, int64_t F, int64_t T,
                              const int32_t* t_iv, int64_t n_t, const int32_t* f_iv, int64_t n_f, const float* mask_value,
                              hipStream_t stream) {
    SCONF_REQUIRE(B >= 0 && F >= 0 && T >= 0 && n_t >= 0 && n_f >= 0 && src_batch_stride >= 0, "sconf_spec_mask: negative size");
    SCONF_REQUIRE(T <= 0x7fffffffL && F <= 0x7fffffffL, "sconf_spec_mask: F and T must fit 32 bits (intervals are int32)");
    SCONF_REQUIRE(B * F <= 0x7fffffffL && cdiv(T, MASK_CHUNK) <= 65535, "sconf_spec_mask: grid too large (B*F=%ld, T=%ld)", (long)(B * F), (long)T);
    SCONF_REQUIRE(n_t <= 64 && n_f <= 64, "sconf_spec_mask: at most 64 masks per axis");
    if (B == 0 || F == 0 || T == 0) return 0;
    SCONF_REQUIRE(src && dst && mask_value && (n_t == 0 || t_iv) && (n_f == 0 || f_iv), "sconf_spec_mask: null pointer");
    hipLaunchKernelGGL(spec_mask_kernel, dim3((unsigned)(B * F), (unsigned)cdiv(T, MASK_CHUNK)), dim3(256), 0, stream, src,
                       (long)src_batch_stride, dst, (int)F, (long)T, t_iv, (int)n_t, f_iv, (int)n_f, mask_value);
    SCONF_LAUNCH_OK("sconf_spec_mask");
    return 0;
}

SCONF_API int64_t sconf_mean_f32_workspace(int64_t n) { (void)n; return (int64_t)MEAN_BLOCKS * sizeof(double); }

// *out = mean of x (B,R,T) f32 contiguous, over t < lengths[b] only if lengths (B, int32) is given: specgram.mean() and its
// masked form, augmentation.py:73.  Fixed summation order (no float atomics): the same input gives the same bits.
SCONF_API int sconf_mean_f32(const float* x, int64_t B, int64_t R, int64_t T, const int32_t* lengths, float* out, void* ws,
                             int64_t ws_bytes, hipStream_t stream) {
    SCONF_REQUIRE(B >= 0 && R >= 0 && T >= 0, "sconf_mean_f32: negative size");
    SCONF_REQUIRE(ws && ws_bytes >= sconf_mean_f32_workspace(B * R * T), "sconf_mean_f32: workspace missing or too small");
    SCONF_REQUIRE(out, "sconf_mean_f32: null output");
    const long n = B * R * T;
    SCONF_REQUIRE(n == 0 || x, "sconf_mean_f32: null input");
    const long work = lengths ? B * R : cdiv(n, 256 * 16);      // rows, or 16 elements per thread
    const int blocks = (int)std::max<long>(1, std::min<long>(work, MEAN_BLOCKS));
    hipLaunchKernelGGL(mean_partial_kernel, dim3(blocks), dim3(256), 0, stream, x, (long)B, (long)R, (long)T, lengths, (double*)ws);
    SCONF_LAUNCH_OK("sconf_mean_f32");
    hipLaunchKernelGGL(mean_finish_kernel, dim3(1), dim3(64), 0, stream, (const double*)ws, blocks, (long)B, (long)R, (long)T, lengths, out);
    SCONF_LAUNCH_OK("sconf_mean_f32");
    return 0;
}

// Greedy CTC labels of B sequences x (B,N,C) f32 (log-probs or logits): arg-max per frame (first index on ties), repeats
// merged, blanks dropped, frames >= lengths[b] ignored -> targets (B,S_cap) int32 zero-padded, target_lengths (B) int32
// (-1: more than S_cap labels).  idx (B*N int32) receives the frame arg-maxes.  Replaces GreedyCTCDecoder.forward
// (lcasr/decoding/greedy.py:19-21) + the re-encoding of dynamic_eval.py:92-93 without a host round trip.
SCONF_API int sconf_ctc_collapse(const float* x, int64_t B, int64_t N, int64_t C, const int32_t* lengths, int32_t blank, int32_t* idx,
                                 int32_t* targets, int64_t S_cap, int32_t* target_lengths, hipStream_t stream) {
    SCONF_REQUIRE(C % 4 == 0 && C > 0, "sconf_ctc_collapse: C=%ld must be a positive multiple of 4", (long)C);
    SCONF_REQUIRE(B >= 0 && N >= 0 && S_cap >= 0 && B <= 0x7fffffffL, "sconf_ctc_collapse: bad size");
    if (B == 0) return 0;
    SCONF_REQUIRE(target_lengths && (S_cap == 0 || targets) && (N == 0 || (x && idx)), "sconf_ctc_collapse: null pointer");
    if (S_cap > 0 && hipMemsetAsync(targets, 0, (size_t)B * S_cap * sizeof(int32_t), stream) != hipSuccess)
        return sconf_set_error("sconf_ctc_collapse: memset failed");
    if (N > 0 && sconf_argmax_rows(x, B * N, C, idx, stream)) return 1;
    hipLaunchKernelGGL(collapse_compact_kernel, dim3((unsigned)B), dim3(64), 0, stream, idx, (long)N, lengths, (int)blank, targets,
                       (long)S_cap, target_lengths);
    SCONF_LAUNCH_OK("sconf_ctc_collapse");
    return 0;
}
