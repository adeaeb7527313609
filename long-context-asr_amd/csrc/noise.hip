// Noise corruption (include/sconf_noise.h): Gaussian noise and a background clip mixed into a waveform at a set SNR, and the mean
// square both factors are made from.  Compiled without -ffast-math (Makefile): the normals are logf, sqrtf and sincospif of the HIP
// math library, and the f64 sums keep the order written here.
//
// Three streaming kernels of 256 threads, one workgroup per (row, tile); a tile is TILE = 16384 consecutive samples = 4096 quads of
// four, thread t taking quads t, t + 256, ... (QPT = 16 of them), so that a wave reads and writes 1 KiB at a time.  A quad whose 16
// bytes are aligned and inside the row goes as one float4, any other quad element by element (VEC = false: every quad); the
// arithmetic per element is the same, so both forms give the same bits.
//   power_tile_kernel   a thread squares its samples in f64 (exact) into four sums, one per position in the quad, u ascending;
//                       (a0 + a1) + (a2 + a3), a butterfly over the wave, the four waves through LDS: one f64 per tile in ws.
//   power_row_kernel    one wave per row adds the tile sums in tile order, 256 at a time through LDS while the next 256 are loaded,
//                       and divides by len.
//   gaussian_kernel     quads are those of the ABSOLUTE sample position first_sample + i, one Philox4x32-10 call and two Box-Muller
//                       pairs each; the K factors wait in LDS, and the K rows are stored from the one z.
//   background_kernel   the clip is gathered at (off + i) mod nl: one 64-bit remainder per thread, then steps with a conditional
//                       subtraction.
// All positions are 64-bit.  No atomics, no inline assembly.
#include "common.h"
#include "../../include/sconf_noise.h"

namespace {

constexpr int NT = 256;                         // threads per workgroup
constexpr int QPT = 16;                         // quads per thread
constexpr int QT = NT * QPT;                    // quads per tile
constexpr int TILE = 4 * QT;                    // samples per tile
constexpr int MAXK = 16;                        // levels per call
constexpr int RCH = 256;                        // tile sums the row kernel holds at a time: 4 per lane

__device__ __forceinline__ int64_t clamp_len(const int64_t* lengths, int64_t b, int64_t L) {
    const int64_t n = lengths ? lengths[b] : L;
    return n < 0 ? 0 : n > L ? L : n;
}

// (p + step) mod n for 0 <= p < n, 0 <= step: the remainder is taken only where one subtraction is not enough (n < step)
__device__ __forceinline__ int64_t wrap_add(int64_t p, int64_t step, int64_t n) {
    p += step;
    if (p >= n) {
        p -= n;
        if (p >= n) p %= n;
    }
    return p;
}

__device__ __forceinline__ int64_t wrap_into(int64_t off, int64_t n) {             // any offset -> 0 .. n - 1, n >= 1
    off %= n;
    return off < 0 ? off + n : off;
}

// ---- mean square -------------------------------------------------------------------------------------------------------------
template <bool VEC, bool WRAP>
__global__ __launch_bounds__(NT) void power_tile_kernel(const float* __restrict__ src, int64_t row_stride, int64_t src_rows,
                                                        const int64_t* __restrict__ lengths, const int64_t* __restrict__ src_lengths,
                                                        const int64_t* __restrict__ offsets, int64_t L, int64_t tiles, double* __restrict__ ws) {
    __shared__ double part[NT / 64];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
    const int64_t r = src_rows == 1 ? 0 : b;
    const int64_t len = clamp_len(lengths, b, L);
    const float* row = src + r * row_stride;
    const int64_t i_tile = tile * TILE;

    int64_t sl = 1, p = 0;
    bool live = i_tile < len;
    if (WRAP) {
        sl = src_lengths ? src_lengths[r] : L;
        live = live && sl >= 1;
        if (live) p = wrap_add(wrap_into(offsets ? offsets[b] : 0, sl), i_tile + 4 * tid, sl);
    }
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    if (live) {
#pragma unroll 2
        for (int u = 0; u < QPT; ++u) {
            const int64_t i0 = i_tile + 4 * (int64_t)(u * NT + tid);
            if (i0 < len) {
                float x[4];
                if (!WRAP && VEC && i0 + 4 <= len) {
                    load4(row + i0, x);
                } else {
                    int64_t pj = p;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const bool ok = i0 + j < len;
                        x[j] = ok ? row[WRAP ? pj : i0 + j] : 0.f;
                        if (WRAP) pj = pj + 1 == sl ? 0 : pj + 1;
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) a[j] = fma((double)x[j], (double)x[j], a[j]);      // the square is exact: one rounding
            }
            if (WRAP) p = wrap_add(p, 4 * NT, sl);
        }
    }
    double s = (a[0] + a[1]) + (a[2] + a[3]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((tid & 63) == 0) part[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) ws[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

__global__ __launch_bounds__(64) void power_row_kernel(const double* __restrict__ ws, const int64_t* __restrict__ lengths, int64_t L,
                                                       int64_t tiles, double* __restrict__ power) {
    __shared__ double buf[RCH];
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t len = clamp_len(lengths, b, L);
    const double* w = ws + b * tiles;
    double s = 0.0, v[RCH / 64];
    auto fetch = [&](int64_t t0) {                                     // + 0.0 behind the last tile changes no bit of a sum >= 0
#pragma unroll
        for (int c = 0; c < RCH / 64; ++c) {
            const int64_t t = t0 + c * 64 + lane;
            v[c] = t < tiles ? w[t] : 0.0;
        }
    };
    fetch(0);
    for (int64_t t0 = 0; t0 < tiles; t0 += RCH) {
#pragma unroll
        for (int c = 0; c < RCH / 64; ++c) buf[c * 64 + lane] = v[c];
        __syncthreads();
        fetch(t0 + RCH);                                               // the next chunk is on its way under the chain of additions
#pragma unroll 16
        for (int j = 0; j < RCH; ++j) s += buf[j];                     // every lane the same chain: broadcast reads
        __syncthreads();
    }
    if (lane == 0) power[b] = len > 0 ? s / (double)len : 0.0;
}

// ---- the normals ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&r)[4]) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

__device__ __forceinline__ void box_muller(uint32_t ra, uint32_t rb, float& za, float& zb) {
    const float u = ((float)(ra >> 9) + 0.5f) * 0x1p-23f;              // in (0, 1), exact
    const float rad = sqrtf(-2.f * logf(u));
    float s, c;
    sincospif((float)(rb >> 9) * 0x1p-22f, &s, &c);                    // 2 U, exact
    za = rad * c;
    zb = rad * s;
}

// the factor of level k of row b: (float)(sqrt(ratio) 10^(-snr / 20)) in f64, 0 for a ratio of 0
__device__ __forceinline__ float level_factor(double ratio, float snr_db) {
    return ratio > 0.0 ? (float)(sqrt(ratio) * pow(10.0, -(double)snr_db / 20.0)) : 0.f;
}

// the K rows of one quad: y = fmaf(f_k, z, x) inside the row's length, 0 behind it, x itself where the factor is 0
template <bool VEC>
__device__ __forceinline__ void store_levels(float* __restrict__ out0, int64_t out_stride, int K, const float* __restrict__ fac, int64_t i0,
                                             int64_t len, int64_t L, const float (&x)[4], const float (&z)[4]) {
    for (int k = 0; k < K; ++k) {
        const float f = fac[k];
        float y[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = i0 + j < len ? (f == 0.f ? x[j] : fmaf(f, z[j], x[j])) : 0.f;
        float* o = out0 + k * out_stride;
        if (VEC && i0 + 4 <= L) {
            store4(o + i0, y);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (i0 + j >= 0 && i0 + j < L) o[i0 + j] = y[j];
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(NT) void gaussian_kernel(const float* __restrict__ wave, int64_t row_stride, const int64_t* __restrict__ lengths,
                                                      int64_t L, int64_t tiles, const double* __restrict__ power, const float* __restrict__ snr_db,
                                                      int K, uint32_t k0, uint32_t k1, int64_t first_row, int64_t first_sample,
                                                      float* __restrict__ out, int64_t out_stride) {
    __shared__ float fac[MAXK];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
    if (tid < K) fac[tid] = level_factor(power[b], snr_db[b * K + tid]);
    __syncthreads();
    const int64_t len = clamp_len(lengths, b, L);
    const float* row = wave + b * row_stride;
    float* out0 = out + b * K * out_stride;
    const int phase = (int)(first_sample & 3);                        // VEC: 0
    const uint64_t q_first = (uint64_t)first_sample >> 2, id = (uint64_t)(first_row + b);

#pragma unroll 2
    for (int u = 0; u < QPT; ++u) {
        const int64_t q = tile * QT + u * NT + tid;                    // the quad of absolute samples 4 (q_first + q) ..
        const int64_t i0 = 4 * q - phase;                              // .. which are samples i0 .. i0 + 3 of the row (i0 >= -3)
        if (i0 >= L) continue;
        float x[4] = {0.f, 0.f, 0.f, 0.f}, z[4] = {0.f, 0.f, 0.f, 0.f};
        if (i0 < len) {
            if (VEC && i0 + 4 <= len) {
                load4(row + i0, x);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) x[j] = i0 + j >= 0 && i0 + j < len ? row[i0 + j] : 0.f;
            }
            const uint64_t qa = q_first + (uint64_t)q;
            uint32_t r[4];
            philox4x32_10((uint32_t)qa, (uint32_t)(qa >> 32), (uint32_t)id, (uint32_t)(id >> 32), k0, k1, r);
            box_muller(r[0], r[1], z[0], z[1]);
            box_muller(r[2], r[3], z[2], z[3]);
        }
        store_levels<VEC>(out0, out_stride, K, fac, i0, len, L, x, z);
    }
}

template <bool VEC>
__global__ __launch_bounds__(NT) void background_kernel(const float* __restrict__ wave, int64_t row_stride, const int64_t* __restrict__ lengths,
                                                        int64_t L, int64_t tiles, const float* __restrict__ noise, int64_t noise_stride,
                                                        int64_t noise_rows, const int64_t* __restrict__ noise_lengths,
                                                        const int64_t* __restrict__ offsets, const double* __restrict__ power,
                                                        const double* __restrict__ noise_power, const float* __restrict__ snr_db, int K,
                                                        float* __restrict__ out, int64_t out_stride) {
    __shared__ float fac[MAXK];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
    const int64_t nr = noise_rows == 1 ? 0 : b;
    const int64_t nl = noise_lengths ? noise_lengths[nr] : L;
    if (tid < K) {
        const double pv = noise_power[b];
        fac[tid] = nl >= 1 && pv >= 1e-18 ? level_factor(power[b] / pv, snr_db[b * K + tid]) : 0.f;
    }
    __syncthreads();
    const int64_t len = clamp_len(lengths, b, L);
    const float* row = wave + b * row_stride;
    const float* clip = noise + nr * noise_stride;
    float* out0 = out + b * K * out_stride;
    const int64_t i_tile = tile * TILE;
    const bool live = nl >= 1;
    int64_t p = live ? wrap_add(wrap_into(offsets ? offsets[b] : 0, nl), i_tile + 4 * tid, nl) : 0;

#pragma unroll 2
    for (int u = 0; u < QPT; ++u) {
        const int64_t i0 = i_tile + 4 * (int64_t)(u * NT + tid);
        if (i0 < L) {
            float x[4] = {0.f, 0.f, 0.f, 0.f}, v[4] = {0.f, 0.f, 0.f, 0.f};
            if (i0 < len) {
                if (VEC && i0 + 4 <= len) {
                    load4(row + i0, x);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) x[j] = i0 + j < len ? row[i0 + j] : 0.f;
                }
                int64_t pj = p;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    v[j] = live && i0 + j < len ? clip[pj] : 0.f;
                    pj = pj + 1 >= nl ? 0 : pj + 1;
                }
            }
            store_levels<VEC>(out0, out_stride, K, fac, i0, len, L, x, v);
        }
        if (live) p = wrap_add(p, 4 * NT, nl);
    }
}

inline bool aligned4(const void* p, int64_t stride, int64_t rows) {
    return ((uintptr_t)p & 15) == 0 && (rows <= 1 || (stride & 3) == 0);
}

inline int64_t tiles_of(int64_t n) { return (n + TILE - 1) / TILE; }

}  // namespace

SCONF_API int sconf_noise_tile(void) { return TILE; }

SCONF_API int sconf_noise_max_levels(void) { return MAXK; }

SCONF_API int64_t sconf_noise_workspace(int64_t B, int64_t L) {
    if (B < 0 || L < 0) return -1;
    const int64_t tiles = tiles_of(L);
    if (tiles > 0 && B > 0x7fffffff / tiles) return -1;
    return B * tiles * (int64_t)sizeof(double);
}

SCONF_API int sconf_noise_power(const float* src, int64_t row_stride, int64_t src_rows, const int64_t* lengths, const int64_t* src_lengths,
                                const int64_t* offsets, int64_t L, int64_t B, double* power, void* ws, int64_t ws_bytes, sconf_stream_t stream) {
    SCONF_REQUIRE(L >= 0 && B >= 0, "sconf_noise_power: negative size L = %ld or B = %ld", (long)L, (long)B);
    if (B == 0) return 0;
    SCONF_REQUIRE(src && power, "sconf_noise_power: null pointer");
    SCONF_REQUIRE(src_rows == 1 || src_rows == B, "sconf_noise_power: src_rows = %ld, must be 1 or B = %ld", (long)src_rows, (long)B);
    SCONF_REQUIRE(row_stride >= 0 && (src_rows == 1 || src_lengths || row_stride >= L), "sconf_noise_power: row stride %ld < L = %ld",
                  (long)row_stride, (long)L);
    const int64_t need = sconf_noise_workspace(B, L);
    SCONF_REQUIRE(need >= 0, "sconf_noise_power: %ld rows of %ld tiles: too many workgroups", (long)B, (long)tiles_of(L));
    SCONF_REQUIRE(ws_bytes >= need && (ws || need == 0), "sconf_noise_power: workspace of %ld bytes, sconf_noise_workspace says %ld",
                  (long)ws_bytes, (long)need);
    const int64_t tiles = tiles_of(L);
    if (tiles > 0) {
        const dim3 grid((unsigned)(B * tiles));
        double* w = (double*)ws;
        if (offsets || src_lengths)
            hipLaunchKernelGGL((power_tile_kernel<false, true>), grid, dim3(NT), 0, stream, src, row_stride, src_rows, lengths, src_lengths, offsets, L, tiles, w);
        else if (aligned4(src, row_stride, src_rows))
            hipLaunchKernelGGL((power_tile_kernel<true, false>), grid, dim3(NT), 0, stream, src, row_stride, src_rows, lengths, src_lengths, offsets, L, tiles, w);
        else
            hipLaunchKernelGGL((power_tile_kernel<false, false>), grid, dim3(NT), 0, stream, src, row_stride, src_rows, lengths, src_lengths, offsets, L, tiles, w);
        SCONF_LAUNCH_OK("sconf_noise_power");
    }
    hipLaunchKernelGGL(power_row_kernel, dim3((unsigned)B), dim3(64), 0, stream, (const double*)ws, lengths, L, tiles, power);
    SCONF_LAUNCH_OK("sconf_noise_power");
    return 0;
}

// what both mixing launchers refuse; `tiles` of the quads the kernel walks
static int check_mix(const char* name, const void* wave, int64_t row_stride, int64_t L, int64_t B, const void* power, const void* snr_db,
                     int64_t K, const void* out, int64_t out_stride, int64_t span) {
    SCONF_REQUIRE(L >= 0 && B >= 0, "%s: negative size L = %ld or B = %ld", name, (long)L, (long)B);
    SCONF_REQUIRE(K >= 1 && K <= MAXK, "%s: K = %ld levels, must be in 1..%d (sconf_noise_max_levels)", name, (long)K, MAXK);
    SCONF_REQUIRE(out_stride >= L && (B <= 1 || row_stride >= L), "%s: out stride %ld or row stride %ld < L = %ld", name, (long)out_stride,
                  (long)row_stride, (long)L);
    if (B == 0 || L == 0) return 0;
    SCONF_REQUIRE(wave && power && snr_db && out, "%s: null pointer", name);
    SCONF_REQUIRE(B <= 0x7fffffff / tiles_of(span), "%s: %ld rows of %ld tiles: too many workgroups", name, (long)B, (long)tiles_of(span));
    return 0;
}

SCONF_API int sconf_noise_add_gaussian(const float* wave, int64_t row_stride, const int64_t* lengths, int64_t L, int64_t B, const double* power,
                                       const float* snr_db, int64_t K, int64_t seed, int64_t first_row, int64_t first_sample, float* out,
                                       int64_t out_stride, sconf_stream_t stream) {
    SCONF_REQUIRE(first_row >= 0 && first_sample >= 0 && (L < 0 || first_sample <= INT64_MAX - L - 8) && (B < 0 || first_row <= INT64_MAX - B),
                  "sconf_noise_add_gaussian: bad first_row = %ld or first_sample = %ld", (long)first_row, (long)first_sample);
    const int phase = (int)(first_sample & 3);
    if (int rc = check_mix("sconf_noise_add_gaussian", wave, row_stride, L, B, power, snr_db, K, out, out_stride, L + phase)) return rc;
    if (B == 0 || L == 0) return 0;
    const int64_t tiles = tiles_of(L + phase);
    const dim3 grid((unsigned)(B * tiles));
    const uint32_t k0 = (uint32_t)(uint64_t)seed, k1 = (uint32_t)((uint64_t)seed >> 32);
    if (phase == 0 && aligned4(wave, row_stride, B) && aligned4(out, out_stride, B * K))
        hipLaunchKernelGGL(gaussian_kernel<true>, grid, dim3(NT), 0, stream, wave, row_stride, lengths, L, tiles, power, snr_db, (int)K, k0, k1,
                           first_row, first_sample, out, out_stride);
    else
        hipLaunchKernelGGL(gaussian_kernel<false>, grid, dim3(NT), 0, stream, wave, row_stride, lengths, L, tiles, power, snr_db, (int)K, k0, k1,
                           first_row, first_sample, out, out_stride);
    SCONF_LAUNCH_OK("sconf_noise_add_gaussian");
    return 0;
}

SCONF_API int sconf_noise_add_background(const float* wave, int64_t row_stride, const int64_t* lengths, int64_t L, int64_t B, const float* noise,
                                         int64_t noise_stride, int64_t noise_rows, const int64_t* noise_lengths, const int64_t* offsets,
                                         const double* power, const double* noise_power, const float* snr_db, int64_t K, float* out,
                                         int64_t out_stride, sconf_stream_t stream) {
    if (int rc = check_mix("sconf_noise_add_background", wave, row_stride, L, B, power, snr_db, K, out, out_stride, L)) return rc;
    SCONF_REQUIRE(noise_rows == 1 || noise_rows == B, "sconf_noise_add_background: noise_rows = %ld, must be 1 or B = %ld", (long)noise_rows, (long)B);
    SCONF_REQUIRE(noise_stride >= 0, "sconf_noise_add_background: negative noise stride %ld", (long)noise_stride);
    if (B == 0 || L == 0) return 0;
    SCONF_REQUIRE(noise && noise_power, "sconf_noise_add_background: null pointer");
    const int64_t tiles = tiles_of(L);
    const dim3 grid((unsigned)(B * tiles));
    if (aligned4(wave, row_stride, B) && aligned4(out, out_stride, B * K))
        hipLaunchKernelGGL(background_kernel<true>, grid, dim3(NT), 0, stream, wave, row_stride, lengths, L, tiles, noise, noise_stride, noise_rows,
                           noise_lengths, offsets, power, noise_power, snr_db, (int)K, out, out_stride);
    else
        hipLaunchKernelGGL(background_kernel<false>, grid, dim3(NT), 0, stream, wave, row_stride, lengths, L, tiles, noise, noise_stride, noise_rows,
                           noise_lengths, offsets, power, noise_power, snr_db, (int)K, out, out_stride);
    SCONF_LAUNCH_OK("sconf_noise_add_background");
    return 0;
}
