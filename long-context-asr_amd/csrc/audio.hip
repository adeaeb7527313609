// Audio front end (include/sconf_audio.h): 16 kHz waveform -> (B, n_mels, T) mel spectrogram, with the per-row mean / std
// normalisation of lcasr/utils/audio_tools.py:44-57.
//
// One workgroup (4 waves) owns TF = 32 consecutive frames of one row at a time; two workgroups per CU stay resident and walk the
// tiles of all rows, so the filter taps, twiddles and window are set up once per workgroup.
//   1. The 160 * 31 + 512 samples under them go HBM -> LDS once, reflected at the row's own ends.
//   2. A wave takes two frames at a time as the real and the imaginary part of one 512-point complex FFT: 64 lanes x 8 points,
//      three radix-8 passes (n = j + 64 m, k = p + 8 r + 64 s) with two exchanges through a padded LDS image (row stride 72, and 9
//      between the j0 of the second image: both the stores and the loads of a half-wave touch 32 different banks).  The two spectra
//      come apart as X_a = (Z_k + conj Z_{512-k}) / 2, X_b = (Z_k - conj Z_{512-k}) / 2i; their powers go to P[frame][bin] in LDS.
//   3. Mel: thread = (frame, mel group).  The 32 lanes of a half-wave share the mel (its taps are LDS broadcasts) and differ in the
//      frame (P rows are 257 floats apart: 32 banks), so a store is 32 consecutive frames of one output row.  Only the non-zero
//      taps of a filter are visited (514 of 257 x 80).
//   4. The same lanes reduce (n, mean, M2) of the tile in f64; a second kernel merges the tiles of a row in a fixed order.
// Normalisation is one more pass over the f32 mel values (in place for f32 output).
#include "common.h"
#include "../../include/sconf_audio.h"

namespace {

constexpr int NFFT = 512, HOP = 160, NBIN = 257, PADL = 256;
constexpr int TF = 32;                          // frames per workgroup
constexpr int NT = 256;                         // threads per workgroup
constexpr int NS = HOP * (TF - 1) + NFFT;       // staged samples
constexpr int XROW = 72, XSZ = 8 * XROW;        // exchange image of one wave, in float2
constexpr int TAPCAP = 1024, MAXMEL = 128;
constexpr int MG = NT / TF;                     // mel groups: filters m, m + MG, ... per thread
constexpr size_t TABLE_BYTES = NFFT * sizeof(float2) + NFFT * sizeof(float);
constexpr size_t LDS_BYTES = (NS + TF * NBIN) * sizeof(float) + 4 * XSZ * sizeof(float2) + TAPCAP * sizeof(float) + 3 * MAXMEL * sizeof(int);

// tw[i] = exp(-2 pi i / 512) and the 400-sample periodic Hann window in the middle of 512, evaluated in f64
__global__ void audio_table_kernel(float2* tw, float* win) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= NFFT) return;
    double s, c;
    sincospi(i / 256.0, &s, &c);
    tw[i] = make_float2((float)c, (float)-s);
    const int n = i - (NFFT - 400) / 2;
    win[i] = n >= 0 && n < 400 ? (float)(0.5 - 0.5 * cospi(n / 200.0)) : 0.f;
}

__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// forward 8-point DFT in place, decimation in frequency: v[q] ends as X[BREV[q]]
__device__ constexpr int BREV[8] = {0, 4, 2, 6, 1, 5, 3, 7};
__device__ __forceinline__ void dft8(float2 (&v)[8]) {
    const float h = 0.70710678118654752f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float2 t = csub(v[i], v[i + 4]);
        v[i] = cadd(v[i], v[i + 4]);
        v[i + 4] = i == 0 ? t : i == 1 ? make_float2(h * (t.x + t.y), h * (t.y - t.x)) : i == 2 ? make_float2(t.y, -t.x)
                                                                                             : make_float2(h * (t.y - t.x), -h * (t.x + t.y));
    }
#pragma unroll
    for (int b = 0; b < 8; b += 4) {
        float2 t = csub(v[b], v[b + 2]);
        v[b] = cadd(v[b], v[b + 2]);
        v[b + 2] = t;
        t = csub(v[b + 1], v[b + 3]);
        v[b + 1] = cadd(v[b + 1], v[b + 3]);
        v[b + 3] = make_float2(t.y, -t.x);
    }
#pragma unroll
    for (int b = 0; b < 8; b += 2) {
        const float2 t = csub(v[b], v[b + 1]);
        v[b] = cadd(v[b], v[b + 1]);
        v[b + 1] = t;
    }
}

// LDS traffic between the lanes of ONE wave: the stores before it are visible to the loads after it
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ double half_wave_sum(double v) {          // over the 32 lanes that share a mel
#pragma unroll
    for (int o = TF / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ int64_t row_frames(const int64_t* lengths, int64_t b, int64_t L, int64_t T, int64_t& len) {
    len = lengths ? lengths[b] : L;
    len = len < 0 ? 0 : len > L ? L : len;
    const int64_t tb = len > PADL ? 1 + len / HOP : 0;
    return tb < T ? tb : T;
}

template <typename OutT>
__global__ __launch_bounds__(NT) void melspec_kernel(const float* __restrict__ wave, int64_t wave_stride, const int64_t* __restrict__ lengths,
                                                     int64_t L, const float* __restrict__ fb, const int32_t* __restrict__ ranges,
                                                     const float2* __restrict__ tw, const float* __restrict__ win, OutT* __restrict__ out,
                                                     double* __restrict__ partials, int64_t T, int n_mels, int64_t tiles, int64_t B) {
    extern __shared__ __align__(16) unsigned char smem[];
    float* xs = reinterpret_cast<float*>(smem);                       // [NS]
    float* P = xs + NS;                                               // [TF][NBIN]
    float2* X = reinterpret_cast<float2*>(P + TF * NBIN);             // [4][XSZ]
    float* taps = reinterpret_cast<float*>(X + 4 * XSZ);              // [TAPCAP]
    int* meta = reinterpret_cast<int*>(taps + TAPCAP);                // [MAXMEL][3] = first bin, taps, offset into taps

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int f = tid % TF, g = tid / TF;

    // ---- once per workgroup: the non-zero taps of every filter, packed (offsets = a prefix sum over the filters, by wave 0)
    if (wv == 0) {
        int lo[2], cnt[2], off[2], carry = 0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int m = lane + 64 * h;
            lo[h] = cnt[h] = 0;
            if (m < n_mels) {
                int a = ranges[2 * m], e = ranges[2 * m + 1];
                a = a < 0 ? 0 : a > NBIN ? NBIN : a;
                e = e < a ? a : e > NBIN ? NBIN : e;
                lo[h] = a; cnt[h] = e - a;
            }
            int sc = cnt[h];
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int v = __shfl_up(sc, o, 64);
                if (lane >= o) sc += v;
            }
            off[h] = carry + sc - cnt[h];
            carry += __shfl(sc, 63, 64);
            if (off[h] >= TAPCAP) cnt[h] = 0;
            else if (cnt[h] > TAPCAP - off[h]) cnt[h] = TAPCAP - off[h];
            if (m < n_mels) { meta[3 * m] = lo[h]; meta[3 * m + 1] = cnt[h]; meta[3 * m + 2] = off[h]; }
        }
    }
    __syncthreads();
    for (int m = tid; m < n_mels; m += NT) {
        const int lo = meta[3 * m], cnt = meta[3 * m + 1], off = meta[3 * m + 2];
        for (int i = 0; i < cnt; ++i) taps[off + i] = fb[(int64_t)(lo + i) * n_mels + m];
    }
    float2 tw1[8], tw2[8];
    float wn[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        tw1[i] = tw[(lane * i) & (NFFT - 1)];                         // W512^(j p), j = lane
        tw2[i] = tw[(8 * (lane & 7) * i) & (NFFT - 1)];               // W64^(j0 r), j0 = lane & 7
        wn[i] = win[lane + 64 * i];
    }
    float2* Xw = X + wv * XSZ;
    const int lo3 = lane & 7, hi3 = lane >> 3;

    // ---- tiles of all rows, row-major, strided over the resident workgroups
    for (int64_t id = blockIdx.x; id < B * tiles; id += gridDim.x) {
        const int64_t b = id / tiles, tile = id - b * tiles;
        const int64_t t0 = tile * TF;
        int64_t len;
        const int64_t tb = row_frames(lengths, b, L, T, len);
        const int nv = (int)(tb - t0 < 0 ? 0 : tb - t0 > TF ? TF : tb - t0);          // frames of this tile inside the row
        const int64_t t = t0 + f;

        if (nv == 0) {                                                    // beyond the row: zeros, and empty partials
            for (int m = g; m < n_mels; m += MG) {
                if (t < T) st_f(out + ((b * n_mels + m) * T + t), 0.f);
                if (partials && f == 0) {
                    double* p = partials + ((b * n_mels + m) * tiles + tile) * 3;
                    p[0] = 0.0; p[1] = 0.0; p[2] = 0.0;
                }
            }
            continue;
        }

        // ---- 1. samples, reflected at the row's own ends; nothing at or beyond len is read.  All loads of a thread are issued
        // before the first store (the address is clamped into the row, the value dropped where it is not wanted).
        {
            const float* row = wave + b * wave_stride;
            const int64_t g0 = t0 * HOP - PADL;
            const int need = HOP * (nv - 1) + NFFT;
            constexpr int NLD = (NS + NT - 1) / NT;
            float v[NLD];
#pragma unroll
            for (int j = 0; j < NLD; ++j) {
                const int i = tid + j * NT;
                int64_t s = g0 + i;
                if (s < 0) s = -s;
                if (s >= len) s = 2 * (len - 1) - s;
                const bool ok = i < need && s >= 0 && s < len;
                const float x = row[ok ? s : 0];                      // len > 256 here: sample 0 exists
                v[j] = ok ? x : 0.f;
            }
#pragma unroll
            for (int j = 0; j < NLD; ++j) {
                const int i = tid + j * NT;
                if (i < NS) xs[i] = v[j];
            }
        }
        __syncthreads();                                                  // xs (and, the first time, taps) complete; P of the last tile consumed

        // ---- 2. two frames per 512-point complex FFT
        for (int q = wv; 2 * q < nv; q += 4) {
            const float* xa = xs + (2 * q) * HOP;
            const float* xb = xa + HOP;                                   // frame 2q + 1 <= TF - 1 (its P row is unused when it is >= nv)
            float2 v[8];
#pragma unroll
            for (int m = 0; m < 8; ++m) v[m] = make_float2(wn[m] * xa[lane + 64 * m], wn[m] * xb[lane + 64 * m]);
            dft8(v);                                                      // over m -> p
#pragma unroll
            for (int i = 0; i < 8; ++i) Xw[BREV[i] * XROW + lane] = cmul(v[i], tw1[BREV[i]]);
            wave_sync();
#pragma unroll
            for (int j1 = 0; j1 < 8; ++j1) v[j1] = Xw[hi3 * XROW + lo3 + 8 * j1];       // lane = j0 + 8 p
            wave_sync();
            dft8(v);                                                      // over j1 -> r
#pragma unroll
            for (int i = 0; i < 8; ++i) Xw[hi3 * XROW + lo3 * 9 + BREV[i]] = cmul(v[i], tw2[BREV[i]]);
            wave_sync();
#pragma unroll
            for (int j0 = 0; j0 < 8; ++j0) v[j0] = Xw[hi3 * XROW + j0 * 9 + lo3];       // lane = r + 8 p
            wave_sync();
            dft8(v);                                                      // over j0 -> s: bin k = p + 8 r + 64 s
#pragma unroll
            for (int i = 0; i < 8; ++i) Xw[BREV[i] * XROW + lane] = v[i];
            wave_sync();
            float* pa = P + (2 * q) * NBIN;
            float* pb = pa + NBIN;
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const int k = lane + 64 * i;
                if (k < NBIN) {
                    const int k2 = (NFFT - k) & (NFFT - 1);
                    const float2 a = Xw[(k >> 6) * XROW + ((k >> 3) & 7) + 8 * (k & 7)];
                    const float2 c = Xw[(k2 >> 6) * XROW + ((k2 >> 3) & 7) + 8 * (k2 & 7)];
                    const float ar = a.x + c.x, ai = a.y - c.y, br = a.x - c.x, bi = a.y + c.y;
                    pa[k] = 0.25f * (ar * ar + ai * ai);
                    pb[k] = 0.25f * (br * br + bi * bi);
                }
            }
            wave_sync();
        }
        __syncthreads();

        // ---- 3. + 4. mel values of frame f, filters g, g + MG, ...; tile statistics in f64
        const bool valid = f < nv;
        const float* pf = P + f * NBIN;
        for (int m = g; m < n_mels; m += MG) {
            const int lo = meta[3 * m], cnt = meta[3 * m + 1], off = meta[3 * m + 2];
            float acc = 0.f;
#pragma unroll 4
            for (int i = 0; i < cnt; ++i) acc = fmaf(taps[off + i], pf[lo + i], acc);
            const float x = valid ? acc : 0.f;
            if (t < T) st_f(out + ((b * n_mels + m) * T + t), x);
            if (partials) {
                const double mean = half_wave_sum((double)x) / nv;
                const double d = valid ? (double)x - mean : 0.0;
                const double m2 = half_wave_sum(d * d);
                if (f == 0) {
                    double* p = partials + ((b * n_mels + m) * tiles + tile) * 3;
                    p[0] = (double)nv; p[1] = mean; p[2] = m2;
                }
            }
        }
    }
}

struct Moments { double n, mean, m2; };
// Chan's merge of two (n, mean, M2); `a` is the earlier range
__device__ __forceinline__ Moments merge(Moments a, Moments b) {
    if (b.n == 0.0) return a;
    if (a.n == 0.0) return b;
    const double n = a.n + b.n, d = b.mean - a.mean;
    return {n, a.mean + d * (b.n / n), a.m2 + b.m2 + d * d * (a.n * b.n / n)};
}

// one workgroup per (row, mel): each thread merges a contiguous run of tiles in order, then a fixed tree over the threads
__global__ __launch_bounds__(NT) void melspec_stats_kernel(const double* partials, double* stats, int64_t tiles) {
    __shared__ Moments sh[NT];
    const int64_t r = blockIdx.x;
    const int64_t per = (tiles + NT - 1) / NT;
    const double* p = partials + r * tiles * 3;
    Moments a = {0.0, 0.0, 0.0};
    const int64_t i0 = threadIdx.x * per, i1 = i0 + per < tiles ? i0 + per : tiles;
    for (int64_t i = i0; i < i1; ++i) a = merge(a, Moments{p[3 * i], p[3 * i + 1], p[3 * i + 2]});
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int s = 1; s < NT; s <<= 1) {
        if ((threadIdx.x & (2 * s - 1)) == 0) sh[threadIdx.x] = merge(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        stats[2 * r] = sh[0].mean;
        stats[2 * r + 1] = sqrt(sh[0].m2 / (sh[0].n - 1.0));          // unbiased; one frame or none: NaN, as torch.std
    }
}

// out = (raw - mean) / std inside the row, 0 behind it; raw may be out (f32, in place)
template <typename OutT>
__global__ __launch_bounds__(NT) void melspec_normalise_kernel(const float* raw, OutT* out, const double* stats, const int64_t* lengths,
                                                               int64_t L, int64_t T, int n_mels) {
    const int64_t r = blockIdx.x, b = r / n_mels;
    int64_t len;
    const int64_t tb = row_frames(lengths, b, L, T, len);
    const float mean = (float)stats[2 * r], sd = (float)stats[2 * r + 1];
    const float* src = raw + r * T;
    OutT* dst = out + r * T;
    const int64_t base = (int64_t)blockIdx.y * (NT * 8);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int64_t t = base + i * NT + threadIdx.x;
        if (t < T) st_f(dst + t, t < tb ? (src[t] - mean) / sd : 0.f);
    }
}

int64_t workspace_bytes_for(int64_t B, int64_t T, int64_t n_mels) {
    const int64_t tiles = (T + TF - 1) / TF;
    return (int64_t)TABLE_BYTES + B * n_mels * 2 * 8 + B * n_mels * tiles * 3 * 8;
}

}  // namespace

SCONF_API int sconf_audio_tile_frames(void) { return TF; }

SCONF_API int64_t sconf_audio_melspec_workspace(int64_t B, int64_t T, int64_t n_mels) {
    if (B < 1 || T < 1 || n_mels < 1 || n_mels > MAXMEL) return -1;
    return workspace_bytes_for(B, T, n_mels);
}

SCONF_API int sconf_audio_melspec(const float* wave, int64_t wave_stride, const int64_t* lengths, int64_t L, const float* fb,
                                  const int32_t* ranges, void* spec, int spec_dtype, float* raw, int normalise, void* workspace,
                                  int64_t workspace_bytes, int64_t B, int64_t T, int64_t n_mels, sconf_stream_t stream) {
    SCONF_REQUIRE(wave && fb && ranges && spec && workspace, "sconf_audio_melspec: null pointer");
    SCONF_REQUIRE(n_mels >= 1 && n_mels <= MAXMEL, "sconf_audio_melspec: n_mels %ld outside 1..%d", (long)n_mels, MAXMEL);
    SCONF_REQUIRE(L > PADL, "sconf_audio_melspec: %ld samples: reflect padding needs more than %d", (long)L, PADL);
    SCONF_REQUIRE(T == 1 + L / HOP, "sconf_audio_melspec: T = %ld, but 1 + L / 160 = %ld", (long)T, (long)(1 + L / HOP));
    SCONF_REQUIRE(B >= 1 && B * n_mels <= 0x7fffffff && wave_stride >= L, "sconf_audio_melspec: bad batch %ld or row stride %ld < L", (long)B, (long)wave_stride);
    SCONF_REQUIRE(spec_dtype == SCONF_F32 || spec_dtype == SCONF_BF16, "sconf_audio_melspec: bad spec_dtype %d", spec_dtype);
    SCONF_REQUIRE(workspace_bytes >= workspace_bytes_for(B, T, n_mels), "sconf_audio_melspec: workspace of %ld bytes, needs %ld",
                  (long)workspace_bytes, (long)workspace_bytes_for(B, T, n_mels));
    SCONF_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "sconf_audio_melspec: workspace must be 8-byte aligned");
    const bool two_pass = normalise && spec_dtype == SCONF_BF16;
    SCONF_REQUIRE(!two_pass || raw, "sconf_audio_melspec: normalised bf16 output needs the raw f32 scratch");
    const int64_t tiles = (T + TF - 1) / TF;
    SCONF_REQUIRE(tiles <= 0x7fffffff, "sconf_audio_melspec: too many frames");

    unsigned char* ws = static_cast<unsigned char*>(workspace);
    float2* tw = reinterpret_cast<float2*>(ws);
    float* win = reinterpret_cast<float*>(ws + NFFT * sizeof(float2));
    double* stats = reinterpret_cast<double*>(ws + TABLE_BYTES);
    double* partials = normalise ? stats + B * n_mels * 2 : nullptr;

    static bool lds_set = false;
    lds_limit_once(lds_set, {(const void*)melspec_kernel<float>, (const void*)melspec_kernel<bf16>}, LDS_BYTES);
    hipLaunchKernelGGL(audio_table_kernel, dim3(NFFT / NT), dim3(NT), 0, stream, tw, win);
    const int64_t resident = 2 * (int64_t)num_cus();                  // two workgroups fit one CU's LDS
    const dim3 grid((unsigned)(B * tiles < resident ? B * tiles : resident));
    if (spec_dtype == SCONF_F32 || two_pass) {
        float* dst = two_pass ? raw : static_cast<float*>(spec);
        hipLaunchKernelGGL(melspec_kernel<float>, grid, dim3(NT), LDS_BYTES, stream, wave, wave_stride, lengths, L, fb, ranges, tw, win,
                           dst, partials, T, (int)n_mels, tiles, B);
    } else {
        hipLaunchKernelGGL(melspec_kernel<bf16>, grid, dim3(NT), LDS_BYTES, stream, wave, wave_stride, lengths, L, fb, ranges, tw, win,
                           static_cast<bf16*>(spec), partials, T, (int)n_mels, tiles, B);
    }
    if (normalise) {
        hipLaunchKernelGGL(melspec_stats_kernel, dim3((unsigned)(B * n_mels)), dim3(NT), 0, stream, partials, stats, tiles);
        const dim3 ngrid((unsigned)(B * n_mels), (unsigned)cdiv(T, NT * 8));
        if (two_pass)
            hipLaunchKernelGGL(melspec_normalise_kernel<bf16>, ngrid, dim3(NT), 0, stream, raw, static_cast<bf16*>(spec), stats, lengths, L, T, (int)n_mels);
        else
            hipLaunchKernelGGL(melspec_normalise_kernel<float>, ngrid, dim3(NT), 0, stream, static_cast<const float*>(spec), static_cast<float*>(spec),
                               stats, lengths, L, T, (int)n_mels);
    }
    SCONF_LAUNCH_OK("sconf_audio_melspec");
    return 0;
}
