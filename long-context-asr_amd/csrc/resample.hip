// Resampler (include/sconf_resample.h): a waveform at any rate -> the rate of the audio front end, the polyphase windowed-sinc
// filter of torchaudio.transforms.Resample with the compact table utils/audio_tools.py builds.
//
// Workgroups of 256 threads stay resident and walk the (row, tile) items; a tile is TILE = 1024 consecutive outputs of one row.
//   0. Once per workgroup the table goes to LDS: taps (P, K) at a row stride KS = K | 1 (odd: the 32 lanes of a half-wave hold 32
//      consecutive phases and read tap k of each, at addresses KS apart - 32 different banks), and first (P).
//   1. Per tile, the input span under its outputs - (TILE - 1) O / P + K + 3 samples from q0 O + first[p0] on - goes HBM -> LDS
//      once, 0 outside [0, len), nothing at or beyond len read.  With mix the channels are added in channel order and divided
//      while staging: a stereo recording is read once and no mono copy exists.
//   2. Thread t sums outputs j0 + t + 256 u, u = 0..3, over k ascending with one fmaf each, the four sums interleaved: neighbouring
//      lanes read neighbouring phases of the table and samples O / P apart, and store 256 consecutive outputs.
// An output whose K samples are not inside the staged span (possible only with a table that does not advance the way the
// reference's does) is summed from memory in the same order.  All positions are 64-bit; LDS offsets are int.
#include "common.h"
#include "../../include/sconf_resample.h"

namespace {

constexpr int NT = 256;                         // threads per workgroup
constexpr int OPT = 4;                          // outputs per thread
constexpr int TILE = NT * OPT;                  // outputs per workgroup and tile
constexpr int MAXTAB = 16384;                   // P * K
constexpr int MAXCH = 64;
constexpr size_t LDS_MAX = 160 * 1024;

struct Geometry { int ks; int span; size_t lds; bool fits; };

Geometry geometry_of(int64_t O, int64_t P, int64_t K) {
    Geometry g{};
    g.ks = (int)(K | 1);
    const int64_t span = (int64_t)(TILE - 1) * O / P + K + 3;
    const int64_t floats = P * g.ks + P + span;
    g.fits = floats * 4 <= (int64_t)LDS_MAX;
    g.span = g.fits ? (int)span : 0;
    g.lds = g.fits ? (size_t)floats * 4 : 0;
    return g;
}

int64_t out_length(int64_t L, int64_t O, int64_t P) {
    if (L < 0 || O < 1 || P < 1 || L > (INT64_MAX - O) / P) return -1;
    return (P * L + O - 1) / O;
}

// sample `pos` of the row: its channel 0, or the mean of its channels added in channel order
template <bool MIX>
__device__ __forceinline__ float sample_at(const float* __restrict__ row, int64_t chan_stride, int channels, int64_t pos) {
    float x = row[pos];
    if (MIX) {
        for (int c = 1; c < channels; ++c) x += row[c * chan_stride + pos];
        x = x / (float)channels;
    }
    return x;
}

template <bool MIX>
__global__ __launch_bounds__(NT) void resample_kernel(const float* __restrict__ wave, int64_t chan_stride, int64_t row_stride, int channels,
                                                      const int64_t* __restrict__ lengths, int64_t L, const float* __restrict__ taps,
                                                      const int32_t* __restrict__ first, int O, int P, int K, int KS, float* __restrict__ out,
                                                      int64_t out_stride, int64_t L_out, int64_t tiles, int64_t items, int span) {
    extern __shared__ __align__(16) unsigned char smem[];
    float* tab = reinterpret_cast<float*>(smem);                      // [P][KS]
    int* fst = reinterpret_cast<int*>(tab + P * KS);                  // [P]
    float* xs = reinterpret_cast<float*>(fst + P);                    // [span]
    const int tid = threadIdx.x;

    // ---- 0. once per workgroup: the table
    for (int i = tid; i < P * K; i += NT) {
        const int p = i / K;
        tab[p * KS + (i - p * K)] = taps[i];
    }
    for (int p = tid; p < P; p += NT) fst[p] = first[p];

    for (int64_t id = blockIdx.x; id < items; id += gridDim.x) {
        const int64_t b = id / tiles, tile = id - b * tiles;
        const int64_t j0 = tile * TILE;
        int64_t len = lengths ? lengths[b] : L;
        len = len < 0 ? 0 : len > L ? L : len;
        int64_t n_out = ((int64_t)P * len + O - 1) / O;
        n_out = n_out < L_out ? n_out : L_out;
        float* orow = out + b * out_stride;

        if (j0 >= n_out) {                                            // behind the row (the same for every thread): zeros
#pragma unroll
            for (int u = 0; u < OPT; ++u) {
                const int64_t j = j0 + tid + u * NT;
                if (j < L_out) orow[j] = 0.f;
            }
            continue;
        }
        __syncthreads();                                              // the table complete; xs of the last tile consumed

        const int64_t q0 = j0 / P;
        const int p0 = (int)(j0 - q0 * P);
        const int64_t lo = q0 * O + fst[p0];                          // the first sample output j0 reads
        const float* row = wave + b * row_stride;

        // ---- 1. the span, zero outside [0, len); len >= 1 here, so sample 0 exists for the clamped addresses.  The loads of a
        // thread are issued before its stores.
        for (int i0 = 0; i0 < span; i0 += NT * 4) {
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = i0 + tid + u * NT;
                const int64_t pos = lo + i;
                const bool ok = i < span && pos >= 0 && pos < len;
                const float x = sample_at<MIX>(row, chan_stride, channels, ok ? pos : 0);
                v[u] = ok ? x : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = i0 + tid + u * NT;
                if (i < span) xs[i] = v[u];
            }
        }
        __syncthreads();

        // ---- 2. four outputs per thread, k ascending
        float acc[OPT];
        int rel[OPT], tp[OPT];
        int64_t s[OPT];
        bool inside[OPT];
#pragma unroll
        for (int u = 0; u < OPT; ++u) {
            const int jj = p0 + tid + u * NT;                         // < P + TILE
            const int dq = jj / P, p = jj - dq * P;
            s[u] = (q0 + dq) * O + fst[p];
            const int64_t r = s[u] - lo;
            inside[u] = r >= 0 && r + K <= span;
            rel[u] = inside[u] ? (int)r : 0;
            tp[u] = p * KS;
            acc[u] = 0.f;
        }
#pragma unroll 2
        for (int k = 0; k < K; ++k) {
#pragma unroll
            for (int u = 0; u < OPT; ++u) acc[u] = fmaf(tab[tp[u] + k], xs[rel[u] + k], acc[u]);
        }
#pragma unroll
        for (int u = 0; u < OPT; ++u) {
            if (!inside[u]) {                                         // not under the staged span: the same sum from memory
                float a = 0.f;
                for (int k = 0; k < K; ++k) {
                    const int64_t pos = s[u] + k;
                    const bool ok = pos >= 0 && pos < len;
                    const float x = sample_at<MIX>(row, chan_stride, channels, ok ? pos : 0);
                    a = fmaf(tab[tp[u] + k], ok ? x : 0.f, a);
                }
                acc[u] = a;
            }
            const int64_t j = j0 + tid + u * NT;
            if (j < L_out) orow[j] = j < n_out ? acc[u] : 0.f;
        }
    }
}

}  // namespace

SCONF_API int sconf_resample_tile(void) { return TILE; }

SCONF_API int sconf_resample_max_table(void) { return MAXTAB; }

SCONF_API int64_t sconf_resample_out_length(int64_t L, int64_t O, int64_t P) { return out_length(L, O, P); }

SCONF_API int sconf_resample_rows(const float* wave, int64_t chan_stride, int64_t row_stride, int channels, int mix, const int64_t* lengths,
                                  int64_t L, const float* taps, const int32_t* first, int64_t O, int64_t P, int64_t K, float* out,
                                  int64_t out_stride, int64_t L_out, int64_t B, sconf_stream_t stream) {
    SCONF_REQUIRE(wave && taps && first && out, "sconf_resample_rows: null pointer");
    SCONF_REQUIRE(O >= 1 && O <= 0x7fffffff && P >= 1 && K >= 1, "sconf_resample_rows: bad O = %ld, P = %ld or K = %ld", (long)O, (long)P, (long)K);
    SCONF_REQUIRE(P <= MAXTAB && K <= MAXTAB && P * K <= MAXTAB, "sconf_resample_rows: table of %ld x %ld taps, at most %d are kept in LDS",
                  (long)P, (long)K, MAXTAB);
    SCONF_REQUIRE(channels >= 1 && channels <= MAXCH && (mix == 0 || mix == 1), "sconf_resample_rows: bad channels %d (1..%d) or mix %d",
                  channels, MAXCH, mix);
    SCONF_REQUIRE(L >= 1 && out_length(L, O, P) >= 1, "sconf_resample_rows: bad length L = %ld", (long)L);
    SCONF_REQUIRE(L_out == out_length(L, O, P), "sconf_resample_rows: L_out = %ld, but ceil(P L / O) = %ld", (long)L_out, (long)out_length(L, O, P));
    SCONF_REQUIRE(B >= 1 && out_stride >= L_out && (B == 1 || row_stride >= L) && (!mix || channels == 1 || chan_stride >= L),
                  "sconf_resample_rows: bad batch %ld, out stride %ld < L_out, row stride %ld < L or channel stride %ld < L", (long)B,
                  (long)out_stride, (long)row_stride, (long)chan_stride);
    const Geometry g = geometry_of(O, P, K);
    SCONF_REQUIRE(g.fits, "sconf_resample_rows: O = %ld, P = %ld, K = %ld: table and input span do not fit %d KiB of LDS", (long)O, (long)P,
                  (long)K, (int)(LDS_MAX / 1024));
    const int64_t tiles = (L_out + TILE - 1) / TILE;
    SCONF_REQUIRE(tiles <= 0x7fffffff / B, "sconf_resample_rows: %ld rows of %ld tiles: too many workgroups", (long)B, (long)tiles);
    const int64_t items = B * tiles;

    static bool lds_set = false;
    lds_limit_once(lds_set, {(const void*)resample_kernel<false>, (const void*)resample_kernel<true>}, LDS_MAX);
    int64_t per_cu = (int64_t)(LDS_MAX / g.lds);
    per_cu = per_cu < 1 ? 1 : per_cu > 8 ? 8 : per_cu;                // 8 workgroups of 4 waves fill a CU's wave slots
    const int64_t resident = per_cu * num_cus();
    const dim3 grid((unsigned)(items < resident ? items : resident));
    if (mix && channels > 1)
        hipLaunchKernelGGL(resample_kernel<true>, grid, dim3(NT), g.lds, stream, wave, chan_stride, row_stride, channels, lengths, L, taps, first,
                           (int)O, (int)P, (int)K, g.ks, out, out_stride, L_out, tiles, items, g.span);
    else
        hipLaunchKernelGGL(resample_kernel<false>, grid, dim3(NT), g.lds, stream, wave, chan_stride, row_stride, 1, lengths, L, taps, first,
                           (int)O, (int)P, (int)K, g.ks, out, out_stride, L_out, tiles, items, g.span);
    SCONF_LAUNCH_OK("sconf_resample_rows");
    return 0;
}
