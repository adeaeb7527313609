// Attention maps for gfx950: the scaled score matrix and the offset profile of the attention probabilities.
//
//  * sconf_attn_scores: out (B,H,N,N) = scale * q_i . k_j with -inf at masked positions - the reference's `a_weight`
//    (attention.py:431-434, ReturnAttention / CollectAttentionProbs), for contexts where an N x N matrix is affordable.
//  * sconf_attn_offset_profile: prof[b,h,delta + N - 1] = sum over live rows i of P[b,h,i,i + delta] with
//    P = exp(scale * q_i . k_j - lse_i): how the attention mass is spread over relative distance, 2N - 1 numbers per head
//    with no N x N intermediate anywhere.
//
// Both kernels share one tile shape: a workgroup of 4 waves takes 32 query rows x 256 keys, wave w the two 32-key blocks
// 64 w and 64 w + 32.  A block is S^T = K Q^T on v_mfma_f32_32x32x16_bf16 (f32 accumulation) with both operands read straight
// from global memory in MFMA fragment order (16 bytes per lane and k-step): every key row is used by exactly one wave of the
// workgroup, so an LDS stage for K would share nothing, and the 32 query rows are 8 KiB that the four waves hit in L1.  As in the
// forward the query sits on the lane, so the row's log-sum-exp is one scalar per lane.  The tile then goes through LDS
// ([32][LD] f32, row = query) because neither consumer wants it one-query-per-lane:
//  * the scores kernel stores it row by row, thread t the key t of the tile: 256 consecutive elements per store instruction;
//  * the profile kernel sums it along its diagonals.
//
// Offset profile: a workgroup owns a BAND of 224 offsets [d0, d0 + 224) and a chunk of query rows, and walks the chunk in
// 32-row tiles.  For the tile at row i0 the keys i0 + d0 .. i0 + d0 + 255 cover every (row, offset) pair of the band
// (224 + 31 = 255), so 7/8 of the computed products are used.  In the LDS image offset d0 + t of row i is element [i][i + t]:
// thread t reads addresses i * (LD + 1) + t, consecutive over t (no bank conflict), adds its 32 elements in row order and keeps
// ONE running sum in a register for the whole chunk.  Nothing is added across threads and nothing atomically: the order of every
// sum is fixed by the launch geometry.  Each workgroup writes its 224 sums to its own row of the caller's workspace and a second
// kernel adds the chunks of a band in chunk order.  With a window only the bands that meet [-left, right] exist, so both the
// work and the workspace scale with N * window, not N^2.  (The other obvious design - a workgroup owns a QUERY tile and keeps an
// LDS array of all offsets it meets - needs (keys visited + 127) floats of LDS per workgroup, 64 KiB at N = 16384 and past
// the CU's 160 KiB from N = 40960 on unless it is flushed to memory in pieces, and its per-tile diagonal sums land on a
// different accumulator every tile; here the accumulator never moves.)
#include "common.h"
#include <algorithm>

namespace {

constexpr int MAPS_QT = 32;         // query rows per tile
constexpr int MAPS_KT = 256;        // keys per tile (4 waves x 2 blocks of 32)
constexpr int MAPS_BAND = 224;      // offsets per workgroup of the profile: MAPS_KT - MAPS_QT
constexpr int MAPS_CHUNK = 512;     // query rows per workgroup of the profile
constexpr int MAPS_LD = 257;        // LDS row pitch (floats): odd, so the 32 query lanes of a store fall on 32 banks
constexpr float LOG2E = 1.4426950408889634f;

struct MapsParams {
    const bf16 *q, *k;                // (B,N,H,D) views: element (b,n,h,d) at b*sb + n*sn + h*sh + d
    long q_sb, q_sn, q_sh, k_sb, k_sn, k_sh;
    const float* lse;                 // (B,H,N), profile only
    const int* lengths;               // int32 [B] or null
    void* out;                        // scores: (B,H,N,N) f32 or bf16; profile: the partial sums (workspace)
    int B, N, H;
    int win_left, win_right;          // -1 = unbounded
    float scale;
    int d_lo, nbands, nchunks;        // profile: first offset of band 0, bands and query chunks per (b, h)
};

// MFMA operand fragments of 32 rows of a (rows, D) bf16 view straight from global: row row0 + (lane & 31), k-step st holds
// d = 16 st + 8 (lane >> 5) + 0..7.  Rows outside [0, nrows) are zeros (never read: no access outside the tensor).
template <int D> __device__ __forceinline__ void load_frags(bf16x8 (&f)[D / 16], const bf16* base, long sn, int row0, int nrows, int lane) {
    const int r = row0 + (lane & 31);
    const bool ok = r >= 0 && r < nrows;
    const bf16* src = base + (long)(ok ? r : 0) * sn + 8 * (lane >> 5);
#pragma unroll
    for (int st = 0; st < D / 16; ++st) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (ok) v = *reinterpret_cast<const uint4*>(src + 16 * st);
        f[st] = __builtin_bit_cast(bf16x8, v);
    }
}
// S^T block: rows = the 32 keys of kf, columns = the 32 queries of qf.  Lane holds query (lane & 31), register r key acc_row(r, lane >> 5).
template <int D> __device__ __forceinline__ f32x16 st_block(const bf16x8 (&kf)[D / 16], const bf16x8 (&qf)[D / 16]) {
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int st = 0; st < D / 16; ++st) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[st], qf[st], s, 0, 0, 0);
    return s;
}

__device__ __forceinline__ bool visible(int i, int j, int len, int wl, int wr) {
    bool ok = i < len && j >= 0 && j < len;
    if (wl >= 0) ok = ok && j >= i - wl;
    if (wr >= 0) ok = ok && j <= i + wr;
    return ok;
}

// =============================================================================================
// scores: grid (key tiles, query tiles, B * H)
// =============================================================================================
template <int D, typename OutT>
__global__ __launch_bounds__(256) void attn_scores_kernel(const MapsParams p) {
    __shared__ float tile[MAPS_QT * MAPS_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hh = lane >> 5;
    const int b = blockIdx.z / p.H, h = blockIdx.z % p.H;
    const int i0 = blockIdx.y * MAPS_QT, j0 = blockIdx.x * MAPS_KT;
    const int len = p.lengths ? min(max(p.lengths[b], 0), p.N) : p.N;
    // a tile with no visible element is written without touching q or k (workgroup-uniform)
    bool any = i0 < len && j0 < len;
    if (p.win_left >= 0) any = any && j0 + MAPS_KT - 1 >= i0 - p.win_left;
    if (p.win_right >= 0) any = any && j0 <= i0 + MAPS_QT - 1 + p.win_right;
    if (any) {
        const bf16* qp = p.q + b * p.q_sb + h * p.q_sh;
        const bf16* kp = p.k + b * p.k_sb + h * p.k_sh;
        bf16x8 qf[D / 16], kf[D / 16];
        load_frags<D>(qf, qp, p.q_sn, i0, p.N, lane);
        const int i = i0 + (lane & 31);
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            const int jb = wave * 64 + blk * 32;
            load_frags<D>(kf, kp, p.k_sn, j0 + jb, p.N, lane);
            const f32x16 s = st_block<D>(kf, qf);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int jl = jb + acc_row(r, hh);
                tile[(lane & 31) * MAPS_LD + jl] = visible(i, j0 + jl, len, p.win_left, p.win_right) ? s[r] * p.scale : -INFINITY;
            }
        }
        __syncthreads();
    }
    // row by row, thread t the key j0 + t: one store instruction covers 256 consecutive elements of a row
    const int j = j0 + tid;
    if (j < p.N) {
        OutT* out = (OutT*)p.out + ((long)blockIdx.z * p.N + i0) * (long)p.N + j;
        const int rows = min(MAPS_QT, p.N - i0);
        for (int r = 0; r < rows; ++r) st_f<OutT>(out + (long)r * p.N, any ? tile[r * MAPS_LD + tid] : -INFINITY);
    }
}

// =============================================================================================
// offset profile: grid (bands, query chunks, B * H) -> partial sums [b h][chunk][band][224]
// =============================================================================================
template <int D>
__global__ __launch_bounds__(256) void attn_offset_partial_kernel(const MapsParams p) {
    __shared__ float tile[MAPS_QT * MAPS_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hh = lane >> 5;
    const int b = blockIdx.z / p.H, h = blockIdx.z % p.H;
    const int d0 = p.d_lo + blockIdx.x * MAPS_BAND;
    const int len = p.lengths ? min(max(p.lengths[b], 0), p.N) : p.N;
    // rows of this chunk that have a key inside [0, len) at some offset of the band: i + d0 < len and i + d0 + 223 >= 0
    const int c0 = blockIdx.y * MAPS_CHUNK;
    const int i_begin = max(c0, (max(0, -(d0 + MAPS_BAND - 1)) / MAPS_QT) * MAPS_QT);
    const int i_end = min(min(c0 + MAPS_CHUNK, len), len - d0);
    const bf16* qp = p.q + b * p.q_sb + h * p.q_sh;
    const bf16* kp = p.k + b * p.k_sb + h * p.k_sh;
    const float* lse = p.lse + (long)blockIdx.z * p.N;
    const float c = p.scale * LOG2E;
    float acc = 0.f;
    // The tile moves 32 keys per step: a wave's second key block is its first block of the next tile, so one key block and the 32
    // query rows are loaded per tile, written one tile AHEAD of their use: the workgroup's tiles are a serial chain of load, MFMA
    // and LDS round trip with nothing else to hide the latency.  (The lse load below still makes the compiler wait for them
    // early; what that costs and what comes next: DESIGN section 11.)
    bf16x8 qf[D / 16], kf[2][D / 16], qn[D / 16], kn[D / 16];
    load_frags<D>(qf, qp, p.q_sn, i_begin, p.N, lane);
    load_frags<D>(kf[0], kp, p.k_sn, i_begin + d0 + wave * 64, p.N, lane);
    load_frags<D>(kf[1], kp, p.k_sn, i_begin + d0 + wave * 64 + 32, p.N, lane);
    for (int i0 = i_begin; i0 < i_end; i0 += MAPS_QT) {
        const int j0 = i0 + d0;                                       // key of tile column 0 (may be negative)
        load_frags<D>(qn, qp, p.q_sn, i0 + MAPS_QT, i0 + MAPS_QT < i_end ? p.N : 0, lane);               // zeros after the last tile
        load_frags<D>(kn, kp, p.k_sn, j0 + wave * 64 + 64, i0 + MAPS_QT < i_end ? p.N : 0, lane);
        const int i = i0 + (lane & 31);
        // -lse log2(e); +inf lse (padded row, row without a visible key) -> -inf -> P = 0
        const float nl = i < len ? -lse[i] * LOG2E : -INFINITY;
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            const int jb = wave * 64 + blk * 32;
            const f32x16 s = st_block<D>(kf[blk], qf);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int jl = jb + acc_row(r, hh);
                const float e = __builtin_amdgcn_exp2f(s[r] * c + nl);
                tile[(lane & 31) * MAPS_LD + jl] = visible(i, j0 + jl, len, p.win_left, p.win_right) ? e : 0.f;
            }
        }
        __syncthreads();
        if (tid < MAPS_BAND) {
            float t = 0.f;
#pragma unroll 8
            for (int r = 0; r < MAPS_QT; ++r) t += tile[r * (MAPS_LD + 1) + tid];
            acc += t;
        }
#pragma unroll
        for (int st = 0; st < D / 16; ++st) { kf[0][st] = kf[1][st]; kf[1][st] = kn[st]; qf[st] = qn[st]; }
        __syncthreads();
    }
    if (tid < MAPS_BAND)
        ((float*)p.out)[(((long)blockIdx.z * p.nchunks + blockIdx.y) * p.nbands + blockIdx.x) * MAPS_BAND + tid] = acc;
}

// prof (B*H, 2N-1): offset delta = x - (N - 1); inside [d_lo, d_hi] the chunk sums of its band in chunk order, outside exactly 0
__global__ __launch_bounds__(256) void attn_offset_combine_kernel(const float* __restrict__ part, float* __restrict__ prof, int N, int d_lo, int d_hi,
                                                                  int nbands, int nchunks) {
    const int x = blockIdx.x * 256 + threadIdx.x, W = 2 * N - 1;
    if (x >= W) return;
    const int delta = x - (N - 1);
    float t = 0.f;
    if (delta >= d_lo && delta <= d_hi) {
        const int band = (delta - d_lo) / MAPS_BAND, o = (delta - d_lo) % MAPS_BAND;
        const float* src = part + ((long)blockIdx.y * nchunks * nbands + band) * MAPS_BAND + o;
        for (int ch = 0; ch < nchunks; ++ch) t += src[(long)ch * nbands * MAPS_BAND];
    }
    prof[(long)blockIdx.y * W + x] = t;
}

struct ProfGeom { int d_lo, d_hi, nbands, nchunks; };
ProfGeom prof_geom(int64_t N, int win_left, int win_right) {
    ProfGeom g;
    g.d_lo = win_left < 0 ? -(int)(N - 1) : -(int)std::min<int64_t>(win_left, N - 1);
    g.d_hi = win_right < 0 ? (int)(N - 1) : (int)std::min<int64_t>(win_right, N - 1);
    g.nbands = cdiv((long)g.d_hi - g.d_lo + 1, MAPS_BAND);
    g.nchunks = cdiv(N, MAPS_CHUNK);
    return g;
}

int check_maps(const char* fn, const void* q, const void* k, int64_t B, int64_t N, int64_t H, int64_t D, const int64_t* qs, const int64_t* ks) {
    if (!(D == 32 || D == 64 || D == 128 || D == 256)) return sconf_set_error("%s: head_dim %ld not supported (32, 64, 128 or 256)", fn, (long)D);
    if (B <= 0 || N <= 0 || H <= 0) return sconf_set_error("%s: empty problem", fn);
    if (B * H > 65535) return sconf_set_error("%s: B * H must be <= 65535", fn);
    if (N > (1L << 30)) return sconf_set_error("%s: N must be <= 2^30", fn);
    if (!q || !k || !qs || !ks) return sconf_set_error("%s: null q, k or strides", fn);
    for (int i = 0; i < 3; ++i)
        if (qs[i] % 8 != 0 || ks[i] % 8 != 0 || qs[i] < 0 || ks[i] < 0) return sconf_set_error("%s: strides must be non-negative multiples of 8 elements", fn);
    if (((uintptr_t)q | (uintptr_t)k) & 15) return sconf_set_error("%s: q and k must be 16-byte aligned", fn);
    return 0;
}

MapsParams make_params(const void* q, const void* k, const int32_t* lengths, int64_t B, int64_t N, int64_t H, const int64_t* qs, const int64_t* ks,
                       int win_left, int win_right, float scale) {
    MapsParams p = {};
    p.q = (const bf16*)q; p.k = (const bf16*)k; p.lengths = lengths;
    p.q_sb = qs[0]; p.q_sn = qs[1]; p.q_sh = qs[2]; p.k_sb = ks[0]; p.k_sn = ks[1]; p.k_sh = ks[2];
    p.B = (int)B; p.N = (int)N; p.H = (int)H; p.win_left = win_left < 0 ? -1 : win_left; p.win_right = win_right < 0 ? -1 : win_right; p.scale = scale;
    return p;
}

template <int D> void launch_scores(const MapsParams& p, int out_dtype, dim3 grid, hipStream_t stream) {
    if (out_dtype == SCONF_F32) hipLaunchKernelGGL((attn_scores_kernel<D, float>), grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL((attn_scores_kernel<D, bf16>), grid, dim3(256), 0, stream, p);
}

}  // namespace

// out (B,H,N,N) f32 or bf16 = scale * q_i . k_j; -inf where j >= length, i >= length or j outside [i - win_left, i + win_right].
SCONF_API int sconf_attn_scores(const void* q, const void* k, void* out, int out_dtype, const int32_t* lengths, int64_t B, int64_t N,
                                int64_t H, int64_t D, const int64_t* q_strides, const int64_t* k_strides, int win_left, int win_right,
                                float scale, hipStream_t stream) {
    if (check_maps("sconf_attn_scores", q, k, B, N, H, D, q_strides, k_strides)) return 1;
    SCONF_REQUIRE(out != nullptr, "sconf_attn_scores: null out");
    SCONF_REQUIRE(out_dtype == SCONF_F32 || out_dtype == SCONF_BF16, "sconf_attn_scores: out_dtype must be 0 (f32) or 1 (bf16)");
    SCONF_REQUIRE(cdiv(N, MAPS_QT) <= 65535, "sconf_attn_scores: N must be <= %d", 65535 * MAPS_QT);
    MapsParams p = make_params(q, k, lengths, B, N, H, q_strides, k_strides, win_left, win_right, scale);
    p.out = out;
    const dim3 grid((unsigned)cdiv(N, MAPS_KT), (unsigned)cdiv(N, MAPS_QT), (unsigned)(B * H));
    if (D == 32) launch_scores<32>(p, out_dtype, grid, stream);
    else if (D == 64) launch_scores<64>(p, out_dtype, grid, stream);
    else if (D == 128) launch_scores<128>(p, out_dtype, grid, stream);
    else launch_scores<256>(p, out_dtype, grid, stream);
    SCONF_LAUNCH_OK("sconf_attn_scores");
    return 0;
}

// bytes of workspace sconf_attn_offset_profile needs: one 224-float row per (b, h, 512-row query chunk, band of 224 offsets); with a
// window the bands cover [-win_left, win_right] only.  -1 for invalid sizes.
SCONF_API int64_t sconf_attn_offset_profile_workspace(int64_t B, int64_t N, int64_t H, int win_left, int win_right) {
    if (B <= 0 || N <= 0 || H <= 0 || N > (1L << 30)) return -1;
    const ProfGeom g = prof_geom(N, win_left, win_right);
    return B * H * (int64_t)g.nchunks * g.nbands * MAPS_BAND * (int64_t)sizeof(float);
}

SCONF_API int sconf_attn_offset_profile(const void* q, const void* k, const float* lse, float* prof, const int32_t* lengths, int64_t B,
                                        int64_t N, int64_t H, int64_t D, const int64_t* q_strides, const int64_t* k_strides, int win_left,
                                        int win_right, float scale, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
    if (check_maps("sconf_attn_offset_profile", q, k, B, N, H, D, q_strides, k_strides)) return 1;
    SCONF_REQUIRE(lse != nullptr && prof != nullptr, "sconf_attn_offset_profile: null lse or prof");
    const ProfGeom g = prof_geom(N, win_left, win_right);
    const int64_t need = sconf_attn_offset_profile_workspace(B, N, H, win_left, win_right);
    SCONF_REQUIRE(workspace != nullptr && workspace_bytes >= need, "sconf_attn_offset_profile: workspace of %ld bytes needed, %ld given",
                  (long)need, (long)(workspace ? workspace_bytes : 0));
    SCONF_REQUIRE(g.nchunks <= 65535 && cdiv(2 * N - 1, 256) <= 0x7fffffffL, "sconf_attn_offset_profile: N too large");
    MapsParams p = make_params(q, k, lengths, B, N, H, q_strides, k_strides, win_left, win_right, scale);
    p.lse = lse; p.out = workspace; p.d_lo = g.d_lo; p.nbands = g.nbands; p.nchunks = g.nchunks;
    const dim3 grid((unsigned)g.nbands, (unsigned)g.nchunks, (unsigned)(B * H));
    if (D == 32) hipLaunchKernelGGL((attn_offset_partial_kernel<32>), grid, dim3(256), 0, stream, p);
    else if (D == 64) hipLaunchKernelGGL((attn_offset_partial_kernel<64>), grid, dim3(256), 0, stream, p);
    else if (D == 128) hipLaunchKernelGGL((attn_offset_partial_kernel<128>), grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL((attn_offset_partial_kernel<256>), grid, dim3(256), 0, stream, p);
    SCONF_LAUNCH_OK("sconf_attn_offset_profile");
    hipLaunchKernelGGL(attn_offset_combine_kernel, dim3((unsigned)cdiv(2 * N - 1, 256), (unsigned)(B * H)), dim3(256), 0, stream,
                       (const float*)workspace, prof, (int)N, g.d_lo, g.d_hi, g.nbands, g.nchunks);
    SCONF_LAUNCH_OK("sconf_attn_offset_profile");
    return 0;
}
