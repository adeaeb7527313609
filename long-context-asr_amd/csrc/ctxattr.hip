// Context attribution (include/sconf_ctxattr.h): window means, the masked batch, and the I x J matrix of edit distances of the spliced
// hypotheses, from two boundary DPs over the clean hypothesis and |middle| rows per pair.
//
// A DP row of R + 1 cells is held in V space, V[k] = D[k] - k, so that a Levenshtein row is one min-plus prefix scan with no index
// arithmetic:  U[k] = min(V[k] + 1, V[k-1] - (ref[k-1] == x)),  V'[k] = prefixmin U.  Thread t holds the CPT cells from t * CPT on
// in registers.  row_step: a serial scan of the thread's cells, an inclusive prefix-min over the wave (__shfl_up), the wave totals
// through LDS (double-buffered by row parity: one barrier per row), and the thread's first cell takes V[k-1] from its left
// neighbour's last cell by one more __shfl_up - lane 0 of a wave takes it from the partials it has just read: the prefix-min over the
// waves before it IS the last cell of the wave before it.  Thread 0 has no left neighbour: its `left` is BIG for good, which leaves
// U[0] = V[0] + 1.
//
// The reference ids sit beside the cells in registers up to 32 cells per thread; at 64 (1024 threads leave 128 VGPRs) they are
// re-read per row from a padded copy in the workspace (256 KB, resident in L2), 16 bytes at a time.  The padded copy holds
// refpad[k] = ref[k-1], so no cell needs a bounds check: cells past R compute values that no cell at or below R ever reads (the scan
// runs left to right) and the final reduction leaves them out.
//
// The backward rows are the same DP on both sequences reversed; they are dumped reversed, so that B_i[k] lies beside F_i[k].
#include "common.h"
#include "../../include/sconf_ctxattr.h"
#include <algorithm>
#include <vector>

namespace {

constexpr int MAX_REF = 65535;
constexpr int MAX_WINDOW = 8192;                // g - f + 1: the collapsed middle in LDS, 32 KB
constexpr int BIG = 1 << 29;
constexpr int STAGE_WINDOWS = 224;              // windows per staging launch: 3584 bytes of kernel arguments

inline bool ref_ok(int64_t R) { return R >= 0 && R <= MAX_REF; }
inline int cpt_of(int64_t R) {
    const int64_t cells = R + 1;
    int c = 1;
    while ((int64_t)1024 * c < cells) c *= 2;
    return c;
}
inline int threads_of(int64_t R) {
    const int64_t cells = R + 1;
    int nt = 64;
    while (nt < 1024 && nt < cells) nt *= 2;
    return nt;
}

struct Parts { int64_t win, ref, rows; };
inline Parts parts(int64_t I, int64_t R) {
    const int64_t P = (int64_t)threads_of(R) * cpt_of(R);
    return {round256(16 * I), round256(8 * P), round256(4 * I * P)};
}

// ---- window means and the masked batch -------------------------------------------------------------------------------------------
__device__ __forceinline__ void clamped_window(const int* __restrict__ windows, long j, int T, int& s, int& e) {
    s = min(max(windows[2 * j], 0), T);
    e = min(max(windows[2 * j + 1], 0), T);
}

__global__ __launch_bounds__(256) void ctxattr_means_kernel(const float* __restrict__ spec, const int* __restrict__ windows,
                                                            float* __restrict__ means, int F, int T) {
    __shared__ double red[256];
    const int j = blockIdx.x, tid = threadIdx.x;
    int s, e;
    clamped_window(windows, j, T, s, e);
    double acc = 0.0;
    for (int r = 0; r < F; ++r)
        for (int c = s + tid; c < e; c += 256) acc += (double)spec[(long)r * T + c];
    red[tid] = acc;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    if (tid == 0) means[j] = e > s ? __double2float_rn(__ddiv_rn(red[0], (double)F * (double)(e - s))) : 0.f;
}

// grid (column blocks, b * F rows); VEC = 4 needs T % 4 == 0 and 16-byte aligned spec and dst
template <int VEC>
__global__ __launch_bounds__(256) void ctxattr_fill_kernel(const float* __restrict__ spec, const int* __restrict__ windows,
                                                           const float* __restrict__ means, float* __restrict__ dst, int F, int T, int j0) {
    const int row = blockIdx.y, k = row / F, r = row - k * F;
    int s, e;
    clamped_window(windows, j0 + k, T, s, e);
    const float m = means[j0 + k];
    const float* __restrict__ src = spec + (long)r * T;
    float* __restrict__ out = dst + (long)row * T;
    for (int t = (blockIdx.x * 256 + threadIdx.x) * VEC; t < T; t += gridDim.x * 256 * VEC) {
        if constexpr (VEC == 4) {
            float4 v = *(const float4*)(src + t);
            if (t >= s && t < e) v.x = m;
            if (t + 1 >= s && t + 1 < e) v.y = m;
            if (t + 2 >= s && t + 2 < e) v.z = m;
            if (t + 3 >= s && t + 3 < e) v.w = m;
            *(float4*)(out + t) = v;
        } else {
            out[t] = (t >= s && t < e) ? m : src[t];
        }
    }
}

// ---- staging: the windows (f, g, k-th window by f, k-th window by g) and the padded reference, both ways --------------------------
struct WinChunk { int4 w[STAGE_WINDOWS]; };

__global__ __launch_bounds__(256) void ctxattr_stage_kernel(const WinChunk chunk, int n, int w0, int4* __restrict__ win,
                                                            const int* __restrict__ ref, int R, int P, int* __restrict__ refpad, int with_ref) {
    if (blockIdx.x == 0 && (int)threadIdx.x < n) win[w0 + threadIdx.x] = chunk.w[threadIdx.x];
    if (with_ref)
        for (int k = blockIdx.x * 256 + threadIdx.x; k < P; k += gridDim.x * 256) {
            const bool in = k >= 1 && k <= R;
            refpad[k] = in ? ref[k - 1] : 0;                 // forward: cell k compares ref[k-1]
            refpad[P + k] = in ? ref[R - k] : 0;             // backward: cell m compares reversed(ref)[m-1] = ref[R-m]
        }
}

// ---- one DP row ----------------------------------------------------------------------------------------------------------------
template <int CPT>
__device__ __forceinline__ void load_cells(int (&dst)[CPT], const int* __restrict__ src) {
    if constexpr (CPT >= 4) {
#pragma unroll
        for (int q = 0; q < CPT / 4; ++q) {
            const int4 v = ((const int4*)src)[q];
            dst[4 * q] = v.x; dst[4 * q + 1] = v.y; dst[4 * q + 2] = v.z; dst[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int c = 0; c < CPT; ++c) dst[c] = src[c];
    }
}

template <int CPT>
__device__ __forceinline__ void store_cells(int* __restrict__ dst, const int (&src)[CPT]) {
    if constexpr (CPT >= 4) {
#pragma unroll
        for (int q = 0; q < CPT / 4; ++q) ((int4*)dst)[q] = make_int4(src[4 * q], src[4 * q + 1], src[4 * q + 2], src[4 * q + 3]);
    } else {
#pragma unroll
        for (int c = 0; c < CPT; ++c) dst[c] = src[c];
    }
}

// V: the thread's cells; left: V[k-1] of its first cell (BIG in thread 0); rr: its reference ids (HOLD) or mine = refpad + tid * CPT;
// part: LDS [2][16], par: the row's parity.  One __syncthreads.
template <int CPT, bool HOLD>
__device__ __forceinline__ void row_step(int (&V)[CPT], int& left, const int (&rr)[HOLD ? CPT : 1], const int* __restrict__ mine, int x,
                                         int (*part)[16], int par) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int prev = left, run = BIG;
    if constexpr (HOLD) {
#pragma unroll
        for (int c = 0; c < CPT; ++c) {
            const int u = min(V[c] + 1, prev - (rr[c] == x ? 1 : 0));
            prev = V[c];
            run = min(run, u);
            V[c] = run;
        }
    } else {
#pragma unroll
        for (int h = 0; h < CPT / 16; ++h) {                     // 16 ids at a time: four 16-byte loads in flight, no more (registers)
            int4 r4[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) r4[q] = ((const int4*)mine)[4 * h + q];
            asm volatile("" ::: "memory");
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r[4] = {r4[q].x, r4[q].y, r4[q].z, r4[q].w};
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    const int c = 16 * h + 4 * q + d;
                    const int u = min(V[c] + 1, prev - (r[d] == x ? 1 : 0));
                    prev = V[c];
                    run = min(run, u);
                    V[c] = run;
                }
            }
        }
    }
    int incl = run;                                           // inclusive prefix-min of the threads' totals over the wave
#pragma unroll
    for (int d = 1; d < 64; d *= 2) {
        const int o = __shfl_up(incl, d, 64);
        if (lane >= d) incl = min(incl, o);
    }
    if (lane == 63) part[par][wave] = incl;
    int before = __shfl_up(incl, 1, 64);                      // exclusive
    if (lane == 0) before = BIG;
    __syncthreads();
    int waves_before = BIG;
    for (int w = 0; w < wave; ++w) waves_before = min(waves_before, part[par][w]);
    before = min(before, waves_before);
#pragma unroll
    for (int c = 0; c < CPT; ++c) V[c] = min(V[c], before);
    const int from_lane = __shfl_up(V[CPT - 1], 1, 64);
    if (threadIdx.x != 0) left = lane == 0 ? waves_before : from_lane;
}

// ---- 1. the boundary rows --------------------------------------------------------------------------------------------------------
// Block 0: forward over the frames 0 .. N-1, F_i dumped before frame f_i is consumed.  Block 1: backward over N-1 .. 0 on the reversed
// reference, B_i dumped (reversed) before frame ge_i - 1 is consumed, ge = min(g + 1, N).
template <int CPT, bool HOLD, bool BACK>
__device__ __forceinline__ void boundary_run(const int* __restrict__ clean, int N, int blank, const int* __restrict__ refpad,
                                             const int4* __restrict__ win, int I, int R, int P, int* __restrict__ rows,
                                             int* __restrict__ clean_errors, int* __restrict__ clean_len, int (*part)[16], int* labs) {
    const int tid = threadIdx.x, NT = blockDim.x;
    const int* __restrict__ mine = refpad + (BACK ? P : 0) + tid * CPT;
    int V[CPT], rr[HOLD ? CPT : 1];
    if constexpr (HOLD) load_cells<CPT>(rr, mine);
#pragma unroll
    for (int c = 0; c < CPT; ++c) V[c] = 0;
    int left = tid ? 0 : BIG, par = 0, count = 0, cur = 0;

    // the k-th dump: its window, and the frame before which it is due (forward: f; backward: ge - 1), -1 when none is left
    auto window_of = [&](int k) { return BACK ? win[I - 1 - k].w : win[k].z; };
    auto due = [&](int k) -> int {
        if (k >= I) return -1;
        const int4 w = win[window_of(k)];
        return BACK ? min(w.y + 1, N) - 1 : w.x;
    };
    auto dump = [&](int k) {
        int* __restrict__ row = rows + (long)window_of(k) * P;
        if constexpr (!BACK) {
            store_cells<CPT>(row + tid * CPT, V);
        } else {
            const int last = R - tid * CPT;                  // cell m = tid * CPT + c goes to row[R - m] = top[-c], while c <= last
            int* __restrict__ top = row + last;
#pragma unroll
            for (int c = 0; c < CPT; ++c) if (c <= last) top[-c] = V[c];
        }
    };
    int next = due(0);
    for (int base = 0; base < N; base += NT) {
        if (base + tid < N) {
            const int t = BACK ? N - 1 - (base + tid) : base + tid;
            const int a = clean[t];
            labs[tid] = (a != blank && (t == 0 || a != clean[t - 1])) ? a : -1;
        }
        __syncthreads();
        const int n = min(NT, N - base);
        for (int q = 0; q < n; ++q) {
            const int t = BACK ? N - 1 - (base + q) : base + q;
            while (next == t) { dump(cur); next = due(++cur); }
            const int x = labs[q];
            if (x >= 0) { row_step<CPT, HOLD>(V, left, rr, mine, x, part, par); par ^= 1; ++count; }
        }
        __syncthreads();
    }
    while (cur < I) dump(cur++);                               // forward: f = N
    if constexpr (!BACK) {
#pragma unroll
        for (int c = 0; c < CPT; ++c) if (tid * CPT + c == R) *clean_errors = V[c] + R;
        if (tid == 0) *clean_len = count;
    }
}

template <int CPT, bool HOLD>
__global__ __launch_bounds__(1024) void ctxattr_boundary_kernel(const int* __restrict__ clean, int N, int blank, const int* __restrict__ refpad,
                                                                const int4* __restrict__ win, int I, int R, int P, int* __restrict__ Frows,
                                                                int* __restrict__ Brows, int* __restrict__ clean_errors,
                                                                int* __restrict__ clean_len) {
    __shared__ int part[2][16];
    __shared__ int labs[1024];
    if (blockIdx.x == 0) boundary_run<CPT, HOLD, false>(clean, N, blank, refpad, win, I, R, P, Frows, clean_errors, clean_len, part, labs);
    else boundary_run<CPT, HOLD, true>(clean, N, blank, refpad, win, I, R, P, Brows, clean_errors, clean_len, part, labs);
}

// ---- 2. the pairs ----------------------------------------------------------------------------------------------------------------
template <int CPT, bool HOLD>
__global__ __launch_bounds__(1024) void ctxattr_pair_kernel(const int* __restrict__ clean, const int* __restrict__ masked, int N, int blank,
                                                            const int* __restrict__ refpad, const int4* __restrict__ win, int R, int P,
                                                            const int* __restrict__ Frows, const int* __restrict__ Brows, int J,
                                                            int* __restrict__ errors, int* __restrict__ mid_len, int* __restrict__ mid_tokens,
                                                            int mid_cap) {
    __shared__ int part[2][16];
    __shared__ int wsum[16];
    __shared__ int wmin[16];
    __shared__ int mid[MAX_WINDOW];
    const int tid = threadIdx.x, NT = blockDim.x, lane = tid & 63, wave = tid >> 6, NW = NT >> 6;
    const int j = blockIdx.x, i = blockIdx.y;
    const int f = win[i].x, g = win[i].y, ge = min(g + 1, N), L = ge - f;
    const int* __restrict__ aj = masked + (long)j * N;

    // the middle: the thread's frames, counted, placed by a prefix sum over the workgroup, written to LDS in order
    const int per = (L + NT - 1) / NT, t0 = min(f + tid * per, ge), t1 = min(t0 + per, ge);
    auto lab = [&](int t) { return t >= f && t < g ? aj[t] : clean[t]; };
    int cnt = 0;
    {
        int p = t0 > 0 && t0 < t1 ? lab(t0 - 1) : -1;
        for (int t = t0; t < t1; ++t) { const int a = lab(t); cnt += (a != blank && (t == 0 || a != p)); p = a; }
    }
    int incl = cnt;
#pragma unroll
    for (int d = 1; d < 64; d *= 2) { const int o = __shfl_up(incl, d, 64); if (lane >= d) incl += o; }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int off = incl - cnt, len = 0;
    for (int w = 0; w < NW; ++w) { const int s = wsum[w]; if (w < wave) off += s; len += s; }
    {
        int p = t0 > 0 && t0 < t1 ? lab(t0 - 1) : -1;
        for (int t = t0; t < t1; ++t) { const int a = lab(t); if (a != blank && (t == 0 || a != p)) mid[off++] = a; p = a; }
    }
    __syncthreads();
    const long pair = (long)i * J + j;
    if (tid == 0) mid_len[pair] = len;
    if (mid_tokens)
        for (int q = tid; q < mid_cap; q += NT) mid_tokens[pair * mid_cap + q] = q < len ? mid[q] : 0;

    // F_i advanced by the middle
    const int* __restrict__ mine = refpad + tid * CPT;
    const int* __restrict__ frow = Frows + (long)i * P + tid * CPT;
    int V[CPT], rr[HOLD ? CPT : 1];
    if constexpr (HOLD) load_cells<CPT>(rr, mine);
    load_cells<CPT>(V, frow);
    int left = tid ? frow[-1] : BIG, par = 0;
    for (int q = 0; q < len; ++q) { row_step<CPT, HOLD>(V, left, rr, mine, mid[q], part, par); par ^= 1; }

    // min_k M[k] + B_i[k] = R + min_k V[k] + VB[k]
    const int* __restrict__ brow = Brows + (long)i * P + tid * CPT;
    int best = BIG;
    const int last = R - tid * CPT;                            // the thread's cells c <= last are cells of the row
#pragma unroll
    for (int c = 0; c < CPT; ++c) if (c <= last) best = min(best, V[c] + brow[c]);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) best = min(best, __shfl_xor(best, d, 64));
    if (lane == 0) wmin[wave] = best;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < NW; ++w) best = min(best, wmin[w]);
        errors[pair] = best + R;
    }
}

template <int CPT, bool HOLDB, bool HOLD>
void launch_score(int nt, hipStream_t stream, const int* clean, const int* masked, int N, int blank, const int* refpad, const int4* win, int I,
                  int J, int R, int P, int* Frows, int* Brows, int* errors, int* clean_errors, int* clean_len, int* mid_len, int* mid_tokens,
                  int mid_cap) {
    hipLaunchKernelGGL((ctxattr_boundary_kernel<CPT, HOLDB>), dim3(2), dim3(nt), 0, stream, clean, N, blank, refpad, win, I, R, P, Frows, Brows,
                       clean_errors, clean_len);
    hipLaunchKernelGGL((ctxattr_pair_kernel<CPT, HOLD>), dim3((unsigned)J, (unsigned)I), dim3(nt), 0, stream, clean, masked, N, blank, refpad, win,
                       R, P, (const int*)Frows, (const int*)Brows, J, errors, mid_len, mid_tokens, mid_cap);
}

}  // namespace

SCONF_API int sconf_ctxattr_max_ref(void) { return MAX_REF; }
SCONF_API int sconf_ctxattr_max_window_frames(void) { return MAX_WINDOW; }
SCONF_API int sconf_ctxattr_threads(int64_t R) { return ref_ok(R) ? threads_of(R) : -1; }
SCONF_API int sconf_ctxattr_cells_per_thread(int64_t R) { return ref_ok(R) ? cpt_of(R) : -1; }

SCONF_API int64_t sconf_ctxattr_score_workspace(int64_t N, int64_t I, int64_t J, int64_t R) {
    if (N < 1 || I < 1 || I > 65535 || J < 1 || !ref_ok(R) || N > 0x7fffffff / J) return -1;
    const Parts p = parts(I, R);
    return p.win + p.ref + 2 * p.rows;
}

SCONF_API int sconf_ctxattr_window_means(const float* spec, const int32_t* windows, float* means, int64_t F, int64_t T, int64_t J,
                                         sconf_stream_t stream) {
    if (J == 0) return 0;
    SCONF_REQUIRE(F >= 1 && T >= 1 && J >= 1 && T <= 0x7fffffff && J <= 0x7fffffff && F <= 0x7fffffff,
                  "sconf_ctxattr_window_means: bad sizes F = %ld, T = %ld, J = %ld", (long)F, (long)T, (long)J);
    SCONF_REQUIRE(spec && windows && means, "sconf_ctxattr_window_means: null pointer");
    hipLaunchKernelGGL(ctxattr_means_kernel, dim3((unsigned)J), dim3(256), 0, stream, spec, windows, means, (int)F, (int)T);
    SCONF_LAUNCH_OK("sconf_ctxattr_window_means");
    return 0;
}

SCONF_API int sconf_ctxattr_mask_fill(const float* spec, const int32_t* windows, const float* means, float* dst, int64_t F, int64_t T, int64_t J,
                                      int64_t j0, int64_t b, sconf_stream_t stream) {
    if (b == 0) return 0;
    SCONF_REQUIRE(F >= 1 && T >= 1 && J >= 1 && T <= 0x7fffffff && J <= 0x7fffffff && F <= 65535,
                  "sconf_ctxattr_mask_fill: bad sizes F = %ld, T = %ld, J = %ld", (long)F, (long)T, (long)J);
    SCONF_REQUIRE(j0 >= 0 && b >= 1 && j0 <= J - b && b * F <= 65535,
                  "sconf_ctxattr_mask_fill: bad batch j0 = %ld, b = %ld of J = %ld windows (b F <= 65535)", (long)j0, (long)b, (long)J);
    SCONF_REQUIRE(spec && windows && means && dst, "sconf_ctxattr_mask_fill: null pointer");
    const bool vec = T % 4 == 0 && ((uintptr_t)spec | (uintptr_t)dst) % 16 == 0;
    const dim3 grid((unsigned)std::min<int64_t>(cdiv(T, vec ? 1024 : 256), 1024), (unsigned)(b * F));
    if (vec) hipLaunchKernelGGL(ctxattr_fill_kernel<4>, grid, dim3(256), 0, stream, spec, windows, means, dst, (int)F, (int)T, (int)j0);
    else hipLaunchKernelGGL(ctxattr_fill_kernel<1>, grid, dim3(256), 0, stream, spec, windows, means, dst, (int)F, (int)T, (int)j0);
    SCONF_LAUNCH_OK("sconf_ctxattr_mask_fill");
    return 0;
}

SCONF_API int sconf_ctxattr_score(const int32_t* clean, const int32_t* masked, const int32_t* ref, const int32_t* frame_windows, int32_t* errors,
                                  int32_t* clean_errors, int32_t* clean_len, int32_t* mid_len, int32_t* mid_tokens, void* workspace,
                                  int64_t workspace_bytes, int64_t N, int64_t I, int64_t J, int64_t R, int64_t mid_cap, int blank,
                                  sconf_stream_t stream) {
    SCONF_REQUIRE(ref_ok(R), "sconf_ctxattr_score: %ld reference ids: at most %d", (long)R, MAX_REF);
    SCONF_REQUIRE(N >= 1 && I >= 1 && I <= 65535 && J >= 1 && N <= 0x7fffffff / J, "sconf_ctxattr_score: bad sizes N = %ld, I = %ld, J = %ld",
                  (long)N, (long)I, (long)J);
    SCONF_REQUIRE(clean && masked && (ref || R == 0) && frame_windows && errors && clean_errors && clean_len && mid_len && workspace,
                  "sconf_ctxattr_score: null pointer");
    int64_t widest = 1;
    for (int64_t i = 0; i < I; ++i) {
        const int64_t f = frame_windows[2 * i], g = frame_windows[2 * i + 1];
        SCONF_REQUIRE(f >= 0 && f <= g && g <= N, "sconf_ctxattr_score: frame window %ld = [%ld, %ld) is not within 0 <= f <= g <= N = %ld", (long)i,
                      (long)f, (long)g, (long)N);
        SCONF_REQUIRE(g - f + 1 <= MAX_WINDOW, "sconf_ctxattr_score: frame window %ld = [%ld, %ld) is wider than the bound: g - f + 1 <= %d", (long)i,
                      (long)f, (long)g, MAX_WINDOW);
        widest = std::max(widest, std::min(g + 1, N) - f);
    }
    SCONF_REQUIRE(!mid_tokens || (mid_cap >= widest && mid_cap <= MAX_WINDOW), "sconf_ctxattr_score: mid_cap %ld, the widest middle has %ld frames",
                  (long)mid_cap, (long)widest);
    SCONF_REQUIRE(workspace_bytes >= sconf_ctxattr_score_workspace(N, I, J, R), "sconf_ctxattr_score: workspace of %ld bytes, %ld needed",
                  (long)workspace_bytes, (long)sconf_ctxattr_score_workspace(N, I, J, R));
    const int nt = threads_of(R), cpt = cpt_of(R), P = nt * cpt;
    const Parts p = parts(I, R);
    char* ws = (char*)workspace;
    int4* win = (int4*)ws;
    int* refpad = (int*)(ws + p.win);
    int* Frows = (int*)(ws + p.win + p.ref);
    int* Brows = (int*)(ws + p.win + p.ref + p.rows);

    // the two orders: by f (forward dumps) and by g (backward dumps, taken from the far end)
    std::vector<int> by_f((size_t)I), by_g((size_t)I);
    for (int64_t i = 0; i < I; ++i) by_f[i] = by_g[i] = (int)i;
    std::stable_sort(by_f.begin(), by_f.end(), [&](int a, int b) { return frame_windows[2 * a] < frame_windows[2 * b]; });
    std::stable_sort(by_g.begin(), by_g.end(), [&](int a, int b) { return frame_windows[2 * a + 1] < frame_windows[2 * b + 1]; });
    for (int64_t w0 = 0; w0 < I; w0 += STAGE_WINDOWS) {
        WinChunk chunk;
        const int n = (int)std::min<int64_t>(STAGE_WINDOWS, I - w0);
        for (int k = 0; k < n; ++k) chunk.w[k] = make_int4(frame_windows[2 * (w0 + k)], frame_windows[2 * (w0 + k) + 1], by_f[w0 + k], by_g[w0 + k]);
        for (int k = n; k < STAGE_WINDOWS; ++k) chunk.w[k] = make_int4(0, 0, 0, 0);
        hipLaunchKernelGGL(ctxattr_stage_kernel, dim3(w0 == 0 ? (unsigned)cdiv(P, 256) : 1u), dim3(256), 0, stream, chunk, n, (int)w0, win, ref, (int)R,
                           P, refpad, w0 == 0 ? 1 : 0);
    }
#define SCORE(CPT, HOLDB, HOLD) launch_score<CPT, HOLDB, HOLD>(nt, stream, clean, masked, (int)N, blank, refpad, win, (int)I, (int)J, (int)R, P, Frows, Brows, errors, \
                                                 clean_errors, clean_len, mid_len, mid_tokens, mid_tokens ? (int)mid_cap : 0)
    switch (cpt) {
        case 1: SCORE(1, true, true); break;
        case 2: SCORE(2, true, true); break;
        case 4: SCORE(4, true, true); break;
        case 8: SCORE(8, true, true); break;
        case 16: SCORE(16, true, true); break;
        case 32: SCORE(32, false, true); break;
        default: SCORE(64, false, false); break;
    }
#undef SCORE
    SCONF_LAUNCH_OK("sconf_ctxattr_score");
    return 0;
}
