// CTC forced alignment (include/sconf_align.h): the Viterbi path of a transcript through (B, N, C) log-probs, token spans and
// per-token log-probabilities.  The lattice is the one of ctc.hip in the (max, +) semiring, plus back-pointers and a walk back.
//
// Structure (serial in time, B-way batch parallelism, as the loss):
//   1. gather    em[b][t] = [log-prob of label 0 .. S-1 | pad | log-prob of the blank]: every blank state has the same emission, so
//                the compact row is half of the loss's (N, 2 S + 1) one, and a thread's adjacent states read CONTIGUOUS labels.
//   2. lattice   one workgroup per sample; a thread owns MAXS adjacent states, the row lives in LDS (double-buffered, one raw barrier
//                per frame), emissions are prefetched G frames ahead into registers with unconditional, clamped vector loads.  The
//                step is LDS read, two compares, one add in the state type, LDS write - no transcendental; what leaves per frame is
//                one BYTE per cell (the step taken), the thread's MAXS bytes as one vector store.  Waves whose states are all
//                unreachable (s > 2 i + 1) or can no longer reach the end (s < L - 2 (T - i)) skip the arithmetic and the store.
//                The loss's long-lattice form stages emissions by LDS-DMA because MAXS strided dword loads and MAXS strided f32
//                stores per thread and frame filled the memory pipeline; here a thread's emissions are MAXS / 2 contiguous floats
//                (one or two 16-byte loads) and its output is at most 16 bytes, so the register prefetch is kept for every length.
//   3. walk back one wave per sample.  The state falls by at most 2 per frame, so the back-pointers of K frames lie within 2 K - 1
//                cells per row below the current state: the wave fetches K rows x 32 cells at once and lane 0 walks them in LDS.
//   4. frames    one thread per frame: labels, and the span boundaries where the path changes state.
//   5. tokens    one thread per token: spans of absent tokens, and the token's log-probabilities summed in frame order.
// Steps 1, 3, 4 and 5 are in align_common.h, shared with the long form of the same contract (align_long.hip).
#include "align_common.h"
#include "../../include/sconf_align.h"

namespace {

constexpr int MAX_LABELS = 8191;               // 16383 states, the loss's limit

struct Geometry { int nt, maxs, state_bytes; size_t lds; };
inline Geometry geometry(int64_t Smax) {
    const int Lmax = (int)(2 * Smax + 1);
    Geometry g;
    g.nt = Lmax <= 256 ? 256 : (Lmax <= 512 ? 512 : 1024);       // the serial step costs a barrier + the slowest thread: few states each
    const int spt = cdiv(Lmax, g.nt);
    g.maxs = spt <= 1 ? 1 : spt <= 2 ? 2 : spt <= 4 ? 4 : spt <= 8 ? 8 : spt <= 12 ? 12 : 16;
    const size_t cells = (size_t)2 * (Lmax + g.maxs + 2);         // two rows: two guard cells in front, maxs cells of slack behind
    g.state_bytes = cells * 8 <= 160 * 1024 ? 8 : 4;
    g.lds = cells * g.state_bytes;
    return g;
}

// One workgroup per sample.  MAXS = adjacent states per thread (1, or even); LT = the state type.  `endst[b]` receives the end state,
// or -1 for a sample with no path (infeasible, poisoned, non-finite score); score[b] as the header defines it.
template <int MAXS, typename LT>
__global__ __launch_bounds__(1024) void align_lattice_kernel(const float* __restrict__ em, const int* __restrict__ targets,
                                                             const int* __restrict__ in_len, const int* __restrict__ tg_len,
                                                             unsigned char* __restrict__ bp, int* __restrict__ endst,
                                                             double* __restrict__ score, int N, int C, int Smax, int LP, int BPW) {
    extern __shared__ double lat_raw[];                 // LT [2][W]
    LT* lat = reinterpret_cast<LT*>(lat_raw);
    const int b = blockIdx.x, nt = blockDim.x, tid = threadIdx.x;
    const int T = len_of(in_len, b, N), S = len_of(tg_len, b, Smax), L = 2 * S + 1, Lmax = 2 * Smax + 1;
    const int W = Lmax + MAXS + 2;
    const LT NEG = (LT)-INFINITY;
    {                                                   // poisoned samples, as ctc_alphabeta_kernel defines them
        int bad = (T > N) | (S < 0) | (S > Smax);
        if (!bad) for (int i = tid; i < S; i += nt) { const int lab = targets[(long)b * Smax + i]; bad |= (lab < 0) | (lab >= C); }
        if (__syncthreads_or(bad)) { if (tid == 0) { score[b] = (double)NAN; endst[b] = -1; } return; }
    }
    if (T <= 0) { if (tid == 0) { score[b] = -(double)INFINITY; endst[b] = -1; } return; }

    const int sp0 = tid * MAXS, cnt = min(max(L - sp0, 0), MAXS);
    unsigned skip_ok = 0;                               // bit k: state sp0 + k may be entered from two states below
#pragma unroll
    for (int k = 0; k < MAXS; ++k) {
        const int sp = sp0 + k;
        if (sp < L && sp >= 3 && (sp & 1) && targets[(long)b * Smax + (sp >> 1)] != targets[(long)b * Smax + (sp >> 1) - 1]) skip_ok |= 1u << k;
    }
    for (int i = tid; i < 2 * W; i += nt) lat[i] = NEG;
    __syncthreads();
    if (tid == 0) lat[W + 2] = (LT)0;                    // virtual frame -1 (row 1): state 0 at 0, so frame 0 is the general step (0 + e = e exactly)
    __syncthreads();

    // Emissions of this thread: NL contiguous labels and the blank (MAXS == 1: the one emission of its state).  Loads are
    // unconditional, from clamped (always valid) addresses; what the clamped ones bring belongs to states the thread does not own.
    constexpr int NL = MAXS == 1 ? 1 : MAXS / 2, NE = MAXS == 1 ? 1 : NL + 1;
    constexpr int G = MAXS <= 4 ? 4 : 2;                // frames prefetched together
    const int j0 = MAXS == 1 ? ((tid & 1) ? min(tid >> 1, LP - 1) : LP) : min(tid * NL, LP - NL);
    const float* eb = em + (long)b * N * (LP + 4);
    float pf[G][NE], nx[G][NE];
    auto load_group = [&](float (&dst)[G][NE], int i0) {
#pragma unroll
        for (int j = 0; j < G; ++j) {
            const float* r = eb + (long)min(i0 + j, T - 1) * (LP + 4);
            if constexpr (MAXS == 1) dst[j][0] = r[j0];
            else {
                float lv[NL];
                load_labels<NL>(r + j0, lv);
#pragma unroll
                for (int k = 0; k < NL; ++k) dst[j][k] = lv[k];
                dst[j][NL] = r[LP];
            }
        }
    };
    load_group(pf, 0);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int w0 = wave * 64 * MAXS, w1 = w0 + 64 * MAXS - 1;     // the wave's range of states
    unsigned char* brow = bp + (long)b * N * BPW + sp0;
    for (int i0 = 0; i0 < T; i0 += G) {
        load_group(nx, i0 + G);
#pragma unroll
        for (int j = 0; j < G; ++j) {
            const int i = i0 + j;
            if (i < T) {                                  // uniform across the workgroup
                LT* cur = lat + (i & 1) * W + 2;
                const LT* prev = lat + ((i & 1) ^ 1) * W + 2;
                const int hi = 2 * i + 1, lo = L - 2 * (T - i);       // live band of states at this frame
                if (w0 <= hi && w1 >= lo) {                           // wave-uniform
                    if (cnt > 0) {
                        LT pv[MAXS + 2];
#pragma unroll
                        for (int q = 0; q < MAXS + 2; ++q) pv[q] = prev[sp0 - 2 + q];
                        unsigned pk[(MAXS + 3) / 4] = {};
#pragma unroll
                        for (int k = 0; k < MAXS; ++k) {
                            const float e = MAXS == 1 ? pf[j][0] : ((k & 1) ? pf[j][k >> 1] : pf[j][NL]);
                            LT best = pv[k + 2];
                            unsigned step = 0;
                            if (pv[k + 1] > best) { best = pv[k + 1]; step = 1; }
                            if (((skip_ok >> k) & 1) && pv[k] > best) { best = pv[k]; step = 2; }
                            cur[sp0 + k] = best + (LT)e;              // (cells past L fall into the slack behind the row)
                            pk[k / 4] |= step << (8 * (k & 3));
                        }
                        unsigned char* o = brow + (long)i * BPW;
                        if constexpr (MAXS == 1) *o = (unsigned char)pk[0];
                        else if constexpr (MAXS == 2) *reinterpret_cast<unsigned short*>(o) = (unsigned short)pk[0];
                        else if constexpr (MAXS == 4) *reinterpret_cast<unsigned*>(o) = pk[0];
                        else if constexpr (MAXS == 8) *reinterpret_cast<uint2*>(o) = make_uint2(pk[0], pk[1]);
                        else if constexpr (MAXS == 12) { unsigned* o4 = reinterpret_cast<unsigned*>(o); o4[0] = pk[0]; o4[1] = pk[1]; o4[2] = pk[2]; }
                        else *reinterpret_cast<uint4*>(o) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < MAXS; ++k) if (k < cnt) cur[sp0 + k] = NEG;
                }
                wait_lgkm0_barrier();                     // not __syncthreads(): nothing waits for the frame's global stores
            }
        }
#pragma unroll
        for (int j = 0; j < G; ++j)
#pragma unroll
            for (int k = 0; k < NE; ++k) pf[j][k] = nx[j][k];
    }
    if (tid == 0) {
        const LT* last = lat + ((T - 1) & 1) * W + 2;
        int end = L - 1;
        LT v = last[L - 1];
        if (L > 1 && last[L - 2] > v) { v = last[L - 2]; end = L - 2; }
        score[b] = (double)v;
        endst[b] = v > NEG ? end : -1;                    // -inf: no path fits; NaN: non-finite log-probs, reported as no path
    }
}


}  // namespace

SCONF_API int sconf_align_max_labels(void) { return MAX_LABELS; }
SCONF_API int sconf_align_state_bytes(int64_t Smax) { return Smax < 0 || Smax > MAX_LABELS ? -1 : geometry(Smax).state_bytes; }
SCONF_API int sconf_align_threads(int64_t Smax) { return Smax < 0 || Smax > MAX_LABELS ? -1 : geometry(Smax).nt; }
SCONF_API int sconf_align_states_per_thread(int64_t Smax) { return Smax < 0 || Smax > MAX_LABELS ? -1 : geometry(Smax).maxs; }
SCONF_API int sconf_align_walk_window(void) { return WALK_K; }

SCONF_API int64_t sconf_align_workspace(int64_t B, int64_t N, int64_t Smax) {
    if (B < 1 || N < 1 || Smax < 0 || Smax > MAX_LABELS || B * N > 0x7fffffff) return -1;
    return round256(4 * B) + round256(4 * B * N * (label_pitch(Smax) + 4)) + round256(B * N * bp_pitch(Smax));
}

SCONF_API int sconf_align_ctc(const float* log_probs, const int32_t* targets, const int32_t* input_lengths, const int32_t* target_lengths,
                              int32_t* path, int32_t* labels, int32_t* spans, float* token_logp, double* score, void* workspace,
                              int64_t workspace_bytes, int64_t B, int64_t N, int64_t C, int64_t Smax, int blank, sconf_stream_t stream) {
    if (B == 0) return 0;
    SCONF_REQUIRE(Smax >= 0 && Smax <= MAX_LABELS, "sconf_align_ctc: %ld labels: at most %d (16383 lattice states)", (long)Smax, MAX_LABELS);
    SCONF_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && B * N <= 0x7fffffff, "sconf_align_ctc: bad sizes B = %ld, N = %ld", (long)B, (long)N);
    SCONF_REQUIRE(C >= 4 && C % 4 == 0 && C * 4 <= 64 * 1024, "sconf_align_ctc: C must be a multiple of 4 and one row must fit LDS (%ld classes)", (long)C);
    SCONF_REQUIRE(blank >= 0 && blank < C, "sconf_align_ctc: blank %d out of range", blank);
    SCONF_REQUIRE(log_probs && path && labels && score && workspace && (Smax == 0 || (targets && spans && token_logp)), "sconf_align_ctc: null pointer");
    SCONF_REQUIRE(workspace_bytes >= sconf_align_workspace(B, N, Smax), "sconf_align_ctc: workspace of %ld bytes, %ld needed",
                  (long)workspace_bytes, (long)sconf_align_workspace(B, N, Smax));
    const int LP = label_pitch(Smax), BPW = bp_pitch(Smax);
    int* endst = (int*)workspace;
    float* em = (float*)((char*)workspace + round256(4 * B));
    unsigned char* bp = (unsigned char*)em + round256(4 * B * N * (LP + 4));
    hipLaunchKernelGGL(align_gather_kernel, dim3((unsigned)std::min<long>(B * N, 65536)), dim3(256), (size_t)C * 4, stream, log_probs, targets,
                       input_lengths, target_lengths, em, (int)B, (int)N, (int)C, (int)Smax, LP, blank);
    const Geometry g = geometry(Smax);
#define L2(MS, LT) do { \
        if (g.lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)align_lattice_kernel<MS, LT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds); \
        hipLaunchKernelGGL((align_lattice_kernel<MS, LT>), dim3((unsigned)B), dim3(g.nt), g.lds, stream, em, targets, input_lengths, \
                           target_lengths, bp, endst, score, (int)N, (int)C, (int)Smax, LP, BPW); } while (0)
#define L(MS) do { if (g.state_bytes == 8) L2(MS, double); else L2(MS, float); } while (0)
    switch (g.maxs) { case 1: L(1); break; case 2: L(2); break; case 4: L(4); break; case 8: L(8); break; case 12: L(12); break; default: L(16); }
#undef L2
#undef L
    const int K = walk_window();
    hipLaunchKernelGGL(align_walk_kernel, dim3((unsigned)B), dim3(64), 0, stream, bp, endst, input_lengths, path, spans, (int)N, (int)Smax, BPW, K);
    hipLaunchKernelGGL(align_frames_kernel, dim3((unsigned)cdiv(N, 256), (unsigned)B), dim3(256), 0, stream, targets, endst, input_lengths,
                       path, labels, spans, (int)N, (int)Smax, blank);
    if (Smax > 0)
        hipLaunchKernelGGL(align_tokens_kernel, dim3((unsigned)cdiv(Smax, 256), (unsigned)B), dim3(256), 0, stream, log_probs, targets, endst,
                           input_lengths, target_lengths, spans, token_logp, (int)N, (int)C, (int)Smax);
    SCONF_LAUNCH_OK("sconf_align_ctc");
    return 0;
}
