// The lattice of the short form of CTC forced alignment (csrc/align.hip: one workgroup per sample, up to 8191 labels): its launch
// geometry, the kernel and its launch.  An internal header in the manner of align_common.h: csrc/align.hip and csrc/seg.hip each
// instantiate their own copy.  The kernel sees emissions (the compact rows of align_gather_kernel) and label ids only; `C` is the
// number of label values it accepts, one more than the classes where the caller counts a star label (csrc/seg.hip).
#pragma once
#include "align_common.h"

namespace {

constexpr int ALIGN_MAX_LABELS = 8191;               // 16383 states, the loss's limit

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

// The lattice launch of one call: the instantiation the geometry of Smax names, one workgroup per sample.
inline void launch_align_lattice(const float* em, const int* targets, const int* input_lengths, const int* target_lengths, unsigned char* bp,
                                 int* endst, double* score, int64_t B, int64_t N, int64_t C, int64_t Smax, int LP, int BPW, hipStream_t stream) {
    const Geometry g = geometry(Smax);
#define L2(MS, LT) do { \
        if (g.lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)align_lattice_kernel<MS, LT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds); \
        hipLaunchKernelGGL((align_lattice_kernel<MS, LT>), dim3((unsigned)B), dim3(g.nt), g.lds, stream, em, targets, input_lengths, \
                           target_lengths, bp, endst, score, (int)N, (int)C, (int)Smax, LP, BPW); } while (0)
#define L(MS) do { if (g.state_bytes == 8) L2(MS, double); else L2(MS, float); } while (0)
    switch (g.maxs) { case 1: L(1); break; case 2: L(2); break; case 4: L(4); break; case 8: L(8); break; case 12: L(12); break; default: L(16); }
#undef L2
#undef L
}

}  // namespace
