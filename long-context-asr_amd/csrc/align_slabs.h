// The lattice of the long form of CTC forced alignment (csrc/align_long.hip: state slabs launched one after the other, up to 65535
// labels): the sample kernel, the slab kernel and their launch sequence.  An internal header in the manner of align_common.h:
// csrc/align_long.hip and csrc/seg.hip each instantiate their own copy.  The kernels see emissions (the compact rows of
// align_gather_kernel) and label ids only; `C` is the number of label values the sample kernel accepts, one more than the classes
// where the caller counts a star label (csrc/seg.hip).
#pragma once
#include "align_common.h"

namespace {

constexpr int LALIGN_MAX_LABELS = 65535;               // 131071 states
constexpr int LALIGN_DEFAULT_SLAB = 8192;              // 1024 threads x 8 states: two f64 rows of 3 + 1024 x 9 cells are 147 504 bytes of LDS

inline int slab_of(int slab_states) { return slab_states == 0 ? LALIGN_DEFAULT_SLAB : slab_states; }
inline bool slab_ok(int slab_states) {
    const int w = slab_of(slab_states);
    return w >= 256 && w <= 8192 && (w & (w - 1)) == 0;
}
inline bool smax_ok(int64_t Smax) { return Smax >= 0 && Smax <= LALIGN_MAX_LABELS; }
inline int threads_of(int w) { return std::min(1024, w); }
// LDS row of a slab: per thread MAXS cells and, from 2 states per thread on, one cell of padding; the guard cells in front
__host__ __device__ constexpr int row_pitch(int maxs) { return maxs == 1 ? 1 : maxs + 1; }
__host__ __device__ constexpr int row_guard(int maxs) { return maxs == 1 ? 2 : 3; }
inline size_t lds_bytes(int w) { const int nt = threads_of(w), ms = w / nt; return (size_t)2 * (row_guard(ms) + nt * row_pitch(ms)) * 8; }

// The frames [f0, f1] at which the slab of `w` states from s0 on is live (f1 < f0: never).  s0 is even.
__device__ __forceinline__ void live_frames(int s0, int w, int T, int L, int& f0, int& f1) {
    const int s1 = s0 + w - 1;
    f0 = s0 >> 1;                                                   // s0 <= 2 i + 1
    f1 = s1 >= L - 1 ? T - 1 : T - ((L - s1 + 1) >> 1);             // s1 >= L - 2 (T - i)
}

// info[b] = (T, S, status, 0); status 0: healthy with T >= 1; 1: poisoned; 2: no frames.  Samples of status 1 and 2 are finished here.
__global__ __launch_bounds__(256) void lalign_sample_kernel(const int* __restrict__ targets, const int* __restrict__ in_len,
                                                            const int* __restrict__ tg_len, int4* __restrict__ info, int* __restrict__ endst,
                                                            double* __restrict__ score, int N, int C, int Smax) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int T = len_of(in_len, b, N), S = len_of(tg_len, b, Smax);
    int bad = (T > N) | (S < 0) | (S > Smax);           // poisoned samples, as ctc_alphabeta_kernel defines them
    if (!bad) for (int i = tid; i < S; i += 256) { const int lab = targets[(long)b * Smax + i]; bad |= (lab < 0) | (lab >= C); }
    bad = __syncthreads_or(bad);
    if (tid == 0) {
        info[b] = make_int4(T, S, bad ? 1 : (T <= 0 ? 2 : 0), 0);
        if (bad) { score[b] = (double)NAN; endst[b] = -1; }
        else if (T <= 0) { score[b] = -(double)INFINITY; endst[b] = -1; }
    }
}

// One workgroup per sample, the slab of blockDim.x * MAXS states from s0 on.  ein: the edge column the slab below wrote (nullptr for
// slab 0), eout: the one this slab writes; both (B, N, 2) f64, [.][i] = v[i][top - 1], v[i][top] of the writing slab.
template <int MAXS>
__global__ __launch_bounds__(1024) void lalign_slab_kernel(const float* __restrict__ em, const int* __restrict__ targets,
                                                           const int4* __restrict__ info, const double* __restrict__ ein,
                                                           double* __restrict__ eout, unsigned char* __restrict__ bp, int* __restrict__ endst,
                                                           double* __restrict__ score, int N, int Smax, int LP, int BPW, int s0) {
    extern __shared__ double lat[];                     // [2][W]
    const int b = blockIdx.x, nt = blockDim.x, tid = threadIdx.x;
    // A thread's MAXS cells are adjacent in LDS and the next thread's follow after ONE cell of padding (none for MAXS = 1): at a
    // pitch of 2, 4 or 8 cells the lanes of a wave would start 16, 32 or 64 bytes apart and 2, 4 or 16 of every 32 would meet in
    // the same banks; at 3, 5 or 9 cells (6, 10, 18 banks) the 32 lanes of a pass start in 32 different bank pairs.  GUARD cells in
    // front of each row stay -inf: the two cells below the first thread's.
    constexpr int PITCH = row_pitch(MAXS), GUARD = row_guard(MAXS);
    const int w = nt * MAXS, W = GUARD + nt * PITCH;
    const int base = GUARD + tid * PITCH;                // this thread's first cell in a row; the two below it: base - GUARD, + 1
    const int4 inf = info[b];
    const int T = inf.x, S = inf.y, L = 2 * S + 1;
    if (inf.z != 0 || s0 >= L) return;                  // finished by the sample kernel, or a slab past this sample's lattice
    const double NEG = -(double)INFINITY;
    int f0, f1, g0 = 0, g1 = -1;                        // live frames of this slab and of the one below
    live_frames(s0, w, T, L, f0, f1);
    if (s0 > 0) live_frames(s0 - w, w, T, L, g0, g1);
    const bool last = s0 + w >= L;                      // the sample's last slab: takes the end state, has nobody to write an edge for
    const double* ecol = s0 > 0 ? ein + (long)b * N * 2 : nullptr;

    const int sp0 = tid * MAXS, sg0 = s0 + sp0, cnt = min(max(L - sg0, 0), MAXS);
    unsigned skip_ok = 0;                               // bit k: state sg0 + k may be entered from two states below
#pragma unroll
    for (int k = 0; k < MAXS; ++k) {
        const int sg = sg0 + k;                         // (the slab's first label state s0 + 1 compares across the seam: targets is global)
        if (sg < L && sg >= 3 && (sg & 1) && targets[(long)b * Smax + (sg >> 1)] != targets[(long)b * Smax + (sg >> 1) - 1]) skip_ok |= 1u << k;
    }
    for (int i = tid; i < 2 * W; i += nt) lat[i] = NEG;
    __syncthreads();
    if (s0 == 0 && tid == 0) lat[W + GUARD] = 0.0;      // virtual frame -1 (row 1): state 0 at 0, so frame 0 is the general step
    __syncthreads();

    constexpr int NL = MAXS == 1 ? 1 : MAXS / 2, NE = MAXS == 1 ? 1 : NL + 1;
    constexpr int G = MAXS <= 4 ? 4 : 2;                // frames prefetched together
    const int j0 = MAXS == 1 ? ((sg0 & 1) ? min(sg0 >> 1, LP - 1) : LP) : min(sg0 >> 1, LP - NL);
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
    // The cells below the slab at the frame BEFORE each frame of a group, for the threads that own local states 0 and 1.
    const bool reads_edge = s0 > 0 && sp0 < 2;
    double ef[G][2], en[G][2];
    auto load_edge = [&](double (&dst)[G][2], int i0) {
#pragma unroll
        for (int j = 0; j < G; ++j) {
            dst[j][0] = NEG; dst[j][1] = NEG;
            const int fi = i0 + j - 1;
            if (reads_edge && fi >= g0 && fi <= g1) {    // (g1 <= T - 1 < N: inside the column)
                const double2 x = *reinterpret_cast<const double2*>(ecol + (long)fi * 2);
                dst[j][0] = x.x; dst[j][1] = x.y;
            }
        }
    };
    load_group(pf, f0);
    load_edge(ef, f0);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int w0 = s0 + wave * 64 * MAXS, w1 = w0 + 64 * MAXS - 1;     // the wave's range of states
    const bool writes_edge = !last && sp0 + MAXS > w - 2;              // (all of this thread's cells are below L then)
    unsigned char* brow = bp + (long)b * N * BPW + sg0;
    double* ocol = eout + (long)b * N * 2;
    for (int i0 = f0; i0 <= f1; i0 += G) {
        load_group(nx, i0 + G);
        load_edge(en, i0 + G);
#pragma unroll
        for (int j = 0; j < G; ++j) {
            const int i = i0 + j;
            if (i <= f1) {                                // uniform across the workgroup
                double* cur = lat + (i & 1) * W + base;
                const double* prev = lat + ((i & 1) ^ 1) * W + base;
                const int hi = 2 * i + 1, lo = L - 2 * (T - i);       // live band of states at this frame
                double val[MAXS];
#pragma unroll
                for (int k = 0; k < MAXS; ++k) val[k] = NEG;
                if (w0 <= hi && w1 >= lo) {                           // wave-uniform
                    if (cnt > 0) {
                        double pv[MAXS + 2];
#pragma unroll
                        for (int q = 0; q < MAXS; ++q) pv[q + 2] = prev[q];
                        pv[0] = prev[-GUARD]; pv[1] = prev[1 - GUARD];
                        if (reads_edge) {
                            if (sp0 == 0) { pv[0] = ef[j][0]; pv[1] = ef[j][1]; }
                            else pv[0] = ef[j][1];                    // (MAXS == 1: local state 1)
                        }
                        unsigned pk[(MAXS + 3) / 4] = {};
#pragma unroll
                        for (int k = 0; k < MAXS; ++k) {
                            const float e = MAXS == 1 ? pf[j][0] : ((k & 1) ? pf[j][k >> 1] : pf[j][NL]);
                            double best = pv[k + 2];
                            unsigned step = 0;
                            if (pv[k + 1] > best) { best = pv[k + 1]; step = 1; }
                            if (((skip_ok >> k) & 1) && pv[k] > best) { best = pv[k]; step = 2; }
                            val[k] = best + (double)e;
                            cur[k] = val[k];                          // (cells past L stay inside the slab's row)
                            pk[k / 4] |= step << (8 * (k & 3));
                        }
                        unsigned char* o = brow + (long)i * BPW;
                        if constexpr (MAXS == 1) *o = (unsigned char)pk[0];
                        else if constexpr (MAXS == 2) *reinterpret_cast<unsigned short*>(o) = (unsigned short)pk[0];
                        else if constexpr (MAXS == 4) *reinterpret_cast<unsigned*>(o) = pk[0];
                        else *reinterpret_cast<uint2*>(o) = make_uint2(pk[0], pk[1]);
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < MAXS; ++k) if (k < cnt) cur[k] = NEG;
                }
                if (writes_edge) {                        // every live frame of the slab, -inf where the top wave is outside the band
                    double* o = ocol + (long)i * 2;
                    if constexpr (MAXS == 1) o[sp0 - (w - 2)] = val[0];
                    else *reinterpret_cast<double2*>(o) = make_double2(val[MAXS - 2], val[MAXS - 1]);
                }
                wait_lgkm0_barrier();                     // not __syncthreads(): nothing waits for the frame's global stores
            }
        }
#pragma unroll
        for (int j = 0; j < G; ++j) {
#pragma unroll
            for (int k = 0; k < NE; ++k) pf[j][k] = nx[j][k];
            ef[j][0] = en[j][0]; ef[j][1] = en[j][1];
        }
    }
    if (last && tid == 0) {
        // f1 = T - 1 here.  A last slab that never became live (f0 > f1) still ends the sample: its rows are -inf, and when it holds
        // the one state L - 1, L - 2 is the top cell of the slab below, at frame T - 1 in the edge column.
        const double* row = lat + ((T - 1) & 1) * W + GUARD;
        auto cell = [&](int c) { return row[c / MAXS * PITCH + c % MAXS]; };       // local state c of the slab
        const bool ran = f0 <= f1;
        int end = L - 1;
        double v = ran ? cell(L - 1 - s0) : NEG;
        if (L > 1) {
            double u;
            if (L - 2 >= s0) u = ran ? cell(L - 2 - s0) : NEG;
            else u = (T - 1 >= g0 && T - 1 <= g1) ? ecol[(long)(T - 1) * 2 + 1] : NEG;
            if (u > v) { v = u; end = L - 2; }
        }
        score[b] = v;
        endst[b] = v > NEG ? end : -1;                    // -inf: no path fits; NaN: non-finite log-probs, reported as no path
    }
}

struct Parts { int64_t endst, info, edge, em, bp; };
inline Parts parts(int64_t B, int64_t N, int64_t Smax) {
    return {round256(4 * B), round256(16 * B), round256(2 * 16 * B * N), round256(4 * B * N * (label_pitch(Smax) + 4)), round256(B * N * bp_pitch(Smax))};
}

// The workspace of one call, as parts() lays it out.
struct Sections { int* endst; int4* info; double* edge[2]; float* em; unsigned char* bp; };
inline Sections sections(void* workspace, int64_t B, int64_t N, int64_t Smax) {
    const Parts p = parts(B, N, Smax);
    char* ws = (char*)workspace;
    Sections s;
    s.endst = (int*)ws;
    s.info = (int4*)(ws + p.endst);
    s.edge[0] = (double*)(ws + p.endst + p.info);
    s.edge[1] = s.edge[0] + B * N * 2;
    s.em = (float*)(ws + p.endst + p.info + p.edge);
    s.bp = (unsigned char*)s.em + p.em;
    return s;
}

inline void launch_lalign_sample(const int* targets, const int* input_lengths, const int* target_lengths, const Sections& s, double* score,
                                 int64_t B, int64_t N, int64_t C, int64_t Smax, hipStream_t stream) {
    hipLaunchKernelGGL(lalign_sample_kernel, dim3((unsigned)B), dim3(256), 0, stream, targets, input_lengths, target_lengths, s.info, s.endst, score,
                       (int)N, (int)C, (int)Smax);
}

// The slab launches of one call, one after the other on the stream.
inline void launch_lalign_slabs(const int* targets, const Sections& s, double* score, int64_t B, int64_t N, int64_t Smax, int LP, int BPW,
                                int slab_states, hipStream_t stream) {
    const int w = slab_of(slab_states), nt = threads_of(w), slabs = cdiv(2 * Smax + 1, w);
    const size_t lds = lds_bytes(w);
#define SLABS(MS) do { \
        static bool raised = false; \
        if (lds > 48 * 1024) lds_limit_once(raised, {(const void*)lalign_slab_kernel<MS>}, lds); \
        for (int k = 0; k < slabs; ++k) \
            hipLaunchKernelGGL((lalign_slab_kernel<MS>), dim3((unsigned)B), dim3(nt), lds, stream, s.em, targets, s.info, \
                               k ? s.edge[(k - 1) & 1] : (const double*)nullptr, s.edge[k & 1], s.bp, s.endst, score, (int)N, (int)Smax, LP, BPW, k * w); \
    } while (0)
    switch (w / nt) { case 1: SLABS(1); break; case 2: SLABS(2); break; case 4: SLABS(4); break; default: SLABS(8); }
#undef SLABS
}

}  // namespace
