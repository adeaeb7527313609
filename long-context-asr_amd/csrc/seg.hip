// CTC segmentation (include/sconf_seg.h): forced alignment in which star labels absorb any audio, and one confidence per utterance.
//
// sconf_seg_align is the alignment of align.hip (up to 8191 labels) or align_long.hip (above, the default slab) with ONE difference:
// the label value C is the star, whose emission is `star_logp` at every frame.  It enters where the emissions are gathered
// (align_gather_kernel<true> writes star_logp into the star's cell of the compact row) and where tokens are summed
// (align_tokens_kernel<true>); the lattice and walk kernels of align_lattice.h / align_slabs.h see emissions and label ids only, with
// C + 1 as the number of label values they accept.  No pass over the log-probs and no (B, N, C + 1) copy is added.  One kernel more,
// seg_frame_logp_kernel, reads the emission of the path's state per frame back from the compact rows.
//
// sconf_seg_score: one workgroup of TILE threads per utterance.  A round takes TILE frames: an f64 inclusive scan (wave shuffles,
// then the wave totals through LDS) on top of the carried sum gives the running sums P[e] = sum of g over [f0, f0 + e), which go to
// a ring of RING cells in LDS; the thread of frame e - 1 then takes P[e] - P[e - w], the sum of the window that ends there, into its
// running minimum.  A window reaches back over at most MAX_WINDOW cells and a round overwrites the cells RING behind the ones it
// writes: RING >= MAX_WINDOW + TILE keeps the two apart, so one barrier between a round's writes and its reads is the only one the
// ring needs.  Built without fast-math (csrc/Makefile): the sums keep their written order and the finiteness test stays a test.
#include "align_lattice.h"
#include "align_slabs.h"
#include "../../include/sconf_seg.h"
#include <cfloat>

namespace {

constexpr int TILE = 256;                       // threads of a score workgroup = frames per round
constexpr int MAX_WINDOW = 1024;
constexpr int RING = 2048;                      // a power of two >= MAX_WINDOW + TILE
static_assert(RING >= MAX_WINDOW + TILE && (RING & (RING - 1)) == 0, "ring too small");

inline bool sizes_ok(int64_t B, int64_t N, int64_t Smax) {
    return B >= 1 && B <= 65535 && N >= 1 && B * N <= 0x7fffffff && Smax >= 0 && Smax <= LALIGN_MAX_LABELS;
}

// One thread per frame: the emission of the state the path occupies, from the compact row the lattice read.
__global__ __launch_bounds__(256) void seg_frame_logp_kernel(const float* __restrict__ em, const int* __restrict__ endst,
                                                             const int* __restrict__ in_len, const int* __restrict__ path,
                                                             float* __restrict__ frame_logp, int N, int LP) {
    const int b = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
    if (t >= N) return;
    const long o = (long)b * N + t;
    float v = 0.f;
    if (endst[b] >= 0 && t < len_of(in_len, b, N)) {        // (T is in 1..N: the lattice has checked it)
        const int s = path[o];                              // 0 <= s <= 2 S: the walk never leaves the lattice
        v = em[o * (LP + 4) + ((s & 1) ? (s >> 1) : LP)];
    }
    frame_logp[o] = v;
}

__global__ __launch_bounds__(TILE) void seg_score_kernel(const int* __restrict__ spans, const float* __restrict__ g,
                                                         const double* __restrict__ score, const int* __restrict__ in_len,
                                                         const int* __restrict__ tg_len, const int* __restrict__ utt,
                                                         const int* __restrict__ utt_counts, int* __restrict__ utt_frames,
                                                         float* __restrict__ utt_logp, float* __restrict__ utt_conf, int N, int Smax, int Umax,
                                                         int window) {
    __shared__ double ring[RING];
    __shared__ double wsum[TILE / 64], wmin[TILE / 64];
    const int b = blockIdx.y, u = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long o = (long)b * Umax + u;
    const int count = utt_counts ? min(max(utt_counts[b], 0), Umax) : Umax;
    int f0 = -1, f1 = -1;                                   // (every thread decides alike: the same addresses, the same values)
    bool ok = false;
    if (u < count) {
        const int S = len_of(tg_len, b, Smax), T = len_of(in_len, b, N);
        const double sc = score[b];
        if (S >= 0 && S <= Smax && T >= 1 && T <= N && fabs(sc) < (double)INFINITY) {       // (NaN fails the comparison)
            const int j0 = utt[2 * o], j1 = utt[2 * o + 1];
            if (j0 >= 0 && j0 < j1 && j1 <= S) {
                f0 = spans[((long)b * Smax + j0) * 2];
                f1 = spans[((long)b * Smax + j1 - 1) * 2 + 1];
                ok = f0 >= 0 && f0 < f1 && f1 <= T;
            }
        }
    }
    if (!ok) {
        if (tid == 0) {
            const float v = u < count ? NAN : 0.f;
            utt_frames[2 * o] = -1; utt_frames[2 * o + 1] = -1;
            utt_logp[o] = v; utt_conf[o] = v;
        }
        return;
    }
    const int n = f1 - f0, w = min(window, n);
    const float* row = g + (long)b * N + f0;
    double carry = 0.0, mn = (double)INFINITY;
    if (tid == 0) ring[0] = 0.0;
    for (int r0 = 0; r0 < n; r0 += TILE) {
        const int idx = r0 + tid;
        double x = idx < n ? (double)row[idx] : 0.0;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const double y = __shfl_up(x, d); if (lane >= d) x += y; }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        double below = carry, total = carry;
#pragma unroll
        for (int k = 0; k < TILE / 64; ++k) { if (k < wave) below += wsum[k]; total += wsum[k]; }
        const double P = below + x;                         // the sum of g over [f0, f0 + idx + 1)
        if (idx < n) ring[(idx + 1) & (RING - 1)] = P;
        __syncthreads();                                    // (also: wsum is read by everyone before the next round writes it)
        if (idx < n && idx + 1 >= w) mn = fmin(mn, P - ring[(idx + 1 - w) & (RING - 1)]);
        carry = total;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mn = fmin(mn, __shfl_xor(mn, d));
    if (lane == 0) wmin[wave] = mn;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int k = 1; k < TILE / 64; ++k) mn = fmin(mn, wmin[k]);
        utt_frames[2 * o] = f0; utt_frames[2 * o + 1] = f1;
        utt_logp[o] = (float)(carry / (double)n);
        utt_conf[o] = (float)(mn / (double)w);
    }
}

}  // namespace

SCONF_API int sconf_seg_star_label(int64_t C) { return C < 1 || C > 0x7ffffffe ? -1 : (int)C; }
SCONF_API int sconf_seg_max_window(void) { return MAX_WINDOW; }
SCONF_API int sconf_seg_score_tile(void) { return TILE; }

SCONF_API int64_t sconf_seg_workspace(int64_t B, int64_t N, int64_t Smax, int64_t Umax) {
    if (B < 1 || N < 1 || B * N > 0x7fffffff || Smax < 0 || Smax > LALIGN_MAX_LABELS || Umax < 0) return -1;
    if (Smax <= ALIGN_MAX_LABELS) return round256(4 * B) + round256(4 * B * N * (label_pitch(Smax) + 4)) + round256(B * N * bp_pitch(Smax));
    const Parts p = parts(B, N, Smax);
    return p.endst + p.info + p.edge + p.em + p.bp;
}

SCONF_API int sconf_seg_align(const float* log_probs, const int32_t* targets, const int32_t* input_lengths, const int32_t* target_lengths,
                              int32_t* path, int32_t* labels, int32_t* spans, float* token_logp, double* score, float* frame_logp,
                              void* workspace, int64_t workspace_bytes, int64_t B, int64_t N, int64_t C, int64_t Smax, int blank,
                              float star_logp, sconf_stream_t stream) {
    if (B == 0) return 0;
    SCONF_REQUIRE(Smax >= 0 && Smax <= LALIGN_MAX_LABELS, "sconf_seg_align: %ld labels: at most %d (131071 lattice states)", (long)Smax, LALIGN_MAX_LABELS);
    SCONF_REQUIRE(sizes_ok(B, N, Smax), "sconf_seg_align: bad sizes B = %ld, N = %ld", (long)B, (long)N);
    SCONF_REQUIRE(C >= 4 && C % 4 == 0 && C * 4 <= 64 * 1024, "sconf_seg_align: C must be a multiple of 4 and one row must fit LDS (%ld classes)", (long)C);
    SCONF_REQUIRE(blank >= 0 && blank < C, "sconf_seg_align: blank %d out of range", blank);
    SCONF_REQUIRE(star_logp <= 0.f && star_logp >= -FLT_MAX, "sconf_seg_align: star_logp %g: it must be finite and <= 0", (double)star_logp);
    SCONF_REQUIRE(log_probs && path && labels && score && frame_logp && workspace && (Smax == 0 || (targets && spans && token_logp)),
                  "sconf_seg_align: null pointer");
    const int64_t need = sconf_seg_workspace(B, N, Smax, 0);
    SCONF_REQUIRE(workspace_bytes >= need, "sconf_seg_align: workspace of %ld bytes, %ld needed", (long)workspace_bytes, (long)need);
    const int LP = label_pitch(Smax), BPW = bp_pitch(Smax);
    const int64_t labels_ok = C + 1;                        // the lattice kernels accept the label values [0, C]
    int* endst;
    float* em;
    unsigned char* bp;
    if (Smax <= ALIGN_MAX_LABELS) {
        endst = (int*)workspace;
        em = (float*)((char*)workspace + round256(4 * B));
        bp = (unsigned char*)em + round256(4 * B * N * (LP + 4));
        launch_align_gather<true>(log_probs, targets, input_lengths, target_lengths, em, B, N, C, Smax, LP, blank, star_logp, stream);
        launch_align_lattice(em, targets, input_lengths, target_lengths, bp, endst, score, B, N, labels_ok, Smax, LP, BPW, stream);
    } else {
        const Sections s = sections(workspace, B, N, Smax);
        endst = s.endst; em = s.em; bp = s.bp;
        launch_lalign_sample(targets, input_lengths, target_lengths, s, score, B, N, labels_ok, Smax, stream);
        launch_align_gather<true>(log_probs, targets, input_lengths, target_lengths, em, B, N, C, Smax, LP, blank, star_logp, stream);
        launch_lalign_slabs(targets, s, score, B, N, Smax, LP, BPW, 0, stream);
    }
    launch_align_outputs<true>(log_probs, targets, input_lengths, target_lengths, bp, endst, path, labels, spans, token_logp, B, N, C, Smax, BPW,
                               blank, star_logp, stream);
    hipLaunchKernelGGL(seg_frame_logp_kernel, dim3((unsigned)cdiv(N, 256), (unsigned)B), dim3(256), 0, stream, em, endst, input_lengths, path,
                       frame_logp, (int)N, LP);
    SCONF_LAUNCH_OK("sconf_seg_align");
    return 0;
}

SCONF_API int sconf_seg_score(const int32_t* spans, const float* frame_logp, const double* score, const int32_t* input_lengths,
                              const int32_t* target_lengths, const int32_t* utt, const int32_t* utt_counts, int window, int32_t* utt_frames,
                              float* utt_logp, float* utt_conf, int64_t B, int64_t N, int64_t Smax, int64_t Umax, sconf_stream_t stream) {
    if (B == 0 || Umax == 0) return 0;
    SCONF_REQUIRE(sizes_ok(B, N, Smax) && Umax >= 1 && B * Umax <= 0x3fffffff, "sconf_seg_score: bad sizes B = %ld, N = %ld, Smax = %ld, Umax = %ld",
                  (long)B, (long)N, (long)Smax, (long)Umax);
    SCONF_REQUIRE(window >= 1 && window <= MAX_WINDOW, "sconf_seg_score: window %d: 1 .. %d", window, MAX_WINDOW);
    SCONF_REQUIRE(frame_logp && score && utt && utt_frames && utt_logp && utt_conf && (Smax == 0 || spans), "sconf_seg_score: null pointer");
    hipLaunchKernelGGL(seg_score_kernel, dim3((unsigned)Umax, (unsigned)B), dim3(TILE), 0, stream, spans, frame_logp, score, input_lengths,
                       target_lengths, utt, utt_counts, utt_frames, utt_logp, utt_conf, (int)N, (int)Smax, (int)Umax, window);
    SCONF_LAUNCH_OK("sconf_seg_score");
    return 0;
}
