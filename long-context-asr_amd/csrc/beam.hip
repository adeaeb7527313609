// CTC prefix beam search without a language model (include/sconf_beam.h): the n best transcripts of (B, N, C) log-probs, with the
// frame at which each token was created.  Serial in time like the loss and the alignment, parallel over beams x kept tokens.
//
// Structure:
//   1. compact   (beam_compact_kernel in beam_common.h, shared with beam_lm.hip)  one workgroup per (sample, frame): the row goes
//                to LDS with 16-byte loads (align_gather_kernel's scheme) and leaves as
//                a record [blank's log-prob | slot count | (class, log-prob) x Kmax] of the kept tokens in ascending class order.  The
//                only pass over the (N, C) tensor.  A row with at most Kmax qualifying classes (nearly all rows) is one load pass
//                (count, argmax) and one ordered pass over LDS; a row over the cap first finds the Kmax-th largest qualifying entry
//                by Kmax block-wide arg-max rounds and keeps what is not behind it.
//   2. search    one workgroup per sample.  Beam state (pb, pnb, prefix hash, parent's hash, length, last token, trie node), the
//                frame's candidates and the records of two chunks of G frames live in LDS; the next chunk is fetched into registers
//                before the current one is searched.  A frame with a kept token: stay candidates, extensions, the fold lookup
//                (prefix_i + c = prefix_j  <=>  len_j = len_i + 1, parent_hash_j = hash_i, last_j = c: n x n compares, no
//                trie walk and no dependence on WHICH node holds a prefix), the selection by (total descending, candidate index
//                ascending), and the re-ranking.  A frame of at most RANK_MAX candidates is selected by counting: each candidate
//                counts those in front of it (every lane reads the same LDS address: a broadcast) and the first W ranks are
//                written in order - one barrier instead of the ~log^2 of a sort; a larger frame is sorted, a bitonic sort of the next
//                power of two of its n (k + 1) candidates.  The compact position n + i k_f + k of an extension is monotone in its
//                candidate index W + i Kmax + k, so the position is the tie-break.
//                A frame with no kept token moves every total by lp[blank] and sets pnb = -inf: each thread updates its own beam and
//                no barrier, lookup or sort is paid.
//   3. backtrace one wave per (sample, rank): the -1 fill in parallel, lane 0 walks the trie from the leaf.
//
// All score arithmetic is f64; this file is compiled without -ffast-math (see the Makefile).
#include "beam_common.h"
#include "../../include/sconf_beam.h"

namespace {

// One workgroup per sample.  Pmax = the largest sort (pow2ceil(W (Kmax + 1))).  LDS as carved below.
__global__ __launch_bounds__(1024) void beam_search_kernel(const int* __restrict__ rec, const int* __restrict__ in_len,
                                                           int4* __restrict__ trie, Fin* __restrict__ fin, int* __restrict__ nlive,
                                                           int N, int W, int Kmax, double prune, int Pmax) {
    extern __shared__ double sm[];
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int T = len_of(in_len, b, N);
    if (T > N || T < 0) { if (tid == 0) nlive[b] = -1; return; }          // poisoned: nothing is indexed with T
    const int RS = 2 + 2 * Kmax, CH = G * RS;
    double* pb = sm;                                    // [2][W]
    double* pnb = pb + 2 * W;                           // [2][W]
    double* spb = pnb + 2 * W;                          // [W]  stay candidates
    double* spnb = spb + W;                             // [W]
    double* tot = spnb + W;                             // [W]  lse(pb, pnb) of the current beams
    double* skey = tot + W;                             // [W]  the first W totals in order, ranked path
    double* key = skey + W;                             // [Pmax]
    unsigned long long* hash = reinterpret_cast<unsigned long long*>(key + Pmax);   // [2][W]
    unsigned long long* phash = hash + 2 * W;           // [2][W]  hash of the prefix without its last token
    int* len = reinterpret_cast<int*>(phash + 2 * W);   // [2][W]
    int* last = len + 2 * W;                            // [2][W]
    int* node = last + 2 * W;                           // [2][W]
    int* fsrc = node + 2 * W;                           // [W]  the beam whose extension folds into this one, or -1
    int* sidx = fsrc + W;                               // [W]
    int* idx = sidx + W;                                // [Pmax]
    int* rbuf = idx + Pmax;                             // [2][CH]
    int* misc = rbuf + 2 * CH;                          // [4]
    const double NEG = -(double)INFINITY;

    if (tid == 0) { pb[0] = 0.0; pnb[0] = NEG; hash[0] = H0; phash[0] = 0; len[0] = 0; last[0] = -1; node[0] = -1; }
    const int* rb = rec + (long)b * N * RS;
    const long TR = (long)T * RS;
    for (int e = tid; e < CH; e += nt) rbuf[e] = e < TR ? rb[e] : 0;
    __syncthreads();
    int cur = 0, n = 1;
    int4* tb = trie + (long)b * N * W;
    for (int ch = 0; ch * G < T; ++ch) {
        int pf[NPF];                                    // the next chunk, in flight while this one is searched
#pragma unroll
        for (int q = 0; q < NPF; ++q) {
            const int e = tid + q * nt;
            const long ge = (long)(ch + 1) * CH + e;
            pf[q] = (e < CH && ge < TR) ? rb[ge] : 0;
        }
        const int* R = rbuf + (ch & 1) * CH;
        for (int j = 0; j < G; ++j) {
            const int t = ch * G + j;
            if (t >= T || n == 0) break;                // (uniform)
            const int* fr = R + j * RS;
            const float lpb = __int_as_float(fr[0]);
            const int Kf = min(max(fr[1], 0), Kmax);
            if (Kf == 0 && lpb > -INFINITY && lpb < INFINITY) {           // no kept token: the order cannot change
                if (tid < n) {
                    const int o = cur * W + tid;
                    const double a = pb[o], c = pnb[o];
                    pb[o] = (c == NEG ? a : lse2(a, c)) + (double)lpb;     // (lse(a, -inf) = a exactly: inside a run no exp / log1p)
                    pnb[o] = NEG;
                }
                continue;
            }
            const int M = n * (1 + Kf);
            const bool ranked = M <= RANK_MAX;          // (uniform)
            int P = 2;
            while (P < M) P <<= 1;
            const int co = cur * W;
            if (tid < n) {                              // stay candidates
                const double a = pb[co + tid], c = pnb[co + tid];
                const double tt = lse2(a, c);
                tot[tid] = tt;
                spb[tid] = tt + (double)lpb;
                const int l = last[co + tid];
                double s = NEG;
                for (int k = 0; k < Kf; ++k) if (fr[2 + 2 * k] == l) s = c + (double)__int_as_float(fr[3 + 2 * k]);
                spnb[tid] = s;
                fsrc[tid] = -1;
            }
            __syncthreads();
            for (int e = tid; e < n * Kf; e += nt) {    // extensions, at compact position n + i Kf + k
                const int i = e / Kf, k = e - i * Kf;
                const int c = fr[2 + 2 * k];
                key[n + e] = (double)__int_as_float(fr[3 + 2 * k]) + (c == last[co + i] ? pb[co + i] : tot[i]);
            }
            for (int p = tid; p < n * n; p += nt) {     // fold lookup: is beam i the parent prefix of beam j
                const int jj = p / n, i = p - jj * n;
                if (len[co + jj] == len[co + i] + 1 && phash[co + jj] == hash[co + i]) fsrc[jj] = i;
            }
            __syncthreads();
            if (tid < n && fsrc[tid] >= 0) {            // beam i extended by last_j IS beam j: into its stay candidate
                const int i = fsrc[tid], l = last[co + tid];
                for (int k = 0; k < Kf; ++k)
                    if (fr[2 + 2 * k] == l) {
                        const int at = n + i * Kf + k;
                        spnb[tid] = lse2(spnb[tid], key[at]);
                        key[at] = NEG;
                    }
            }
            __syncthreads();
            for (int p = tid; p < (ranked ? M : P); p += nt) {
                double x = p < n ? lse2(spb[p], spnb[p]) : (p < M ? key[p] : NEG);
                if (!(x > NEG)) x = NEG;                // (NaN is dropped with -inf)
                key[p] = x;
                idx[p] = p;
            }
            if (tid == 0) misc[0] = 0;
            if (ranked && tid < W) skey[tid] = NEG;     // ranks behind the candidates: dropped
            __syncthreads();
            if (ranked) {                               // rank = the number of candidates in front; only the first W ranks matter
                for (int p = tid; p < M; p += nt) {
                    const double x = key[p];
                    int r = 0;
#pragma unroll 8
                    for (int q = 0; q < M; ++q) { const double y = key[q]; r += (y > x) | ((y == x) & (q < p)); }
                    if (r < W) { skey[r] = x; sidx[r] = p; }
                }
                __syncthreads();
            }
            for (int k = 2; !ranked && k <= P; k <<= 1)
                for (int s = k >> 1; s > 0; s >>= 1) {
                    for (int p = tid; p < (P >> 1); p += nt) {
                        const int lo = 2 * p - (p & (s - 1)), hi = lo + s;
                        const double ka = key[lo], kb = key[hi];
                        const int ia = idx[lo], ib = idx[hi];
                        const bool a_first = ka > kb || (ka == kb && ia < ib);
                        if (((lo & k) == 0) != a_first) { key[lo] = kb; key[hi] = ka; idx[lo] = ib; idx[hi] = ia; }
                    }
                    __syncthreads();
                }
            const int no = (cur ^ 1) * W, top = ranked ? W : min(W, P);
            const double* ok = ranked ? skey : key;     // the candidates in order (the first W of them on the ranked path)
            const int* oi = ranked ? sidx : idx;
            if (tid < top) {                            // re-ranking: survivor `tid` of the ordered candidates becomes beam `tid`
                const double floor_ = ok[0] + prune, x = ok[tid];
                if (x > NEG && !(x < floor_)) {
                    const bool more = tid + 1 < top && ok[tid + 1] > NEG && !(ok[tid + 1] < floor_);
                    if (!more) misc[0] = tid + 1;
                    const int p = oi[tid];
                    if (p < n) {
                        pb[no + tid] = spb[p]; pnb[no + tid] = spnb[p]; hash[no + tid] = hash[co + p]; phash[no + tid] = phash[co + p];
                        len[no + tid] = len[co + p]; last[no + tid] = last[co + p]; node[no + tid] = node[co + p];
                    } else {
                        const int e = p - n, i = e / Kf, k = e - i * Kf;
                        const int c = fr[2 + 2 * k];
                        pb[no + tid] = NEG; pnb[no + tid] = x; phash[no + tid] = hash[co + i]; hash[no + tid] = extend_hash(hash[co + i], c);
                        len[no + tid] = len[co + i] + 1; last[no + tid] = c; node[no + tid] = t * W + tid;
                        tb[(long)t * W + tid] = make_int4(node[co + i], c, t, 0);
                    }
                }
            }
            __syncthreads();
            n = misc[0];
            cur ^= 1;
        }
        int* nb = rbuf + ((ch + 1) & 1) * CH;
#pragma unroll
        for (int q = 0; q < NPF; ++q) {
            const int e = tid + q * nt;
            if (e < CH) nb[e] = pf[q];
        }
        __syncthreads();
    }
    if (tid < n) {
        const int o = cur * W + tid;
        Fin f;
        f.node = node[o]; f.len = len[o]; f.score = lse2(pb[o], pnb[o]);
        fin[(long)b * W + tid] = f;
    }
    if (tid == 0) nlive[b] = n;
}

// One wave per (sample, rank): every element of the rank's outputs, and count[b] from rank 0.
__global__ __launch_bounds__(64) void beam_backtrace_kernel(const int4* __restrict__ trie, const Fin* __restrict__ fin,
                                                            const int* __restrict__ nlive, int* __restrict__ count, int* __restrict__ tokens,
                                                            int* __restrict__ lengths, int* __restrict__ frames, double* __restrict__ scores,
                                                            int N, int W, int nbest, long Lmax) {
    const int r = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const int nl = nlive[b], cnt = min(max(nl, 0), nbest);
    const long o = (long)b * nbest + r;
    int L = 0, leaf = -1;
    double sc = nl < 0 ? (double)NAN : -(double)INFINITY;
    if (r < cnt) { const Fin f = fin[(long)b * W + r]; L = max(f.len, 0); leaf = f.node; sc = f.score; }
    if (lane == 0) { if (r == 0) count[b] = cnt; lengths[o] = L; scores[o] = sc; }
    int* tk = tokens + o * Lmax;
    int* tf = frames + o * Lmax;
    for (long p = min((long)L, Lmax) + lane; p < Lmax; p += 64) { tk[p] = -1; tf[p] = -1; }
    if (lane == 0) {
        const int4* tb = trie + (long)b * N * W;
        const long nodes = (long)N * W;
        int nd = leaf;
        for (long pos = L - 1; pos >= 0; --pos) {
            int4 v = make_int4(-1, -1, -1, 0);
            if (nd >= 0 && nd < nodes) v = tb[nd];      // (always, for a trie the search wrote)
            if (pos < Lmax) { tk[pos] = v.y; tf[pos] = v.z; }
            nd = v.x;
        }
    }
}

inline size_t search_lds(int W, int Kmax, int Pmax) {
    return (size_t)8 * (8 * W + Pmax) + (size_t)8 * 4 * W + (size_t)4 * (8 * W + Pmax + 2 * G * (2 + 2 * Kmax) + 4);
}

}  // namespace

SCONF_API int sconf_beam_max_width(void) { return MAX_W; }
SCONF_API int sconf_beam_max_tokens(void) { return MAX_K; }
SCONF_API int sconf_beam_threads(int64_t W, int64_t Kmax) { return sizes_ok(W, Kmax) ? search_threads(W, Kmax) : -1; }
SCONF_API int sconf_beam_sort_size(int64_t candidates) {
    return candidates < 1 || candidates > (int64_t)MAX_W * (MAX_K + 1) ? -1 : (candidates <= RANK_MAX ? 0 : pow2ceil(candidates));
}
SCONF_API int sconf_beam_rank_limit(void) { return RANK_MAX; }
SCONF_API int sconf_beam_prefetch_frames(void) { return G; }

SCONF_API int64_t sconf_beam_workspace(int64_t B, int64_t N, int64_t W, int64_t Kmax) {
    if (B < 1 || N < 1 || !sizes_ok(W, Kmax) || B * N > 0x7fffffff || B * N * W > 0x7fffffff) return -1;
    return round256(B * N * (8 + 8 * Kmax)) + round256(16 * B * N * W) + round256(16 * B * W) + round256(4 * B);
}

SCONF_API int sconf_beam_ctc(const float* log_probs, const int32_t* input_lengths, int32_t* count, int32_t* tokens, int32_t* lengths,
                             int32_t* token_frames, double* scores, void* workspace, int64_t workspace_bytes, int64_t B, int64_t N, int64_t C,
                             int blank, int beam_width, int nbest, float token_min_logp, double beam_prune_logp, int max_tokens_per_frame,
                             int64_t Lmax, sconf_stream_t stream) {
    if (B == 0) return 0;
    const int W = beam_width, Kmax = max_tokens_per_frame;
    SCONF_REQUIRE(W >= 1 && W <= MAX_W, "sconf_beam_ctc: beam_width %d: from 1 to %d", W, MAX_W);
    SCONF_REQUIRE(Kmax >= 1 && Kmax <= MAX_K, "sconf_beam_ctc: max_tokens_per_frame %d: from 1 to %d", Kmax, MAX_K);
    SCONF_REQUIRE(nbest >= 1 && nbest <= W, "sconf_beam_ctc: nbest %d: from 1 to beam_width = %d", nbest, W);
    SCONF_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && B * N <= 0x7fffffff && B * N * W <= 0x7fffffff && Lmax >= 1 && nbest * Lmax <= 0x7fffffff,
                  "sconf_beam_ctc: bad sizes B = %ld, N = %ld, Lmax = %ld", (long)B, (long)N, (long)Lmax);
    SCONF_REQUIRE(C >= 4 && C % 4 == 0 && C * 4 <= 64 * 1024, "sconf_beam_ctc: C must be a multiple of 4 and one row must fit LDS (%ld classes)", (long)C);
    SCONF_REQUIRE(blank >= 0 && blank < C, "sconf_beam_ctc: blank %d out of range", blank);
    SCONF_REQUIRE(beam_prune_logp <= 0.0, "sconf_beam_ctc: beam_prune_logp must be <= 0 (-inf: no pruning)");
    SCONF_REQUIRE(log_probs && count && tokens && lengths && token_frames && scores && workspace, "sconf_beam_ctc: null pointer");
    SCONF_REQUIRE(workspace_bytes >= sconf_beam_workspace(B, N, W, Kmax), "sconf_beam_ctc: workspace of %ld bytes, %ld needed",
                  (long)workspace_bytes, (long)sconf_beam_workspace(B, N, W, Kmax));
    int* rec = (int*)workspace;
    int4* trie = (int4*)((char*)workspace + round256(B * N * (8 + 8 * Kmax)));
    Fin* fin = (Fin*)((char*)trie + round256(16 * B * N * W));
    int* nlive = (int*)((char*)fin + round256(16 * B * W));
    const size_t lds_c = (size_t)C * 4 + 4 * (12 + 8 * MAX_K);
    static bool big_c = false, big_s = false;
    if (lds_c > 48 * 1024) lds_limit_once(big_c, {(const void*)beam_compact_kernel}, 64 * 1024 + 4 * (12 + 8 * MAX_K));
    hipLaunchKernelGGL(beam_compact_kernel, dim3((unsigned)std::min<long>(B * N, 65536)), dim3(256), lds_c, stream, log_probs, input_lengths,
                       rec, (int)B, (int)N, (int)C, blank, token_min_logp, Kmax);
    const int Pmax = pow2ceil((long)W * (Kmax + 1));
    const size_t lds_s = search_lds(W, Kmax, Pmax);
    if (lds_s > 48 * 1024) lds_limit_once(big_s, {(const void*)beam_search_kernel}, search_lds(MAX_W, MAX_K, pow2ceil((long)MAX_W * (MAX_K + 1))));
    hipLaunchKernelGGL(beam_search_kernel, dim3((unsigned)B), dim3(search_threads(W, Kmax)), lds_s, stream, rec, input_lengths, trie, fin, nlive,
                       (int)N, W, Kmax, beam_prune_logp, Pmax);
    hipLaunchKernelGGL(beam_backtrace_kernel, dim3((unsigned)nbest, (unsigned)B), dim3(64), 0, stream, trie, fin, nlive, count, tokens, lengths,
                       token_frames, scores, (int)N, W, nbest, (long)Lmax);
    SCONF_LAUNCH_OK("sconf_beam_ctc");
    return 0;
}
