// CTC prefix beam search with a back-off n-gram language model fused in (include/sconf_lm.h): the search of csrc/beam.hip whose
// ranking key is the acoustic total plus a per-prefix bonus, bonus' = bonus + alpha ln P(token | LM state) + beta per created token.
//
// Structure: the three kernels of beam.hip.
//   1. compact   beam_compact_kernel of beam_common.h, unchanged: the LM does not decide which tokens are kept.
//   2. search    beam_search_kernel with, per beam, bonus[2][W] (f64) and lm_state[2][W], and, per candidate position, ebonus[Pmax]
//                and estate[Pmax].  The LM is an automaton in HBM (states with failure arcs, children sorted by token, a dense unigram
//                table; see the header).  The walk of extension (i, k) is taken by the thread that finalises that candidate's key,
//                AFTER the fold has been applied (a folded extension has key -inf and takes no walk), so it costs no barrier: it sits
//                in the pass that already rewrites every key before the selection.  Each level is one 16-byte state load, a binary
//                search over the state's sorted 16-byte entries, and the hit's log-prob and next state from the entry that
//                matched; the empty context is one 8-byte load, asked for before the levels above it.
//                New bonus and state are KEPT IN LDS beside key / idx (indexed by the candidate's compact position, which the
//                selection carries in idx: the sort does not move them) rather than looked up again for the survivors: the key of
//                every candidate needs its walk before the selection anyway, a second walk for the W survivors would add one more
//                dependent chain of HBM / L2 loads (microseconds) to every frame of a search that is serial in time, and the 48 KB
//                fit (see search_lds).  The survivor's ACOUSTIC total is recomputed from LDS with the expression that made it (the
//                key is acoustic + bonus, summed last; subtracting would not give the acoustic total back).
//                The frame without a kept token is the code of beam.hip: no barrier, no transcendental, no LM access.
//   3. backtrace beam.hip's, writing logit_scores as the sixth output.
//
// No synchronisation between workgroups, no atomics; the image is only read.  All score arithmetic is f64; compiled without
// -ffast-math (see the Makefile).
#include "beam_common.h"
#include "../../include/sconf_lm.h"

namespace {

constexpr int MAX_ORDER = 5;

struct FinLm { int node, len; double score, logit; };

// The image as the launcher carves it; the sizes clamp every index read from it.
struct LmImage {
    const int4* states;                                 // [n_states]  first_child, n_children, backoff f32, backoff_state
    const int4* entries;                                // [n_entries] token, logp f32, next_state, 0
    const int2* dense;                                  // [num_tokens] logp f32, next_state
    int n_states, n_entries, num_tokens, order;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// step(state, token) of the header: q, the f64 sum of the f32 values met, and the next state.
__device__ __forceinline__ double lm_step(const LmImage* Ld, int s, int c, int& next) {
    LmImage L;                                          // (field by field: scalars in registers, no private-memory copy of the struct)
    L.states = Ld->states; L.entries = Ld->entries; L.dense = Ld->dense;
    L.n_states = Ld->n_states; L.n_entries = Ld->n_entries; L.num_tokens = Ld->num_tokens; L.order = Ld->order;
    next = 0;
    if (c < 0 || c >= L.num_tokens) return 0.0;         // a class the model does not know
    double q = 0.0;
    s = clampi(s, 0, L.n_states - 1);
    const int2 d = L.dense[c];                          // the empty context's record, asked for first: it is in flight under the levels above
    for (int lvl = 1; lvl < L.order && s != 0; ++lvl) { // a context of an order-n model has at most n - 1 words: n - 1 levels
        const int4 st = L.states[s];
        int lo = clampi(st.x, 0, L.n_entries);
        int hi = lo + clampi(st.y, 0, L.n_entries - lo);
        for (int it = 0; it < 32 && lo < hi; ++it) {    // bisection over the sorted children (four probes a step measured no faster)
            const int mid = lo + ((hi - lo) >> 1);
            const int4 e = L.entries[mid];
            if (e.x == c) { next = clampi(e.z, 0, L.n_states - 1); return q + (double)__int_as_float(e.y); }
            if (e.x < c) lo = mid + 1; else hi = mid;
        }
        q += (double)__int_as_float(st.z);
        s = clampi(st.w, 0, L.n_states - 1);
    }                                                   // the empty context (also where a damaged image's chain is cut off)
    next = clampi(d.y, 0, L.n_states - 1);
    return q + (double)__int_as_float(d.x);
}

// One workgroup per sample.  beam_search_kernel of beam.hip plus the LM; Pmax = the largest sort.  LDS as carved below.
__global__ __launch_bounds__(1024) void beam_search_lm_kernel(const int* __restrict__ rec, const int* __restrict__ in_len,
                                                              int4* __restrict__ trie, FinLm* __restrict__ fin, int* __restrict__ nlive,
                                                              LmImage image, int start_state, double alpha_, double beta_,
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
    double* skey = tot + W;                             // [W]  the first W keys in order, ranked path
    double* bonus = skey + W;                           // [2][W]  the LM's share of the key
    double* key = bonus + 2 * W;                        // [Pmax]
    double* ebonus = key + Pmax;                        // [Pmax]  a candidate extension's new bonus, by compact position
    unsigned long long* hash = reinterpret_cast<unsigned long long*>(ebonus + Pmax);   // [2][W]
    unsigned long long* phash = hash + 2 * W;           // [2][W]  hash of the prefix without its last token
    int* len = reinterpret_cast<int*>(phash + 2 * W);   // [2][W]
    int* last = len + 2 * W;                            // [2][W]
    int* node = last + 2 * W;                           // [2][W]
    int* lmst = node + 2 * W;                           // [2][W]  LM state
    int* fsrc = lmst + 2 * W;                           // [W]  the beam whose extension folds into this one, or -1
    int* sidx = fsrc + W;                               // [W]
    int* idx = sidx + W;                                // [Pmax]
    int* estate = idx + Pmax;                           // [Pmax]  a candidate extension's new LM state, by compact position
    int* rbuf = estate + Pmax;                          // [2][CH]
    int* misc = rbuf + 2 * CH;                          // [4]
    // The image's descriptor and the two weights are read from LDS where a walk is taken, not held in scalar registers across the
    // frame loop: the frame without a kept token keeps the register budget it has in beam.hip.
    LmImage* Ls = reinterpret_cast<LmImage*>(misc + 4); // [1]  (8-byte aligned: every int array above has an even length)
    double* wts = reinterpret_cast<double*>(Ls + 1);    // [2]  alpha, beta
    const double NEG = -(double)INFINITY;

    if (tid == 0) {
        pb[0] = 0.0; pnb[0] = NEG; hash[0] = H0; phash[0] = 0; len[0] = 0; last[0] = -1; node[0] = -1;
        bonus[0] = 0.0; lmst[0] = clampi(start_state, 0, image.n_states - 1);
        Ls->states = image.states; Ls->entries = image.entries; Ls->dense = image.dense;
        Ls->n_states = image.n_states; Ls->n_entries = image.n_entries; Ls->num_tokens = image.num_tokens; Ls->order = image.order;
        wts[0] = alpha_; wts[1] = beta_;
    }
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
            if (Kf == 0 && lpb > -INFINITY && lpb < INFINITY) {           // no kept token: every key moves by lpb, the order cannot change
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
            for (int e = tid; e < n * Kf; e += nt) {    // extensions, at compact position n + i Kf + k: the acoustic total
                const int i = e / Kf, k = e - i * Kf;
                const int c = fr[2 + 2 * k];
                key[n + e] = (double)__int_as_float(fr[3 + 2 * k]) + (c == last[co + i] ? pb[co + i] : tot[i]);
            }
            for (int p = tid; p < n * n; p += nt) {     // fold lookup: is beam i the parent prefix of beam j
                const int jj = p / n, i = p - jj * n;
                if (len[co + jj] == len[co + i] + 1 && phash[co + jj] == hash[co + i]) fsrc[jj] = i;
            }
            __syncthreads();
            if (tid < n && fsrc[tid] >= 0) {            // beam i extended by last_j IS beam j: into its stay candidate (acoustic mass only)
                const int i = fsrc[tid], l = last[co + tid];
                for (int k = 0; k < Kf; ++k)
                    if (fr[2 + 2 * k] == l) {
                        const int at = n + i * Kf + k;
                        spnb[tid] = lse2(spnb[tid], key[at]);
                        key[at] = NEG;
                    }
            }
            __syncthreads();
            for (int p = tid; p < (ranked ? M : P); p += nt) {             // the keys: acoustic total + bonus, the sum done last
                double x = NEG;
                if (p < n) {
                    const double a = lse2(spb[p], spnb[p]);
                    if (a > NEG) x = a + bonus[co + p];
                } else if (p < M) {
                    const double a = key[p];
                    if (a > NEG) {                      // a live extension that was not folded: its step through the LM
                        const int e = p - n, i = e / Kf, k = e - i * Kf;
                        int ns;
                        const double q = lm_step(Ls, lmst[co + i], fr[2 + 2 * k], ns);
                        const double nb = bonus[co + i] + __dadd_rn(__dmul_rn(wts[0], q), wts[1]);       // (two roundings, never an fma: the contract's value)
                        ebonus[p] = nb;
                        estate[p] = ns;
                        x = a + nb;
                    }
                }
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
                        bonus[no + tid] = bonus[co + p]; lmst[no + tid] = lmst[co + p];
                    } else {
                        const int e = p - n, i = e / Kf, k = e - i * Kf;
                        const int c = fr[2 + 2 * k];
                        pb[no + tid] = NEG;             // the acoustic total, by the expression that made it
                        pnb[no + tid] = (double)__int_as_float(fr[3 + 2 * k]) + (c == last[co + i] ? pb[co + i] : tot[i]);
                        phash[no + tid] = hash[co + i]; hash[no + tid] = extend_hash(hash[co + i], c);
                        len[no + tid] = len[co + i] + 1; last[no + tid] = c; node[no + tid] = t * W + tid;
                        bonus[no + tid] = ebonus[p]; lmst[no + tid] = estate[p];
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
        FinLm f;
        f.node = node[o]; f.len = len[o]; f.logit = lse2(pb[o], pnb[o]); f.score = f.logit + bonus[o];
        fin[(long)b * W + tid] = f;
    }
    if (tid == 0) nlive[b] = n;
}

// One wave per (sample, rank): every element of the rank's outputs, and count[b] from rank 0.
__global__ __launch_bounds__(64) void beam_backtrace_lm_kernel(const int4* __restrict__ trie, const FinLm* __restrict__ fin,
                                                               const int* __restrict__ nlive, int* __restrict__ count,
                                                               int* __restrict__ tokens, int* __restrict__ lengths, int* __restrict__ frames,
                                                               double* __restrict__ scores, double* __restrict__ logits, int N, int W,
                                                               int nbest, long Lmax) {
    const int r = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const int nl = nlive[b], cnt = min(max(nl, 0), nbest);
    const long o = (long)b * nbest + r;
    int L = 0, leaf = -1;
    double sc = nl < 0 ? (double)NAN : -(double)INFINITY, lg = sc;
    if (r < cnt) { const FinLm f = fin[(long)b * W + r]; L = max(f.len, 0); leaf = f.node; sc = f.score; lg = f.logit; }
    if (lane == 0) { if (r == 0) count[b] = cnt; lengths[o] = L; scores[o] = sc; logits[o] = lg; }
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

// beam.hip's search_lds plus bonus[2][W], ebonus[Pmax] (f64), lmst[2][W], estate[Pmax] (int32) and 64 bytes for the image's
// descriptor and the weights.
// W = 128, Kmax = 16 (Pmax = 4096): 8 (10 W + 2 Pmax) + 32 W + 4 (10 W + 2 Pmax + 2 G (2 + 2 Kmax) + 4) + 64 = 122 192 bytes.
inline size_t search_lds(int W, int Kmax, int Pmax) {
    static_assert(sizeof(LmImage) + 2 * sizeof(double) <= 64, "the descriptor's LDS slot");
    return (size_t)8 * (10 * W + 2 * Pmax) + (size_t)8 * 4 * W + (size_t)4 * (10 * W + 2 * Pmax + 2 * G * (2 + 2 * Kmax) + 4) + 64;
}

}  // namespace

SCONF_API int sconf_lm_max_order(void) { return MAX_ORDER; }
SCONF_API int sconf_lm_beam_threads(int64_t W, int64_t Kmax) { return sizes_ok(W, Kmax) ? search_threads(W, Kmax) : -1; }

SCONF_API int64_t sconf_lm_beam_workspace(int64_t B, int64_t N, int64_t W, int64_t Kmax) {
    if (B < 1 || N < 1 || !sizes_ok(W, Kmax) || B * N > 0x7fffffff || B * N * W > 0x7fffffff) return -1;
    return round256(B * N * (8 + 8 * Kmax)) + round256(16 * B * N * W) + round256(24 * B * W) + round256(4 * B);
}

SCONF_API int sconf_lm_beam_ctc(const float* log_probs, const int32_t* input_lengths, const void* image, int64_t n_states,
                                int64_t n_entries, int64_t num_tokens, int order, int start_state, int32_t* count, int32_t* tokens,
                                int32_t* lengths, int32_t* token_frames, double* scores, double* logit_scores, void* workspace,
                                int64_t workspace_bytes, int64_t B, int64_t N, int64_t C, int blank, int beam_width, int nbest,
                                float token_min_logp, double beam_prune_logp, int max_tokens_per_frame, int64_t Lmax, double alpha,
                                double beta, sconf_stream_t stream) {
    if (B == 0) return 0;
    const int W = beam_width, Kmax = max_tokens_per_frame;
    SCONF_REQUIRE(W >= 1 && W <= MAX_W, "sconf_lm_beam_ctc: beam_width %d: from 1 to %d", W, MAX_W);
    SCONF_REQUIRE(Kmax >= 1 && Kmax <= MAX_K, "sconf_lm_beam_ctc: max_tokens_per_frame %d: from 1 to %d", Kmax, MAX_K);
    SCONF_REQUIRE(nbest >= 1 && nbest <= W, "sconf_lm_beam_ctc: nbest %d: from 1 to beam_width = %d", nbest, W);
    SCONF_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && B * N <= 0x7fffffff && B * N * W <= 0x7fffffff && Lmax >= 1 && nbest * Lmax <= 0x7fffffff,
                  "sconf_lm_beam_ctc: bad sizes B = %ld, N = %ld, Lmax = %ld", (long)B, (long)N, (long)Lmax);
    SCONF_REQUIRE(C >= 4 && C % 4 == 0 && C * 4 <= 64 * 1024, "sconf_lm_beam_ctc: C must be a multiple of 4 and one row must fit LDS (%ld classes)", (long)C);
    SCONF_REQUIRE(blank >= 0 && blank < C, "sconf_lm_beam_ctc: blank %d out of range", blank);
    SCONF_REQUIRE(beam_prune_logp <= 0.0, "sconf_lm_beam_ctc: beam_prune_logp must be <= 0 (-inf: no pruning)");
    SCONF_REQUIRE(order >= 1 && order <= MAX_ORDER, "sconf_lm_beam_ctc: order %d: from 1 to %d", order, MAX_ORDER);
    SCONF_REQUIRE(num_tokens >= 1 && num_tokens <= C, "sconf_lm_beam_ctc: num_tokens %ld: from 1 to C = %ld", (long)num_tokens, (long)C);
    SCONF_REQUIRE(n_states >= 1 && n_entries >= 0 && n_states <= 0x7fffffff && n_entries <= 0x7fffffff &&
                  4 * (n_states + n_entries) + 2 * num_tokens <= 0x7fffffff,
                  "sconf_lm_beam_ctc: bad image sizes: %ld states, %ld entries", (long)n_states, (long)n_entries);
    SCONF_REQUIRE(start_state >= 0 && start_state < n_states, "sconf_lm_beam_ctc: start_state %d out of range", start_state);
    SCONF_REQUIRE(std::isfinite(alpha) && std::isfinite(beta), "sconf_lm_beam_ctc: alpha and beta must be finite");
    SCONF_REQUIRE(log_probs && image && count && tokens && lengths && token_frames && scores && logit_scores && workspace,
                  "sconf_lm_beam_ctc: null pointer");
    SCONF_REQUIRE(((uintptr_t)image & 15) == 0, "sconf_lm_beam_ctc: the image must be 16-byte aligned");
    SCONF_REQUIRE(workspace_bytes >= sconf_lm_beam_workspace(B, N, W, Kmax), "sconf_lm_beam_ctc: workspace of %ld bytes, %ld needed",
                  (long)workspace_bytes, (long)sconf_lm_beam_workspace(B, N, W, Kmax));
    int* rec = (int*)workspace;
    int4* trie = (int4*)((char*)workspace + round256(B * N * (8 + 8 * Kmax)));
    FinLm* fin = (FinLm*)((char*)trie + round256(16 * B * N * W));
    int* nlive = (int*)((char*)fin + round256(24 * B * W));
    LmImage L;
    L.states = (const int4*)image;
    L.entries = L.states + n_states;
    L.dense = (const int2*)(L.entries + n_entries);
    L.n_states = (int)n_states; L.n_entries = (int)n_entries; L.num_tokens = (int)num_tokens; L.order = order;
    const size_t lds_c = (size_t)C * 4 + 4 * (12 + 8 * MAX_K);
    static bool big_c = false, big_s = false;
    if (lds_c > 48 * 1024) lds_limit_once(big_c, {(const void*)beam_compact_kernel}, 64 * 1024 + 4 * (12 + 8 * MAX_K));
    hipLaunchKernelGGL(beam_compact_kernel, dim3((unsigned)std::min<long>(B * N, 65536)), dim3(256), lds_c, stream, log_probs, input_lengths,
                       rec, (int)B, (int)N, (int)C, blank, token_min_logp, Kmax);
    const int Pmax = pow2ceil((long)W * (Kmax + 1));
    const size_t lds_s = search_lds(W, Kmax, Pmax);
    if (lds_s > 48 * 1024) lds_limit_once(big_s, {(const void*)beam_search_lm_kernel}, search_lds(MAX_W, MAX_K, pow2ceil((long)MAX_W * (MAX_K + 1))));
    hipLaunchKernelGGL(beam_search_lm_kernel, dim3((unsigned)B), dim3(search_threads(W, Kmax)), lds_s, stream, rec, input_lengths, trie, fin, nlive,
                       L, start_state, alpha, beta, (int)N, W, Kmax, beam_prune_logp, Pmax);
    hipLaunchKernelGGL(beam_backtrace_lm_kernel, dim3((unsigned)nbest, (unsigned)B), dim3(64), 0, stream, trie, fin, nlive, count, tokens,
                       lengths, token_frames, scores, logit_scores, (int)N, W, nbest, (long)Lmax);
    SCONF_LAUNCH_OK("sconf_lm_beam_ctc");
    return 0;
}
