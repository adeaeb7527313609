// CTC prefix beam search with hotword boosting (include/sconf_hot.h): the search of csrc/beam_lm.hip with a second automaton walked
// beside the LM, the Aho-Corasick automaton of the hotword phrases over tokens.  A created token adds weight emit[new state] to its
// prefix's bonus for good (every phrase that ends there), and while the search runs a beam's key also holds weight phi[state], the
// credit of the phrase it is in the middle of, which goes with the state.
//
// Structure: the three kernels of beam_lm.hip.
//   1. compact   beam_compact_kernel of beam_common.h, unchanged: hotwords do not decide which tokens are kept.
//   2. search    beam_search_lm_kernel with, per beam, hot[2][W] (f64, the permanent credit), wphi[2][W] (f64, weight phi of the
//                beam's state) and hst[2][W] (the state), and, per candidate position, ehst[Pmax] beside ebonus / estate.  The
//                hotword walk of extension (i, k) is taken by the thread that takes its LM walk, in the pass that finalises every
//                key after the fold is known: no barrier is added.  The two chains of loads are independent, but each is a loop
//                with a data-dependent exit and the thread ends one before it starts the other: they do NOT overlap (measured,
//                +7 to 12 % a call).  Each round of the walk is one 16-byte state load and a bisection over the
//                state's sorted 8-byte children; then one 8-byte credit record (emit, phi) of the state reached.  Only the new STATE
//                is kept per candidate (4 bytes): a survivor reads its credit record once more for hot' = hot + weight emit - a
//                record the same frame has just touched - instead of 16 more bytes of LDS per candidate position.
//                With weight = 0 or an image of the root alone no walk is taken and every credit is 0: the keys are those of
//                beam_lm.hip bit for bit (x + 0.0 = x: no bonus and no total is ever -0.0).
//                The frame without a kept token is the code of beam.hip: phi and bonus do not change there.
//                After the last frame phi is dropped and the n <= W survivors are ranked by acoustic total + bonus, by counting in
//                LDS (stable: equal keys keep their order).
//   3. backtrace beam_lm.hip's, writing hot_scores as the seventh output.
//
// No synchronisation between workgroups, no atomics; the images are only read.  All score arithmetic is f64; compiled without
// -ffast-math (see the Makefile), and every product and sum of the contract is written with the _rn intrinsics so that none is fused.
#include "beam_common.h"
#include "../../include/sconf_hot.h"

namespace {

constexpr int MAX_ORDER = 5;                            // sconf_lm_max_order()
constexpr int MAX_LEN = 32;                             // tokens of the longest phrase

struct FinHot { int node, len; double score, logit, hot; };

// The images as the launcher carves them; the sizes clamp every index read from them.
struct LmImage {
    const int4* states;                                 // [n_states]  first_child, n_children, backoff f32, backoff_state
    const int4* entries;                                // [n_entries] token, logp f32, next_state, 0
    const int2* dense;                                  // [num_tokens] logp f32, next_state
    int n_states, n_entries, num_tokens, order;         // n_states = 0: no LM
};

struct HotImage {
    const int4* states;                                 // [n_states]  first_child, n_children, fail_state, 0
    const float2* credit;                               // [n_states]  emit, phi
    const int2* entries;                                // [n_entries] token, next_state
    int n_states, n_entries, max_len, pad;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// step(state, token) of sconf_lm.h: q, the f64 sum of the f32 values met, and the next state (beam_lm.hip's).
__device__ __forceinline__ double lm_step(const LmImage* Ld, int s, int c, int& next) {
    LmImage L;
    L.states = Ld->states; L.entries = Ld->entries; L.dense = Ld->dense;
    L.n_states = Ld->n_states; L.n_entries = Ld->n_entries; L.num_tokens = Ld->num_tokens; L.order = Ld->order;
    next = 0;
    if (c < 0 || c >= L.num_tokens) return 0.0;         // a class the model does not know
    double q = 0.0;
    s = clampi(s, 0, L.n_states - 1);
    const int2 d = L.dense[c];
    for (int lvl = 1; lvl < L.order && s != 0; ++lvl) {
        const int4 st = L.states[s];
        int lo = clampi(st.x, 0, L.n_entries);
        int hi = lo + clampi(st.y, 0, L.n_entries - lo);
        for (int it = 0; it < 32 && lo < hi; ++it) {
            const int mid = lo + ((hi - lo) >> 1);
            const int4 e = L.entries[mid];
            if (e.x == c) { next = clampi(e.z, 0, L.n_states - 1); return q + (double)__int_as_float(e.y); }
            if (e.x < c) lo = mid + 1; else hi = mid;
        }
        q += (double)__int_as_float(st.z);
        s = clampi(st.w, 0, L.n_states - 1);
    }
    next = clampi(d.y, 0, L.n_states - 1);
    return q + (double)__int_as_float(d.x);
}

// step(state, token) of the header: the next state.  n_states >= 1; at most max_len + 1 rounds (the depth falls with every failure arc).
__device__ __forceinline__ int hot_step(const HotImage* Hd, int s, int c) {
    const int4* states = Hd->states;
    const int2* entries = Hd->entries;
    const int S = Hd->n_states, E = Hd->n_entries, rounds = Hd->max_len + 1;
    s = clampi(s, 0, S - 1);
    for (int r = 0; r < rounds; ++r) {
        const int4 st = states[s];
        int lo = clampi(st.x, 0, E);
        int hi = lo + clampi(st.y, 0, E - lo);
        for (int it = 0; it < 32 && lo < hi; ++it) {    // bisection over the sorted children
            const int mid = lo + ((hi - lo) >> 1);
            const int2 e = entries[mid];
            if (e.x == c) return clampi(e.y, 0, S - 1);
            if (e.x < c) lo = mid + 1; else hi = mid;
        }
        if (s == 0) return 0;
        s = clampi(st.z, 0, S - 1);
    }
    return 0;                                           // (only a damaged image's chain gets here)
}

// One workgroup per sample.  beam_search_lm_kernel of beam_lm.hip plus the hotwords; Pmax = the largest sort.  LDS as carved below.
__global__ __launch_bounds__(1024) void beam_search_hot_kernel(const int* __restrict__ rec, const int* __restrict__ in_len,
                                                               int4* __restrict__ trie, FinHot* __restrict__ fin, int* __restrict__ nlive,
                                                               LmImage image, HotImage himage, int start_state, double alpha_, double beta_,
                                                               double weight_, int N, int W, int Kmax, double prune, int Pmax) {
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
    double* bonus = skey + W;                           // [2][W]  the LM's and the finished hotwords' share of the key
    double* hot = bonus + 2 * W;                        // [2][W]  the finished hotwords' share alone
    double* wphi = hot + 2 * W;                         // [2][W]  weight phi[hst]: the share of the hotword in progress
    double* key = wphi + 2 * W;                         // [Pmax]
    double* ebonus = key + Pmax;                        // [Pmax]  a candidate extension's new bonus, by compact position
    unsigned long long* hash = reinterpret_cast<unsigned long long*>(ebonus + Pmax);   // [2][W]
    unsigned long long* phash = hash + 2 * W;           // [2][W]  hash of the prefix without its last token
    int* len = reinterpret_cast<int*>(phash + 2 * W);   // [2][W]
    int* last = len + 2 * W;                            // [2][W]
    int* node = last + 2 * W;                           // [2][W]
    int* lmst = node + 2 * W;                           // [2][W]  LM state
    int* hst = lmst + 2 * W;                            // [2][W]  hotword state
    int* fsrc = hst + 2 * W;                            // [W]  the beam whose extension folds into this one, or -1
    int* sidx = fsrc + W;                               // [W]
    int* idx = sidx + W;                                // [Pmax]
    int* estate = idx + Pmax;                           // [Pmax]  a candidate extension's new LM state, by compact position
    int* ehst = estate + Pmax;                          // [Pmax]  and its new hotword state
    int* rbuf = ehst + Pmax;                            // [2][CH]
    int* misc = rbuf + 2 * CH;                          // [4]
    // The descriptors and the weights are read from LDS where a walk is taken, not held in scalar registers across the frame loop
    // (beam_lm.hip): the frame without a kept token keeps the register budget it has in beam.hip.
    LmImage* Ls = reinterpret_cast<LmImage*>(misc + 4); // [1]  (8-byte aligned: every int array above has an even length)
    HotImage* Hs = reinterpret_cast<HotImage*>(Ls + 1); // [1]
    double* wts = reinterpret_cast<double*>(Hs + 1);    // [3]  alpha, beta, weight (0 also where the image holds only the root)
    const double NEG = -(double)INFINITY;
    const bool boost = weight_ > 0.0 && himage.n_states > 1;              // (uniform) else: no walk, no credit, no re-rank

    if (tid == 0) {
        pb[0] = 0.0; pnb[0] = NEG; hash[0] = H0; phash[0] = 0; len[0] = 0; last[0] = -1; node[0] = -1;
        bonus[0] = 0.0; hot[0] = 0.0; wphi[0] = 0.0; hst[0] = 0;
        lmst[0] = image.n_states > 0 ? clampi(start_state, 0, image.n_states - 1) : 0;
        Ls->states = image.states; Ls->entries = image.entries; Ls->dense = image.dense;
        Ls->n_states = image.n_states; Ls->n_entries = image.n_entries; Ls->num_tokens = image.num_tokens; Ls->order = image.order;
        Hs->states = himage.states; Hs->credit = himage.credit; Hs->entries = himage.entries;
        Hs->n_states = himage.n_states; Hs->n_entries = himage.n_entries; Hs->max_len = himage.max_len; Hs->pad = 0;
        wts[0] = alpha_; wts[1] = beta_; wts[2] = boost ? weight_ : 0.0;
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
            for (int p = tid; p < (ranked ? M : P); p += nt) {             // the keys: acoustic total + (bonus + weight phi), the sums in that order
                double x = NEG;
                if (p < n) {
                    const double a = lse2(spb[p], spnb[p]);
                    if (a > NEG) x = a + __dadd_rn(bonus[co + p], wphi[co + p]);
                } else if (p < M) {
                    const double a = key[p];
                    if (a > NEG) {                      // a live extension that was not folded: its step through both automata
                        const int e = p - n, i = e / Kf, k = e - i * Kf;
                        const int c = fr[2 + 2 * k];
                        const double w = wts[2];
                        int hs = 0;
                        if (w > 0.0) hs = hot_step(Hs, hst[co + i], c);    // (ends before the LM's walk starts: the two do not overlap)
                        int ns = 0;
                        double term = 0.0;
                        if (Ls->n_states > 0) {
                            const double q = lm_step(Ls, lmst[co + i], c, ns);
                            term = __dadd_rn(__dmul_rn(wts[0], q), wts[1]);                       // (two roundings, never an fma: the contract's value)
                        }
                        float2 cr = make_float2(0.f, 0.f);
                        if (w > 0.0) cr = Hs->credit[hs];
                        const double nb = __dadd_rn(__dadd_rn(bonus[co + i], term), __dmul_rn(w, (double)cr.x));
                        ebonus[p] = nb;
                        estate[p] = ns;
                        ehst[p] = hs;
                        x = a + __dadd_rn(nb, __dmul_rn(w, (double)cr.y));
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
                        hot[no + tid] = hot[co + p]; wphi[no + tid] = wphi[co + p]; hst[no + tid] = hst[co + p];
                    } else {
                        const int e = p - n, i = e / Kf, k = e - i * Kf;
                        const int c = fr[2 + 2 * k];
                        pb[no + tid] = NEG;             // the acoustic total, by the expression that made it
                        pnb[no + tid] = (double)__int_as_float(fr[3 + 2 * k]) + (c == last[co + i] ? pb[co + i] : tot[i]);
                        phash[no + tid] = hash[co + i]; hash[no + tid] = extend_hash(hash[co + i], c);
                        len[no + tid] = len[co + i] + 1; last[no + tid] = c; node[no + tid] = t * W + tid;
                        bonus[no + tid] = ebonus[p]; lmst[no + tid] = estate[p];
                        const double w = wts[2];
                        const int hs = ehst[p];         // (in range: hot_step clamps what it returns)
                        float2 cr = make_float2(0.f, 0.f);
                        if (w > 0.0) cr = Hs->credit[hs];                  // the record its key was made from
                        hot[no + tid] = __dadd_rn(hot[co + i], __dmul_rn(w, (double)cr.x));
                        wphi[no + tid] = __dmul_rn(w, (double)cr.y);
                        hst[no + tid] = hs;
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
    // The end: phi is dropped.  With a boost the n <= W survivors are ranked by their final key (counting, stable); else rank = tid.
    FinHot f;
    f.node = -1; f.len = 0; f.score = NEG; f.logit = NEG; f.hot = 0.0;
    if (tid < n) {
        const int o = cur * W + tid;
        f.node = node[o]; f.len = len[o]; f.logit = lse2(pb[o], pnb[o]); f.score = f.logit + bonus[o]; f.hot = hot[o];
        if (boost) skey[tid] = f.score > NEG ? f.score : NEG;             // (W <= Pmax / 2; NaN ranks with -inf, so ranks stay a permutation)
    }
    int r = tid;
    if (boost) {
        __syncthreads();
        if (tid < n) {
            const double x = skey[tid];
            r = 0;
            for (int q = 0; q < n; ++q) { const double y = skey[q]; r += (y > x) | ((y == x) & (q < tid)); }
        }
    }
    if (tid < n) fin[(long)b * W + r] = f;
    if (tid == 0) nlive[b] = n;
}

// One wave per (sample, rank): every element of the rank's outputs, and count[b] from rank 0.
__global__ __launch_bounds__(64) void beam_backtrace_hot_kernel(const int4* __restrict__ trie, const FinHot* __restrict__ fin,
                                                                const int* __restrict__ nlive, int* __restrict__ count,
                                                                int* __restrict__ tokens, int* __restrict__ lengths, int* __restrict__ frames,
                                                                double* __restrict__ scores, double* __restrict__ logits,
                                                                double* __restrict__ hots, int N, int W, int nbest, long Lmax) {
    const int r = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const int nl = nlive[b], cnt = min(max(nl, 0), nbest);
    const long o = (long)b * nbest + r;
    int L = 0, leaf = -1;
    double sc = nl < 0 ? (double)NAN : -(double)INFINITY, lg = sc, ht = sc;
    if (r < cnt) { const FinHot f = fin[(long)b * W + r]; L = max(f.len, 0); leaf = f.node; sc = f.score; lg = f.logit; ht = f.hot; }
    if (lane == 0) { if (r == 0) count[b] = cnt; lengths[o] = L; scores[o] = sc; logits[o] = lg; hots[o] = ht; }
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

// beam_lm.hip's search_lds (less its 64-byte descriptor slot) plus hot[2][W], wphi[2][W] (f64), hst[2][W], ehst[Pmax] (int32) and
// 128 bytes for the two descriptors and the three weights.
// W = 128, Kmax = 16 (Pmax = 4096): 8 (14 W + 2 Pmax) + 32 W + 4 (12 W + 3 Pmax + 2 G (2 + 2 Kmax) + 4) + 128 = 143 760 bytes.
inline size_t search_lds(int W, int Kmax, int Pmax) {
    static_assert(sizeof(LmImage) + sizeof(HotImage) + 3 * sizeof(double) <= 128, "the descriptors' LDS slot");
    return (size_t)8 * (14 * W + 2 * Pmax) + (size_t)8 * 4 * W + (size_t)4 * (12 * W + 3 * Pmax + 2 * G * (2 + 2 * Kmax) + 4) + 128;
}

}  // namespace

SCONF_API int sconf_hot_max_len(void) { return MAX_LEN; }
SCONF_API int sconf_hot_max_width(void) { return MAX_W; }
SCONF_API int sconf_hot_max_tokens(void) { return MAX_K; }
SCONF_API int sconf_hot_beam_threads(int64_t W, int64_t Kmax) { return sizes_ok(W, Kmax) ? search_threads(W, Kmax) : -1; }

SCONF_API int64_t sconf_hot_beam_workspace(int64_t B, int64_t N, int64_t W, int64_t Kmax) {
    if (B < 1 || N < 1 || !sizes_ok(W, Kmax) || B * N > 0x7fffffff || B * N * W > 0x7fffffff) return -1;
    return round256(B * N * (8 + 8 * Kmax)) + round256(16 * B * N * W) + round256(32 * B * W) + round256(4 * B);
}

SCONF_API int sconf_hot_beam_ctc(const float* log_probs, const int32_t* input_lengths, const void* lm_image, int64_t n_states,
                                 int64_t n_entries, int64_t num_tokens, int order, int start_state, const void* hot_image,
                                 int64_t hot_states, int64_t hot_entries, int hot_max_len, double weight, int32_t* count, int32_t* tokens,
                                 int32_t* lengths, int32_t* token_frames, double* scores, double* logit_scores, double* hot_scores,
                                 void* workspace, int64_t workspace_bytes, int64_t B, int64_t N, int64_t C, int blank, int beam_width,
                                 int nbest, float token_min_logp, double beam_prune_logp, int max_tokens_per_frame, int64_t Lmax,
                                 double alpha, double beta, sconf_stream_t stream) {
    if (B == 0) return 0;
    const int W = beam_width, Kmax = max_tokens_per_frame;
    SCONF_REQUIRE(W >= 1 && W <= MAX_W, "sconf_hot_beam_ctc: beam_width %d: from 1 to %d", W, MAX_W);
    SCONF_REQUIRE(Kmax >= 1 && Kmax <= MAX_K, "sconf_hot_beam_ctc: max_tokens_per_frame %d: from 1 to %d", Kmax, MAX_K);
    SCONF_REQUIRE(nbest >= 1 && nbest <= W, "sconf_hot_beam_ctc: nbest %d: from 1 to beam_width = %d", nbest, W);
    SCONF_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && B * N <= 0x7fffffff && B * N * W <= 0x7fffffff && Lmax >= 1 && nbest * Lmax <= 0x7fffffff,
                  "sconf_hot_beam_ctc: bad sizes B = %ld, N = %ld, Lmax = %ld", (long)B, (long)N, (long)Lmax);
    SCONF_REQUIRE(C >= 4 && C % 4 == 0 && C * 4 <= 64 * 1024, "sconf_hot_beam_ctc: C must be a multiple of 4 and one row must fit LDS (%ld classes)", (long)C);
    SCONF_REQUIRE(blank >= 0 && blank < C, "sconf_hot_beam_ctc: blank %d out of range", blank);
    SCONF_REQUIRE(beam_prune_logp <= 0.0, "sconf_hot_beam_ctc: beam_prune_logp must be <= 0 (-inf: no pruning)");
    const bool with_lm = lm_image != nullptr || n_states != 0;
    if (with_lm) {
        SCONF_REQUIRE(lm_image != nullptr, "sconf_hot_beam_ctc: null pointer (an LM of %ld states without an image)", (long)n_states);
        SCONF_REQUIRE(order >= 1 && order <= MAX_ORDER, "sconf_hot_beam_ctc: order %d: from 1 to %d", order, MAX_ORDER);
        SCONF_REQUIRE(num_tokens >= 1 && num_tokens <= C, "sconf_hot_beam_ctc: num_tokens %ld: from 1 to C = %ld", (long)num_tokens, (long)C);
        SCONF_REQUIRE(n_states >= 1 && n_entries >= 0 && n_states <= 0x7fffffff && n_entries <= 0x7fffffff &&
                      4 * (n_states + n_entries) + 2 * num_tokens <= 0x7fffffff,
                      "sconf_hot_beam_ctc: bad image sizes: %ld states, %ld entries", (long)n_states, (long)n_entries);
        SCONF_REQUIRE(start_state >= 0 && start_state < n_states, "sconf_hot_beam_ctc: start_state %d out of range", start_state);
        SCONF_REQUIRE(((uintptr_t)lm_image & 15) == 0, "sconf_hot_beam_ctc: the LM image must be 16-byte aligned");
    } else {
        SCONF_REQUIRE(n_entries == 0 && num_tokens == 0, "sconf_hot_beam_ctc: bad image sizes: no LM image, but %ld entries and %ld tokens",
                      (long)n_entries, (long)num_tokens);
    }
    SCONF_REQUIRE(std::isfinite(alpha) && std::isfinite(beta), "sconf_hot_beam_ctc: alpha and beta must be finite");
    SCONF_REQUIRE(std::isfinite(weight) && weight >= 0.0, "sconf_hot_beam_ctc: weight must be finite and >= 0");
    SCONF_REQUIRE(hot_states >= 1 && hot_entries >= 0 && hot_states <= 0x7fffffff && hot_entries <= 0x7fffffff &&
                  6 * hot_states + 2 * hot_entries <= 0x7fffffff,
                  "sconf_hot_beam_ctc: bad hotword image sizes: %ld states, %ld entries", (long)hot_states, (long)hot_entries);
    SCONF_REQUIRE(hot_max_len >= 0 && hot_max_len <= MAX_LEN, "sconf_hot_beam_ctc: hot_max_len %d: from 0 to %d", hot_max_len, MAX_LEN);
    SCONF_REQUIRE(log_probs && hot_image && count && tokens && lengths && token_frames && scores && logit_scores && hot_scores && workspace,
                  "sconf_hot_beam_ctc: null pointer");
    SCONF_REQUIRE(((uintptr_t)hot_image & 15) == 0, "sconf_hot_beam_ctc: the hotword image must be 16-byte aligned");
    SCONF_REQUIRE(workspace_bytes >= sconf_hot_beam_workspace(B, N, W, Kmax), "sconf_hot_beam_ctc: workspace of %ld bytes, %ld needed",
                  (long)workspace_bytes, (long)sconf_hot_beam_workspace(B, N, W, Kmax));
    int* rec = (int*)workspace;
    int4* trie = (int4*)((char*)workspace + round256(B * N * (8 + 8 * Kmax)));
    FinHot* fin = (FinHot*)((char*)trie + round256(16 * B * N * W));
    int* nlive = (int*)((char*)fin + round256(32 * B * W));
    LmImage L;
    L.states = (const int4*)lm_image;
    L.entries = with_lm ? L.states + n_states : nullptr;
    L.dense = with_lm ? (const int2*)(L.entries + n_entries) : nullptr;
    L.n_states = (int)n_states; L.n_entries = (int)n_entries; L.num_tokens = (int)num_tokens; L.order = with_lm ? order : 0;
    HotImage H;
    H.states = (const int4*)hot_image;
    H.credit = (const float2*)(H.states + hot_states);
    H.entries = (const int2*)(H.credit + hot_states);
    H.n_states = (int)hot_states; H.n_entries = (int)hot_entries; H.max_len = hot_max_len; H.pad = 0;
    const size_t lds_c = (size_t)C * 4 + 4 * (12 + 8 * MAX_K);
    static bool big_c = false, big_s = false;
    if (lds_c > 48 * 1024) lds_limit_once(big_c, {(const void*)beam_compact_kernel}, 64 * 1024 + 4 * (12 + 8 * MAX_K));
    hipLaunchKernelGGL(beam_compact_kernel, dim3((unsigned)std::min<long>(B * N, 65536)), dim3(256), lds_c, stream, log_probs, input_lengths,
                       rec, (int)B, (int)N, (int)C, blank, token_min_logp, Kmax);
    const int Pmax = pow2ceil((long)W * (Kmax + 1));
    const size_t lds_s = search_lds(W, Kmax, Pmax);
    if (lds_s > 48 * 1024) lds_limit_once(big_s, {(const void*)beam_search_hot_kernel}, search_lds(MAX_W, MAX_K, pow2ceil((long)MAX_W * (MAX_K + 1))));
    hipLaunchKernelGGL(beam_search_hot_kernel, dim3((unsigned)B), dim3(search_threads(W, Kmax)), lds_s, stream, rec, input_lengths, trie, fin, nlive,
                       L, H, with_lm ? start_state : 0, alpha, beta, weight, (int)N, W, Kmax, beam_prune_logp, Pmax);
    hipLaunchKernelGGL(beam_backtrace_hot_kernel, dim3((unsigned)nbest, (unsigned)B), dim3(64), 0, stream, trie, fin, nlive, count, tokens,
                       lengths, token_frames, scores, logit_scores, hot_scores, (int)N, W, nbest, (long)Lmax);
    SCONF_LAUNCH_OK("sconf_hot_beam_ctc");
    return 0;
}
