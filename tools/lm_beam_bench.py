"""Micro-benchmark of the beam search with an n-gram LM fused in (sconf_lm_beam_ctc) beside the LM-free search (sconf_beam_ctc), a
sibling of tools/beam_bench.py and on its inputs: 'spiky', 'noise' and 'quiet' at B=1, N=16384 and B=16, N=2048 (C=4096), beam widths
16 and 100.  Whole calls between HIP events, output allocation included, in the order A / B / A in one process: LM-free, fused
(alpha = 0.5, beta = 1.5), LM-free again.  The LM is a synthetic trigram image of about 10^6 grams over 4095 tokens made from a seed
(every token has 60 bigram children, every bigram 3 trigram children): 19.8 MB, more than an XCD's L2 and less than the Infinity
Cache.  Before timing, the fused search at alpha = beta = 0 must return the LM-free tokens.

Per-kernel times come from a kernel trace of a run of its own, which this tool also reads:
    rocprofv3 --kernel-trace -d DIR -o kt -- python tools/lm_beam_bench.py --kernels-only --manifest DIR/manifest.json [--shape long]
    python tools/lm_beam_bench.py --trace DIR/kt_results.db --manifest DIR/manifest.json
The second command matches the search kernels' dispatches (beam_search_kernel / beam_search_lm_kernel), in order, with the calls the
manifest lists and reports, fused beside LM-free: the search kernel's time, its time per frame without a kept token (the 'quiet'
input) and per frame with a selection (the rest of the 'spiky' / 'noise' time over their frames with a kept token)."""
import argparse
import json
import os
import sqlite3
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import beam_bench as BB                                                    # the inputs, the frame count and the timer

SHAPES, WIDTHS, KINDS = BB.SHAPES, BB.WIDTHS, BB.KINDS
ALPHA, BETA = 0.5, 1.5
V, BIGRAMS_PER_TOKEN, TRIGRAMS_PER_BIGRAM = 4095, 60, 3


def _sorted_distinct(rng, rows, k, V):
    """(rows, k) ascending distinct tokens of [0, V) per row."""
    import numpy as np
    return np.sort(rng.integers(0, V - k + 1, (rows, k)), axis=1) + np.arange(k)


def synthetic_trigram(seed=0):
    """An NGramLM whose image is built array by array (no ARPA text, no dict): states = the empty context, V unigrams, V x 60 bigrams;
    entries = the bigrams and V x 60 x 3 trigrams; log-probs and back-offs uniform in natural-log ranges a trained model has."""
    import numpy as np
    from lcasr_amd.decoding.lm import NGramLM
    rng = np.random.default_rng(seed)
    K2, K3 = BIGRAMS_PER_TOKEN, TRIGRAMS_PER_BIGRAM
    n2, n3 = V * K2, V * K2 * K3
    S, E = 1 + V + n2, n2 + n3
    bits = lambda lo, hi, n: rng.uniform(lo, hi, n).astype(np.float32).view(np.int32)
    image = np.zeros(4 * S + 4 * E + 2 * V, dtype=np.int32)
    st, en, de = image[:4 * S].reshape(-1, 4), image[4 * S:4 * (S + E)].reshape(-1, 4), image[4 * (S + E):].reshape(-1, 2)
    b_tok = _sorted_distinct(rng, V, K2, V)                                # children of (a,)
    bigram_state = np.full((V, V), -1, dtype=np.int32)
    bigram_state[np.repeat(np.arange(V), K2), b_tok.reshape(-1)] = 1 + V + np.arange(n2)
    st[1:1 + V] = np.stack([np.arange(V) * K2, np.full(V, K2), bits(-2.0, -0.1, V), np.zeros(V, dtype=np.int64)], 1)
    en[:n2] = np.stack([b_tok.reshape(-1), bits(-6.0, -0.5, n2), 1 + V + np.arange(n2), np.zeros(n2, dtype=np.int64)], 1)
    c_tok = _sorted_distinct(rng, n2, K3, V)                               # children of (a, b)
    st[1 + V:] = np.stack([n2 + np.arange(n2) * K3, np.full(n2, K3), bits(-1.5, -0.05, n2), 1 + b_tok.reshape(-1)], 1)
    b_of = np.repeat(b_tok.reshape(-1), K3)
    nxt = bigram_state[b_of, c_tok.reshape(-1)]                            # the longest suffix of (a, b, c) that is a state: (b, c) or (c,)
    en[n2:] = np.stack([c_tok.reshape(-1), bits(-4.0, -0.2, n3), np.where(nxt >= 0, nxt, 1 + c_tok.reshape(-1)), np.zeros(n3, dtype=np.int64)], 1)
    de[:] = np.stack([bits(-12.0, -4.0, V), 1 + np.arange(V)], 1)
    return NGramLM(image, S, E, V, 3, 0)


def searches(lp, lm):
    import lcasr_amd.hip.beam as K
    import lcasr_amd.hip.lm as L
    B, N, C = lp.shape
    im = lm.device_image(lp.device)
    free = lambda W: K.ctc_beam(lp, None, C - 1, W, 1, -5.0, -10.0, 16, N)
    fused = lambda W, a=ALPHA, b=BETA: L.ctc_beam_lm(lp, None, im, lm.n_states, lm.n_entries, lm.num_tokens, lm.order, lm.start_state,
                                                     C - 1, W, 1, -5.0, -10.0, 16, N, a, b)
    return free, fused


def run(a):
    import torch
    import lcasr_amd.hip.lm as L
    lm = synthetic_trigram(a.seed)
    print(f'[lm] synthetic trigram: {V + lm.n_entries} grams, {lm.n_states} states, {lm.n_entries} entries, image {lm.image.nbytes} bytes')
    manifest = []
    for name in (SHAPES if a.shape == 'all' else [a.shape]):
        B, N, C = SHAPES[name]
        for kind in KINDS:
            lp = BB.inputs(kind, B, N, C)
            kept = BB.frames_with_a_token(lp, C - 1)
            free, fused = searches(lp, lm)
            for W in WIDTHS:
                x, y = free(W), fused(W, 0.0, 0.0)
                manifest += [dict(shape=name, kind=kind, W=W, lm=with_lm, check=True) for with_lm in (False, True)]
                assert torch.equal(x.tokens, y.tokens) and torch.equal(x.scores, y.scores) and torch.equal(y.scores, y.logit_scores), \
                    f'{name} {kind} W={W}: the fused search at alpha = beta = 0 is not the LM-free search'
            if a.kernels_only:
                for W in WIDTHS:
                    for with_lm in (False, True, False, True):
                        (fused if with_lm else free)(W)
                        manifest.append(dict(shape=name, kind=kind, B=B, N=N, C=C, W=W, lm=with_lm, frames_with_a_token=kept))
                torch.cuda.synchronize()
                continue
            n = a.reps or (3 if kind == 'noise' else 5)
            out = fused(16)
            print(f'[{name} {kind}] B={B} N={N} C={C}: {kept} of {B * N} frames keep a token; fused best hypothesis of sample 0: '
                  f'{int(out.lengths[0, 0])} tokens, score {float(out.scores[0, 0]):.3f}, acoustic {float(out.logit_scores[0, 0]):.3f}; '
                  f'workspace {L.beam_workspace(B, N, 16, 16)} bytes at W=16, {L.beam_workspace(B, N, 100, 16)} at W=100')
            for W in WIDTHS:
                a0, b0, a1 = BB.timed(lambda: free(W), n), BB.timed(lambda: fused(W), n), BB.timed(lambda: free(W), n)
                print(f'[{name} {kind}] W={W}: LM-free {a0:.3f} ms | fused {b0:.3f} ms | LM-free {a1:.3f} ms   '
                      f'(A/B/A spread {abs(a1 - a0):.3f} ms; fused / LM-free {b0 / min(a0, a1):.3f})')
    if a.kernels_only and a.manifest:
        json.dump(manifest, open(a.manifest, 'w'))


def report(a):
    calls = json.load(open(a.manifest))
    db = sqlite3.connect(a.trace)
    cur = db.cursor()
    tabs = [r[0] for r in cur.execute("select name from sqlite_master where type='table'")]
    kd = [t for t in tabs if t.startswith('rocpd_kernel_dispatch')][0]
    ks = [t for t in tabs if t.startswith('rocpd_info_kernel_symbol')][0]
    rows = cur.execute(f"select s.kernel_name, d.start, d.end - d.start from {kd} d join {ks} s on d.kernel_id = s.id order by d.start").fetchall()
    # the manifest lists EVERY search call of the run in order, the equality checks in front of each input too (check=True)
    seq = [(('beam_search_lm_kernel' in n), ns) for n, _, ns in rows if 'beam_search_kernel' in n or 'beam_search_lm_kernel' in n]
    assert len(seq) == len(calls), (len(seq), len(calls))
    best = {}
    for (is_lm, ns), c in zip(seq, calls):
        assert is_lm == c['lm'], (c, is_lm)
        if c.get('check'): continue
        key = (c['shape'], c['kind'], c['W'], c['lm'])
        if key not in best or ns < best[key][0]: best[key] = (ns, c)
    for (shape, kind, W, is_lm), (ts, c) in sorted(best.items(), key=lambda kv: (kv[0][0], kv[0][1], kv[0][2], kv[0][3])):
        if is_lm: continue
        tl = best[(shape, kind, W, True)][0]
        frames, kept = c['B'] * c['N'], c['frames_with_a_token']
        line = f'[{shape} {kind} W={W}] search LM-free {ts / 1e3:.1f} us | fused {tl / 1e3:.1f} us | ratio {tl / ts:.3f}'
        q0, q1 = best.get((shape, 'quiet', W, False)), best.get((shape, 'quiet', W, True))
        if q0 is not None and q1 is not None:
            pb0, pb1 = q0[0] / c['N'], q1[0] / c['N']
            line += f' | per frame without a token {pb0 / 1e3:.3f} / {pb1 / 1e3:.3f} us'
            if kind != 'quiet' and kept:
                pk0 = (ts - pb0 * (frames - kept) / c['B']) / (kept / c['B'])
                pk1 = (tl - pb1 * (frames - kept) / c['B']) / (kept / c['B'])
                line += f' | per frame with a selection {pk0 / 1e3:.3f} / {pk1 / 1e3:.3f} us (+{(pk1 - pk0) / 1e3:.3f} us, ratio {pk1 / pk0:.3f})'
        print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', choices=list(SHAPES) + ['all'], default='all')
    ap.add_argument('--kernels-only', action='store_true', help='per input the equality checks, then two calls per width and search, and no timing: for the kernel trace')
    ap.add_argument('--manifest', help='with --kernels-only: write the list of calls here; with --trace: read it')
    ap.add_argument('--trace', help='a rocprofv3 results database of a --kernels-only run: report per-kernel figures')
    ap.add_argument('--reps', type=int, default=0, help='calls per timing window (default: 5, 3 on the noise input)')
    ap.add_argument('--seed', type=int, default=0, help='seed of the synthetic trigram')
    a = ap.parse_args()
    report(a) if a.trace else run(a)


if __name__ == '__main__':
    main()
