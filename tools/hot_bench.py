"""Micro-benchmark of the beam search with hotword boosting (sconf_hot_beam_ctc) beside the search with an n-gram LM alone
(sconf_lm_beam_ctc), a sibling of tools/lm_beam_bench.py: one recording of N = 16384 frames, C = 144 classes, beam width 100,
max_tokens_per_frame 16, on the 'spiky' and 'noise' inputs of tools/beam_bench.py.  Four searches with the SAME LM (a synthetic
trigram over 143 tokens, lm_beam_bench's builder): the LM search, and the hotword search with 0, 10 and 1000 phrases of 1 to 6 seeded
tokens (0 phrases: an image of the root alone - no walk is taken - so this column shows what the larger kernel costs by itself).

Whole calls between HIP events, output allocation included.  All four are timed in ONE run, alternating: `--rounds` rounds of
LM / 0 / 10 / 1000, each window `--reps` calls after two warm-up calls; reported per search are the median and the least window,
the ratio of medians to the LM search, and the spread (largest - least window) of each search over the rounds, which is what a
difference has to exceed to mean anything.  Before timing, the hotword search at weight 0 must return the LM search's six outputs bit
for bit, and the boosted searches report how many hotword tokens their best hypothesis was credited with."""
import argparse
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import beam_bench as BB                                                    # the inputs and the timer
import lm_beam_bench as LB                                                 # the synthetic trigram

N, C, W, KMAX = 16384, 144, 100, 16
ALPHA, BETA, WEIGHT = 0.5, 1.5, 10.0
COUNTS = (0, 10, 1000)


def lm_over(V, seed):
    """lm_beam_bench's synthetic trigram over V tokens: every token 40 bigram children, every bigram 3 trigram children."""
    saved = LB.V, LB.BIGRAMS_PER_TOKEN, LB.TRIGRAMS_PER_BIGRAM
    LB.V, LB.BIGRAMS_PER_TOKEN, LB.TRIGRAMS_PER_BIGRAM = V, 40, 3
    try:
        return LB.synthetic_trigram(seed)
    finally:
        LB.V, LB.BIGRAMS_PER_TOKEN, LB.TRIGRAMS_PER_BIGRAM = saved


def phrases(n, V, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    return [tuple(int(c) for c in rng.integers(0, V, int(rng.integers(1, 7)))) for _ in range(n)]


def run(a):
    import torch
    import lcasr_amd.hip.hot as H
    import lcasr_amd.hip.lm as L
    from lcasr_amd.decoding.hotwords import HotwordSet
    V = C - 1
    lm = lm_over(V, a.seed)
    sets = {n: HotwordSet(phrases(n, V, a.seed + n)) for n in COUNTS}
    print(f'[hot] LM image {lm.image.nbytes} bytes ({lm.n_states} states); hotword images: ' +
          ', '.join(f'{n} phrases {s.image.nbytes} bytes ({s.n_states} states, longest {s.max_len})' for n, s in sets.items()))
    for kind in a.kinds:
        lp = BB.inputs(kind, 1, N, C)
        im = lm.device_image(lp.device)
        lm_args = (im, lm.n_states, lm.n_entries, lm.num_tokens, lm.order, lm.start_state)
        tail = (C - 1, W, 1, -5.0, -10.0, KMAX, N, ALPHA, BETA)
        fused = lambda: L.ctc_beam_lm(lp, None, *lm_args, *tail)
        hot = lambda n, w=WEIGHT: H.ctc_beam_hot(lp, None, *lm_args, sets[n].device_image(lp.device), sets[n].n_states, sets[n].n_entries,
                                                 sets[n].max_len, w, *tail)
        x, y = fused(), hot(1000, 0.0)
        assert all(torch.equal(p.view(torch.uint8), q.view(torch.uint8)) for p, q in zip(x, y[:6])), \
            f'{kind}: the hotword search at weight 0 is not the LM search'
        kept = BB.frames_with_a_token(lp, C - 1)
        credit = {n: float(hot(n).hot_scores[0, 0]) for n in COUNTS}
        print(f'[{kind}] N={N} C={C} W={W} Kmax={KMAX}: {kept} frames keep a token; best hypothesis {int(x.lengths[0, 0])} tokens; hotword credit of '
              f'the best hypothesis at weight {WEIGHT}: ' + ', '.join(f'{n} phrases {credit[n]:.1f}' for n in COUNTS) +
              f'; workspace {H.beam_workspace(1, N, W, KMAX)} bytes')
        names = ['lm'] + [f'hot-{n}' for n in COUNTS]
        calls = {'lm': fused, **{f'hot-{n}': (lambda n=n: hot(n)) for n in COUNTS}}
        times = {k: [] for k in names}
        for _ in range(a.rounds):
            for k in names:
                times[k].append(BB.timed(calls[k], a.reps))
        base = statistics.median(times['lm'])
        for k in names:
            t = times[k]
            print(f'[{kind}] {k:9s} median {statistics.median(t):8.3f} ms | least {min(t):8.3f} ms | spread {max(t) - min(t):6.3f} ms over {a.rounds} '
                  f'rounds of {a.reps} calls | median / LM median {statistics.median(t) / base:.3f}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kinds', nargs='+', choices=BB.KINDS, default=['spiky', 'noise'])
    ap.add_argument('--rounds', type=int, default=5, help='alternating rounds of the four searches')
    ap.add_argument('--reps', type=int, default=3, help='calls per timing window')
    ap.add_argument('--seed', type=int, default=0, help='seed of the synthetic trigram and of the phrases')
    run(ap.parse_args())


if __name__ == '__main__':
    main()
