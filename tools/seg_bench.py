"""Benchmark of CTC segmentation (csrc/seg.hip through lcasr_amd.hip.seg): what does the star cost?

Whole-call timings with device events, in one process, in the order A / B / A: sconf_align_ctc (A) and sconf_seg_align (B) on the
same log-probs at the two shapes of align_bench.py, (B=16, N=2048, S=512, C=4096) and (B=1, N=16384, S=4096, C=4096).  B's targets
are A's with every 16th label replaced by the star (and the first and last), so both walk lattices of the same size; B also
writes frame_logp.  The spread between the two A timings is the noise floor the difference B - A has to be read against.  Then
sconf_seg_score alone on B's outputs: one utterance per 16 labels, window 30.
Usage:  python tools/seg_bench.py [--shape bench|long|all] [--reps N]      (prints one JSON line per shape)"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from align_bench import SHAPES, inputs, timed
from lcasr_amd.hip import align as K
from lcasr_amd.hip import seg as KS

EVERY = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', choices=list(SHAPES) + ['all'], default='all')
    ap.add_argument('--reps', type=int, default=20)
    a = ap.parse_args()
    for name in (SHAPES if a.shape == 'all' else [a.shape]):
        B, N, S, C = SHAPES[name]
        lp, tg, il, tl = inputs(B, N, S, C)
        stars = tg.clone()
        stars[:, ::EVERY] = C
        stars[:, -1] = C
        plain = lambda: K.ctc_align(lp, tg, il, tl, C - 1)
        star = lambda: KS.align(lp, stars, il, tl, C - 1, -1.0)
        a0, b, a1 = timed(plain, a.reps), timed(star, a.reps), timed(plain, a.reps)
        same = all(torch.equal(x, y) for x, y in zip(KS.align(lp, tg, il, tl, C - 1, -1.0)[:5], plain()))       # no star: the same bits
        out = star()
        U = S // EVERY
        j0 = torch.arange(U, device='cuda', dtype=torch.int32) * EVERY + 1
        utt = torch.stack([j0, j0 + EVERY - 1], -1)[None].expand(B, U, 2).contiguous()
        score = lambda: KS.score(out.spans, out.frame_logp, out.score, il, tl, utt, None, 30)
        s = timed(score, 10 * a.reps)
        sc = score()
        print(json.dumps({'shape': name, 'B': B, 'N': N, 'S': S, 'C': C, 'reps': a.reps, 'stars_per_row': int((stars[0] == C).sum()),
                          'align_ms_first': round(a0, 4), 'seg_align_ms': round(b, 4), 'align_ms_second': round(a1, 4),
                          'aba_spread_ms': round(abs(a0 - a1), 4), 'star_minus_mean_align_ms': round(b - (a0 + a1) / 2, 4),
                          'no_star_bits_equal': bool(same), 'finite': bool(torch.isfinite(out.score).all()),
                          'utterances': B * U, 'seg_score_ms': round(s, 4), 'scores_finite': bool(torch.isfinite(sc.utt_conf).all())}), flush=True)
        del lp, out
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
