"""Benchmark of CTC keyword search (csrc/kws.hip through lcasr_amd.hip.kws): what does the one pass over the log-scores cost, what
does the serial walk cost per frame, and what does packing keywords into lanes buy?

One hour at 8x subsampling, (N, C) = (45000, 144) and (45000, 4096), 1000 keywords of 2 - 6 labels.  Whole-call timings with device
events, in one process, in ROUNDS that alternate the variants (so that clock and cache drift hit all of them alike); the figure of a
variant is the median over the rounds and the spread is max - min of its rounds:

  packed     the image of KeywordSet(phrases): keywords end to end in the lanes of a wave
  unpacked   the same code with one_per_wave=True: every keyword in a wave of its own
  gather     the packed call with input_lengths = 0: the gather works on every frame (it does not look at the lengths), the walk
             only fills its slots, so this is the gather and two launches; packed - gather is the walk over the N frames

The gather's rate is taken over its algorithmic bytes, 4 N (classes + Upad), beside the 6.3 TB/s the project takes as achievable.
The outputs of packed and unpacked are compared bit for bit.
Usage:  python tools/kws_bench.py [--classes 144 4096] [--keywords 1000] [--rounds 7] [--reps 5]      (one JSON line per shape)"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from lcasr_amd.decoding.kws import KeywordSet
from lcasr_amd.hip import kws as K

N = 45000
HBM = 6.3e12


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--classes', type=int, nargs='+', default=[144, 4096])
    ap.add_argument('--keywords', type=int, default=1000)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    for C in a.classes:
        rng = np.random.default_rng(C)
        blank = C - 1
        phrases = [tuple(int(c) for c in rng.integers(0, blank, size=int(rng.integers(2, 7)))) for _ in range(a.keywords)]
        packed, unpacked = KeywordSet(phrases, -1.0), KeywordSet(phrases, -1.0, one_per_wave=True)
        g = torch.Generator(device='cuda').manual_seed(C)
        x = torch.log_softmax(torch.randn(1, N, C, generator=g, device='cuda') * 3, -1).contiguous()     # peaked rows, as a trained model's
        zero = torch.zeros(1, dtype=torch.int32, device='cuda')
        call = lambda ks, il=None: K.search(x, ks.device_image('cuda'), ks.n_waves, ks.U, ks.K, blank, il, 16)
        variants = {'packed': lambda: call(packed), 'unpacked': lambda: call(unpacked), 'gather': lambda: call(packed, zero)}
        out_p, out_u = call(packed), call(unpacked)
        same = all(torch.equal(p.view(torch.int32) if p.is_floating_point() else p, q.view(torch.int32) if q.is_floating_point() else q)
                   for p, q in zip(out_p, out_u))
        for fn in variants.values():
            for _ in range(2): fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items(): times[k].append(timed(fn, a.reps))
        med = {k: statistics.median(v) for k, v in times.items()}
        spread = {k: max(v) - min(v) for k, v in times.items()}
        bytes_ = 4 * N * (C + (packed.U + 3) // 4 * 4)
        walk, walk_u = med['packed'] - med['gather'], med['unpacked'] - med['gather']
        print(json.dumps({'N': N, 'classes': C, 'keywords': a.keywords, 'labels': sum(len(p) for p in phrases), 'U': packed.U,
                          'rounds': a.rounds, 'reps': a.reps, 'waves_packed': packed.n_waves, 'waves_unpacked': unpacked.n_waves,
                          'bits_equal': bool(same), 'hits': int(out_p.hit_count.sum()),
                          'call_ms': {k: round(v, 4) for k, v in med.items()}, 'spread_ms': {k: round(v, 4) for k, v in spread.items()},
                          'gather_bytes': bytes_, 'gather_TBps': round(bytes_ / (med['gather'] * 1e-3) / 1e12, 3),
                          'gather_of_achievable': round(bytes_ / (med['gather'] * 1e-3) / HBM, 3),
                          'walk_ms_packed': round(walk, 4), 'walk_ms_unpacked': round(walk_u, 4),
                          'walk_us_per_frame_packed': round(walk * 1e3 / N, 4), 'walk_us_per_frame_unpacked': round(walk_u * 1e3 / N, 4),
                          'unpacked_over_packed_walk': round(walk_u / walk, 3) if walk > 0 else None}), flush=True)
        del x, out_p, out_u
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
