"""Benchmark of the confidence scores (csrc/confid.hip through lcasr_amd.hip.confid): sconf_confid_frames beside sconf_argmax_rows
on the same buffers - the argmax kernel reads the same bytes and is the natural floor - for (M, classes) = (45000, 144), one hour
of audio at 8x subsampling, (262144, 144) and (65536, 4096), with the measures max_prob, shannon and tsallis at alpha = 1/3.
Device events after warm-up; ROUNDS rounds that alternate between the kernels of a shape, each of enough repetitions for a window
of about a fifth of a second.  A shape smaller than the 256 MB last-level cache is timed over as many copies of the buffer as take
768 MB, visited in turn, so that every launch reads from HBM.

Per kernel: ms (median and spread over the rounds), achieved bytes/s over the algorithmic bytes (the rows read once; the outputs
are 4 or 8 bytes per row) and that rate as a share of the measured 6.3 TB/s.  `greedy` times decoding.confidence.greedy_confidence
end to end (three launches and one copy of the labels, spans and confidences to the host) beside the host collapse of
GreedyCTCDecoder.forward (argmax on the device, unique_consecutive(...).tolist() and the blank filter in Python) on the first shape.
Usage:  python tools/confid_bench.py [hour] [long] [wide] [greedy]      (prints one JSON line per kernel)"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from lcasr_amd.decoding.confidence import ConfidenceConfig, greedy_confidence
from lcasr_amd.decoding.greedy import GreedyCTCDecoder
from lcasr_amd.hip import confid as K
from lcasr_amd.hip import ops

HBM = 6.3e12
SHAPES = {'hour': (45000, 144), 'long': (262144, 144), 'wide': (65536, 4096)}
MEASURES = {'max_prob': ('max_prob', 'lin'), 'shannon': ('shannon', 'exp'), 'tsallis_1/3': ('tsallis', 'exp')}
ROUNDS = int(os.environ.get('ROUNDS', '5'))
WINDOW_MS = float(os.environ.get('WINDOW_MS', '200'))
COLD_BYTES = 768 << 20


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def bench(name):
    M, C = SHAPES[name]
    copies = max(1, -(-COLD_BYTES // (4 * M * C))) if 4 * M * C < COLD_BYTES else 1
    bufs = [torch.randn(M, C, device='cuda') * 3 for _ in range(copies)]
    turn = [0]

    def buf():
        turn[0] = (turn[0] + 1) % copies
        return bufs[turn[0]]

    fns = {'argmax_rows': lambda: ops.argmax_rows(buf())}
    for k, (method, norm) in MEASURES.items():
        fns['frames_' + k] = lambda method=method, norm=norm: K.frames(buf(), C, method, norm, 1.0 / 3.0)
    reps = {}
    for k, fn in fns.items():
        for _ in range(3): fn()
        reps[k] = max(copies, int(WINDOW_MS / timed(fn, max(2, copies))) + 1)
    ms = {k: [] for k in fns}
    for _ in range(ROUNDS):                                                # alternating: every kernel once per round
        for k, fn in fns.items():
            ms[k].append(timed(fn, reps[k]))
    floor = statistics.median(ms['argmax_rows'])
    for k in fns:
        med, algo = statistics.median(ms[k]), 4 * M * C + (4 if k == 'argmax_rows' else 8) * M
        print(json.dumps({'shape': name, 'kernel': k, 'M': M, 'classes': C, 'buffers': copies, 'algorithmic_bytes': algo, 'rounds': ROUNDS,
                          'reps': reps[k], 'ms': round(med, 4), 'ms_min': round(min(ms[k]), 4), 'ms_max': round(max(ms[k]), 4),
                          'GB_per_s': round(algo / (med * 1e-3) / 1e9, 1), 'share_of_6.3TBps': round(algo / (med * 1e-3) / HBM, 4),
                          'times_argmax_rows': round(med / floor, 3)}), flush=True)


def greedy():
    M, C = SHAPES['hour']
    x = torch.randn(M, C, device='cuda')
    t = torch.arange(M, device='cuda')                                     # as in a transcript: a label over two frames, then eight blanks
    label = torch.randint(0, C - 1, (M // 10 + 1,), device='cuda')[t // 10]
    x[t, torch.where(t % 10 < 2, label, torch.full_like(label, C - 1))] += 12
    cfg, dec = ConfidenceConfig(), GreedyCTCDecoder(blank_id=C - 1)

    def wall(fn, n=10):
        fn(); torch.cuda.synchronize()
        out = []
        for _ in range(n):
            t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return out
    a, b = wall(lambda: greedy_confidence(x, C - 1, cfg)), wall(lambda: dec(x, decode=False))
    tokens = len(dec(x, decode=False))
    assert greedy_confidence(x, C - 1, cfg).tokens == dec(x, decode=False)
    print(json.dumps({'shape': 'hour', 'workload': 'greedy', 'M': M, 'classes': C, 'tokens': tokens,
                      'greedy_confidence_ms': round(statistics.median(a), 3), 'greedy_confidence_ms_min': round(min(a), 3),
                      'host_collapse_ms': round(statistics.median(b), 3), 'host_collapse_ms_min': round(min(b), 3)}), flush=True)


def main():
    for name in [a for a in sys.argv[1:] if a in SHAPES or a == 'greedy'] or list(SHAPES) + ['greedy']:
        greedy() if name == 'greedy' else bench(name)
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
