"""Benchmark of the calibration unit (csrc/calib.hip through lcasr_amd.hip.calib).

align   sconf_edit_align on one pair of n x n ids with 10 % edits, n = 2500, 5000, 10000, 30000, beside sconf_edit_counts on the same
        buffers (the same DP without storing its directions or walking back).  Per size: ms (median of ROUNDS), DP cells per second of
        the whole call, the workspace bytes, the ratio to sconf_edit_counts.  From the four sizes a least-squares fit
        ms = a n^2 + b n + c: b n is what grows with H + R, the backtrace together with the per-row costs of the forward pass, an upper
        bound of the backtrace's share.  The host path the kernel replaces - the cell-by-cell Python DP of tests/calib_refs.py - is timed
        at HOST_N x HOST_N and scaled by cells.
sweep   sconf_calib_frames_sweep at K = 1, 4, 16 over an hour of frames (45000 rows) at 144 and 4096 classes, beside K launches of
        sconf_confid_frames, each on a buffer of its own as K scaled copies would be (the pass that would make the copies, one read
        and one write of x per temperature, is not timed: the time of a launch does not depend on the values).  Buffers smaller than
        the last-level cache are rotated over 768 MB, as tools/confid_bench.py does, for both.  Per K: ms, bytes/s over one read of x plus the
        outputs, that rate as a share of the measured 6.3 TB/s, and the ratio to the K launches.
Device events after warm-up.  Usage:  python tools/calib_bench.py [align] [sweep]      (prints one JSON line per figure)"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch

import calib_refs as AR
from lcasr_amd.hip import calib as K
from lcasr_amd.hip import confid, ops

HBM = 6.3e12
ROUNDS = int(os.environ.get('ROUNDS', '5'))
WINDOW_MS = float(os.environ.get('WINDOW_MS', '200'))
HOST_N = int(os.environ.get('HOST_N', '300'))
COLD_BYTES = 768 << 20
SIZES = (2500, 5000, 10000, 30000)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def align():
    rows = []
    for n in SIZES:
        hyp, ref = AR.pair_case('edits', n, n, seed=n)
        dev = [torch.from_numpy(a).cuda() for a in (hyp, np.array([0, n], dtype=np.int64), ref, np.array([0, n], dtype=np.int64))]
        nbytes = K.pair_bytes(n, n)
        wo = torch.tensor([0, nbytes], dtype=torch.int64, device='cuda')
        ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
        fns = {'edit_align': lambda: K.edit_align(*dev, wo, ws), 'edit_counts': lambda: ops.edit_counts(*dev)}
        assert torch.equal(fns['edit_align']()[2], fns['edit_counts']())
        reps = {k: max(1, int(WINDOW_MS / timed(fn, 1))) for k, fn in fns.items()}
        ms = {k: [] for k in fns}
        for _ in range(ROUNDS):
            for k, fn in fns.items(): ms[k].append(timed(fn, reps[k]))
        a, c = statistics.median(ms['edit_align']), statistics.median(ms['edit_counts'])
        rows.append((n, a))
        print(json.dumps({'workload': 'align', 'n': n, 'edits': int(fns['edit_counts']()[0, 0]), 'workspace_bytes': nbytes, 'rounds': ROUNDS,
                          'edit_align_ms': round(a, 3), 'edit_align_ms_min': round(min(ms['edit_align']), 3), 'edit_align_ms_max': round(max(ms['edit_align']), 3),
                          'edit_counts_ms': round(c, 3), 'cells_per_s': round(n * n / (a * 1e-3), 0), 'times_edit_counts': round(a / c, 3)}), flush=True)
        del ws
        torch.cuda.empty_cache()
    n, t = np.array([r[0] for r in rows], dtype=np.float64), np.array([r[1] for r in rows])
    (qa, qb, qc), *_ = np.linalg.lstsq(np.stack([n * n, n, np.ones_like(n)], axis=1), t, rcond=None)
    hyp, ref = AR.pair_case('edits', HOST_N, HOST_N, seed=1)
    t0 = time.perf_counter(); AR.align_plain(hyp.tolist(), ref.tolist()); host = time.perf_counter() - t0
    for size, ms in rows:
        print(json.dumps({'workload': 'align_fit', 'n': size, 'ms': round(ms, 3), 'fit_ms_per_cell': qa, 'fit_ms_per_id': qb, 'fit_ms_const': qc,
                          'linear_share': round(qb * size / ms, 4), 'host_python_n': HOST_N, 'host_python_s': round(host, 3),
                          'host_python_cells_per_s': round(HOST_N * HOST_N / host, 0),
                          'host_scaled_s': round(host * size * size / (HOST_N * HOST_N), 1),
                          'times_faster_than_host': round(host * size * size / (HOST_N * HOST_N) / (ms * 1e-3), 0)}), flush=True)


def sweep():
    M = 45000
    for C in (144, 4096):
        copies = max(1, -(-COLD_BYTES // (4 * M * C))) if 4 * M * C < COLD_BYTES else 1
        bufs = [torch.randn(M, C, device='cuda') * 3 for _ in range(copies)]
        turn = [0]

        def buf():
            turn[0] = (turn[0] + 1) % len(bufs)
            return bufs[turn[0]]

        for Kn in (1, 4, 16):
            temps = [1.0] + [0.5 + 0.15 * k for k in range(Kn - 1)]
            inv = torch.tensor([1.0 / t for t in temps], dtype=torch.float32, device='cuda')
            for name, (method, norm) in {'max_prob': ('max_prob', 'lin'), 'tsallis_1/3': ('tsallis', 'exp')}.items():
                fns = {'sweep': lambda: K.frames_sweep(buf(), inv, C, method, norm, 1.0 / 3.0),
                       'separate': lambda: [confid.frames(buf(), C, method, norm, 1.0 / 3.0) for _ in range(Kn)]}
                reps = {}
                for k, fn in fns.items():
                    for _ in range(2): fn()
                    reps[k] = max(copies, int(WINDOW_MS / timed(fn, max(2, copies))) + 1)
                ms = {k: [] for k in fns}
                for _ in range(ROUNDS):
                    for k, fn in fns.items(): ms[k].append(timed(fn, reps[k]))
                med, algo = statistics.median(ms['sweep']), 4 * M * C + 4 * M * (Kn + 1)
                sep = statistics.median(ms['separate'])
                print(json.dumps({'workload': 'sweep', 'M': M, 'classes': C, 'K': Kn, 'measure': name, 'buffers': copies, 'rounds': ROUNDS,
                                  'sweep_ms': round(med, 4), 'sweep_ms_min': round(min(ms['sweep']), 4), 'sweep_ms_max': round(max(ms['sweep']), 4),
                                  'GB_per_s': round(algo / (med * 1e-3) / 1e9, 1), 'share_of_6.3TBps': round(algo / (med * 1e-3) / HBM, 4),
                                  'separate_launches_ms': round(sep, 4), 'separate_over_sweep': round(sep / med, 3)}), flush=True)
        del bufs
        torch.cuda.empty_cache()


def main():
    for name in [a for a in sys.argv[1:] if a in ('align', 'sweep')] or ['align', 'sweep']:
        {'align': align, 'sweep': sweep}[name]()


if __name__ == '__main__':
    main()
