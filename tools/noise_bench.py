"""Benchmark of the noise corruption (csrc/noise.hip through lcasr_amd.hip.noise): the three kernels on one row of 57.6 M samples (one
hour at 16 kHz) and on a batch of 128 x 256000, the Gaussian mix at K = 1, 4 and 8 levels per launch, the background mix at K = 1
with a 10 s clip that wraps.  Device events after warm-up; ROUNDS rounds that alternate between the kernels of a workload, each of
enough repetitions for a window of about a fifth of a second.

Per kernel: ms (median and spread over the rounds), achieved bytes/s over the algorithmic bytes (the waveform read once, every
level written once; the power pass reads only), and that rate as a share of the measured 6.29 TB/s.  `sweep` times the corruption
step of eval.run.snr_sweep for K = 8 on the hour (one power pass, one mix launch) beside what the package asked its users to do
before, per level: copy the waveform to the host, draw the normals and mix in numpy there, copy the result back.
Usage:  python tools/noise_bench.py [hour] [batch] [sweep]      (prints one JSON line per kernel)"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from lcasr_amd.hip import noise as N
from lcasr_amd.utils import audio_tools as A

HBM = 6.29e12
WORKLOADS = {'hour': (1, 3600 * 16000), 'batch': (128, 256000)}
ROUNDS = int(os.environ.get('ROUNDS', '5'))
WINDOW_MS = float(os.environ.get('WINDOW_MS', '200'))


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernels_of(B, L):
    wave = torch.empty(B, L, device='cuda').uniform_(-0.3, 0.3)
    clip = torch.empty(160000, device='cuda').uniform_(-0.1, 0.1)[None]
    zero = torch.zeros(B, dtype=torch.int64, device='cuda')
    p = N.power(wave)
    pv = N.power(clip, None, None, zero, L=L, B=B)
    snr = {K: torch.linspace(0.0, 30.0, K, device='cuda')[None].expand(B, -1).contiguous() for K in (1, 4, 8)}
    fns = {'power': (lambda: N.power(wave), 4 * B * L),
           'power_wrapped_clip': (lambda: N.power(clip, None, None, zero, L=L, B=B), 4 * B * L),
           'background_K1': (lambda: N.add_background(wave, None, clip, None, zero, p, pv, snr[1]), 8 * B * L)}
    for K in (1, 4, 8):
        fns[f'gaussian_K{K}'] = (lambda K=K: N.add_gaussian(wave, None, p, snr[K], 17925), 4 * B * L * (1 + K))
    return fns


def bench(name):
    B, L = WORKLOADS[name]
    fns = kernels_of(B, L)
    reps = {}
    for k, (fn, _) in fns.items():
        for _ in range(3): fn()
        reps[k] = max(2, int(WINDOW_MS / timed(fn, 2)) + 1)
    ms = {k: [] for k in fns}
    for _ in range(ROUNDS):                                                # alternating: every kernel once per round
        for k, (fn, _) in fns.items():
            ms[k].append(timed(fn, reps[k]))
    for k, (fn, algo) in fns.items():
        med = statistics.median(ms[k])
        print(json.dumps({'workload': name, 'kernel': k, 'B': B, 'L': L, 'algorithmic_bytes': algo, 'rounds': ROUNDS, 'reps': reps[k],
                          'ms': round(med, 4), 'ms_min': round(min(ms[k]), 4), 'ms_max': round(max(ms[k]), 4),
                          'GB_per_s': round(algo / (med * 1e-3) / 1e9, 1), 'share_of_6.29TBps': round(algo / (med * 1e-3) / HBM, 4)}), flush=True)


def sweep():
    L, K = WORKLOADS['hour'][1], 8
    x = torch.empty(L, device='cuda').uniform_(-0.3, 0.3)
    snrs = [float(s) for s in np.linspace(0.0, 35.0, K)]
    fn = lambda: A.add_gaussian_snr(x, snrs)
    for _ in range(3): fn()
    reps = max(2, int(WINDOW_MS / timed(fn, 2)) + 1)
    ms = [timed(fn, reps) for _ in range(ROUNDS)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for snr in snrs:                                                       # the host detour, per level as the reference's drivers run it
        h = x.cpu().numpy()
        sigma = np.sqrt(np.mean(h.astype(np.float64) ** 2)) * 10.0 ** (-snr / 20.0)
        y = h + np.random.default_rng(17925).normal(0.0, sigma, size=L).astype(np.float32)
        torch.from_numpy(y).cuda()
    torch.cuda.synchronize()
    host_ms = (time.perf_counter() - t0) * 1e3
    med = statistics.median(ms)
    print(json.dumps({'workload': 'sweep', 'L': L, 'K': K, 'rounds': ROUNDS, 'reps': reps, 'device_ms': round(med, 4), 'device_ms_min': round(min(ms), 4),
                      'device_ms_max': round(max(ms), 4), 'host_numpy_ms_with_copies': round(host_ms, 1), 'host_threads': torch.get_num_threads(),
                      'speedup_vs_host': round(host_ms / med, 1)}), flush=True)


def main():
    for name in [a for a in sys.argv[1:] if a in WORKLOADS or a == 'sweep'] or list(WORKLOADS) + ['sweep']:
        sweep() if name == 'sweep' else bench(name)
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
