"""Benchmark of the audio front end (csrc/audio.hip through utils.audio_tools.to_spectogram) beside the torch composite on the same
device: torch.stft, the power, the matmul with the same filterbank and the mean / std normalisation.  Two workloads: one one-hour
recording (B = 1, L = 57 600 000) and the benchmark's training shape (B = 128, L = 16384 * 160).  Device events after warm-up; the
two paths alternate inside one call, ROUNDS rounds of enough repetitions for a window of at least a second per path and workload.

Per path: ms (median and spread over the rounds), achieved bytes/s over the algorithmic bytes (4 L in, one write of the output, one
re-read and re-write for the normalisation), that rate as a share of the measured 6.29 TB/s, and the peak of
torch.cuda.max_memory_allocated above the input.  The fused path's peak is asserted to be the output plus the queried workspace.
If torch.stft does not run on the device, the tool says so and reports the fused path alone.
Usage:  python tools/melspec_bench.py [hour] [train]      (ROUNDS=5; prints one JSON line per workload)"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from lcasr_amd.hip import audio
from lcasr_amd.utils import audio_tools as A

HBM = 6.29e12
SHAPES = {'hour': (1, 57_600_000), 'train': (128, 16384 * 160)}
ROUNDS = int(os.environ.get('ROUNDS', '5'))


def composite(wave, fb, window):
    st = torch.stft(wave, 512, hop_length=160, win_length=400, window=window, center=True, pad_mode='reflect', normalized=False,
                    onesided=True, return_complex=True)
    spec = torch.matmul(st.abs().pow(2).transpose(1, 2), fb).transpose(1, 2)
    return (spec - spec.mean(-1, keepdim=True)) / spec.std(-1, keepdim=True)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def peak_above(fn, base):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def main():
    for name in [a for a in sys.argv[1:] if a in SHAPES] or list(SHAPES):
        B, L = SHAPES[name]
        T = 1 + L // 160
        wave = torch.empty(B, L, device='cuda').uniform_(-0.3, 0.3)
        fb, _ = A._device_tables(wave.device, 80)
        window = torch.hann_window(400, periodic=True, device='cuda')
        out_bytes, ws_bytes = B * 80 * T * 4, audio.melspec_workspace(B, T, 80)
        algo = 4 * B * L + 3 * out_bytes
        paths = {'fused': lambda: A.to_spectogram(wave)}
        try:
            ref = composite(wave, fb, window)
            got = A.to_spectogram(wave)
            diff = float((got - ref).abs().max())
            del ref, got
            paths['composite'] = lambda: composite(wave, fb, window)
        except RuntimeError as e:
            diff = None
            print(f'[melspec_bench] {name}: torch.stft did not run on the device ({str(e).splitlines()[0]}): composite not measured')
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        res = {'workload': name, 'B': B, 'L': L, 'T': T, 'output_bytes': out_bytes, 'workspace_bytes': ws_bytes, 'algorithmic_bytes': algo,
               'max_abs_diff_fused_vs_composite': diff, 'rounds': ROUNDS}
        reps = {}
        for k, fn in paths.items():
            for _ in range(2): fn()
            reps[k] = max(2, int(1000.0 / timed(fn, 2)) + 1)                      # a window of at least a second
        ms = {k: [] for k in paths}
        for _ in range(ROUNDS):                                                   # the paths alternate inside the call
            for k, fn in paths.items():
                ms[k].append(timed(fn, reps[k]))
        for k, fn in paths.items():
            med = statistics.median(ms[k])
            peak = peak_above(fn, base)
            res[k] = {'ms': round(med, 4), 'ms_min': round(min(ms[k]), 4), 'ms_max': round(max(ms[k]), 4), 'reps': reps[k],
                      'bytes_per_s': round(algo / (med * 1e-3), 1), 'share_of_6.29TBps': round(algo / (med * 1e-3) / HBM, 4),
                      'peak_bytes_above_input': peak}
        slack = 2 * 512                                                           # the allocator rounds each of the two blocks to 512 B
        assert out_bytes + ws_bytes <= res['fused']['peak_bytes_above_input'] <= out_bytes + ws_bytes + slack, \
            (res['fused']['peak_bytes_above_input'], out_bytes, ws_bytes)
        if 'composite' in res:
            res['speedup_median'] = round(res['composite']['ms'] / res['fused']['ms'], 2)
            res['speedup_worst_case'] = round(res['composite']['ms_min'] / res['fused']['ms_max'], 2)
        print(json.dumps(res))
        del wave


if __name__ == '__main__':
    main()
