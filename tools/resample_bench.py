"""Benchmark of the resampler (csrc/resample.hip through utils.audio_tools.resample): one hour of audio to 16 kHz.  Workloads: 44.1 kHz
mono, 44.1 kHz stereo mixed to the channel mean in the same pass, 48 kHz mono and 48 kHz stereo mean.  Device events after warm-up,
ROUNDS rounds of enough repetitions for a window of at least half a second each.

Per workload: ms (median and spread over the rounds), achieved bytes/s over the algorithmic bytes (every input channel read once,
the output written once), that rate as a share of the measured 6.29 TB/s, and the peak of torch.cuda.max_memory_allocated above
the input, asserted to be the output alone (no workspace, no mono copy).  The baseline is what the package asked its users to do
before: the f32 restatement of torchaudio's Resample (conv1d with the dense (P, 1, 2 width + O) kernel at stride O) on the host's
threads, on the same input (the first BASELINE_SECONDS of it, scaled to the hour; the host copy of the result is not counted).
Usage:  python tools/resample_bench.py [44100-mono] [44100-stereo] [48000-mono] [48000-stereo]      (prints one JSON line each)"""
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from lcasr_amd.utils import audio_tools as A

HBM = 6.29e12
WORKLOADS = {'44100-mono': (44100, 1), '44100-stereo': (44100, 2), '48000-mono': (48000, 1), '48000-stereo': (48000, 2)}
ROUNDS = int(os.environ.get('ROUNDS', '5'))
BASELINE_SECONDS = int(os.environ.get('BASELINE_SECONDS', '600'))


def host_resample(x, orig, new):
    """torchaudio.transforms.Resample(orig, new) in f32 on the CPU: x (1, L) -> (1, ceil(new L / orig))."""
    g = math.gcd(orig, new)
    O, P = orig // g, new // g
    base = min(O, P) * A.ROLLOFF
    width = math.ceil(A.LOWPASS_FILTER_WIDTH * O / base)
    idx = torch.arange(-width, width + O, dtype=torch.float64)[None] / O
    t = ((torch.arange(0, -P, -1, dtype=torch.float64)[:, None] / P + idx) * base).clamp(-A.LOWPASS_FILTER_WIDTH, A.LOWPASS_FILTER_WIDTH)
    k = torch.cos(t * math.pi / A.LOWPASS_FILTER_WIDTH / 2) ** 2 * (base / O)
    t = t * math.pi
    k = (k * torch.where(t == 0, torch.ones_like(t), t.sin() / t)).float()
    y = torch.nn.functional.conv1d(torch.nn.functional.pad(x, (width, width + O))[:, None], k[:, None], stride=O)
    return y.transpose(1, 2).reshape(1, -1)[:, :-(-(P * x.shape[1]) // O)]


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    for name in [a for a in sys.argv[1:] if a in WORKLOADS] or list(WORKLOADS):
        sr, channels = WORKLOADS[name]
        L = 3600 * sr
        wave = torch.empty(channels, L, device='cuda').uniform_(-0.3, 0.3)
        mix = 'mean' if channels > 1 else None
        fn = lambda: A.resample(wave, sr, A.SR, mix=mix)
        L_out = int(A.resampled_lengths(L, sr, A.SR))
        algo = 4 * channels * L + 4 * L_out
        # parity with the baseline on the first seconds, and the baseline's time
        n = BASELINE_SECONDS * sr
        head = wave[:, :n].cpu()
        mono = head.mean(0, keepdim=True) if channels > 1 else head
        t0 = time.perf_counter()
        ref = host_resample(mono, sr, A.SR)
        host_ms = (time.perf_counter() - t0) * 1e3
        got = A.resample(wave[:, :n].contiguous(), sr, A.SR, mix=mix).reshape(1, -1)
        diff = float((got.cpu() - ref).abs().max())
        del got, ref, head, mono
        for _ in range(3): fn()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        assert tuple(out.shape)[-1] == L_out and 4 * L_out <= peak <= 4 * L_out + (2 << 20), (peak, L_out)     # the allocator rounds large blocks to 2 MiB
        del out
        reps = max(2, int(500.0 / timed(fn, 2)) + 1)
        ms = [timed(fn, reps) for _ in range(ROUNDS)]
        med = statistics.median(ms)
        res = {'workload': name, 'sample_rate': sr, 'channels': channels, 'L': L, 'L_out': L_out, 'algorithmic_bytes': algo, 'rounds': ROUNDS,
               'reps': reps, 'ms': round(med, 4), 'ms_min': round(min(ms), 4), 'ms_max': round(max(ms), 4),
               'bytes_per_s': round(algo / (med * 1e-3), 1), 'share_of_6.29TBps': round(algo / (med * 1e-3) / HBM, 4),
               'peak_bytes_above_input': peak, 'host_threads': torch.get_num_threads(), 'host_f32_conv1d_ms_per_hour': round(host_ms * 3600 / BASELINE_SECONDS, 1),
               'host_seconds_measured': BASELINE_SECONDS, 'max_abs_diff_vs_host': diff,
               'speedup_vs_host': round(host_ms * 3600 / BASELINE_SECONDS / med, 1)}
        print(json.dumps(res), flush=True)
        del wave


if __name__ == '__main__':
    main()
