"""Benchmark of the posterior unit (csrc/post.hip through lcasr_amd.hip.post).

At (B, T, L, C) = (1, 2048, 600, 129) and (8, 2048, 600, 129) - a 2048-frame window with 600 labels, rows peaky along a sampled
alignment as tests/post_refs.parity_case makes them - the time of each of the three launches (lattice, neighbours, slots; the op
layer's allocations included, as a caller pays them), and as a yardstick one sconf_ctc_fwd (ops.ctc_fwd) of the same batch on the
same machine in the same process; that entry point takes class counts that are multiples of 4, so it runs on the same rows widened
to 132 columns.  Per figure: ms, the median of ROUNDS windows of at least WINDOW_MS each, device events after warm-up; for the
neighbours also the chain steps (the frames each chain visits, summed) per second.
Usage:  python tools/post_bench.py      (prints one JSON line per figure)"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch

import post_refs as PR
from lcasr_amd.hip import ops
from lcasr_amd.hip import post as K

ROUNDS = int(os.environ.get('ROUNDS', '5'))
WINDOW_MS = float(os.environ.get('WINDOW_MS', '300'))
SHAPES = ((1, 2048, 600, 129), (8, 2048, 600, 129))


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def chain_steps(T, L, C):
    """Frames visited by the chains of one sample: slot i and gap j start at frame i / j and end L - 1 - i / L - j frames before the
    last, but for the two rows that run to the end."""
    sub = sum(max(T - 1 - (L - 2 - i) - i, 0) if i < L - 1 else T - i for i in range(L))
    ins = sum(max(T - 1 - (L - 1 - j) - j, 0) if j < L else T - j for j in range(L + 1))
    return (sub + ins) * C


def main():
    for B, T, L, C in SHAPES:
        lp, tg, il, tl, blank = PR.parity_case([(T, L)] * B, C, 7, pad_frames=0, pad_labels=0)
        dev = [torch.from_numpy(a).cuda() for a in (lp, tg, il, tl)]
        wide = torch.full((B, T, 132), -30.0, dtype=torch.float32, device='cuda')
        wide[:, :, :C] = torch.nan_to_num(dev[0], neginf=-30.0)             # (the loss kernel's time does not depend on the values)
        lat = K.lattice(*dev, blank)
        sub, ins = K.neighbours(*dev, blank, lat)
        assert bool(torch.isfinite(lat.loglik).all()) and not bool(torch.isnan(sub).any())
        fns = {'lattice': lambda: K.lattice(*dev, blank), 'neighbours': lambda: K.neighbours(*dev, blank, lat),
               'slots': lambda: K.slots(sub, ins, dev[1], blank), 'ctc_fwd': lambda: ops.ctc_fwd(wide, dev[1], dev[2], dev[3], 131)}
        for name, fn in fns.items():
            for _ in range(3): fn()
            torch.cuda.synchronize()
            reps = max(1, int(WINDOW_MS / timed(fn, 1)))
            ms = [timed(fn, reps) for _ in range(ROUNDS)]
            row = {'bench': 'post', 'B': B, 'T': T, 'L': L, 'C': C, 'launch': name, 'ms': round(statistics.median(ms), 4),
                   'ms_min': round(min(ms), 4), 'ms_max': round(max(ms), 4), 'reps': reps}
            if name == 'neighbours':
                row['chain_steps'] = B * chain_steps(T, L, C)
                row['steps_per_s'] = round(row['chain_steps'] / (row['ms'] * 1e-3), 0)
            if name == 'lattice':
                row['workspace_bytes'] = K.workspace_bytes(B, T, L)
            print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
