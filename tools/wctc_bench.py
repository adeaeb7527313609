"""Micro-benchmark of the wild-card CTC loss (sconf_wctc_fwd / sconf_wctc_bwd, all three modes) with the CTC kernels (sconf_ctc_fwd /
sconf_ctc_bwd) timed at the same shapes in the same process as the yardstick: B = 128, N = 2048, C = 144, Smax = 256 and 512
(DESIGN.md §19).  HIP events; the rounds alternate between the operators so that a drift of the machine shows in all of them.
`--rounds R --iters I`; `--kernels-only` runs each operator a few times without timing, for `rocprofv3 --kernel-trace --stats`,
whose per-kernel time of wctc_grad_kernel gives the gradient pass's achieved bytes/s (the bytes are printed here)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import lcasr_amd.hip.ops as ops
from lcasr_amd.hip import wctc

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--iters', type=int, default=5)
ap.add_argument('--kernels-only', action='store_true')
args = ap.parse_args()
B, N, C = 128, 2048, 144


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


for S in (256, 512):
    g = torch.Generator().manual_seed(S)
    lp = torch.log_softmax(torch.randn(B, N, C, generator=g), -1).cuda()
    tg = torch.randint(0, C - 1, (B, S), generator=g, dtype=torch.int32).cuda()
    il = torch.full((B,), N, device='cuda', dtype=torch.int32); tl = torch.full((B,), S, device='cuda', dtype=torch.int32)
    blank = C - 1
    work = {}
    nll, ws = ops.ctc_fwd(lp, tg, il, tl, blank)
    work['ctc fwd'] = lambda: ops.ctc_fwd(lp, tg, il, tl, blank)
    work['ctc bwd'] = lambda nll=nll, ws=ws: ops.ctc_bwd(lp, ws, nll, tg, il, tl, None, blank)
    for mode in wctc.MODES:
        _, w = wctc.wctc_fwd(lp, tg, il, tl, blank, mode)
        work[f'wctc {mode} fwd'] = lambda mode=mode: wctc.wctc_fwd(lp, tg, il, tl, blank, mode)
        work[f'wctc {mode} bwd'] = lambda mode=mode, w=w: wctc.wctc_bwd(lp.shape, w, tg, il, tl, None, blank, mode)
    for fn in work.values():                                     # warm-up: code objects, the allocator's blocks
        fn(); fn()
    torch.cuda.synchronize()
    W = 2 * S + 1
    grad_bytes = B * N * (W * 4 + C * 4) + B * S * 4
    print(f'S = {S}: the gradient pass (wctc_grad_kernel) moves {grad_bytes} bytes: the products (B, N, {W}) f32 in, grad (B, N, {C}) f32 out; '
          f'workspace {wctc.workspace_bytes(B, N, S, "soft")} bytes')
    if args.kernels_only:
        continue
    times = {k: [] for k in work}
    for _ in range(args.rounds):
        for k, fn in work.items():
            times[k].append(timed(fn, args.iters))
    for k, v in times.items():
        print(f'S = {S}: {k:22s} {min(v):8.3f} ms (rounds: {" ".join(f"{x:.3f}" for x in v)})')
    ctc = min(times['ctc fwd']) + min(times['ctc bwd'])
    for mode in wctc.MODES:
        tot = min(times[f'wctc {mode} fwd']) + min(times[f'wctc {mode} bwd'])
        print(f'S = {S}: wctc {mode} fwd + bwd {tot:.3f} ms = {tot / ctc:.2f} x ctc fwd + bwd ({ctc:.3f} ms)')
