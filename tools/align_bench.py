"""Micro-benchmark of CTC forced alignment (sconf_align_ctc) beside the CTC loss forward (ops.ctc_fwd) on the same inputs, in one
process, in the order A / B / A: ctc_fwd, align, ctc_fwd (HIP events around whole calls, output allocation included).  Shapes: the
one of ctc_bench.py (B=16, N=2048, S=512, C=4096) and the long lattice (B=1, N=16384, S=4096, C=4096).  The walk back is also timed
one frame per fetch (SCONF_ALIGN_WALK_WINDOW=1) against the windowed fetch.

Per-stage times (gather, lattice, walk back, frames + tokens; and the loss's own gather and lattice) come from the kernel trace:
    rocprofv3 --kernel-trace -d DIR -o kt -- python tools/align_bench.py --kernels-only [--shape long]
    python tools/rocpd_stats.py DIR/kt_results.db
The kernels are align_gather_kernel, align_lattice_kernel<MAXS, LT>, align_walk_kernel, align_frames_kernel, align_tokens_kernel,
ctc_gather_kernel and ctc_alphabeta_kernel<MAXS, LT>.

--long measures the long form (sconf_lalign_ctc, the lattice cut into state slabs launched one after the other) instead: at
B=1, N=16384, S=4096, the one shape both forms take in f64 at full size, in the order sconf_align_ctc / sconf_lalign_ctc /
sconf_align_ctc with the outputs compared bit for bit, then alone at a whole-recording shape (B=1, N=45000, S=12288, C=4096) with the
slab count and the workspace.  --slab-states picks the slab size (0: the default).  The time of each slab launch
(lalign_slab_kernel<MAXS>, one row per launch) comes from the kernel trace of --long --kernels-only."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

SHAPES = {'bench': (16, 2048, 512, 4096), 'long': (1, 16384, 4096, 4096)}
RECORDING = (1, 45000, 12288, 4096)             # an hour of speech: past what the short unit takes


def inputs(B, N, S, C, seed=0):
    """Log-probs with a planted monotone path (a trained model's posteriors are peaked, and the band the path lives in matters to
    nothing here but the walk back), targets without adjacent repeats."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    step = torch.randint(1, C - 1, (B, S), generator=g, device='cuda')
    tg = ((torch.randint(0, C - 1, (B, 1), generator=g, device='cuda') + step.cumsum(1)) % (C - 1)).to(torch.int32)
    x = torch.randn(B, N, C, generator=g, device='cuda')
    at = (torch.arange(N, device='cuda') * S // N).clamp(max=S - 1)
    x.scatter_add_(2, tg[:, at].long()[..., None], torch.full((B, N, 1), 3.0, device='cuda'))
    il = torch.full((B,), N, device='cuda', dtype=torch.int32)
    tl = torch.full((B,), S, device='cuda', dtype=torch.int32)
    return torch.log_softmax(x, -1).contiguous(), tg.contiguous(), il, tl


def timed(fn, n):
    for _ in range(2): fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def long_form(a):
    import lcasr_amd.hip.align as K
    import lcasr_amd.hip.align_long as KL
    lib, w = KL.load(), a.slab_states
    geo = f'{lib.sconf_lalign_threads(w)} threads x {lib.sconf_lalign_states_per_thread(w)} states'
    B, N, S, C = SHAPES['long']
    lp, tg, il, tl = inputs(B, N, S, C)
    short = lambda: K.ctc_align(lp, tg, il, tl, C - 1)
    long_ = lambda: KL.ctc_align(lp, tg, il, tl, C - 1, slab_states=w)
    if a.kernels_only:
        for _ in range(3): short()
        for _ in range(3): long_()
    else:
        n = a.reps or 5
        ref, out = short(), long_()
        assert K.state_bytes(S) == 8 and all(torch.equal(x, y) for x, y in zip(ref, out)), 'the two forms disagree'
        a0, b0, a1 = timed(short, n), timed(long_, n), timed(short, n)
        print(f'[shared] B={B} N={N} S={S} C={C}: {KL.slabs(S, w)} slabs of {geo}, workspace {KL.align_workspace(B, N, S, w)} bytes '
              f'(short form {K.align_workspace(B, N, S)}); outputs bit-equal')
        print(f'[shared] align {a0:.3f} ms | align long {b0:.3f} ms | align {a1:.3f} ms   (ratio {2 * b0 / (a0 + a1):.3f}, A/A spread of the '
              f'short form {abs(a1 - a0):.3f} ms)')
    del lp, tg, il, tl, short, long_
    torch.cuda.empty_cache()
    B, N, S, C = RECORDING
    lp, tg, il, tl = inputs(B, N, S, C)
    long_ = lambda: KL.ctc_align(lp, tg, il, tl, C - 1, slab_states=w)
    if a.kernels_only:
        for _ in range(3): long_()
        torch.cuda.synchronize()
        return
    out = long_()
    sp = out.spans[0].cpu()
    t0, t1 = timed(long_, a.reps or 3), timed(long_, a.reps or 3)
    print(f'[recording] B={B} N={N} S={S} C={C}: {KL.slabs(S, w)} slabs of {geo}, workspace {KL.align_workspace(B, N, S, w)} bytes; '
          f'score[0] {float(out.score[0]):.3f}, mean span {float((sp[:, 1] - sp[:, 0]).float().mean()):.2f} frames')
    print(f'[recording] align long {t0:.3f} ms | again {t1:.3f} ms   ({t0 / KL.slabs(S, w):.3f} ms per slab, gather, walk back and outputs included)')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--long', action='store_true', help='the long form (sconf_lalign_ctc) beside the short one, then at a whole recording')
    ap.add_argument('--slab-states', type=int, default=0, help='--long: states per slab (0: the default, 8192)')
    ap.add_argument('--shape', choices=list(SHAPES) + ['all'], default='all')
    ap.add_argument('--kernels-only', action='store_true', help='three calls of each op and nothing else: for the kernel trace')
    ap.add_argument('--reps', type=int, default=0, help='calls per timing window (default: 20 at the bench shape, 5 at the long one)')
    a = ap.parse_args()
    if a.long:
        return long_form(a)
    import lcasr_amd.hip.align as K
    import lcasr_amd.hip.ops as ops
    for name in (SHAPES if a.shape == 'all' else [a.shape]):
        B, N, S, C = SHAPES[name]
        lp, tg, il, tl = inputs(B, N, S, C)
        loss = lambda: ops.ctc_fwd(lp, tg, il, tl, C - 1)
        align = lambda: K.ctc_align(lp, tg, il, tl, C - 1)
        if a.kernels_only:
            for _ in range(3): loss()
            for _ in range(3): align()
            torch.cuda.synchronize()
            continue
        n = a.reps or (20 if name == 'bench' else 5)
        out = align()
        sp = out.spans[0].cpu()
        print(f'[{name}] B={B} N={N} S={S} C={C}: {K.load().sconf_align_threads(S)} threads x {K.load().sconf_align_states_per_thread(S)} states, '
              f'{K.state_bytes(S)}-byte state, workspace {K.align_workspace(B, N, S)} bytes; score[0] {float(out.score[0]):.3f}, '
              f'mean span {float((sp[:, 1] - sp[:, 0]).float().mean()):.2f} frames')
        a0, b0, a1 = timed(loss, n), timed(align, n), timed(loss, n)
        os.environ['SCONF_ALIGN_WALK_WINDOW'] = '1'
        plain = align()
        b1 = timed(align, n)
        del os.environ['SCONF_ALIGN_WALK_WINDOW']
        b2 = timed(align, n)
        assert all(torch.equal(x, y) for x, y in zip(out, plain)), 'the plain and the windowed walk back disagree'
        print(f'[{name}] ctc_fwd {a0:.3f} ms | align {b0:.3f} ms | ctc_fwd {a1:.3f} ms   (A/B/A spread of ctc_fwd {abs(a1 - a0):.3f} ms)')
        print(f'[{name}] align with the plain walk back {b1:.3f} ms | windowed again {b2:.3f} ms   (difference {b1 - b2:.3f} ms)')


if __name__ == '__main__':
    main()
