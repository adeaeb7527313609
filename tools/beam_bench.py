"""Micro-benchmark of CTC prefix beam search (sconf_beam_ctc).  Whole calls between HIP events, output allocation included, in the
order A / B / A: beam width 16, beam width 100, beam width 16 again, beside greedy decoding's row argmax on the same input.
Shapes: one long recording (B=1, N=16384, C=4096) and a batch (B=16, N=2048, C=4096).  Inputs: 'spiky' (a planted path, a token
every 6 frames on average, the blank elsewhere - a trained model's posteriors, with realistic runs of frames in which no token is
kept), 'noise' (log-softmax of unit noise: the arg-max and a few tokens are kept in EVERY frame - the worst case) and 'quiet' (the
blank raised everywhere: no frame keeps a token, what a frame costs that needs no selection).

Per-kernel times come from a kernel trace of a run of its own, which this tool also reads:
    rocprofv3 --kernel-trace -d DIR -o kt -- python tools/beam_bench.py --kernels-only --manifest DIR/manifest.json [--shape long]
    python tools/beam_bench.py --trace DIR/kt_results.db --manifest DIR/manifest.json
The second command matches the beam_compact_kernel / beam_search_kernel / beam_backtrace_kernel dispatches, in order, with the calls
the manifest lists and reports per call: the compaction's bandwidth against the 6.3 TB/s the project takes as achievable, the search
kernel's time per frame - split into frames without a kept token (from the 'quiet' input) and frames with a selection (the rest of the
'spiky' / 'noise' time over their frames with a kept token) - and the two relations of DESIGN.md §15."""
import argparse
import json
import os
import sqlite3
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {'long': (1, 16384, 4096), 'bench': (16, 2048, 4096)}
WIDTHS = (16, 100)
KINDS = ('spiky', 'noise', 'quiet')
HBM = 6.3e12


def inputs(kind, B, N, C, seed=0):
    import torch
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = torch.randn(B, N, C, generator=g, device='cuda')
    blank = C - 1
    if kind == 'quiet':
        x[:, :, blank] += 30.0
    elif kind == 'spiky':
        at = torch.rand(B, N, generator=g, device='cuda') < 1.0 / 6
        lab = torch.randint(0, C - 1, (B, N), generator=g, device='cuda')
        cls = torch.where(at, lab, torch.full_like(lab, blank))
        x.scatter_add_(2, cls[..., None], torch.full((B, N, 1), 12.0, device='cuda'))
    return torch.log_softmax(x, -1).contiguous()


def frames_with_a_token(lp, blank, thr=-5.0):
    nb = lp.clone()
    nb[:, :, blank] = float('-inf')
    return int(((nb.max(-1).values >= thr) | (lp.argmax(-1) != blank)).sum())


def timed(fn, n):
    import torch
    for _ in range(2): fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def run(a):
    import torch
    import lcasr_amd.hip.beam as K
    import lcasr_amd.hip.ops as ops
    manifest = []
    for name in (SHAPES if a.shape == 'all' else [a.shape]):
        B, N, C = SHAPES[name]
        for kind in KINDS:
            lp = inputs(kind, B, N, C)
            kept = frames_with_a_token(lp, C - 1)
            search = lambda W: K.ctc_beam(lp, None, C - 1, W, 1, -5.0, -10.0, 16, N)
            if a.kernels_only:
                for W in WIDTHS:
                    for _ in range(2):
                        search(W)
                        manifest.append(dict(shape=name, kind=kind, B=B, N=N, C=C, W=W, frames_with_a_token=kept))
                torch.cuda.synchronize()
                continue
            n = a.reps or (3 if kind == 'noise' else 5)
            out = search(16)
            g = timed(lambda: ops.argmax_rows(lp.view(B * N, C)), n)
            a0, b0, a1 = timed(lambda: search(16), n), timed(lambda: search(100), n), timed(lambda: search(16), n)
            print(f'[{name} {kind}] B={B} N={N} C={C}: {kept} of {B * N} frames keep a token; best hypothesis of sample 0: '
                  f'{int(out.lengths[0, 0])} tokens, score {float(out.scores[0, 0]):.3f}; workspace {K.beam_workspace(B, N, 16, 16)} bytes at W=16, '
                  f'{K.beam_workspace(B, N, 100, 16)} at W=100; search workgroup {K.load().sconf_beam_threads(16, 16)} / '
                  f'{K.load().sconf_beam_threads(100, 16)} threads')
            print(f'[{name} {kind}] W=16 {a0:.3f} ms | W=100 {b0:.3f} ms | W=16 {a1:.3f} ms   (A/B/A spread {abs(a1 - a0):.3f} ms); '
                  f'greedy row argmax {g:.3f} ms')
    if a.kernels_only and a.manifest:
        json.dump(manifest, open(a.manifest, 'w'))


def report(a):
    calls = json.load(open(a.manifest))
    db = sqlite3.connect(a.trace)
    cur = db.cursor()
    tabs = [r[0] for r in cur.execute("select name from sqlite_master where type='table'")]
    kd = [t for t in tabs if t.startswith('rocpd_kernel_dispatch')][0]
    ks = [t for t in tabs if t.startswith('rocpd_info_kernel_symbol')][0]
    rows = cur.execute(f"select s.kernel_name, d.start, d.end - d.start from {kd} d join {ks} s on d.kernel_id = s.id order by d.start").fetchall()
    stage = {k: [ns for n, _, ns in rows if k in n] for k in ('beam_compact_kernel', 'beam_search_kernel', 'beam_backtrace_kernel')}
    assert all(len(v) == len(calls) for v in stage.values()), {k: len(v) for k, v in stage.items()} | {'calls': len(calls)}
    best = {}                                                              # (shape, kind, W) -> the faster of the two traced calls
    for i, c in enumerate(calls):
        key = (c['shape'], c['kind'], c['W'])
        t = tuple(stage[k][i] for k in ('beam_compact_kernel', 'beam_search_kernel', 'beam_backtrace_kernel'))
        if key not in best or sum(t) < sum(best[key][0]): best[key] = (t, c)
    for (shape, kind, W), ((tc, ts, tb), c) in best.items():
        frames, kept = c['B'] * c['N'], c['frames_with_a_token']
        line = (f'[{shape} {kind} W={W}] compact {tc / 1e3:.1f} us = {frames * c["C"] * 4 / tc * 1e9 / 1e12:.2f} TB/s '
                f'({100 * frames * c["C"] * 4 / tc * 1e9 / HBM:.0f} % of 6.3) | search {ts / 1e3:.1f} us | backtrace {tb / 1e3:.1f} us | '
                f'compaction is {100 * tc / (tc + ts + tb):.1f} % of the kernels')
        quiet = best.get((shape, 'quiet', W))
        if quiet is not None:
            per_blank = quiet[0][1] / c['N']                               # (one workgroup per sample: the samples run side by side)
            line += f' | {per_blank / 1e3:.3f} us per frame without a token'
            if kind != 'quiet' and kept:
                per_kept = (ts - per_blank * (frames - kept) / c['B']) / (kept / c['B'])
                line += f', {per_kept / 1e3:.3f} us per frame with a selection (ratio {per_blank / per_kept:.3f})'
        print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', choices=list(SHAPES) + ['all'], default='all')
    ap.add_argument('--kernels-only', action='store_true', help='two calls per input and width and nothing else: for the kernel trace')
    ap.add_argument('--manifest', help='with --kernels-only: write the list of calls here; with --trace: read it')
    ap.add_argument('--trace', help='a rocprofv3 results database of a --kernels-only run: report per-kernel figures')
    ap.add_argument('--reps', type=int, default=0, help='calls per timing window (default: 5, 3 on the noise input)')
    a = ap.parse_args()
    report(a) if a.trace else run(a)


if __name__ == '__main__':
    main()
