"""Micro-benchmark of context attribution (include/sconf_ctxattr.h), HIP events around whole calls, one process:

  score     sconf_ctxattr_score on synthetic labels at (I = J = 64, N = 16384, R ~ 4096) and at a one-hour shape (W = 176, N = 45000,
            R = 13000), beside what the tree could already do: the full spliced hypotheses through ops.edit_counts.  That route is
            timed on --parent-rows rows of the matrix (J pairs each, one launch per row, as eval.wer scores) and scaled to all I rows;
            its errors are compared with the new unit's on those rows.  Cells: I J H R for the old route, (2 H + sum of the middles) R
            for the new one.
  fill      sconf_ctxattr_mask_fill at F = 80, T = 360000 (an hour), b = 4 against the bytes it must move (read F T once, write
            b F T) at 6.29 TB/s; sconf_ctxattr_window_means beside it.
  e2e       one attribution of a config-3 model (6L / 768D / 6 x 128) at T = 131072, window 2048 (W = 64), random weights and a
            synthetic reference, split into forwards and scoring.

usage: python tools/ctxattr_bench.py [score] [fill] [e2e] [--parent-rows K] [--reps N]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

SHAPES = {'square': (64, 16384, 4096), 'hour': (176, 45000, 13000)}        # (W, N, R)
HBM = 6.29e12


def timed(fn, n):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def labels(rng, W, N, R, vocab=4095):
    """A clean run that emits about R tokens, W masked runs that differ from it in a quarter of the frames of their own window and
    its two neighbours, and a reference that is the clean hypothesis after R / 10 edits: what a model's output looks like."""
    blank = vocab
    clean = rng.integers(0, vocab, N).astype(np.int32)
    clean[rng.random(N) >= R / N] = blank
    edges = [round(k * N / W) for k in range(W + 1)]
    windows = [(edges[k], edges[k + 1]) for k in range(W)]
    masked = np.repeat(clean[None], W, 0)
    for j in range(W):
        lo, hi = edges[max(j - 1, 0)], edges[min(j + 2, W)]
        at = lo + np.flatnonzero(rng.random(hi - lo) < 0.25)
        masked[j, at] = np.where(rng.random(len(at)) < R / N, rng.integers(0, vocab, len(at)), blank)
    hyp = collapse(clean, blank)
    ref = hyp.copy()
    at = rng.random(len(ref)) < 0.1
    ref[at] = rng.integers(0, vocab, int(at.sum()))
    return clean, masked, ref.astype(np.int32), windows, blank


def collapse(s, blank):
    keep = (s != blank) & np.concatenate([[True], s[1:] != s[:-1]])
    return s[keep]


def bench_score(a):
    import lcasr_amd.hip.ctxattr as K
    import lcasr_amd.hip.ops as ops
    lib = K.load()
    for name, (W, N, R0) in SHAPES.items():
        rng = np.random.default_rng(1)
        clean, masked, ref, windows, blank = labels(rng, W, N, R0)
        R, H = len(ref), len(collapse(clean, blank))
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
        c, m, r = dev(clean), dev(masked), dev(ref)
        new = lambda: K.score(c, m, r, windows, blank)
        out = new()
        t_new = timed(new, a.reps)
        mids = int(out.mid_len.sum())
        rows = list(range(0, W, max(W // a.parent_rows, 1)))[:a.parent_rows]
        t_old, worst = 0.0, 0
        for i in rows:
            f, g = windows[i]
            hyps = []
            for j in range(W):
                s = clean.copy(); s[f:g] = masked[j, f:g]
                hyps.append(collapse(s, blank))
            flat = dev(np.concatenate(hyps).astype(np.int32))
            ho = torch.tensor(np.concatenate([[0], np.cumsum([len(h) for h in hyps])]), dtype=torch.int64).cuda()
            rr = r.repeat(W)
            ro = (torch.arange(W + 1, dtype=torch.int64) * R).cuda()
            old = lambda: ops.edit_counts(flat, ho, rr, ro)
            got = old()[:, 0].to(torch.int32)
            worst = max(worst, int((got != out.errors[i]).sum()))
            t_old += timed(old, 1)
        t_old_all = t_old / len(rows) * W
        cells_old, cells_new = W * W * H * R, (2 * H + mids) * R
        print(f'[score {name}] I=J={W} N={N} R={R} H={H}: {lib.sconf_ctxattr_threads(R)} threads x {lib.sconf_ctxattr_cells_per_thread(R)} cells, '
              f'workspace {K.score_workspace(N, W, W, R)} bytes, mean middle {mids / W / W:.1f} tokens, clean errors {int(out.clean_errors)}')
        print(f'[score {name}] sconf_ctxattr_score {t_new:.3f} ms | W^2 hypotheses through ops.edit_counts {t_old_all:.1f} ms ({len(rows)} of {W} rows '
              f'timed: {t_old:.1f} ms; {worst} of their errors differ) | ratio {t_old_all / t_new:.1f} in time, {cells_old / cells_new:.1f} in cells '
              f'({cells_old:.3e} / {cells_new:.3e})')


def bench_fill(a):
    import lcasr_amd.hip.ctxattr as K
    F, T, b, w = 80, 360000, 4, 2048
    spec = torch.randn(F, T, device='cuda')
    windows = torch.tensor([(s, min(s + w, T)) for s in range(0, T, w)], dtype=torch.int32).cuda()
    means = K.window_means(spec, windows)
    t_means = timed(lambda: K.window_means(spec, windows), a.reps)
    t_fill = timed(lambda: K.mask_fill(spec, windows, means, 8, b), a.reps)
    moved = (1 + b) * F * T * 4
    print(f'[fill] F={F} T={T} b={b}: mask_fill {t_fill:.3f} ms (output allocation included) for {moved / 1e6:.1f} MB = {moved / t_fill / 1e9:.2f} TB/s, '
          f'{100 * moved / t_fill / 1e-3 / HBM:.0f} % of 6.29 TB/s | window_means of {len(windows)} windows {t_means:.3f} ms for {F * T * 4 / 1e6:.1f} MB = '
          f'{F * T * 4 / t_means / 1e9:.2f} TB/s')


def bench_e2e(a):
    from lcasr_amd.eval import context_attribution
    from lcasr_amd.models.sconformer_xl import SCConformerXL
    import lcasr_amd.hip.ctxattr as K
    kw = dict(vocab_size=4095, use_rotary=True, rotary_base_freq=1500000, decoder_norm=True, self_conditioning=True, default_norm='layer_norm',
              bias_in_ff=False, n_layers=6, d_model=768, n_heads=6, head_dim=128, subsampling_conv_channels=256)
    torch.manual_seed(12345)
    model = SCConformerXL(**kw).cuda().eval()
    T = 131072
    spec = torch.randn(1, 80, T, device='cuda')

    class Tok:
        def encode(self, text): return [int(w) for w in text.split()]
        def decode(self, ids): return ' '.join(str(int(i)) for i in ids)

    gold = ' '.join(str(int(v)) for v in np.random.default_rng(2).integers(0, 4095, 4000))
    spent = {'score': 0.0}
    inner = K.score

    def score(*args, **kw):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = inner(*args, **kw)
        torch.cuda.synchronize(); spent['score'] += time.perf_counter() - t0
        return out

    K.score = score
    for bs in (4,):
        context_attribution(model, spec, gold, Tok(), seq_len=16384, window_size=2048, batch_size=bs)      # warm-up: allocator, first launches
        spent['score'] = 0.0
        torch.cuda.synchronize(); t0 = time.perf_counter()
        res = context_attribution(model, spec, gold, Tok(), seq_len=16384, window_size=2048, batch_size=bs)
        torch.cuda.synchronize(); total = time.perf_counter() - t0
        W = len(res.windows)
        print(f'[e2e] config 3, T={T} (N={res.frame_labels.shape[1]}), W={W}, R=4000, batch_size={bs}: {total * 1e3:.0f} ms in all, scoring '
              f'{spent["score"] * 1e3:.1f} ms, forwards and the rest {1e3 * (total - spent["score"]):.0f} ms ({1 + -(-W // bs)} model calls; '
              f'the reference procedure: {W * W + 1} forwards); clean errors {int(res.errors[0, W])} of {res.units}')
    K.score = inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('parts', nargs='*', default=['score', 'fill', 'e2e'])
    ap.add_argument('--parent-rows', type=int, default=2)
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    for p in a.parts:
        {'score': bench_score, 'fill': bench_fill, 'e2e': bench_e2e}[p](a)


if __name__ == '__main__':
    main()
