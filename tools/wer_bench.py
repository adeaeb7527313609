"""sconf_edit_counts at the evaluation shapes, timed with HIP events (wrapper calls, workspace allocation included), with the
row-vectorised numpy reference (tests/eval_refs.py) on the host beside it, and the buffered fetch_logits against the averaged one
on the plan of DESIGN.md section 9 (config 3 from seed, 131072 frames, 16384-frame windows, overlap 2048).  Under
`rocprofv3 --kernel-trace --stats -- python tools/wer_bench.py --kernels-only` the kernel trace gives the per-dispatch times quoted
in DESIGN.md section 10."""
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch
import lcasr_amd
from lcasr_amd.hip import ops
import eval_refs as E

kernels_only = '--kernels-only' in sys.argv


def timeit(fn, n):
    fn(); torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / n        # ms


def words(rng, n, edits, vocab=20000):
    """A transcript-like pair: a Zipf-ish reference of n ids and a hypothesis with `edits` planted errors."""
    return E.planted_pair(rng, n, vocab, edits)


rng = np.random.default_rng(0)
lib = ops._lib.load()
print(f'geometry: strip {lib.sconf_edit_strip_cols()} cols, pass {lib.sconf_edit_pass_cols()} cols, block {lib.sconf_edit_block_rows()} rows')
shapes = [('one 16384 x 16384 pair', [words(rng, 16384, 1600)], 5, 1),
          ('256 pairs of 2048 x 2048', [words(rng, 2048, 200) for _ in range(256)], 5, 8)]
ref = rng.integers(0, 20000, 16384).astype(np.int32)
attribution = []
for _ in range(64):                                            # 64 hypotheses against ONE 16384-word reference
    h = ref.copy(); at = rng.integers(0, 16384, 1600); h[at] = rng.integers(0, 20000, 1600)
    attribution.append((np.delete(h, rng.integers(0, 16384, 300)), ref))
shapes.append(('64 hypotheses x one 16384-word reference', attribution, 3, 1))
for name, pairs, n, cpu_pairs in shapes:
    cells = sum(len(h) * len(r) for h, r in pairs)
    dev = [t.cuda() for t in E.ragged([p[0] for p in pairs]) + E.ragged([p[1] for p in pairs])]
    ms = timeit(lambda: ops.edit_counts(*dev), n)
    got = ops.edit_counts(*dev).cpu()
    line = f'edit_counts {name}: {ms:.2f} ms, {cells / ms / 1e6:.2f} G cells/s'
    if not kernels_only:
        t0 = time.perf_counter()
        want = [E._split(E.edit_key_rows(h, r), len(h), len(r)) for h, r in pairs[:cpu_pairs]]
        cpu = time.perf_counter() - t0
        assert got[:cpu_pairs].tolist() == want, name
        sub = sum(len(h) * len(r) for h, r in pairs[:cpu_pairs])
        line += (f'; numpy reference {cpu * 1e3:.0f} ms for {cpu_pairs} of {len(pairs)} pairs = {sub / cpu / 1e9:.3f} G cells/s '
                 f'(whole batch at that rate: {cells / sub * cpu * 1e3:.0f} ms), counts equal')
    print(line + f'; WER {float(got[:, 0].sum()) / sum(len(r) for _, r in pairs):.4f}', flush=True)

if not kernels_only:
    import dyneval_refs as D
    from lcasr_amd.eval.buffered_transcription import fetch_logits as buffered
    from lcasr_amd.eval.utils import fetch_logits as averaged
    from lcasr_amd.models.sconformer_xl import SCConformerXL
    torch.manual_seed(0)
    model = SCConformerXL(vocab_size=4095, n_layers=6, d_model=768, n_heads=6, head_dim=128, subsampling_conv_channels=256, use_rotary=True,
                          rotary_base_freq=1500000, decoder_norm=True, self_conditioning=True, default_norm='layer_norm', bias_in_ff=False).cuda().eval()
    spec = torch.randn(1, 80, 131072, generator=torch.Generator().manual_seed(1)).cuda()
    tok = D.Tok(4095)
    for name, fn in (('averaged', averaged), ('buffered', buffered), ('averaged', averaged), ('buffered', buffered)):
        ms = timeit(lambda: fn(D.Args(), model, spec, 16384, 2048, tok, use_tqdm=False, return_numpy=False), 3)
        out = fn(D.Args(), model, spec, 16384, 2048, tok, use_tqdm=False, return_numpy=False)
        print(f'fetch_logits {name}: {ms:.1f} ms, {tuple(out.shape)} rows, finite {bool(torch.isfinite(out).all())}', flush=True)
