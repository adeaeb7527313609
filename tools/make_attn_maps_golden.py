"""TEST INFRASTRUCTURE ONLY (development container only): the fixture of the attention-map collectors, taken from the imported
reference (fp32, CPU) with return_attention_weights set on every Attention module (lcasr/components/attention.py:424-445,
556-595).  The reference is imported at run time through oracle.make_golden.load_reference(); only numbers are written.

Writes tests/golden/attn_maps_tiny.npz: the model and spectrogram are those of infer_tiny.npz (2 layers, 2 heads x 32, rotary
on); the first 1000 frames give N = 125 tokens, deliberately not a multiple of any tile.
  scores     (L,1,H,N,N) f32  the scaled pre-softmax scores per layer, captured by a forward hook of this script on
                              `return_attention_module` (the reference's own CollectAttentionProbs rounds them to bf16)
  profile    (L,1,H,2N-1) f32 the offset profile of their softmax: profile[.., d + N - 1] = sum_i P[i, i + d]
  collector_shape             the shape the reference's CollectAttentionProbs returns on the same input (checked here)
  yard.*                      the reference's own fp32-versus-bf16-autocast difference of each quantity (scores max, scores mean,
                              profile max): the yardstick the tests double, in the manner of dyneval_cases.npz
Usage:  python tools/make_attn_maps_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle.make_golden import GOLD, REF, load_reference   # noqa: E402

LIMIT = 1 << 20
FRAMES = 1000


def offset_profile(scores):
    """(..., N, N) scores -> (..., 2N-1): the sums of softmax(scores) along its diagonals, in f64."""
    p = scores.double().softmax(-1)
    n = p.shape[-1]
    return torch.stack([p.diagonal(d, -2, -1).sum(-1) for d in range(-(n - 1), n)], -1)


def main():
    assert os.path.isdir(REF), 'reference not present: this script only runs in the development container'
    SC, _, _ = load_reference()
    from lcasr.components.attention import CollectAttentionProbs
    torch.set_num_threads(8)
    src = np.load(os.path.join(GOLD, 'infer_tiny.npz'))
    kw = {k[4:]: (src[k].item() if src[k].shape == () else src[k].tolist()) for k in src.files if k.startswith('cfg.')}
    model = SC(**kw)
    model.load_state_dict({k[2:]: torch.from_numpy(src[k].copy()) for k in src.files if k.startswith('w.')})
    model.eval()
    spec = torch.from_numpy(src['spec'].copy())[:, :, :FRAMES]
    attn = [l.attend.fn for l in model.layers]

    captured = []
    hooks = [a.return_attention_module.register_forward_hook(lambda _m, _i, out: captured.append(out[1].detach().float().clone()))
             for a in attn]
    collector = CollectAttentionProbs(attn)                     # sets return_attention_weights on every module

    def run(autocast):
        captured.clear(); collector.clear()
        with torch.no_grad(), torch.autocast('cpu', dtype=torch.bfloat16, enabled=autocast):
            model(spec)
        return torch.stack(captured, 0), collector()

    s32, c32 = run(False)
    s16, _ = run(True)
    for h in hooks: h.remove()
    L, B, H, N, _ = s32.shape
    assert (L, B, H, N) == (kw['n_layers'], 1, kw['n_heads'], 125) and tuple(c32.shape) == tuple(s32.shape) and c32.dtype == torch.bfloat16
    p32, p16 = offset_profile(s32), offset_profile(s16)
    assert torch.allclose(p32.sum(-1), torch.full((L, B, H), float(N), dtype=torch.float64))
    d = (s32 - s16).abs()
    fx = {'scores': s32.numpy().astype(np.float32), 'profile': p32.numpy().astype(np.float32), 'frames': np.int64(FRAMES),
          'collector_shape': np.array(c32.shape), 'yard.scores_max': np.float64(d.max()), 'yard.scores_mean': np.float64(d.mean()),
          'yard.profile_max': np.float64((p32 - p16).abs().max())}
    print(f'[attn_maps_tiny] scores {tuple(s32.shape)} max|s| {float(s32.abs().max()):.3f}; fp32 vs bf16 autocast: scores max '
          f'{float(d.max()):.4f} mean {float(d.mean()):.5f}, profile max {float((p32 - p16).abs().max()):.4f} (profile peak {float(p32.max()):.3f})')
    path = os.path.join(GOLD, 'attn_maps_tiny.npz')
    np.savez_compressed(path, **fx)
    size = os.path.getsize(path)
    print(f'[attn_maps_tiny] {len(fx)} arrays, {size} bytes')
    assert size < LIMIT, size


if __name__ == '__main__':
    main()
