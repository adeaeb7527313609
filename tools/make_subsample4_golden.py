"""TEST INFRASTRUCTURE ONLY (development container only): fixtures for subsampling factor 4 and for subsampler stages wider than 512
channels, taken straight from the imported reference (fp32, CPU).  oracle/sconformer_ref.py restates the x8 subsampler only, so
nothing here goes through the oracle; the reference is imported at run time through oracle.make_golden.load_reference() and
only numbers and key names are written.

To stay small the fixtures hold SEEDS instead of weights and inputs, plus the float64 sum and sum of squares of every tensor the
seed must reproduce: a test rebuilds the tensors from the seeds and proves with the checksums that it holds the same ones.

Writes tests/golden/{tiny_ss4_ragged, tiny_ss4_odd, sub768, ss4_infer}.npz.      Usage:  python tools/make_subsample4_golden.py
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle.make_golden import GOLD, REF, TINY, load_reference, strided   # noqa: E402
from exact_sums import checksums                                          # noqa: E402  (exact sums: the tests recompute them)

MODEL_SEED, INPUT_SEED = 12345, 0
GS_CAP = 1024                     # 'gs.' entries: gradients outside the subsampler, strided to at most this many elements
LIMIT = 1 << 20


def out_len(n, stages):
    for _ in range(stages):
        n = (n - 1) // 2 + 1
    return n


def synth4(B, T, V, lengths, stages=2):
    """mel ~ N(0,1) (B,80,T) and targets uniform in [0,V) from one seeded generator; S = (T/4)/4 labels, per sample a quarter of
    its own token count."""
    g = torch.Generator().manual_seed(INPUT_SEED)
    x = torch.randn(B, 80, T, generator=g)
    S = max((T // 4) // 4, 1)
    tg = torch.randint(0, V, (B, S), generator=g)
    ln = torch.tensor(lengths)
    tl = torch.tensor([max(1, min(S, out_len(int(l), stages) // 4)) for l in ln], dtype=torch.long)
    return x, ln, tg, tl


def save(tag, fx):
    path = os.path.join(GOLD, tag + '.npz')
    np.savez_compressed(path, **fx)
    size = os.path.getsize(path)
    print(f'[{tag}] {len(fx)} arrays, {size} bytes')
    assert size < LIMIT, (tag, size)


def model_case(SC, tag, B, T, lengths):
    from common_model import rel_l2_errors
    kw = dict(TINY, subsampling_factor=4)
    V = kw['vocab_size']

    def run(bf16):
        torch.manual_seed(MODEL_SEED)
        m = SC(**kw); m.train()
        sd0 = {k: v.clone() for k, v in m.state_dict().items()}
        x, ln, tg, tl = synth4(B, T, V, lengths)
        with torch.autocast('cpu', dtype=torch.bfloat16, enabled=bf16):
            out = m(x, length=ln)
            lp = out['final_posteriors']
        lpf = lp.float()
        lpf.retain_grad()
        loss = torch.nn.CTCLoss(blank=m.decoder.num_classes - 1, reduction='sum')(lpf.transpose(0, 1), tg, out['length'], tl)
        (loss / (T * B) * 100).backward()
        return m, sd0, (x, ln, tg, tl), out['length'], float(loss), lpf, {k: p.grad.detach().float() for k, p in m.named_parameters()}

    m, sd0, (x, ln, tg, tl), olen, loss, lp, grads = run(False)
    for b in range(B):                                               # CTC-feasible: labels + forced blanks between repeats fit the tokens
        t = tg[b, :int(tl[b])]
        assert int(tl[b]) + int((t[1:] == t[:-1]).sum()) <= int(olen[b]), (b, int(tl[b]), int(olen[b]))
    assert np.isfinite(loss) and all(torch.isfinite(g).all() for g in grads.values())
    fx = {'cfg.' + k: np.array(v) for k, v in kw.items()}
    fx.update(model_seed=np.array(MODEL_SEED), input_seed=np.array(INPUT_SEED), B=np.array(B), T=np.array(T),
              sd_names=np.array(list(sd0)), sd_shapes=np.array([','.join(map(str, v.shape)) for v in sd0.values()]),
              sd_checksums=np.stack([checksums(v) for v in sd0.values()]), x_checksum=checksums(x),
              lengths=ln.numpy(), targets=tg.numpy(), target_lengths=tl.numpy(), out_length=olen.numpy(), loss=np.float64(loss),
              logp=lp.detach().numpy(), dlogp=lp.grad.detach().numpy(), gs_cap=np.array(GS_CAP))
    for k, v in grads.items():
        if k.startswith('subsampling.'): fx['g.' + k] = v.numpy()
        else: fx['gs.' + k] = strided(v, GS_CAP).numpy().copy()
    for k, v in m.state_dict().items():
        if 'batch_norm.running' in k or 'num_batches' in k: fx['buf.' + k] = v.numpy()
    # the reference's own bf16-autocast run against its fp32 run: the yardstick the HIP path's figures are reported beside
    _, _, _, _, loss16, lp16, grads16 = run(True)
    e = rel_l2_errors(grads16, {k: v.numpy() for k, v in grads.items()})
    live = [v for k, v in e.items() if not k.endswith('depthwise_conv.bias')]
    d = (lp16.detach() - lp.detach()).abs()
    fx.update({'noise.loss_rel': np.float64(abs(loss16 - loss) / loss), 'noise.logp_max': np.float64(float(d.max())),
               'noise.logp_mean': np.float64(float(d.mean())), 'noise.grad_l2_median': np.float64(np.median(live)),
               'noise.grad_l2_worst': np.float64(max(live))})
    print(f'[{tag}] out lengths {olen.tolist()} target lengths {tl.tolist()} CTC sum {loss:.2f}; {sum(p.numel() for p in m.parameters())} '
          f'parameters in {len(sd0)} tensors; reference bf16 vs fp32: log-probs max {float(d.max()):.3f} mean {float(d.mean()):.4f}, '
          f'loss {abs(loss16 - loss) / loss:.1e}, gradient rel-L2 median {np.median(live):.4f} worst {max(live):.4f}')
    save(tag, fx)


def sub768_case():
    """The bare reference ConvSubsampling at 768 channels (two / three channel slabs of the fused stage), factors 4 and 8."""
    from lcasr.components.subsampling import ConvSubsampling
    seed, C, d = 4321, 768, 64
    fx = dict(seed=np.array(seed), conv_channels=np.array(C), feat_out=np.array(d), gs_cap=np.array(GS_CAP))
    for factor in (4, 8):
        torch.manual_seed(seed)
        sub = ConvSubsampling('dw_striding', factor, 80, d, C, activation=torch.nn.SiLU())
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(2, 64, 80, generator=g)                       # (B, T, feat): the module's own input layout
        ln = torch.tensor([64, 51])
        y, olen = sub(x, ln)
        dy = torch.randn(y.shape, generator=g)
        y.backward(dy)
        p = f'f{factor}.'
        sd = sub.state_dict()
        fx.update({p + 'sd_names': np.array(list(sd)), p + 'sd_shapes': np.array([','.join(map(str, v.shape)) for v in sd.values()]),
                   p + 'sd_checksums': np.stack([checksums(v) for v in sd.values()]), p + 'x_checksum': checksums(x),
                   p + 'dy_checksum': checksums(dy), p + 'lengths': ln.numpy(), p + 'y': y.detach().numpy(), p + 'out_length': olen.numpy()})
        for k, v in sub.named_parameters():
            fx[p + 'gs.' + k] = strided(v.grad, GS_CAP).numpy().copy()
        print(f'[sub768 x{factor}] out {tuple(y.shape)} lengths {olen.tolist()}')
    save('sub768', fx)


def infer_case(SC):
    """The reference's own fetch_logits on the tiny factor-4 model in eval mode (stand-in audio_tools module as in
    oracle.make_golden.infer_case)."""
    at = types.ModuleType('lcasr.utils.audio_tools'); at.total_frames = lambda s: int(s * 100); at.total_seconds = lambda f: f / 100
    sys.modules['lcasr.utils.audio_tools'] = at
    for name, path in [('lcasr.eval', REF + '/lcasr/eval'), ('lcasr.decoding', REF + '/lcasr/decoding')]:
        m = types.ModuleType(name); m.__path__ = [path]; sys.modules[name] = m
    from lcasr.eval.utils import fetch_logits
    kw = dict(TINY, subsampling_factor=4)
    torch.manual_seed(MODEL_SEED)
    model = SC(**kw)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(11)
    model.train()
    with torch.no_grad():
        for _ in range(3):                                           # move the BatchRenorm running statistics off their init
            model(torch.randn(2, 80, 256, generator=g))
    model.eval(); model.device = 'cpu'
    spec = torch.randn(1, 80, 1024, generator=g)

    class Tok:
        def vocab_size(self): return kw['vocab_size']

    class Args: config = {'audio_chunking': {'size': 512, 'overlap': 128}}

    ref = fetch_logits(Args, model, spec.clone(), 256, 64, Tok(), use_tqdm=False)
    assert ref.shape == (256, 128), ref.shape
    fx = {'cfg.' + k: np.array(v) for k, v in kw.items()}
    fx.update(model_seed=np.array(MODEL_SEED), spec_seed=np.array(11), warm_batches=np.array(3), seq_len=np.array(256), overlap=np.array(64),
              sd_names=np.array(list(sd0)), sd_checksums=np.stack([checksums(v) for v in sd0.values()]), spec_checksum=checksums(spec),
              logits=ref)
    for k, v in model.state_dict().items():                          # the statistics after the warm-up batches: stored, not re-derived
        if 'batch_norm.running' in k or 'num_batches' in k: fx['buf.' + k] = v.numpy()
    save('ss4_infer', fx)


def main():
    assert os.path.isdir(REF), 'reference not present: this script only runs in the development container'
    SC, _, _ = load_reference()
    torch.set_num_threads(8)
    model_case(SC, 'tiny_ss4_ragged', 2, 256, [256, 200])
    model_case(SC, 'tiny_ss4_odd', 2, 250, [250, 173])
    sub768_case()
    infer_case(SC)


if __name__ == '__main__':
    main()
