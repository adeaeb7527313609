"""Shared by test_subsample4.py (CPU emulation) and test_subsample4_gpu.py: the seed-built cases of the factor-4 / wide-subsampler
fixtures (tools/make_subsample4_golden.py) and their checks.  TEST INFRASTRUCTURE, plain importable module.

The fixtures hold seeds, not weights: a case is rebuilt from its seeds and proven to be the generator's by exact checksums (the sum and
the sum of squares of every tensor, both evaluated exactly, so they do not depend on a summation order)."""
import numpy as np
import torch

from common_model import rel_l2_errors, run_step, strided_like_fixture
from conftest import golden_cfg, load_golden
from exact_sums import checksums
from test_model_gpu import GRAD_L2_MEDIAN, GRAD_L2_WORST

TINY_SS4_CASES = ['tiny_ss4_ragged', 'tiny_ss4_odd']


def assert_same_tensors(sd, names, shapes, sums, what):
    assert list(sd) == [str(n) for n in names], (what, list(sd), list(names))
    for i, (k, v) in enumerate(sd.items()):
        if shapes is not None:
            assert ','.join(map(str, v.shape)) == str(shapes[i]), (what, k, tuple(v.shape), str(shapes[i]))
        assert np.array_equal(checksums(v), sums[i]), (what, k, checksums(v), sums[i])


def tiny_model(fx):
    """SCConformerXL of a tiny factor-4 fixture under the fixture's seed, proven identical to the reference's initialisation."""
    from lcasr_amd.models.sconformer_xl import SCConformerXL
    torch.manual_seed(int(fx['model_seed']))
    m = SCConformerXL(**golden_cfg(fx))
    assert_same_tensors(m.state_dict(), fx['sd_names'], fx['sd_shapes'] if 'sd_shapes' in fx.files else None, fx['sd_checksums'], 'state_dict')
    return m


def tiny_batch(fx):
    """What common_model.run_step reads of a fixture, with x rebuilt from its seed."""
    g = torch.Generator().manual_seed(int(fx['input_seed']))
    x = torch.randn(int(fx['B']), 80, int(fx['T']), generator=g)
    assert np.array_equal(checksums(x), fx['x_checksum'])
    return dict(x=x.numpy(), lengths=fx['lengths'], targets=fx['targets'], target_lengths=fx['target_lengths'])


def check_tiny_step(case, device, fused_loss):
    """One step of a tiny factor-4 model against its fixture, at the bounds of test_model_gpu.test_tiny_model_vs_reference_fixture:
    exact output lengths, loss <= 2e-3 relative, log-probs max < 0.35 / mean < 0.05, BatchRenorm buffers < 2e-3, gradient relative L2
    worst < GRAD_L2_WORST and median < GRAD_L2_MEDIAN - the subsampler's gradients in full, every other tensor on the fixture's
    strided sample.  The reference's own bf16-autocast-vs-fp32 figures for the case are printed beside the measured ones (they are a
    yardstick to report against, not a bound: on these cases they sit below what any bf16 evaluation of the tiny model measures)."""
    fx = load_golden(case)
    m = tiny_model(fx).to(device).train()
    r = run_step(m, tiny_batch(fx), device, fused_loss=fused_loss)
    cap = int(fx['gs_cap'])
    ref, got = {}, {}
    for k in fx.files:
        if k.startswith('g.'):
            ref[k[2:]], got[k[2:]] = fx[k], r['grads'][k[2:]]
        elif k.startswith('gs.'):
            ref[k[3:]], got[k[3:]] = fx[k], strided_like_fixture(r['grads'][k[3:]], cap)
    assert sorted(ref) == sorted(r['grads'])
    errs = rel_l2_errors(got, ref)
    worst, med = max(errs.values()), float(np.median(list(errs.values())))
    loss_rel = abs(r['loss'] - float(fx['loss'])) / float(fx['loss'])
    tag = f'{case} {device}' + (' fused loss' if fused_loss else '')
    line = f'[{tag}] loss rel {loss_rel:.2e}, gradient rel-L2 median {med:.4f} worst {worst:.4f}'
    d = None
    if r['logp'] is not None:
        d = (r['logp'] - torch.from_numpy(fx['logp'])).abs()
        line += f', log-probs max {float(d.max()):.3f} mean {float(d.mean()):.4f}'
    print(line)
    print(f'[{tag}] reference bf16-autocast vs its fp32: loss rel {float(fx["noise.loss_rel"]):.2e}, gradient rel-L2 median '
          f'{float(fx["noise.grad_l2_median"]):.4f} worst {float(fx["noise.grad_l2_worst"]):.4f}, log-probs max '
          f'{float(fx["noise.logp_max"]):.3f} mean {float(fx["noise.logp_mean"]):.4f}')
    assert torch.equal(r['length'].long(), torch.from_numpy(fx['out_length']).long())
    assert loss_rel < 2e-3, (r['loss'], float(fx['loss']))
    if d is not None:
        assert float(d.max()) < 0.35 and float(d.mean()) < 0.05, (float(d.max()), float(d.mean()))
    assert worst < GRAD_L2_WORST and med < GRAD_L2_MEDIAN, sorted(errs.items(), key=lambda kv: -kv[1])[:5]
    bufs = [k for k in fx.files if k.startswith('buf.')]
    assert bufs
    for k in bufs:
        assert float((r['buffers'][k[4:]] - torch.from_numpy(fx[k]).float()).abs().max()) < 2e-3, k


SUB768_OUT_TOL, SUB768_GRAD_L2 = 1.5e-2, 0.05


def check_sub768(factor, device):
    """The bare ConvSubsampling at 768 channels against the reference's (tests/golden/sub768.npz): output within SUB768_OUT_TOL of its
    max magnitude, every parameter gradient (fixture's strided sample) within SUB768_GRAD_L2 relative L2.  Returns the two figures."""
    from lcasr_amd.components.subsampling import ConvSubsampling
    fx = load_golden('sub768')
    p = f'f{factor}.'
    seed = int(fx['seed'])
    torch.manual_seed(seed)
    sub = ConvSubsampling('dw_striding', factor, 80, int(fx['feat_out']), int(fx['conv_channels']), activation=torch.nn.SiLU())
    assert_same_tensors(sub.state_dict(), fx[p + 'sd_names'], fx[p + 'sd_shapes'], fx[p + 'sd_checksums'], f'sub768 x{factor}')
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, 64, 80, generator=g)
    yref = torch.from_numpy(fx[p + 'y'])
    dy = torch.randn(yref.shape, generator=g)
    assert np.array_equal(checksums(x), fx[p + 'x_checksum']) and np.array_equal(checksums(dy), fx[p + 'dy_checksum'])
    sub = sub.to(device)
    y, olen = sub(x.to(device), torch.from_numpy(fx[p + 'lengths']).to(device))
    y.backward(dy.to(device))
    assert torch.equal(olen.cpu().long(), torch.from_numpy(fx[p + 'out_length']).long())
    out_err = float((y.detach().float().cpu() - yref).abs().max()) / float(yref.abs().max())
    cap = int(fx['gs_cap'])
    errs = {}
    for k, prm in sub.named_parameters():
        r = torch.from_numpy(fx[p + 'gs.' + k]).double()
        gg = strided_like_fixture(prm.grad.detach().float().cpu(), cap).double()
        errs[k] = float((gg - r).norm() / r.norm())
    print(f'[sub768 x{factor} {device}] output max err {out_err:.2e} of max|ref|; gradient rel-L2 ' + ', '.join(f'{k} {v:.4f}' for k, v in errs.items()))
    assert out_err <= SUB768_OUT_TOL, out_err
    assert max(errs.values()) < SUB768_GRAD_L2, errs
    return out_err, max(errs.values())


def infer_model(fx, device='cpu'):
    """The tiny factor-4 model of ss4_infer.npz in eval mode: weights from the seed, BatchRenorm statistics from the fixture."""
    m = tiny_model(fx)
    sd = m.state_dict()
    for k in fx.files:
        if k.startswith('buf.'):
            sd[k[4:]] = torch.from_numpy(fx[k].copy())
    m.load_state_dict(sd)
    return m.to(device).eval()


def check_fetch_logits(device):
    """fetch_logits on the tiny factor-4 model against the reference's own output; batched and unbatched runs agree.  Bounds of
    test_host_logic.test_fetch_logits_and_greedy_decode_against_reference_fixture: max < 0.3, mean < 0.03."""
    from lcasr_amd.eval.utils import fetch_logits
    fx = load_golden('ss4_infer')
    m = infer_model(fx, device)
    g = torch.Generator().manual_seed(int(fx['spec_seed']))
    for _ in range(int(fx['warm_batches'])):
        torch.randn(2, 80, 256, generator=g)                          # the generator's warm-up batches came out of the same stream
    spec = torch.randn(1, 80, 1024, generator=g)
    assert np.array_equal(checksums(spec), fx['spec_checksum'])

    class Tok:
        def vocab_size(self): return int(fx['cfg.vocab_size'])

    class Args: config = {'audio_chunking': {'size': 512, 'overlap': 128}}

    ref = fx['logits']
    outs = []
    for batched in (False, True):
        got = fetch_logits(Args, m, spec.to(device) if device != 'cpu' else spec, int(fx['seq_len']), int(fx['overlap']), Tok(), use_tqdm=False,
                           batched=batched, max_batch=3)
        assert got.shape == ref.shape, (got.shape, ref.shape)
        d = np.abs(got - ref)
        print(f'[fetch_logits x4 {device} batched={batched}] max {float(d.max()):.3f} mean {float(d.mean()):.4f}')
        assert float(d.max()) < 0.3 and float(d.mean()) < 0.03, (batched, float(d.max()), float(d.mean()))
        outs.append(got)
    dd = float(np.abs(outs[0] - outs[1]).max())
    assert dd < 2e-3, dd                                              # same kernels, other batch size (test_model_gpu's bound for this)
    return outs
