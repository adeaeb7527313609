"""CPU tests of head_dim 64 and 256 - the paper's 12-head (12 x 64) and 3-head (3 x 256) models at 6L/768D
(exp_set_rot_12h.yaml, exp_set_rot_3h.yaml): the oracle against the reference-generated fixtures h12_scalars / h3_scalars,
the package's host logic (emulated ops) against the same fixtures, and the C ABI's head_dim check."""
import ctypes

import numpy as np
import pytest
import torch

from common_model import rel_l2_errors, strided_like_fixture
from conftest import golden_cfg, load_golden
from oracle import sconformer_ref as O

CASES = ['h12_scalars', 'h3_scalars']


def fixture_inputs(fx):
    """The fixture's inputs.  `x` is not stored (tools/thin_scalar_fixture.py): it is regenerated from the seed of
    oracle/make_golden.py::synth and checked against the stored sums."""
    from oracle.make_golden import synth
    cfg = golden_cfg(fx)
    B, T = fx['lengths'].shape[0], int(fx['lengths'].max())
    x, ln, tg, tl = synth(B, T, cfg['vocab_size'], fx['lengths'].tolist())
    xd = x.double()
    assert abs(float(xd.sum()) - float(fx['x_sum'])) < 1e-6 and abs(float((xd * xd).sum()) - float(fx['x_sq_sum'])) < 1e-3
    assert torch.equal(tg, torch.from_numpy(fx['targets'])) and torch.equal(tl, torch.from_numpy(fx['target_lengths']))
    return x, ln, tg, tl


@pytest.mark.parametrize('case', CASES)
def test_oracle_head_dim_scalars(case):
    """From torch.manual_seed(12345), B = 2, T = 2048, lengths [2048, 1531]: the oracle reproduces the reference's loss and a
    slice of its log-probabilities (same check as test_oracle_c1_scalars)."""
    fx = load_golden(case)
    from lcasr_amd.models.sconformer_xl import SCConformerXL
    cfg = golden_cfg(fx)
    assert cfg['d_model'] == 768 and cfg['n_heads'] * cfg['head_dim'] == 768 and cfg['head_dim'] in (64, 256)
    torch.manual_seed(12345)
    sd = SCConformerXL(**cfg).state_dict()
    x, ln, tg, tl = fixture_inputs(fx)
    with torch.no_grad():
        loss, _, out = O.train_step_loss(sd, O.make_config(**cfg), x, ln, tg, tl)
    assert torch.equal(out['length'], torch.from_numpy(fx['out_length']))
    assert abs(float(loss) - float(fx['loss'])) / float(fx['loss']) < 1e-5
    assert float((out['final_posteriors'][:, ::17, ::97] - torch.from_numpy(fx['logp_slice'])).abs().max()) < 1e-3


@pytest.fixture
def exact_products(emulated_ops, monkeypatch):
    """The emulated ops with every GEMM product accumulated in float64 and rounded once to its output type.

    The fixtures hold the reference's fp32 gradients (the f32 oracle meets them to 3e-4), so a gradient error here is the noise of
    the package's bf16 rounding points, and WHERE a value falls between two bf16 neighbours is decided by the last bits of the
    f32 accumulation in front of the store.  kernel_refs.gemm accumulates with torch's CPU matmul, whose summation order belongs
    to the machine (its vector width and BLAS kernels), not to the package.  Measured on h12_scalars, relative L2 of
    decoder.ff.bias / decoder.ff.weight (the head's Linear, shared by the five self-conditioning steps; the worst tensors)
    against the bound 0.15:  torch's f32 matmul 0.1563 / 0.1511 (0.1580 / 0.1533 with its AVX2 kernels);  float64 accumulation
    in the trunk's GEMMs only 0.1081 / 0.1081,  in the decoder's only 0.1499 / 0.1454,  in all 0.1159 / 0.1155.  The rounding
    of dl in front of the bias gradient's column sums does not move it (0.1563 -> 0.1564): the error comes down the trunk.
    With the products exact the realisation no longer depends on the machine that runs the test."""
    real = emulated_ops.gemm

    def gemm(*args, **kw):
        old = emulated_ops.f32
        emulated_ops.f32 = torch.float64
        try:
            out = real(*args, **kw)
        finally:
            emulated_ops.f32 = old
        f32 = lambda t: t.to(torch.float32) if t.dtype == torch.float64 else t
        return tuple(f32(t) for t in out) if isinstance(out, tuple) else f32(out)
    monkeypatch.setattr(emulated_ops, 'gemm', gemm)
    return emulated_ops


@pytest.mark.parametrize('case', CASES)
def test_model_head_dim_scalars_emulated(exact_products, case):
    """The package's model (regrouped qkv shadow, rotary tables (N, D/2), rotary backward inside the attention backward) with
    the kernel references standing in for the HIP ops: loss, log-prob slice and gradients against the reference."""
    from lcasr_amd.losses import CTCLoss
    from lcasr_amd.models.sconformer_xl import SCConformerXL
    fx = load_golden(case)
    torch.manual_seed(12345)
    m = SCConformerXL(**golden_cfg(fx)).train()
    x, ln, tg, tl = fixture_inputs(fx)
    out = m(x, length=ln)
    lp = out['final_posteriors']
    loss = CTCLoss(blank=m.decoder.num_classes - 1, reduction='sum')(lp.transpose(0, 1), tg, out['length'], tl)
    (loss / (x.shape[-1] * x.shape[0]) * 100).backward()
    loss = float(loss.detach())
    assert torch.equal(out['length'], torch.from_numpy(fx['out_length']))
    assert abs(loss - float(fx['loss'])) / float(fx['loss']) < 1e-3
    d = (lp.detach()[:, ::17, ::97] - torch.from_numpy(fx['logp_slice'])).abs()
    assert float(d.max()) < 0.35 and float(d.mean()) < 0.05, (float(d.max()), float(d.mean()))
    cap, cap2 = int(fx['gs_cap']), int(fx['gs_cap2'])
    got = {k: strided_like_fixture(strided_like_fixture(p.grad.detach().float(), cap), cap2) for k, p in m.named_parameters()}
    errs = rel_l2_errors(got, {k[3:]: fx[k] for k in fx.files if k.startswith('gs.')})
    assert len(errs) == len(list(m.parameters()))
    assert max(errs.values()) < 0.15 and float(np.median(list(errs.values()))) < 0.065, sorted(errs.items(), key=lambda kv: -kv[1])[:5]


def _attn_args(D, B=0, N=16, H=1):
    s = (ctypes.c_int64 * 3)(N * H * D, H * D, D)
    return B, N, H, D, s


def test_attention_accepts_head_dims_64_and_256():
    """Host-side argument check of the C ABI with B = 0 (nothing is launched): head_dim 64 and 256 pass the head_dim test and
    stop at the empty problem; other head dims are still refused by name."""
    from lcasr_amd.hip import _lib
    lib = _lib.load()
    assert lib.sconf_version() >= 200
    for D, want in ((64, b'empty problem'), (256, b'empty problem'), (96, b'head_dim 96'), (512, b'head_dim 512')):
        B, N, H, D, s = _attn_args(D)
        rc = lib.sconf_attn_fwd(None, None, None, None, None, None, B, N, H, D, s, s, s, s, -1, -1, 1.0, None)
        assert rc != 0 and want in lib.sconf_last_error(), (D, lib.sconf_last_error())
        rc = lib.sconf_attn_bwd(None, None, None, None, None, None, None, None, None, None, None, B, N, H, D,
                                s, s, s, s, s, s, s, s, -1, -1, 1.0, None, None, None)
        assert rc != 0 and want in lib.sconf_last_error(), (D, lib.sconf_last_error())
