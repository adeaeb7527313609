"""GPU tests of subsampling factor 4 and of subsampler stages wider than 512 channels: the channel slabs of the fused stage 0 -> 1
MFMA kernels through the C ABI, the tiny factor-4 model, the bare 768-channel module and sliding-window inference against the
reference's fixtures (tools/make_subsample4_golden.py), and the paper's 4x shape as a property test."""
import numpy as np
import pytest
import torch

import kernel_refs as R
from kernel_test_utils import BF, F32, close, dev, rnd
from subsample4_cases import TINY_SS4_CASES, check_fetch_logits, check_sub768, check_tiny_step

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import lcasr_amd.hip.ops as o
    o._lib.load()
    return o


def _slab_case(ops, B, F, T, C, mel):
    x = rnd(B, F, T, dtype=F32).to(mel)
    w0, b0 = rnd(C, 9, dtype=F32, seed=1) * 0.3, rnd(C, dtype=F32, seed=2) * 0.1
    wd, bd = rnd(C, 9, dtype=F32, seed=3) * 0.3, rnd(C, dtype=F32, seed=4) * 0.1
    assert ops.sub_stage01_slabs(F, C) >= 2 and ops.sub_stage01_slabs(F, C, True) >= 2
    xg, w0g, b0g, wdg, bdg = (dev(t) for t in (x, w0, b0, wd, bd))
    d1 = ops.sub_stage01_fwd(xg, w0g, b0g, wdg, bdg)
    d1r = R.sub_stage01_fwd(x.float(), w0, b0, wd, bd)
    close(d1, d1r, name='stage01 fwd, slabs')
    # a channel's arithmetic does not depend on its slab: the same bits as single-slab launches on slices of the weights
    parts = []
    for c0 in range(0, C, 512):
        c1 = min(C, c0 + 512)
        assert ops.sub_stage01_slabs(F, c1 - c0) == 1
        parts.append(ops.sub_stage01_fwd(xg, w0g[c0:c1].contiguous(), b0g[c0:c1].contiguous(), wdg[c0:c1].contiguous(), bdg[c0:c1].contiguous()))
    assert torch.equal(d1, torch.cat(parts, dim=-1))
    dout = rnd(*d1r.shape, seed=5)
    gr = [torch.zeros(C, 9), torch.zeros(C), torch.zeros(C, 9), torch.zeros(C)]
    g1 = [t.clone().cuda() for t in gr]
    g2 = [t.clone().cuda() for t in gr]
    ops.sub_stage01_bwd_(dev(dout), xg, w0g, b0g, wdg, *g1)
    ops.sub_stage01_bwd_(dev(dout), xg, w0g, b0g, wdg, *g2)
    R.sub_stage01_bwd_(dout, x.float(), w0, b0, wd, *gr)
    for a, a2, r, nm in zip(g1, g2, gr, ('dw0', 'db0', 'dwd', 'dbd')):
        close(a, r, name='stage01 slabs ' + nm, tol=5e-3)
        assert torch.equal(a, a2), nm                                 # fixed-order sums: bitwise repeatable


@pytest.mark.parametrize('mel', [F32, BF], ids=['f32', 'bf16'])
@pytest.mark.parametrize('F,T', [(80, 70), (24, 37)])
@pytest.mark.parametrize('C', [576, 768, 1024])
def test_stage01_channel_slabs(ops, C, F, T, mel):
    """C > 512: the fused stage splits the channels over gridDim.z.  576 = a ragged last slab of 64 channels (two of eight waves
    busy); odd T and F = 24 (F/2 = 12 positions: one MFMA block, F4 = 6) for the ragged ends of both axes."""
    _slab_case(ops, 2, F, T, C, mel)


def test_stage01_channel_slabs_several_row_blocks(ops):
    """T = 9000: 1125 forward and 750 backward row blocks per batch item and slab, so a workgroup row's slabs share a workspace row
    while every row is written by another (row block, batch item).  720 k conv0 positions per channel: long enough that only a
    backward which rounds the depthwise taps as the forward does stays inside 5e-3 of the reference."""
    _slab_case(ops, 2, 80, 9000, 768, F32)


@pytest.mark.parametrize('fused_loss', [False, True])
@pytest.mark.parametrize('case', TINY_SS4_CASES)
def test_tiny_factor4_step_vs_reference_fixture_on_device(ops, case, fused_loss):
    check_tiny_step(case, 'cuda', fused_loss)


@pytest.mark.parametrize('factor', [4, 8])
def test_sub768_module_vs_reference_fixture_on_device(ops, factor):
    """Bounds as in test_subsample4.test_sub768_module_vs_reference_fixture: 1.5e-2 of the output's max, gradients relative L2 < 0.05."""
    check_sub768(factor, 'cuda')


def test_fetch_logits_factor4_on_device(ops):
    check_fetch_logits('cuda')


def test_full_size_properties_paper_4x_shape(ops):
    """exp_set_seq_rotary_base_4x_subample.yaml: 6L/768D/6x128, factor 4, subsampler channels -1 (= 768), per-layer checkpointing; B = 1,
    T = 8192 -> N = 2048 tokens.  Size-independent properties, as test_model_gpu.test_full_size_properties_c5_shape."""
    from lcasr_amd.losses import CTCLoss
    from lcasr_amd.models.sconformer_xl import SCConformerXL
    from lcasr_amd.train import Trainer, synthetic_batch
    lib = ops._lib.load()
    assert lib.sconf_attn_waves(128, 2048, 768) == 8
    assert ops.sub_stage01_slabs(80, 768) >= 2 and ops.sub_stage01_slabs(80, 768, True) >= 2
    torch.manual_seed(12345)
    m = SCConformerXL(vocab_size=4095, n_layers=6, d_model=768, n_heads=6, head_dim=128, subsampling_factor=4, subsampling_conv_channels=-1,
                      use_rotary=True, rotary_base_freq=10000000, decoder_norm=True, self_conditioning=True, default_norm='layer_norm',
                      checkpoint_every_n_layers=1, ff_checkpoint_lvl=2).cuda().train()
    assert m.subsampling.conv[0].weight.shape[0] == 768 and tuple(m.subsampling.out.weight.shape) == (768, 20 * 768)
    x, ln, tg, tl = synthetic_batch(1, 8192, 4095, subsampling_factor=4)
    assert tg.shape[1] == 512
    out = m(x)
    lp = out['final_posteriors']
    assert lp.shape == (1, 2048, 4096) and int(out['length'][0]) == 2048
    assert float((lp.exp().sum(-1) - 1).abs().max()) < 1e-3                       # rows are distributions
    loss = CTCLoss(blank=4095, reduction='sum')(lp.transpose(0, 1), tg, out['length'], tl)
    lp.retain_grad()
    loss.backward()
    torch.cuda.synchronize()
    assert np.isfinite(float(loss)) and float(loss) > 0
    assert float(lp.grad.sum(-1).abs().max()) < 1e-3                              # CTC gradient frame sums
    assert all(torch.isfinite(p.grad).all() for p in m.parameters())

    def reset():
        for l in m.layers:
            bn = l.conv.fn.batch_norm
            bn.num_batches_tracked.zero_(); bn.running_mean.zero_(); bn.running_std.fill_(1.0)
    with torch.no_grad():
        reset(); a = m(x)['final_posteriors']
        reset(); b = m(x)['final_posteriors']
    assert torch.equal(a, b)                                                      # the forward is bitwise repeatable
    for p in m.parameters(): p.grad = None
    step_loss = Trainer(m, global_batch=1).step(x, ln, tg, tl)
    torch.cuda.synchronize()
    assert np.isfinite(float(step_loss)) and float(step_loss) > 0
