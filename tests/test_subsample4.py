"""CPU tests of subsampling factor 4 and of subsampler stages wider than 512 channels: module and model construction against the
reference's layout and seeded initialisation, one training step and sliding-window inference with the kernel references standing in
for the HIP ops (conftest.emulated_ops), and the host-side channel-slab query of the fused stage 0 -> 1 kernels.
Fixtures: tools/make_subsample4_golden.py (seeds + exact checksums instead of weights; see subsample4_cases.py)."""
import pytest
import torch

from conftest import golden_cfg, load_golden
from subsample4_cases import TINY_SS4_CASES, check_fetch_logits, check_sub768, check_tiny_step, tiny_model


def test_factor4_model_has_the_reference_layout_and_seeded_init():
    """state_dict names and shapes equal the reference's at factor 4 (subsampling.conv.{0,2,3}.*, subsampling.out.weight (d, 20 C)) and
    under the fixture's seed every tensor's exact sum and sum of squares equal the reference's: the initialisation is bit-identical."""
    fx = load_golden('tiny_ss4_ragged')
    m = tiny_model(fx)                                               # asserts names, shapes and checksums
    sd = m.state_dict()
    C, d = int(fx['cfg.subsampling_conv_channels']), int(fx['cfg.d_model'])
    assert sorted(k for k in sd if k.startswith('subsampling.')) == sorted([f'subsampling.conv.{i}.{w}' for i in (0, 2, 3) for w in ('weight', 'bias')] + ['subsampling.out.weight'])
    assert tuple(sd['subsampling.out.weight'].shape) == (d, 20 * C)
    assert m.subsampling.subsampling_factor == 4 and sum(p.numel() for p in m.parameters()) == 250976


@pytest.mark.parametrize('fused_loss', [False, True])
@pytest.mark.parametrize('case', TINY_SS4_CASES)
def test_tiny_factor4_step_vs_reference_fixture(emulated_ops, case, fused_loss):
    check_tiny_step(case, 'cpu', fused_loss)


@pytest.mark.parametrize('factor', [4, 8])
def test_sub768_module_vs_reference_fixture(emulated_ops, factor):
    """The bare module at 768 channels, both factors: output <= 1.5e-2 of the output's max magnitude, gradients relative L2 < 0.05.
    Neither bound comes from a measurement: 1.5e-2 is the bound test_model_gpu puts on blocks that see only bf16 operand rounding
    (the subsampler is one), 0.05 a third of the model-level worst-tensor bound for a block with no BatchRenorm behind it.  The CPU
    emulation, which shares the bf16 rounding points, measures 5.2e-3 / 0.0054 (x4) and 3.4e-3 / 0.0061 (x8): inside both."""
    check_sub768(factor, 'cpu')


def test_factor_and_channel_arguments():
    from lcasr_amd.components.subsampling import ConvSubsampling
    from lcasr_amd.models.sconformer_xl import SCConformerXL
    from lcasr_amd.train import synthetic_batch
    for factor in (2, 16):
        with pytest.raises(NotImplementedError):
            ConvSubsampling('dw_striding', factor, 80, 64, 32, activation=torch.nn.SiLU())
    with pytest.raises(ValueError):
        ConvSubsampling('dw_striding', 6, 80, 64, 32, activation=torch.nn.SiLU())
    kw = dict(golden_cfg(load_golden('tiny_ss4_ragged')), subsampling_conv_channels=-1)
    m = SCConformerXL(**kw)
    assert m.subsampling_conv_channels == kw['d_model'] and m.subsampling.conv[0].weight.shape[0] == kw['d_model']
    assert tuple(m.subsampling.out.weight.shape) == (kw['d_model'], 20 * kw['d_model']) and len(m.subsampling.conv) == 5
    x, ln, tg, tl = synthetic_batch(2, 256, 127, device='cpu', subsampling_factor=4)
    assert tuple(tg.shape) == (2, 16) and tl.tolist() == [16, 16] and tuple(x.shape) == (2, 80, 256)
    x8, _, tg8, tl8 = synthetic_batch(2, 256, 127, device='cpu')
    assert tuple(tg8.shape) == (2, 8) and tl8.tolist() == [8, 8] and torch.equal(x8, x)


def test_fetch_logits_factor4_vs_reference_fixture(emulated_ops):
    check_fetch_logits('cpu')


def test_stage01_slab_query_on_the_host():
    """sconf_sub_stage01_slabs: C <= 512 stays ONE slab (the launch the paper's x8 configs always had), wider stages split, a shape
    the MFMA kernels do not take gives 0.  No GPU: the library cross-compiles and the query launches nothing."""
    import __graft_entry__ as g
    g.build()
    import lcasr_amd.hip.ops as ops
    for bwd in (False, True):
        assert ops.sub_stage01_slabs(80, 256, bwd) == 1 and ops.sub_stage01_slabs(80, 512, bwd) == 1
        for C in (576, 768, 1024):
            assert ops.sub_stage01_slabs(80, C, bwd) >= 2, (C, bwd)
        assert ops.sub_stage01_slabs(80, 48, bwd) == 0
        assert ops.sub_stage01_slabs(80, 1056, bwd) == 0 and ops.sub_stage01_slabs(400, 256, bwd) == 0      # C > 1024; F/2 > 64 positions
