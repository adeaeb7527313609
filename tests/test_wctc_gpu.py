"""GPU tests of the wild-card CTC loss (csrc/wctc.hip behind include/sconf_wctc.h) against the float64 numpy restatement
(tests/wctc_refs.py, itself held to the reference's autograd in test_wctc.py), with the tolerances of the CTC kernels' own tests
(tests/test_kernels_gpu.py, the same state discipline): loss to 1e-5 relative, gradient to 2e-4 of its maximum."""
import numpy as np
import pytest
import torch

import footprint as FP
import wctc_footprint_cases as WC
import wctc_refs as WR
from conftest import load_golden
from kernel_test_utils import close, dev

pytestmark = pytest.mark.gpu

FX = load_golden('wctc_cases')
CASES = [str(c) for c in FX['cases']]


@pytest.fixture(scope='module')
def wctc():
    import __graft_entry__ as g
    g.build()
    from lcasr_amd.hip import wctc
    wctc.load()
    return wctc


def pad4(lp):
    C = lp.shape[-1]
    return lp if C % 4 == 0 else torch.nn.functional.pad(lp, (0, 4 - C % 4), value=-1e30)


def on_device(wctc, lp, tg, il, tl, blank, mode, grad_out=None):
    """The two launchers on (B, N, C) log-probs -> (nll (B), grad (B, N, C)) on the host, classes the padding added cut off."""
    x = dev(pad4(lp).contiguous())
    i32 = lambda t: dev(torch.as_tensor(t).to(torch.int32).contiguous())
    tg, il, tl = i32(tg), i32(il), i32(tl)
    nll, ws = wctc.wctc_fwd(x, tg, il, tl, blank, mode)
    grad = wctc.wctc_bwd(x.shape, ws, tg, il, tl, None if grad_out is None else dev(grad_out), blank, mode)
    torch.cuda.synchronize()
    return nll.cpu(), grad.cpu()[..., :lp.shape[-1]]


def check(wctc, lp, tg, il, tl, blank, mode, name, grad_out=None):
    nll, grad = on_device(wctc, lp, tg, il, tl, blank, mode, grad_out)
    nllr, gradr, info = WR.wctc(lp.numpy(), np.asarray(tg), np.asarray(il), np.asarray(tl), blank, mode, None if grad_out is None else grad_out.numpy())
    nllr, gradr = torch.from_numpy(nllr), torch.from_numpy(gradr)
    fin = torch.isfinite(nllr)
    rel = float(((nll[fin].double() - nllr[fin]) / nllr[fin]).abs().max()) if fin.any() else 0.0
    g = float((grad.double() - gradr).abs().max()) / (float(gradr.abs().max()) + 1e-12)
    print(f'[wctc] {name} {mode}: nll {nll.tolist()} rel err {rel:.2e}; grad err {g:.2e} of max {float(gradr.abs().max()):.3e}')
    assert torch.equal(torch.isfinite(nll), fin) and torch.equal(nll[~fin].double(), nllr[~fin])
    assert rel < 1e-5, (nll, nllr)
    close(grad, gradr, tol=2e-4, name=f'{name} {mode} grad')
    return nll, grad, info


def random_case(seed, B, N, C, L, scale, blank=None):
    g = torch.Generator().manual_seed(seed)
    blank = C - 1 if blank is None else blank
    lp = torch.log_softmax(torch.randn(B, N, C, generator=g) * scale, -1)
    tg = torch.randint(0, C - 1, (B, L), generator=g)
    tg[tg >= blank] += 1
    if L > 1: tg[0, 1] = tg[0, 0]                                            # a repeated label (needs the blank in between)
    return lp, tg, blank


# ---- fixture cases: what autograd through the reference gives --------------------------------------------------------------------------
@pytest.mark.parametrize('mode', WR.MODES)
@pytest.mark.parametrize('case', CASES)
def test_fixture_cases(wctc, case, mode):
    lp, tg = torch.from_numpy(FX[f'{case}.lp']), FX[f'{case}.targets']
    il, tl, blank = FX[f'{case}.input_lengths'], FX[f'{case}.target_lengths'], int(FX[f'{case}.blank'])
    nll, grad, _ = check(wctc, lp, tg, il, tl, blank, mode, case)
    rl, rg = torch.from_numpy(FX[f'{case}.{mode}.loss']), torch.from_numpy(FX[f'{case}.{mode}.grad'])
    assert float(((nll.double() - rl) / rl).abs().max()) < 1e-5
    close(grad, rg, tol=2e-4, name=f'{case} {mode} grad against the reference')


# ---- geometry: lattice widths around the workgroup sizes and the states-per-thread steps, T around the offset cadence --------------------
# widths 2L + 1 = 63, 65 (one wave / two), 129, 1023, 1025 (1024 threads of 1 state / of 2) and 4097 (the step from 4 to 5 states per
# thread, the last below sconf_wctc_max_labels), each at T = 2L + 8
@pytest.mark.parametrize('L', [31, 32, 64, 511, 512, 2048])
def test_lattice_widths(wctc, L):
    B, C = 2, 8
    T = 2 * L + 8
    lp, tg, blank = random_case(L, B, T, C, L, 1.0)
    il, tl = torch.tensor([T, T - 5]), torch.tensor([L, max(1, L - 3)])
    check(wctc, lp, tg, il, tl, blank, 'soft', f'width {2 * L + 1}')
    if L in (32, 512): check(wctc, lp, tg, il, tl, blank, 'sum_prob', f'width {2 * L + 1}')


@pytest.mark.parametrize('T', [4, 5, 8, 9])
@pytest.mark.parametrize('mode', WR.MODES)
def test_frame_counts_around_the_offset_cadence(wctc, T, mode):
    lp, tg, blank = random_case(T, 2, T, 12, 2, 2.0, blank=5)
    check(wctc, lp, tg, torch.tensor([T, T - 1]), torch.tensor([2, 1]), blank, mode, f'T = {T}')


def test_the_4096_class_vocabulary(wctc):
    """The paper models' class count: a log-prob row of 16 KB through the gather's LDS copy, labels spread over the gradient kernel's
    class histogram."""
    B, T, C, L = 2, 300, 4096, 140
    lp, tg, blank = random_case(C, B, T, C, L, 1.0)
    for mode in ('soft', 'max_prob'):
        check(wctc, lp, tg, torch.tensor([T, T - 17]), torch.tensor([L, 47]), blank, mode, '4096 classes')


def test_workspace_offsets_past_2_pow_32_bytes(wctc):
    """B = 128, N = 2048, Smax = 512: a workspace of 4.3 GB, so the last samples' rows lie past 2^32 bytes (and their element indices
    past 2^30).  The last sample in the batch must give, bit for bit, what it gives alone."""
    B, T, C, L = 128, 2048, 8, 512
    g = torch.Generator(device='cuda').manual_seed(1)
    lp = torch.log_softmax(torch.randn(B, T, C, generator=g, device='cuda'), -1)
    tg = torch.randint(0, C - 1, (B, L), generator=g, device='cuda', dtype=torch.int32)
    il = torch.full((B,), T, dtype=torch.int32, device='cuda'); tl = torch.full((B,), L, dtype=torch.int32, device='cuda')
    assert wctc.workspace_bytes(B, T, L, 'soft') > 1 << 32
    nll, ws = wctc.wctc_fwd(lp, tg, il, tl, C - 1, 'soft')
    grad = wctc.wctc_bwd(lp.shape, ws, tg, il, tl, None, C - 1, 'soft')
    del ws
    n1, w1 = wctc.wctc_fwd(lp[-1:].contiguous(), tg[-1:].contiguous(), il[-1:], tl[-1:], C - 1, 'soft')
    g1 = wctc.wctc_bwd((1, T, C), w1, tg[-1:].contiguous(), il[-1:], tl[-1:], None, C - 1, 'soft')
    torch.cuda.synchronize()
    assert torch.isfinite(nll).all() and torch.isfinite(grad).all() and float(grad[-1].abs().max()) > 0
    assert torch.equal(n1[0], nll[-1]) and torch.equal(g1[0], grad[-1])


# ---- drift: many frames with w_t < 0 over 2048 frames ------------------------------------------------------------------------------------
def test_soft_mode_does_not_drift_over_2048_frames_of_weak_emissions(wctc):
    B, T, L, C = 2, 2048, 300, 144
    lp, tg, blank = random_case(7, B, T, C, L, 0.3)
    il, tl = torch.tensor([T, T]), torch.tensor([L, L])
    _, _, info = check(wctc, lp, tg, il, tl, blank, 'soft', 'drift')
    for e, w in info:
        neg = int((w < 0).sum())
        print(f'[wctc] drift: {neg} of {T} frames have w_t < 0')
        assert neg >= T // 10                                                # the signed path is exercised


# ---- special samples ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', WR.MODES)
def test_infeasible_and_empty_samples_leave_their_neighbours_alone(wctc, mode):
    B, T, C, L = 4, 24, 8, 6
    lp, tg, blank = random_case(3, B, T, C, L, 1.5)
    tg[1] = 2                                                                # 6 equal labels need 11 frames
    il, tl = torch.tensor([T, 10, 0, T - 3]), torch.tensor([L, L, L, 2])
    nll, grad, _ = check(wctc, lp, tg, il, tl, blank, mode, 'special samples')
    assert nll[1] == float('inf') and nll[2] == float('inf') and not grad[1].any() and not grad[2].any()
    alone = [on_device(wctc, lp[b:b + 1], tg[b:b + 1], il[b:b + 1], tl[b:b + 1], blank, mode) for b in (0, 3)]
    for (n1, g1), b in zip(alone, (0, 3)):
        assert torch.equal(n1[0], nll[b]) and torch.equal(g1[0], grad[b])    # bit for bit what the sample gives alone


def test_device_side_poison(wctc):
    """Lengths and labels on the device cannot be checked without a sync: the sample is poisoned (NaN), its neighbours are not."""
    B, T, C, L = 4, 16, 8, 3
    lp, tg, blank = random_case(5, B, T, C, L, 1.0)
    tg[2, 1] = C + 3
    il, tl = torch.tensor([T, T, T, T + 1]), torch.tensor([L, 0, L, L])
    nll, grad = on_device(wctc, lp, tg, il, tl, blank, 'soft')
    assert torch.isfinite(nll[0]) and torch.isnan(nll[1:]).all() and torch.isfinite(grad[0]).all() and torch.isnan(grad[1:]).all()
    n0, g0 = on_device(wctc, lp[:1], tg[:1], il[:1], tl[:1], blank, 'soft')
    assert torch.equal(n0[0], nll[0]) and torch.equal(g0[0], grad[0])


# ---- autograd path ------------------------------------------------------------------------------------------------------------------------
def test_autograd_path(wctc):
    from lcasr_amd.losses import WCTCLoss, wctc_loss
    B, T, C, L = 3, 50, 10, 7                                                # C % 4 != 0: the Python layer pads the classes
    lp, tg, blank = random_case(11, B, T, C, L, 1.5, blank=4)
    il, tl = torch.tensor([T, 33, T]), torch.tensor([L, 4, 5])
    for b in range(B): tg[b, int(tl[b]):] = -1
    for mode in WR.MODES:
        x = dev(lp.transpose(0, 1).contiguous()).requires_grad_(True)         # (T, B, C), as the reference takes it
        loss = WCTCLoss(blank=blank, mode=mode)(x, dev(tg), dev(il), dev(tl))
        assert loss.shape == (B,)
        loss.sum().backward()
        nll, grad = on_device(wctc, lp, tg, il, tl, blank, mode)
        assert torch.equal(loss.detach().cpu(), nll) and torch.equal(x.grad.transpose(0, 1).cpu(), grad)
        mean = wctc_loss(x.detach(), dev(tg), il, tl, blank=blank, mode=mode, return_mean=True)          # lengths on the host
        assert mean.shape == () and torch.equal(mean, loss.detach().mean())
        flat = wctc_loss(x.detach(), torch.cat([tg[b, :int(tl[b])] for b in range(B)]), il, tl, blank=blank, mode=mode)   # 1-D concatenated targets
        assert torch.equal(flat.cpu(), nll)
        go = torch.tensor([0.37, -2.5, 3.0])
        _, scaled = on_device(wctc, lp, tg, il, tl, blank, mode, grad_out=go)
        want = grad * go[:, None, None]
        ulp = torch.abs(torch.nextafter(want, torch.full_like(want, float('inf'))) - want)
        assert bool(((scaled - want).abs() <= ulp).all())                     # grad_out scaling exact to 1 ulp
        x2 = dev(lp.transpose(0, 1).contiguous()).requires_grad_(True)
        (WCTCLoss(blank=blank, mode=mode)(x2, dev(tg), dev(il), dev(tl)) * dev(go)).sum().backward()
        assert torch.equal(x2.grad.transpose(0, 1).cpu(), scaled)
    with pytest.raises(ValueError, match='at least 1'):
        wctc_loss(x.detach(), dev(tg), il, torch.tensor([L, 0, 5]), blank=blank)


# ---- model step ---------------------------------------------------------------------------------------------------------------------------
def _trainer_step(wildcard):
    from common_model import build_from_fixture
    from lcasr_amd.train import Trainer
    fx = load_golden('tiny_ln_ragged')
    m = build_from_fixture(fx, 'cuda')
    tr = Trainer(m) if wildcard == 'default' else Trainer(m, wildcard=wildcard, fused_loss=wildcard is None)
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    args = [torch.from_numpy(fx[k]).cuda() for k in ('x', 'lengths', 'targets', 'target_lengths')]
    loss = tr.step(*args)
    torch.cuda.synchronize()
    return float(loss), before, {k: p.detach().clone() for k, p in m.named_parameters()}


def test_trainer_step_with_the_wildcard():
    loss, before, after = _trainer_step('soft')
    assert np.isfinite(loss)
    assert all(torch.isfinite(p).all() for p in after.values()) and any(not torch.equal(before[k], after[k]) for k in before)
    plain, _, after_plain = _trainer_step('default')
    none, _, after_none = _trainer_step(None)
    assert plain == none and all(torch.equal(after_plain[k], after_none[k]) for k in after_plain)     # wildcard=None is today's path, bit for bit
    assert loss != plain


# ---- write footprints ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('id', list(WC.CASES))
def test_write_footprint(wctc, id):
    FP.run_on_device(WC.build(id, wctc.load()), wctc.PROTOTYPES)
