"""CPU tests of the wild-card CTC loss (include/sconf_wctc.h, lcasr_amd.hip.wctc, functional.wctc_nll, losses.wctc_loss / WCTCLoss,
Trainer(wildcard=...)): the numpy restatement (tests/wctc_refs.py) against autograd through the reference's own wctc_loss
(tests/golden/wctc_cases.npz, written by tools/make_wctc_golden.py), the header against the binding and the exports, and the
refusals that need no GPU.  The kernels themselves are tested in test_wctc_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import wctc_refs as WR
from cabi_header import assert_binding_is_header, header_abi
from conftest import ROOT, load_golden

HEADER, PREFIX = 'sconf_wctc.h', 'sconf_wctc_'
NAMES = {'sconf_wctc_max_labels', 'sconf_wctc_workspace', 'sconf_wctc_fwd', 'sconf_wctc_bwd'}
FX = load_golden('wctc_cases')
CASES = [str(c) for c in FX['cases']]


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from lcasr_amd.hip import wctc
    return wctc.load()


def case_inputs(c):
    return FX[f'{c}.lp'], FX[f'{c}.targets'], FX[f'{c}.input_lengths'], FX[f'{c}.target_lengths'], int(FX[f'{c}.blank'])


# ---- 1. the restatement is the reference's function ---------------------------------------------------------------------------------
def test_the_fixture_holds_the_cases_the_tests_rely_on():
    assert len(CASES) >= 7
    shapes = {c: FX[f'{c}.lp'].shape for c in CASES}
    assert all(B <= 3 and N <= 64 and C <= 12 for B, N, C in shapes.values())
    tl = {c: FX[f'{c}.target_lengths'] for c in CASES}
    assert any(shapes[c][1] == 1 and tl[c].max() == 1 for c in CASES) and any(tl[c].max() == 1 and shapes[c][1] > 1 for c in CASES)
    blanks = {(int(FX[f'{c}.blank']), shapes[c][2]) for c in CASES}
    assert any(b == 0 for b, _ in blanks) and any(b == C - 1 for b, C in blanks) and any(0 < b < C - 1 for b, C in blanks)
    assert any((FX[f'{c}.targets'] < 0).any() for c in CASES) and any(len(set(tl[c].tolist())) > 1 for c in CASES)
    assert any((FX[f'{c}.input_lengths'] != shapes[c][1]).any() for c in CASES)                      # a ragged batch
    def tight(c):                                                                                   # T exactly labels + repeats
        t = FX[f'{c}.targets'][0, :tl[c][0]]
        return shapes[c][1] == len(t) + int((t[1:] == t[:-1]).sum())
    assert any(tight(c) for c in CASES) and any((FX[f'{c}.targets'][:, 1:] == FX[f'{c}.targets'][:, :-1]).any() for c in CASES)


@pytest.mark.parametrize('mode', WR.MODES)
@pytest.mark.parametrize('case', CASES)
def test_restatement_reproduces_the_reference(case, mode):
    lp, tg, il, tl, blank = case_inputs(case)
    nll, grad, info = WR.wctc(lp, tg, il, tl, blank, mode)
    rl, rg = FX[f'{case}.{mode}.loss'], FX[f'{case}.{mode}.grad']
    assert np.abs(nll - rl).max() <= 1e-10 * np.abs(rl).max(), (nll, rl)
    assert np.abs(grad - rg).max() <= 1e-10 * np.abs(rg).max()
    if mode == 'max_prob':                                                # no near-tie decides a test
        for e, _ in info:
            top = np.sort(e[np.isfinite(e)])[::-1]
            assert len(top) < 2 or top[0] - top[1] > 1e-3


def test_restatement_departures():
    lp, tg, il, tl, blank = case_inputs('ragged_batch')
    nll, grad, _ = WR.wctc(lp, tg, np.array([24, 2, 0]), tl, blank, 'soft')                  # 3 labels in 2 frames; no frames at all
    assert np.isfinite(nll[0]) and nll[1] == np.inf and nll[2] == np.inf and not grad[1:].any()
    nll, grad, _ = WR.wctc(lp, tg, il, np.array([6, 0, 4]), blank, 'sum_prob')               # an empty transcript poisons its sample only
    assert np.isnan(nll[1]) and np.isnan(grad[1, :17]).all() and not grad[1, 17:].any() and np.isfinite(nll[[0, 2]]).all()
    g2 = WR.wctc(lp, tg, il, tl, blank, 'soft', grad_out=np.array([2.0, 0.0, -1.0]))[1]
    g1 = WR.wctc(lp, tg, il, tl, blank, 'soft')[1]
    assert np.array_equal(g2[0], 2 * g1[0]) and not g2[1].any() and np.array_equal(g2[2], -g1[2])
    e, w = WR.wctc(lp, tg, il, tl, blank, 'soft')[2][0]
    assert (w < 0).any() and not np.isfinite(e[:2]).any() and not w[:2].any()                 # signed weights; dead early frames take no part


# ---- 2. the unit: header, binding, exports ------------------------------------------------------------------------------------------
def _declared():
    src = open(os.path.join(ROOT, 'include', HEADER)).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(sconf_[a-z0-9_]+)\s*\(', src)))


def test_binding_is_the_header_and_the_core_does_not_name_it(lib):
    from lcasr_amd.hip import _lib, wctc
    funcs, enums = header_abi(HEADER, PREFIX)
    assert sorted(funcs) == _declared() and set(funcs) == NAMES
    assert_binding_is_header(funcs, wctc.PROTOTYPES, wctc.PLAIN, 'hip/wctc.py')
    assert enums == {'SCONF_WCTC_' + k.upper(): v for k, v in wctc.MODES.items()} and tuple(wctc.MODES) == WR.MODES
    assert not any(n.startswith(PREFIX) for n in list(_lib.PROTOTYPES) + list(_lib.PLAIN))
    for f in (os.path.join('include', 'sconf.h'), os.path.join('long-context-asr_amd', 'hip', '_lib.py')):
        assert 'wctc' not in open(os.path.join(ROOT, f)).read(), f
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in _declared():
        assert hasattr(raw, n), f'{n} declared in include/{HEADER} but not exported'
        assert n in _lib.bound()
    assert lib.sconf_version() == 220


def test_exports_where_ctc_loss_is_exported():
    from lcasr_amd import functional as Fn, losses
    assert issubclass(losses.WCTCLoss, torch.nn.CTCLoss) and callable(losses.wctc_loss) and losses.CTCLoss is not None
    assert losses.WCTCLoss().mode == 'soft' and losses.WCTCLoss(blank=3, mode='max_prob').blank == 3
    assert callable(Fn.wctc_nll) and issubclass(Fn.WCTCFn, torch.autograd.Function)
    with pytest.raises(ValueError, match='mode'):
        losses.WCTCLoss(mode='hard')


# ---- 3. refusals that need no GPU ---------------------------------------------------------------------------------------------------
def test_queries_answer_on_the_host(lib):
    from lcasr_amd.hip import wctc
    assert lib.sconf_wctc_max_labels() == wctc.MAX_LABELS >= 2048
    B, N, S = 3, 40, 6
    W = 2 * S + 1
    r = lambda n: (n + 255) // 256 * 256
    for mode, K in ((0, 2), (1, 1), (2, 1)):
        assert lib.sconf_wctc_workspace(B, N, S, mode) == 2 * r(B * N * W * 4) + r(B * N * W * 8) + 2 * r(B * N * 8) + r(K * B * N * 8) + r(B * 8)
    assert lib.sconf_wctc_workspace(128, 2048, 512, 0) > 1 << 31
    for bad in ((0, N, S, 0), (B, 0, S, 0), (B, N, 0, 0), (B, N, wctc.MAX_LABELS + 1, 0), (B, N, S, 3), (B, N, S, -1), (1 << 20, 1 << 11, S, 0)):
        assert lib.sconf_wctc_workspace(*bad) == -1, bad
    assert lib.sconf_wctc_workspace(1, 1, wctc.MAX_LABELS, 0) > 0
    with pytest.raises(ValueError, match='invalid sizes'):
        wctc.workspace_bytes(1, 1, 0, 'soft')


def test_host_side_validation_sets_the_error_before_any_launch(lib):
    """Every refusal happens before a kernel is enqueued, so none needs a GPU: the pointers are host addresses that are never read."""
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    B, N, C, S = 2, 16, 8, 3
    nb = lib.sconf_wctc_workspace(B, N, S, 0)
    ok = dict(lp=p, tg=p, il=p, tl=p, out=p, ws=p, nb=nb, B=B, N=N, C=C, S=S, blank=0, mode=0)

    def fwd(**kw):
        a = dict(ok, **kw)
        return lib.sconf_wctc_fwd(a['lp'], a['tg'], a['il'], a['tl'], a['out'], a['ws'], a['nb'], a['B'], a['N'], a['C'], a['S'], a['blank'], a['mode'], None)

    def bwd(**kw):
        a = dict(ok, **kw)
        return lib.sconf_wctc_bwd(a['tg'], a['il'], a['tl'], None, a['out'], a['ws'], a['nb'], a['B'], a['N'], a['C'], a['S'], a['blank'], a['mode'], None)

    for call in (fwd, bwd):
        for kw, word in ((dict(mode=3), b'bad mode'), (dict(C=6), b'multiple of 4'), (dict(S=lib.sconf_wctc_max_labels() + 1), b'labels'),
                         (dict(S=0), b'labels'), (dict(tg=None), b'null pointer'), (dict(ws=None), b'null pointer'), (dict(out=None), b'null pointer'),
                         (dict(nb=nb - 1), b'workspace'), (dict(blank=C), b'blank'), (dict(B=0), b'at least 1')):
            assert call(**kw) != 0 and word in lib.sconf_last_error(), (call.__name__, kw, lib.sconf_last_error())
    assert fwd(lp=None) != 0 and b'null pointer' in lib.sconf_last_error()


def test_python_layer_refuses_bad_host_arguments():
    from lcasr_amd import functional as Fn
    lp = torch.zeros(2, 8, 5)
    il, tl = torch.tensor([8, 8]), torch.tensor([2, 1])
    tg = torch.tensor([[1, 2], [3, -1]])
    with pytest.raises(ValueError, match='mode'):
        Fn.wctc_nll(lp, tg, il, tl, 0, 'hard')
    with pytest.raises(ValueError, match='at least 1'):
        Fn.wctc_nll(lp, tg, il, torch.tensor([2, 0]), 0)
    with pytest.raises(ValueError, match='labels must be in'):
        Fn.wctc_nll(lp, torch.tensor([[1, 5], [3, -1]]), il, tl, 0)
    with pytest.raises(ValueError, match='labels must be in'):
        Fn.wctc_nll(lp, torch.tensor([[1, -1], [3, -1]]), il, tl, 0)                          # negative INSIDE the transcript is no padding
    with pytest.raises(ValueError, match='input_lengths'):
        Fn.wctc_nll(lp, tg, torch.tensor([9, 8]), tl, 0)
    with pytest.raises(ValueError, match='do not fit'):
        Fn.wctc_nll(lp, torch.tensor([1, 2]), il, tl, 0)                                      # 1-D targets shorter than the lengths say
    with pytest.raises(ValueError, match='at most'):
        Fn.wctc_nll(torch.zeros(1, 8, 4), torch.zeros(1, 3000, dtype=torch.long), torch.tensor([8]), torch.tensor([3000]), 0)
    with pytest.raises(RuntimeError, match='GPU'):                                            # valid arguments reach the op layer: no CPU fallback
        Fn.wctc_nll(lp, tg, il, tl, 0)
    with pytest.raises(RuntimeError, match='GPU'):
        Fn.wctc_nll(lp, torch.tensor([1, 2, 3]), il, tl, 0)                                   # 1-D concatenated targets are accepted


def test_wctc_loss_on_a_cpu_tensor_raises():
    from lcasr_amd.losses import WCTCLoss, wctc_loss
    lp = torch.zeros(8, 2, 5)                                                                  # (T, B, C), as the reference takes it
    args = (torch.tensor([[1, 2], [3, -1]]), torch.tensor([8, 8]), torch.tensor([2, 1]))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        wctc_loss(lp, *args)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        WCTCLoss(mode='sum_prob')(lp, *args)


def test_trainer_refuses_the_wildcard_with_the_fused_loss():
    from lcasr_amd.train import Trainer
    with pytest.raises(ValueError, match='fused_loss=False'):
        Trainer(None, wildcard='soft', fused_loss=True)
    with pytest.raises(ValueError, match='mode'):
        Trainer(None, wildcard='hard', fused_loss=False)
