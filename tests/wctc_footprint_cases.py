"""Write-footprint cases of the wild-card CTC loss (include/sconf_wctc.h), laid out with tests/footprint.py: the table that
tests/test_wctc_footprint.py checks on the CPU and tests/test_wctc_gpu.py runs on the device.  TEST INFRASTRUCTURE.

CASES maps a case id to (entry point, builder); builder(lib) needs the library only for the workspace query.  nll and grad are OUT
regions (every element written, from the inputs alone, the same bits in both runs: every sum has a fixed order).  The workspace is
SCRATCH at exactly the queried size: the harness fills it with 0xFF bytes in one run and random bytes in the other, so a frame past a
sample's length, a state past its lattice or a part the forward did not write that the backward reads changes the gradient between
the runs.  A backward case runs the forward first (`before`), into the same workspace.  The restatement is tests/wctc_refs.py."""
import torch

import footprint as FP
import wctc_refs as WR
from footprint import IN, OUT, SCRATCH

NO_LAUNCH = {'sconf_wctc_max_labels', 'sconf_wctc_workspace'}                     # return a value, launch nothing
MODE_ID = {'soft': 0, 'max_prob': 1, 'sum_prob': 2}
CASES = {}


def wctc_case(lib, id, bwd, mode, B, N, C, S, input_lengths, target_lengths, grad_out, blank):
    g = torch.Generator().manual_seed(N + C + S)
    lp = torch.log_softmax(torch.randn(B, N, C, generator=g) * 1.5, -1)
    tg = torch.randint(0, C, (B, S), generator=g, dtype=torch.int32)
    tg[tg == blank] = (blank + 1) % C
    tg[0, 1] = tg[0, 0]                                                           # a repeated label
    for b, n in enumerate(target_lengths): tg[b, n:] = -1                         # negative padding past the transcript
    a = FP.Arena()
    r_lp = a.take('log_probs', (B, N, C), torch.float32, IN, init=lp)
    r_tg = a.take('targets', (B, S), torch.int32, IN, init=tg)
    r_il = a.take('input_lengths', B, torch.int32, IN, init=torch.tensor(input_lengths, dtype=torch.int32))
    r_tl = a.take('target_lengths', B, torch.int32, IN, init=torch.tensor(target_lengths, dtype=torch.int32))
    r_nll = a.take('nll', B, torch.float32, OUT, tol=1e-4)
    nbytes = int(lib.sconf_wctc_workspace(B, N, S, MODE_ID[mode]))
    assert nbytes > 0
    r_ws = a.take('workspace', nbytes, torch.uint8, SCRATCH)
    sizes = [nbytes, B, N, C, S, blank, MODE_ID[mode]]
    fwd_args = [r_lp, r_tg, r_il, r_tl, r_nll, r_ws] + sizes
    variant = f'{mode} lattice of {2 * S + 1}'

    def restate(v, with_grad):
        go = v['grad_out'].numpy() if 'grad_out' in v else None
        nll, grad, _ = WR.wctc(v['log_probs'].numpy(), v['targets'].numpy(), v['input_lengths'].numpy(), v['target_lengths'].numpy(), blank, mode, go)
        out = {'nll': torch.from_numpy(nll)}
        if with_grad: out['grad'] = torch.from_numpy(grad)
        return out

    if not bwd:
        return FP.Case(id, 'sconf_wctc_fwd', a, fwd_args, 'wctc_refs.wctc', lambda v: restate(v, False), variant=variant)
    r_go = a.take('grad_out', B, torch.float32, IN, init=torch.tensor(grad_out, dtype=torch.float32)) if grad_out is not None else None
    r_grad = a.take('grad', (B, N, C), torch.float32, OUT, tol=2e-4)
    args = [r_tg, r_il, r_tl, r_go, r_grad, r_ws] + sizes
    return FP.Case(id, 'sconf_wctc_bwd', a, args, 'wctc_refs.wctc', lambda v: restate(v, True), before=[('sconf_wctc_fwd', fwd_args)], variant=variant)


# (mode, B, N, C, S, input_lengths, target_lengths, grad_out, blank): every mode on a ragged batch whose last sample is infeasible
# (6 labels and a repeat in 5 frames), grad_out null and given; then a lattice of two states per thread.
_RAGGED = (3, 40, 8, 6, [40, 23, 5], [6, 3, 6])
for _m, _go, _blank in (('soft', [1.0, 0.5, 2.0], 7), ('max_prob', None, 0), ('sum_prob', [-1.0, 3.0, 0.25], 3)):
    for _bwd in (False, True):
        _id = f'wctc_{"bwd" if _bwd else "fwd"}-{_m}-ragged-infeasible' + ('' if not _bwd else '-grad_out' if _go else '-null_grad_out')
        CASES[_id] = ('sconf_wctc_bwd' if _bwd else 'sconf_wctc_fwd',
                      lambda lib, _id=_id, _bwd=_bwd, _m=_m, _go=_go, _blank=_blank: wctc_case(lib, _id, _bwd, _m, *_RAGGED, _go, _blank))
CASES['wctc_bwd-soft-null_grad_out'] = ('sconf_wctc_bwd', lambda lib: wctc_case(lib, 'wctc_bwd-soft-null_grad_out', True, 'soft', 2, 24, 12, 4, [24, 19], [4, 2], None, 11))
for _bwd in (False, True):
    _id = f'wctc_{"bwd" if _bwd else "fwd"}-soft-two-states-per-thread'
    CASES[_id] = ('sconf_wctc_bwd' if _bwd else 'sconf_wctc_fwd',
                  lambda lib, _id=_id, _bwd=_bwd: wctc_case(lib, _id, _bwd, 'soft', 2, 640, 8, 513, [640, 300], [513, 100], [1.0, 2.0] if _bwd else None, 0))


def build(id, lib):
    return CASES[id][1](lib)
