"""CPU checks of the write-footprint cases of the wild-card CTC loss (tests/wctc_footprint_cases.py): every launching entry point has
a case, every case is laid out soundly and declares what the restatement returns, and the cases cover the launch forms.  The cases
run on the device from tests/test_wctc_gpu.py."""
import pytest
import torch

import footprint as FP
import wctc_footprint_cases as WC


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from lcasr_amd.hip import wctc
    return wctc.load()


def test_every_entry_point_has_a_case_or_launches_nothing():
    from lcasr_amd.hip import wctc
    assert WC.NO_LAUNCH == set(wctc.PLAIN)
    assert {entry for entry, _ in WC.CASES.values()} == set(wctc.PROTOTYPES)
    assert WC.MODE_ID == wctc.MODES


@pytest.mark.parametrize('id', list(WC.CASES))
def test_case_layout(lib, id):
    from lcasr_amd.hip import wctc
    c = WC.build(id, lib)
    assert c.name == WC.CASES[id][0]
    FP.check_layout(c, wctc.PROTOTYPES)
    regions = c.arena.regions
    nbytes, B, N, C, S, blank, mode = c.args[-7:]
    ws = regions['workspace']
    assert ws.cls == FP.SCRATCH and ws.dtype == torch.uint8 and ws.numel == nbytes == lib.sconf_wctc_workspace(B, N, S, mode)
    want = {'nll': (B,)}
    if c.name == 'sconf_wctc_bwd':
        want['grad'] = (B, N, C)
        assert [name for name, _ in c.before] == ['sconf_wctc_fwd'] and c.before[0][1][5] is ws and c.args[5] is ws      # one workspace for both
        assert ('grad_out' in regions) == (c.args[3] is not None)
    for name, shape in want.items():
        r = regions[name]
        assert r.cls == FP.OUT and r.shape == shape and r.dtype == torch.float32 and r.unspecified is None and r.order is None
    assert {n for n, r in regions.items() if r.cls != FP.IN} == set(want) | {'workspace'}
    assert not c.unvalued


def test_the_cases_cover_the_launch_forms(lib):
    built = [WC.build(id, lib) for id in WC.CASES]
    fwd, bwd = ([c for c in built if c.name == n] for n in ('sconf_wctc_fwd', 'sconf_wctc_bwd'))
    assert {c.args[-1] for c in fwd} == {c.args[-1] for c in bwd} == {0, 1, 2}                      # each mode, both ways
    assert {c.args[3] is None for c in bwd} == {True, False}                                      # grad_out null and given
    ragged = lambda c: len(set(c.arena.regions['input_lengths'].init.tolist())) > 1
    assert any(ragged(c) for c in fwd) and any(ragged(c) for c in bwd)
    for c in bwd:                                                                                  # an infeasible sample: +inf, zero rows
        if 'infeasible' in c.id:
            out = c.ref({n: r.init for n, r in c.arena.regions.items() if torch.is_tensor(r.init)})
            assert torch.isinf(out['nll'][-1]) and not out['grad'][-1].any() and torch.isfinite(out['nll'][:-1]).all()
    assert sum('infeasible' in c.id for c in bwd) >= 3
    assert {(2 * c.args[-3] + 1 > 1024) for c in built} == {True, False}                          # one and two lattice states per thread
    assert any((c.arena.regions['targets'].init < 0).any() for c in built)                        # negative padding
