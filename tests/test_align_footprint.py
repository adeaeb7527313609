"""CPU checks of the write-footprint cases of the alignment ABI unit (tests/align_footprint_cases.py): every launching entry point
of lcasr_amd.hip.align has a case, and every case is laid out on a CPU arena - regions disjoint, aligned and guarded, the argument
list as the binding types it, the declared output shapes the shapes the restatement returns, all five outputs declared OUT, the
workspace declared scratch at exactly what the query says.  The library builds here as test_cabi.py builds it."""
import pytest
import torch

import align_footprint_cases as AC
import footprint as FP


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from lcasr_amd.hip import align
    return align.load()


def test_every_align_entry_point_has_a_case_or_launches_nothing():
    from lcasr_amd.hip import align
    assert AC.NO_LAUNCH == set(align.PLAIN)
    assert {entry for entry, _ in AC.CASES.values()} == set(align.PROTOTYPES)


@pytest.mark.parametrize('id', list(AC.CASES))
def test_align_case_layout(lib, id):
    from lcasr_amd.hip import align
    c = AC.build(id, lib)
    assert c.name == AC.CASES[id][0]
    FP.check_layout(c, align.PROTOTYPES)
    B, N, C, Smax = c.args[11:15]
    ws = c.arena.regions['workspace']
    assert ws.cls == FP.SCRATCH and ws.dtype == torch.uint8 and ws.numel == ws.extent == c.args[10] == lib.sconf_align_workspace(B, N, Smax)
    want = {'path': ((B, N), torch.int32), 'labels': ((B, N), torch.int32), 'spans': ((B, Smax, 2), torch.int32),
            'token_logp': ((B, Smax), torch.float32), 'score': ((B,), torch.float64)}
    for name, (shape, dtype) in want.items():
        r = c.arena.regions[name]
        assert r.cls == FP.OUT and r.shape == shape and r.dtype == dtype and r.unspecified is None and r.order is None
    assert {n for n, r in c.arena.regions.items() if r.cls != FP.IN} == set(want) | {'workspace'}
    assert ('input_lengths' in c.arena.regions) == (c.args[2] is not None) and ('target_lengths' in c.arena.regions) == (c.args[3] is not None)


def test_the_cases_cover_the_launch_forms(lib):
    geo = {(lib.sconf_align_threads(AC.build(id, lib).args[14]), lib.sconf_align_states_per_thread(AC.build(id, lib).args[14])) for id in AC.CASES}
    assert {(256, 1), (512, 1), (1024, 2)} <= geo
