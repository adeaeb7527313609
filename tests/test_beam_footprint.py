"""CPU checks of the write-footprint cases of the beam-search ABI unit (tests/beam_footprint_cases.py): every launching entry point
of lcasr_amd.hip.beam has a case, and every case is laid out on a CPU arena - regions disjoint, aligned and guarded, the argument
list as the binding types it, the declared output shapes the shapes the restatement returns, all five outputs declared OUT, the
workspace declared scratch at exactly what the query says.  The library builds here as test_cabi.py builds it."""
import ctypes

import pytest
import torch

import beam_footprint_cases as BC
import footprint as FP


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from lcasr_amd.hip import beam
    return beam.load()


def test_every_beam_entry_point_has_a_case_or_launches_nothing():
    from lcasr_amd.hip import beam
    assert BC.NO_LAUNCH == set(beam.PLAIN)
    assert {entry for entry, _ in BC.CASES.values()} == set(beam.PROTOTYPES)


@pytest.mark.parametrize('id', list(BC.CASES))
def test_beam_case_layout(lib, id):
    from lcasr_amd.hip import beam
    c = BC.build(id, lib)
    assert c.name == BC.CASES[id][0]
    FP.check_layout(c, beam.PROTOTYPES)             # (a double argument is a Python float in the case, like a float one)
    assert beam.PROTOTYPES['sconf_beam_ctc'][15] is ctypes.c_float and beam.PROTOTYPES['sconf_beam_ctc'][16] is ctypes.c_double
    assert isinstance(c.args[15], float) and isinstance(c.args[16], float)
    B, N, C, blank, W, nbest = c.args[9:15]
    Kmax, Lmax = c.args[17:19]
    ws = c.arena.regions['workspace']
    assert ws.cls == FP.SCRATCH and ws.dtype == torch.uint8 and ws.numel == ws.extent == c.args[8] == lib.sconf_beam_workspace(B, N, W, Kmax)
    want = {'count': ((B,), torch.int32), 'tokens': ((B, nbest, Lmax), torch.int32), 'lengths': ((B, nbest), torch.int32),
            'token_frames': ((B, nbest, Lmax), torch.int32), 'scores': ((B, nbest), torch.float64)}
    for name, (shape, dtype) in want.items():
        r = c.arena.regions[name]
        assert r.cls == FP.OUT and r.shape == shape and r.dtype == dtype and r.unspecified is None and r.order is None
    assert {n for n, r in c.arena.regions.items() if r.cls != FP.IN} == set(want) | {'workspace'}
    assert ('input_lengths' in c.arena.regions) == (c.args[1] is not None)


def test_the_cases_cover_the_launch_forms(lib):
    """Every workgroup size of the search kernel, a hypothesis longer than Lmax, an empty sample and ranks behind `count`."""
    threads, long_one, empty, unused = set(), False, False, False
    for id in BC.CASES:
        c = BC.build(id, lib)
        threads.add(lib.sconf_beam_threads(c.args[13], c.args[17]))
        out = c.ref({n: r.init for n, r in c.arena.regions.items() if torch.is_tensor(r.init)})
        long_one |= bool((out['lengths'] > c.args[18]).any())
        empty |= 'input_lengths' in c.arena.regions and 0 in c.arena.regions['input_lengths'].init.tolist()
        unused |= bool((out['count'] < c.args[14]).any())
        assert bool(torch.isfinite(out['scores'][:, 0]).all())               # (no poisoned sample: the harness reads NaN as "unwritten")
    assert threads == {64, 128, 256, 512, 1024} and long_one and empty and unused
