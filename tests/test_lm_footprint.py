"""CPU checks of the write-footprint cases of the LM-fused beam search's ABI unit (tests/lm_footprint_cases.py): every launching entry
point of lcasr_amd.hip.lm has a case, and every case is laid out on a CPU arena - regions disjoint, aligned and guarded, the argument
list as the binding types it, the declared output shapes the shapes the restatement returns, all six outputs declared OUT, the
workspace declared scratch at exactly what the query says, the image and the log-probs inputs.  The library builds here as
test_cabi.py builds it."""
import ctypes

import pytest
import torch

import footprint as FP
import lm_footprint_cases as LC


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from lcasr_amd.hip import lm
    return lm.load()


def test_every_lm_entry_point_has_a_case_or_launches_nothing():
    from lcasr_amd.hip import lm
    assert LC.NO_LAUNCH == set(lm.PLAIN)
    assert {entry for entry, _ in LC.CASES.values()} == set(lm.PROTOTYPES)


@pytest.mark.parametrize('id', list(LC.CASES))
def test_lm_case_layout(lib, id):
    from lcasr_amd.hip import lm
    c = LC.build(id, lib)
    assert c.name == LC.CASES[id][0]
    FP.check_layout(c, lm.PROTOTYPES)
    proto = lm.PROTOTYPES['sconf_lm_beam_ctc']
    assert proto[22] is ctypes.c_float and proto[23] is proto[26] is proto[27] is ctypes.c_double
    assert all(isinstance(c.args[i], float) for i in (22, 23, 26, 27))
    S, E, V, order, start = c.args[3:8]
    B, N, C, blank, W, nbest = c.args[16:22]
    Kmax, Lmax = c.args[24:26]
    im = c.arena.regions['image']
    assert im.cls == FP.IN and im.dtype == torch.int32 and im.numel == 4 * S + 4 * E + 2 * V and im.offset % 16 == 0
    assert 1 <= order <= lib.sconf_lm_max_order() and 0 <= start < S and V <= C and blank >= V
    ws = c.arena.regions['workspace']
    assert ws.cls == FP.SCRATCH and ws.dtype == torch.uint8 and ws.numel == ws.extent == c.args[15] == lib.sconf_lm_beam_workspace(B, N, W, Kmax)
    want = {'count': ((B,), torch.int32), 'tokens': ((B, nbest, Lmax), torch.int32), 'lengths': ((B, nbest), torch.int32),
            'token_frames': ((B, nbest, Lmax), torch.int32), 'scores': ((B, nbest), torch.float64),
            'logit_scores': ((B, nbest), torch.float64)}
    for name, (shape, dtype) in want.items():
        r = c.arena.regions[name]
        assert r.cls == FP.OUT and r.shape == shape and r.dtype == dtype and r.unspecified is None and r.order is None
    assert {n for n, r in c.arena.regions.items() if r.cls != FP.IN} == set(want) | {'workspace'}
    assert ('input_lengths' in c.arena.regions) == (c.args[1] is not None)


def test_the_cases_cover_the_launch_forms(lib):
    """Every workgroup size of the search kernel, a hypothesis longer than Lmax, an empty sample, ranks behind `count`, and an LM
    that changes the result (scores differ from logit_scores)."""
    threads, long_one, empty, unused, lm_on = set(), False, False, False, False
    for id in LC.CASES:
        c = LC.build(id, lib)
        threads.add(lib.sconf_lm_beam_threads(c.args[20], c.args[24]))
        out = c.ref({n: r.init for n, r in c.arena.regions.items() if torch.is_tensor(r.init)})
        long_one |= bool((out['lengths'] > c.args[25]).any())
        empty |= 'input_lengths' in c.arena.regions and 0 in c.arena.regions['input_lengths'].init.tolist()
        unused |= bool((out['count'] < c.args[21]).any())
        lm_on |= bool((out['scores'][:, 0] != out['logit_scores'][:, 0]).any())
        assert bool(torch.isfinite(out['scores'][:, 0]).all())               # (no poisoned sample: the harness reads NaN as "unwritten")
    assert threads == {64, 128, 256, 512, 1024} and long_one and empty and unused and lm_on
