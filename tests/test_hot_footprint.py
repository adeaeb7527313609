"""CPU checks of the write-footprint cases of the hotword beam search's ABI unit (tests/hot_footprint_cases.py): every launching entry
point of lcasr_amd.hip.hot has a case, and every case is laid out on a CPU arena - regions disjoint, aligned and guarded, the argument
list as the binding types it, the declared output shapes the shapes the restatement returns, all seven outputs declared OUT, the
workspace declared scratch at exactly what the query says, the two images and the log-probs inputs.  The library builds here as
test_cabi.py builds it."""
import ctypes

import pytest
import torch

import footprint as FP
import hot_footprint_cases as HC


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from lcasr_amd.hip import hot
    return hot.load()


def test_every_hot_entry_point_has_a_case_or_launches_nothing():
    from lcasr_amd.hip import hot
    assert HC.NO_LAUNCH == set(hot.PLAIN)
    assert {entry for entry, _ in HC.CASES.values()} == set(hot.PROTOTYPES)


@pytest.mark.parametrize('id', list(HC.CASES))
def test_hot_case_layout(lib, id):
    from lcasr_amd.hip import hot
    c = HC.build(id, lib)
    assert c.name == HC.CASES[id][0]
    FP.check_layout(c, hot.PROTOTYPES)
    proto = hot.PROTOTYPES['sconf_hot_beam_ctc']
    assert proto[28] is ctypes.c_float and proto[12] is proto[29] is proto[32] is proto[33] is ctypes.c_double
    assert all(isinstance(c.args[i], float) for i in (12, 28, 29, 32, 33))
    S, E, V, order, start = c.args[3:8]
    HS, HE, hlen, weight = c.args[9:13]
    B, N, C, blank, W, nbest = c.args[22:28]
    Kmax, Lmax = c.args[30:32]
    hi = c.arena.regions['hot_image']
    assert hi.cls == FP.IN and hi.dtype == torch.int32 and hi.numel == 6 * HS + 2 * HE and hi.offset % 16 == 0
    assert HS > 1 and 1 <= hlen <= lib.sconf_hot_max_len() and weight > 0
    tokens = hi.init[6 * HS:].reshape(-1, 2)[:, 0]
    assert int(tokens.max()) < C and not bool((tokens == blank).any())       # no phrase holds the blank or a class outside the model's
    if c.args[2] is None:
        assert (S, E, V, order, start) == (0, 0, 0, 0, 0) and 'lm_image' not in c.arena.regions
    else:
        im = c.arena.regions['lm_image']
        assert im.cls == FP.IN and im.dtype == torch.int32 and im.numel == 4 * S + 4 * E + 2 * V and im.offset % 16 == 0
        assert 1 <= order <= 5 and 0 <= start < S and V <= C and blank >= V
    ws = c.arena.regions['workspace']
    assert ws.cls == FP.SCRATCH and ws.dtype == torch.uint8 and ws.numel == ws.extent == c.args[21] == lib.sconf_hot_beam_workspace(B, N, W, Kmax)
    want = {'count': ((B,), torch.int32), 'tokens': ((B, nbest, Lmax), torch.int32), 'lengths': ((B, nbest), torch.int32),
            'token_frames': ((B, nbest, Lmax), torch.int32), 'scores': ((B, nbest), torch.float64),
            'logit_scores': ((B, nbest), torch.float64), 'hot_scores': ((B, nbest), torch.float64)}
    for name, (shape, dtype) in want.items():
        r = c.arena.regions[name]
        assert r.cls == FP.OUT and r.shape == shape and r.dtype == dtype and r.unspecified is None and r.order is None
    assert {n for n, r in c.arena.regions.items() if r.cls != FP.IN} == set(want) | {'workspace'}
    assert ('input_lengths' in c.arena.regions) == (c.args[1] is not None)


def test_the_cases_cover_the_launch_forms(lib):
    """Every workgroup size of the search kernel, with and without an LM, a hypothesis longer than Lmax, an empty sample, ranks behind
    `count`, and hotwords that change the result (hot_scores above 0)."""
    threads, lms, long_one, empty, unused, hot_on = set(), set(), False, False, False, False
    for id in HC.CASES:
        c = HC.build(id, lib)
        threads.add(lib.sconf_hot_beam_threads(c.args[26], c.args[30]))
        lms.add(c.args[2] is not None)
        out = c.ref({n: r.init for n, r in c.arena.regions.items() if torch.is_tensor(r.init)})
        long_one |= bool((out['lengths'] > c.args[31]).any())
        empty |= 'input_lengths' in c.arena.regions and 0 in c.arena.regions['input_lengths'].init.tolist()
        unused |= bool((out['count'] < c.args[27]).any())
        hot_on |= bool((out['hot_scores'][:, 0] > 0).any())
        assert bool(torch.isfinite(out['scores'][:, 0]).all())               # (no poisoned sample: the harness reads NaN as "unwritten")
    assert threads == {64, 128, 256, 512, 1024} and lms == {False, True} and long_one and empty and unused and hot_on
