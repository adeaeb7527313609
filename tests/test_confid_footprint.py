"""CPU checks of the write-footprint cases of the confidence unit (tests/confid_footprint_cases.py): every launching entry point of
lcasr_amd.hip.confid has a case, every query is known to launch nothing, and every case is laid out on a CPU arena - regions
disjoint, aligned and guarded, the argument list as the binding types it, NaN in the columns behind `classes`, outputs of exactly
S_cap labels.  The library builds here as test_cabi.py builds it; the queries are host-only."""
import numpy as np
import pytest
import torch

import confid_footprint_cases as CC
import confid_refs as CR
import footprint as FP


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from lcasr_amd.hip import confid
    return confid.load()


def test_every_confid_entry_point_has_a_case_or_launches_nothing():
    from lcasr_amd.hip import confid
    assert CC.NO_LAUNCH == set(confid.PLAIN)
    assert {entry for entry, _ in CC.CASES.values()} == set(confid.PROTOTYPES)
    assert (CC.METHOD, CC.NORM, CC.AGG) == (confid.METHOD, confid.NORM, confid.AGGREGATION)


@pytest.mark.parametrize('id', list(CC.CASES))
def test_confid_case_layout(lib, id):
    from lcasr_amd.hip import confid
    c = CC.build(id, lib)
    assert c.name == CC.CASES[id][0]
    FP.check_layout(c, confid.PROTOTYPES)
    R = c.arena.regions
    writable = {n: r.cls for n, r in R.items() if r.cls != FP.IN}
    if c.name == 'sconf_confid_frames':
        M, classes, stride = c.args[1:4]
        assert writable == {'idx': FP.OUT, 'conf': FP.OUT} and R['idx'].shape == R['conf'].shape == (M,) and stride > classes
        x = R['x'].init
        assert bool(torch.isnan(x[:, classes:]).all()) and not bool(torch.isnan(x[:, :classes]).any()) and bool(torch.isinf(x[1]).any())
    elif c.name == 'sconf_confid_runs':
        B, N, s_cap = c.args[2], c.args[3], c.args[8]
        assert writable == {'targets': FP.OUT, 'spans': FP.OUT, 'target_lengths': FP.OUT}
        assert R['targets'].shape == (B, s_cap) and R['spans'].shape == (B, s_cap, 3) and N > lib.sconf_confid_scan_chunk()
        tl = CR.runs(R['idx'].init.numpy(), R['lengths'].init.tolist(), c.args[4], s_cap)[2].tolist()
        assert -1 in tl and any(0 < n < s_cap for n in tl)
    else:
        assert writable == {'out': FP.OUT} and R['out'].shape == (c.args[5],)
        sp = R['spans'].init
        assert bool(((sp[:, 0] >= 0) & (sp[:, 1] <= c.args[3]) & (sp[:, 0] < sp[:, 1])).all())
        assert {1, 63, 64, 65, 1000} <= set((sp[:, 1] - sp[:, 0]).tolist())


def _cpu_launch(name, args, buf, views, leak=False):
    """The restatements of tests/confid_refs.py in the kernels' place; leak: a kernel that reads past what the header lets it read."""
    if name == 'sconf_confid_frames':
        classes = args[2] + (1 if leak else 0)                             # one guard column
        method, norm = [k for k, v in CC.METHOD.items() if v == args[4]][0], [k for k, v in CC.NORM.items() if v == args[5]][0]
        idx, conf = CR.frames(views['x'].numpy(), classes, method, norm, args[6])
        views['idx'].copy_(torch.from_numpy(idx)); views['conf'].copy_(torch.from_numpy(conf.astype(np.float32)))
    elif name == 'sconf_confid_runs':
        N = args[3]
        lens = [N] * args[2] if leak else views['lengths'].tolist()       # frames behind a length
        tg, sp, tl = CR.runs(views['idx'].numpy(), lens, args[4], args[8])
        views['targets'].copy_(torch.from_numpy(tg)); views['spans'].copy_(torch.from_numpy(sp)); views['target_lengths'].copy_(torch.from_numpy(tl))
    else:
        agg = [k for k, v in CC.AGG.items() if v == args[6]][0]
        spans = views['spans'].clone()
        if leak: spans[2:, 1] += 1                                          # one frame behind a span (behind `values` for the last one)
        vals = torch.cat([views['values'], torch.full((1,), 0.01)]).numpy()
        idx = torch.cat([views['idx'], torch.full((1,), 2, dtype=torch.int32)]).numpy() if 'idx' in views else None
        out = CR.aggregate(vals, spans.tolist(), agg, idx, args[2])
        views['out'].copy_(torch.from_numpy(out.astype(np.float32)))


@pytest.mark.parametrize('id', list(CC.CASES))
def test_confid_case_passes_with_the_restatement_as_the_kernel(lib, id):
    """The harness on a CPU arena with the restatement in the kernel's place: the case's own checks hold for a correct evaluation,
    and fail for one that reads a guard column, frames behind a length, or a frame behind a span."""
    c = CC.build(id, lib)
    figures = FP.run_case(c, 'cpu', launch=_cpu_launch)
    assert len(figures['valued']) == {'sconf_confid_frames': 2, 'sconf_confid_runs': 3, 'sconf_confid_aggregate': 1}[c.name]
    assert all(v.endswith('=0.0e+00') for v in figures['valued'])
    with pytest.raises(FP.FootprintError):
        FP.run_case(c, 'cpu', launch=lambda *a: _cpu_launch(*a, leak=True))


def test_the_cases_cover_what_the_kernels_distinguish(lib):
    cases = {id: CC.build(id, lib) for id in CC.CASES}
    cap = lib.sconf_confid_row_capacity()
    f = [c for c in cases.values() if c.name == 'sconf_confid_frames']
    classes = sorted(c.args[2] for c in f)
    block = lib.sconf_confid_block_capacity()
    edges = [0, 64, 128, 192, 256, 512, cap, block, 2 ** 30]                                     # one case between every two changes of geometry
    assert len(classes) == 8 and all(lo < c <= hi for lo, c, hi in zip(edges, classes, edges[1:])) and classes[5] == cap
    assert {c.args[3] % 4 == 0 for c in f} == {True, False} and {c.args[4] for c in f} == {0, 1, 2, 3} and {c.args[5] for c in f} == {0, 1}
    assert any(c.args[2] % 4 for c in f if c.args[3] % 4 == 0)                                    # a partial quad on the 16-byte path
    g = [c for c in cases.values() if c.name == 'sconf_confid_aggregate']
    assert {c.args[1] is None for c in g} == {True, False} and len({c.args[6] for c in g}) == 3
