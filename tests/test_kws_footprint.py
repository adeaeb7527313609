"""CPU checks of the write-footprint cases of the keyword-search unit (tests/kws_footprint_cases.py): the launching entry point of
lcasr_amd.hip.kws has its cases, every query is known to launch nothing, and every case is laid out on a CPU arena - regions
disjoint, aligned and guarded, the argument list as the binding types it, the declared output shapes the shapes the restatement
returns, the three outputs declared OUT at tol = 0, the workspace declared scratch at exactly what the query says, the inputs and
the image IN, NaN in the columns behind `classes`.  The library builds here as test_cabi.py builds it; the queries are host-only."""
import pytest
import torch

import footprint as FP
import kws_footprint_cases as KC
import kws_refs as KR


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from lcasr_amd.hip import kws
    return kws.load()


def test_every_kws_entry_point_has_a_case_or_launches_nothing():
    from lcasr_amd.hip import kws
    assert KC.NO_LAUNCH == set(kws.PLAIN)
    assert {entry for entry, _ in KC.CASES.values()} == set(kws.PROTOTYPES)


@pytest.mark.parametrize('id', list(KC.CASES))
def test_kws_case_layout(lib, id):
    from lcasr_amd.hip import kws
    c = KC.build(id, lib)
    assert c.name == KC.CASES[id][0] == 'sconf_kws_search'
    FP.check_layout(c, kws.PROTOTYPES)
    R = c.arena.regions
    n_waves, U, K = c.args[3:6]
    cap = c.args[9]
    B, N, C, classes, blank = c.args[12:17]
    ws = R['workspace']
    assert ws.cls == FP.SCRATCH and ws.dtype == torch.uint8 and ws.numel == ws.extent == c.args[11] == lib.sconf_kws_workspace(B, N, U)
    want = {'hit_frames': ((B, K, cap, 2), torch.int32), 'hit_score': ((B, K, cap), torch.float32), 'hit_count': ((B, K), torch.int32)}
    assert {n for n, r in R.items() if r.cls != FP.IN} == set(want) | {'workspace'}
    for name, (shape, dtype) in want.items():
        r = R[name]
        assert r.cls == FP.OUT and r.shape == shape and r.dtype == dtype and r.tol == 0.0 and r.unspecified is None and r.order is None
    assert R['image'].cls == FP.IN and R['image'].numel == n_waves * 256 + U and R['x'].cls == FP.IN and R['x'].shape == (B, N, C)
    assert ('input_lengths' in R) == (c.args[1] is not None)
    x = R['x'].init
    assert 1 <= classes <= C and 0 <= blank < classes and not bool(torch.isnan(x[..., :classes]).any())
    assert C == classes or bool(torch.isnan(x[..., classes:]).all())


def _cpu_launch(name, args, buf, views, leak=False):
    """The lane-by-lane restatement of tests/kws_refs.py in the kernels' place; leak: a kernel that reads what it must not."""
    x = views['x']
    classes = args[15]
    il = views.get('input_lengths')
    if leak:                                                               # one column too many, or the frames behind a length
        if x.shape[2] > classes: classes += 1
        else: x = torch.roll(x, 1, 1); il = None
    out = KR.search(x, views['image'], args[3], args[4], args[5], args[16], il, args[9], classes)
    for k, t in out._asdict().items(): views[k].copy_(t)


@pytest.mark.parametrize('id', list(KC.CASES))
def test_kws_case_passes_with_the_restatement_as_the_kernel(lib, id):
    """The harness on a CPU arena with the restatement in the kernel's place: the case's own checks hold for a correct evaluation and
    fail for one that reads what it must not."""
    c = KC.build(id, lib)
    figures = FP.run_case(c, 'cpu', launch=_cpu_launch)
    assert len(figures['valued']) == 3 and all(v.endswith('=0.0e+00') for v in figures['valued'])
    with pytest.raises(FP.FootprintError):
        FP.run_case(c, 'cpu', launch=lambda *a: _cpu_launch(*a, leak=True))


def test_the_cases_cover_what_the_kernels_distinguish(lib):
    cases = {id: KC.build(id, lib) for id in KC.CASES}
    classes = {c.args[15] for c in cases.values()}
    assert min(classes) <= 64 and any(64 < v <= 256 for v in classes) and any(256 < v <= 1024 for v in classes) and max(classes) > 1024
    assert {c.args[14] - c.args[15] for c in cases.values()} >= {0, 15}                      # rows of `classes` and of `classes` + 15
    assert {1, 4, 5} <= {c.args[4] for c in cases.values()}                                 # columns: one, a whole quad, a quad and one
    assert {c.args[3] > 1 for c in cases.values()} == {True, False} and {c.args[1] is None for c in cases.values()} == {True, False}
    reached = False
    for c in cases.values():
        out = c.ref({n: r.init for n, r in c.arena.regions.items() if torch.is_tensor(r.init)})
        assert int(out['hit_count'].sum()) > 0, c.id
        reached |= bool((out['hit_count'] > c.args[9]).any()) and bool((out['hit_count'] < c.args[9]).any())
        if 'input_lengths' in c.arena.regions and 0 in c.arena.regions['input_lengths'].init.tolist():
            assert not bool(out['hit_count'][c.arena.regions['input_lengths'].init == 0].any())
    assert reached
