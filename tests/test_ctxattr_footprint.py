"""CPU checks of the write-footprint cases of context attribution (tests/ctxattr_footprint_cases.py): every launching entry point has
a case, every case is laid out soundly and declares what the restatement returns, and the cases cover the launch forms.  The cases
run on the device from tests/test_ctxattr_gpu.py."""
import ctypes

import pytest
import torch

import ctxattr_footprint_cases as XC
import footprint as FP


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from lcasr_amd.hip import ctxattr
    return ctxattr.load()


def test_every_entry_point_has_a_case_or_launches_nothing():
    from lcasr_amd.hip import ctxattr
    assert XC.NO_LAUNCH == set(ctxattr.PLAIN)
    assert {entry for entry, _ in XC.CASES.values()} == set(ctxattr.PROTOTYPES)


@pytest.mark.parametrize('id', list(XC.CASES))
def test_case_layout(lib, id):
    from lcasr_amd.hip import ctxattr
    c = XC.build(id, lib)
    assert c.name == XC.CASES[id][0]
    FP.check_layout(c, ctxattr.PROTOTYPES)
    regions = c.arena.regions
    if c.name == 'sconf_ctxattr_window_means':
        assert {n for n, r in regions.items() if r.cls != FP.IN} == {'means'} and regions['means'].shape == (c.args[5],)
    elif c.name == 'sconf_ctxattr_mask_fill':
        F, T, J, j0, b = c.args[4:9]
        assert {n for n, r in regions.items() if r.cls != FP.IN} == {'dst'} and regions['dst'].shape == (b, F, T) and 0 <= j0 and j0 + b <= J
    else:
        N, I, J, R, cap = c.args[11:16]
        ws = regions['workspace']
        assert ws.cls == FP.SCRATCH and ws.dtype == torch.uint8 and ws.numel == c.args[10] == lib.sconf_ctxattr_score_workspace(N, I, J, R)
        want = {'errors': (I, J), 'clean_errors': (1,), 'clean_len': (1,), 'mid_len': (I, J)}
        if c.args[8] is not None: want['mid_tokens'] = (I, J, cap)
        for name, shape in want.items():
            r = regions[name]
            assert r.cls == FP.OUT and r.shape == shape and r.dtype == torch.int32 and r.unspecified is None and r.order is None
        assert {n for n, r in regions.items() if r.cls != FP.IN} == set(want) | {'workspace'}
        assert isinstance(c.args[3], ctypes.Array) and len(c.args[3]) == 2 * I                 # the host array
        assert ('ref' in regions) == (R > 0)


def test_the_cases_cover_the_launch_forms(lib):
    built = [XC.build(id, lib) for id in XC.CASES]
    score = [c for c in built if c.name == 'sconf_ctxattr_score']
    geo = {(lib.sconf_ctxattr_threads(c.args[14]), lib.sconf_ctxattr_cells_per_thread(c.args[14])) for c in score}
    assert {(64, 1), (128, 1), (256, 1), (512, 1), (1024, 1), (1024, 2)} <= geo          # every workgroup size of the pair kernel
    assert {c.args[8] is None for c in score} == {True, False}                           # mid_tokens NULL and given
    windows = [list(c.args[3]) for c in score]
    assert any(w[2 * i] == w[2 * i + 1] for w in windows for i in range(len(w) // 2))    # an empty window
    assert any(c.args[14] == 0 for c in score)
    fill = [c for c in built if c.name == 'sconf_ctxattr_mask_fill']
    assert {c.args[5] % 4 == 0 for c in fill} == {True, False} and {c.args[8] for c in fill} >= {1, 3} and any(c.args[7] > 0 for c in fill)
