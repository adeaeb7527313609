"""CPU checks of the write-footprint cases of the calibration unit (tests/calib_footprint_cases.py): both launching entry points of
lcasr_amd.hip.calib have their cases, every query is known to launch nothing, and every case is laid out on a CPU arena - regions
disjoint, aligned and guarded, the argument list as the binding types it, the declared output shapes the shapes the restatement
returns, every output declared OUT at tol = 0, the alignment's workspace declared scratch at exactly ws_off[P] bytes with every
slice what the query says (less 16 bytes where the case starves a pair), the inputs IN, NaN in the columns behind `classes`.  The
library builds here as test_cabi.py builds it; the queries are host-only."""
import numpy as np
import pytest
import torch

import calib_footprint_cases as KC
import calib_refs as AR
import footprint as FP


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from lcasr_amd.hip import calib
    return calib.load()


def test_every_calib_entry_point_has_a_case_or_launches_nothing():
    from lcasr_amd.hip import calib
    assert KC.NO_LAUNCH == set(calib.PLAIN)
    assert {entry for entry, _ in KC.CASES.values()} == set(calib.PROTOTYPES)


@pytest.mark.parametrize('id', list(KC.CASES))
def test_calib_case_layout(lib, id):
    from lcasr_amd.hip import calib
    c = KC.build(id, lib)
    assert c.name == KC.CASES[id][0]
    FP.check_layout(c, calib.PROTOTYPES)
    R = c.arena.regions
    outs = {n for n, r in R.items() if r.cls != FP.IN}
    for n in outs - {'workspace'}:
        r = R[n]
        assert r.cls == FP.OUT and r.tol == 0.0 and r.unspecified is None and r.order is None
    if c.name == 'sconf_edit_align':
        P = c.args[4]
        ho, ro, wo = (R[n].init.tolist() for n in ('hyp_off', 'ref_off', 'ws_off'))
        assert outs == {'hyp_to_ref', 'ref_to_hyp', 'counts', 'workspace'} and len(ho) == len(ro) == len(wo) == P + 1 and ho[0] == ro[0] == wo[0] == 0
        ws = R['workspace']
        assert ws.cls == FP.SCRATCH and ws.dtype == torch.uint8 and ws.numel == ws.extent == wo[P]
        need = [lib.sconf_edit_align_pair_bytes(ho[p + 1] - ho[p], ro[p + 1] - ro[p]) for p in range(P)]
        got = [wo[p + 1] - wo[p] for p in range(P)]
        assert all(g in (n, n - 16) for g, n in zip(got, need)) and all(o % 16 == 0 for o in wo)
        assert (got != need) == ('too-small' in id)
        assert R['hyp_to_ref'].shape == (ho[P],) and R['ref_to_hyp'].shape == (ro[P],) and R['counts'].shape == (P, 4) and R['counts'].dtype == torch.int64
    else:
        M, classes, C = c.args[1:4]
        K = c.args[8]
        assert outs == {'idx', 'conf'} and R['idx'].shape == (M,) and R['conf'].shape == (K, M) and R['inv_temps'].shape == (K,)
        x = R['x'].init
        assert tuple(x.shape) == (M, C) and 2 <= classes <= C and not bool(torch.isnan(x[:, :classes]).any())
        assert C == classes or bool(torch.isnan(x[:, classes:]).all())
        assert 1 <= K <= lib.sconf_calib_max_temps() and 1.0 in R['inv_temps'].init.tolist()


def _cpu_launch(name, args, buf, views, leak=False):
    """The numpy restatement in the kernels' place; leak: a kernel that reads what it must not (a column behind `classes`, an id of
    the neighbouring pair)."""
    if name == 'sconf_edit_align':
        ho = views['hyp_off'].tolist()
        hyp = views['hyp'].numpy()
        if leak:
            hyp = np.roll(hyp, 1)
        h2r, r2h, counts = AR.align_batch(hyp, ho, views['ref'].numpy(), views['ref_off'].tolist(), views['ws_off'].tolist())
        views['hyp_to_ref'].copy_(torch.from_numpy(h2r)); views['ref_to_hyp'].copy_(torch.from_numpy(r2h)); views['counts'].copy_(torch.from_numpy(counts))
        return
    classes = args[2] + (1 if leak and views['x'].shape[1] > args[2] else 0)
    x = views['x'].numpy()
    if leak and classes == args[2]:
        x = np.roll(x, 1, axis=0)
    idx, conf = AR.sweep(x, views['inv_temps'].tolist(), classes, ('max_prob', 'shannon', 'tsallis', 'renyi')[args[4]], ('lin', 'exp')[args[5]], args[6])
    views['idx'].copy_(torch.from_numpy(idx)); views['conf'].copy_(torch.from_numpy(conf.astype(np.float32)))


@pytest.mark.parametrize('id', list(KC.CASES))
def test_calib_case_passes_with_the_restatement_as_the_kernel(lib, id):
    """The harness on a CPU arena with the restatement in the kernel's place: the case's own checks hold for a correct evaluation and
    fail for one that reads what it must not."""
    c = KC.build(id, lib)
    figures = FP.run_case(c, 'cpu', launch=_cpu_launch)
    assert len(figures['valued']) == (3 if c.name == 'sconf_edit_align' else 2) and all(v.endswith('=0.0e+00') for v in figures['valued'])
    with pytest.raises(FP.FootprintError):
        FP.run_case(c, 'cpu', launch=lambda *a: _cpu_launch(*a, leak=True))


def test_the_cases_cover_what_the_kernels_distinguish(lib):
    from lcasr_amd.hip import confid
    cases = {id: KC.build(id, lib) for id in KC.CASES}
    sweeps = [c for c in cases.values() if c.name == 'sconf_calib_frames_sweep']
    classes = {c.args[2] for c in sweeps}
    assert min(classes) <= 64 and any(64 < v <= 256 for v in classes) and any(256 < v <= confid.row_capacity() for v in classes)
    assert any(confid.row_capacity() < v <= confid.block_capacity() for v in classes) and max(classes) > confid.block_capacity()
    assert {c.args[3] - c.args[2] for c in sweeps} >= {0, 15} and {c.args[8] for c in sweeps} >= {1, 3, lib.sconf_calib_max_temps()}
    assert {c.args[4] for c in sweeps} == {0, 1, 2, 3}
    aligns = [c for c in cases.values() if c.name == 'sconf_edit_align']
    strip, pas, rows = lib.sconf_edit_align_strip_cols(), lib.sconf_edit_align_pass_cols(), lib.sconf_edit_align_block_rows()
    sizes = []
    for c in aligns:
        ho, ro = c.arena.regions['hyp_off'].init.tolist(), c.arena.regions['ref_off'].init.tolist()
        sizes += [(ho[p + 1] - ho[p], ro[p + 1] - ro[p]) for p in range(c.args[4])]
    assert any(R > pas for _, R in sizes) and any(strip < R <= pas for _, R in sizes) and any(H > rows for H, _ in sizes)
    assert (0, 0) in sizes and any(H == 0 < R for H, R in sizes) and any(R == 0 < H for H, R in sizes)
    refused = 0
    for c in aligns:
        out = c.ref({n: r.init for n, r in c.arena.regions.items() if torch.is_tensor(r.init)})
        refused += int((out['counts'][:, 0] < 0).sum())
        assert int((out['counts'][:, 0] > 0).sum()) > 0, c.id
    assert refused == 1
