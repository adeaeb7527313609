"""CPU checks of the write-footprint cases of the noise unit (tests/noise_footprint_cases.py): every launching entry point of
lcasr_amd.hip.noise has a case, every query is known to launch nothing, and every case is laid out on a CPU arena - regions
disjoint, aligned and guarded, the argument list as the binding types it, rows one past a tile at strides of their own, NaN
behind every length.  The library builds here as test_cabi.py builds it; the queries are host-only."""
import pytest
import torch

import footprint as FP
import noise_footprint_cases as NC
import noise_refs as NR


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from lcasr_amd.hip import noise
    return noise.load()


def test_every_noise_entry_point_has_a_case_or_launches_nothing():
    from lcasr_amd.hip import noise
    assert NC.NO_LAUNCH == set(noise.PLAIN)
    assert {entry for entry, _ in NC.CASES.values()} == set(noise.PROTOTYPES)


@pytest.mark.parametrize('id', list(NC.CASES))
def test_noise_case_layout(lib, id):
    from lcasr_amd.hip import noise
    c = NC.build(id, lib)
    assert c.name == NC.CASES[id][0]
    FP.check_layout(c, noise.PROTOTYPES)
    R = c.arena.regions
    Q = lib.sconf_noise_tile()
    lens = R['lengths'].init.tolist()
    L = lens[0]
    assert L == Q + 1 and lens[1] == 5 and L // 2 < lens[2] < L and len(lens) == NC.B
    writable = {n: r.cls for n, r in R.items() if r.cls != FP.IN}
    if c.name == 'sconf_noise_power':
        assert writable == {'power': FP.OUT, 'ws': FP.SCRATCH} and R['ws'].shape == (lib.sconf_noise_workspace(NC.B, L),)
        assert R['power'].dtype == torch.float64 and R['power'].shape == (NC.B,)
    else:
        K, out_stride = c.args[7 if c.name == 'sconf_noise_add_gaussian' else 13], c.args[-1]
        assert writable == {'out': FP.OUT} and R['out'].shape == (NC.B * K, L) and R['out'].strides == (out_stride, 1) and out_stride > L
    for name, counts in (('wave', 'lengths'), ('noise', 'noise_lengths')):
        if name in R:
            w, n = R[name].init, R[counts].init.tolist()
            assert R[name].strides[0] > w.shape[1]
            for b in range(w.shape[0]):
                assert bool(torch.isnan(w[b, n[b]:]).all()) and bool(torch.isfinite(w[b, :n[b]]).all())
    if 'offsets' in R:
        nl, off = R['noise_lengths'].init.tolist(), R['offsets'].init.tolist()
        assert all(0 <= o < nl[b if len(nl) > 1 else 0] for b, o in enumerate(off))


def _cpu_launch(name, args, buf, views, leak=False):
    """The f32 restatements of tests/noise_refs.py in the kernels' place; leak: a kernel that ignores the rows' lengths."""
    lens = None if leak else views['lengths']
    if name == 'sconf_noise_power':
        src = views['noise'] if 'noise' in views else views['wave']
        views['power'].copy_(NR.op_power(src, lens, views.get('noise_lengths'), views.get('offsets'), L=args[6], B=args[7]))
    elif name == 'sconf_noise_add_gaussian':
        K, seed, first_row, first_sample = args[7:11]
        out = NR.op_add_gaussian(views['wave'], lens, views['power'], views['snr_db'], seed, first_row, first_sample)
        views['out'].copy_(out.reshape(-1, out.shape[-1]))
    else:
        out = NR.op_add_background(views['wave'], lens, views['noise'], views['noise_lengths'], views['offsets'], views['power'],
                                   views['noise_power'], views['snr_db'])
        views['out'].copy_(out.reshape(-1, out.shape[-1]))


@pytest.mark.parametrize('id', list(NC.CASES))
def test_noise_case_passes_with_the_f32_restatement_as_the_kernel(lib, id):
    """The harness on a CPU arena with an f32 evaluation in the kernel's place: the case's own checks (the bounds against the
    float64 restatement among them) hold for a correct evaluation, and fail for one that reads behind a length."""
    c = NC.build(id, lib)
    figures = FP.run_case(c, 'cpu', launch=_cpu_launch)
    assert figures['valued'] == [f'{"power" if c.name == "sconf_noise_power" else "out"}=0.0e+00']
    with pytest.raises(FP.FootprintError):
        FP.run_case(c, 'cpu', launch=lambda *a: _cpu_launch(*a, leak=True))


def test_the_cases_cover_what_the_kernels_distinguish(lib):
    cases = {id: NC.build(id, lib) for id in NC.CASES}
    g = [c for c in cases.values() if c.name == 'sconf_noise_add_gaussian']
    assert {c.args[1] % 4 == 0 and c.args[10] % 4 == 0 for c in g} == {True, False}         # 16-byte path and element path
    assert any(c.args[10] >= 2 ** 34 and c.args[10] % 4 for c in g) and all(c.args[9] >= 2 ** 32 for c in g)     # the high counter words
    bg = [c for c in cases.values() if c.name == 'sconf_noise_add_background']
    assert {c.args[7] for c in bg} == {1, NC.B} and {c.args[1] % 4 == 0 for c in bg} == {True, False}
    p = [c for c in cases.values() if c.name == 'sconf_noise_power']
    assert {c.args[4] is None for c in p} == {True, False}
