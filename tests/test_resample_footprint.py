"""CPU checks of the write-footprint cases of the resampler's ABI unit (tests/resample_footprint_cases.py): every launching entry
point of lcasr_amd.hip.resample has a case, every query is known to launch nothing, and every case is laid out on a CPU arena -
regions disjoint, aligned and guarded, the argument list as the binding types it, the output one past a tile at a stride of its
own.  The library builds here as test_cabi.py builds it; the queries are host-only."""
import pytest
import torch

import footprint as FP
import resample_footprint_cases as RC


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from lcasr_amd.hip import resample
    return resample.load()


def test_every_resample_entry_point_has_a_case_or_launches_nothing():
    from lcasr_amd.hip import resample
    assert RC.NO_LAUNCH == set(resample.PLAIN)
    assert {entry for entry, _ in RC.CASES.values()} == set(resample.PROTOTYPES)


@pytest.mark.parametrize('id', list(RC.CASES))
def test_resample_case_layout(lib, id):
    from lcasr_amd.hip import resample
    c = RC.build(id, lib)
    assert c.name == RC.CASES[id][0]
    FP.check_layout(c, resample.PROTOTYPES)
    chan_stride, row_stride, channels, mix = c.args[1:5]
    L, (O, P, K), (out_stride, L_out, B) = c.args[6], c.args[9:12], c.args[13:16]
    out, wave, lens = c.arena.regions['out'], c.arena.regions['wave'], c.arena.regions['lengths'].init.tolist()
    assert out.cls == FP.OUT and out.shape == (B, L_out) and out.strides == (out_stride, 1) and out_stride > L_out
    assert L_out == lib.sconf_resample_out_length(L, O, P) > lib.sconf_resample_tile()
    assert wave.strides[0] == row_stride and wave.strides[-1] == 1 and chan_stride > L and row_stride >= channels * chan_stride
    assert lens[0] == L and lens[1] == 5 and L // 2 < lens[2] < L and B == 3
    assert {r.cls for n, r in c.arena.regions.items() if n != 'out'} == {FP.IN}             # no workspace, nothing else written
    w = wave.init
    for b, n in enumerate(lens): assert bool(torch.isnan(w[b, ..., n:]).all()) and bool(torch.isfinite(w[b, ..., 0, :n] if w.dim() == 3 else w[b, :n]).all())
    if channels > 1:
        assert bool(torch.isnan(w[:, 1]).all()) == (not mix)


@pytest.mark.parametrize('id', list(RC.CASES))
def test_resample_case_passes_with_the_f32_restatement_as_the_kernel(lib, id):
    """The harness on a CPU arena with the f32 restatement from the compact table in the kernel's place: the case's own checks
    (the bound against the float64 restatement among them) hold for a correct f32 evaluation, and fail for a kernel that reads
    behind a length."""
    import resample_refs as RR
    c = RC.build(id, lib)

    def launch(name, args, buf, views, leak=False):
        assert name == 'sconf_resample_rows'
        mix, (O, P) = args[4], args[9:11]
        lens = None if leak else views['lengths']
        wave = views['wave'].clone()
        views['out'].copy_(RR.resample_rows(wave, lens, views['taps'], views['first'], O, P, mix=bool(mix)))

    figures = FP.run_case(c, 'cpu', launch=launch)
    assert figures['valued'] == ['out=0.0e+00']
    with pytest.raises(FP.FootprintError, match='out'):
        FP.run_case(c, 'cpu', launch=lambda *a: launch(*a, leak=True))


def test_the_cases_cover_what_the_kernel_distinguishes(lib):
    cases = {id: RC.build(id, lib) for id in RC.CASES}
    kinds = {(c.args[3], c.args[4]) for c in cases.values()}
    assert {(1, 0), (2, 0), (2, 1)} <= kinds                                                 # mono, stereo left, stereo mean
    ratios = {(c.args[9], c.args[10]) for c in cases.values()}
    assert {(441, 160), (1, 2), (3, 1)} <= ratios                                            # span 2.76, 0.5 and 3 times the tile
