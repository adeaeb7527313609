"""CPU checks of the write-footprint cases of the posterior unit (tests/post_footprint_cases.py): all three launching entry points of
lcasr_amd.hip.post have their cases, every query is known to launch nothing, and every case is laid out on a CPU arena - regions
disjoint, aligned and guarded, the argument list as the binding types it, the declared output shapes the shapes the restatement
returns, every output declared OUT, the workspace at exactly sconf_post_workspace bytes (scratch for the lattice, an input it
produced for the neighbours), NaN in the frames behind input_lengths[b], a sample without labels and one without an alignment in
every batch.  The library builds here as test_cabi.py builds it; the queries are host-only."""
import numpy as np
import pytest
import torch

import footprint as FP
import post_footprint_cases as KC
import post_refs as PR


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from lcasr_amd.hip import post
    return post.load()


def test_every_post_entry_point_has_a_case_or_launches_nothing():
    from lcasr_amd.hip import post
    assert KC.NO_LAUNCH == set(post.PLAIN)
    assert {entry for entry, _ in KC.CASES.values()} == set(post.PROTOTYPES)


@pytest.mark.parametrize('id', list(KC.CASES))
def test_post_case_layout(lib, id):
    from lcasr_amd.hip import post
    c = KC.build(id, lib)
    assert c.name == KC.CASES[id][0]
    FP.check_layout(c, post.PROTOTYPES)
    R = c.arena.regions
    outs = {n for n, r in R.items() if r.cls not in (FP.IN,)}
    for n in outs - {'workspace'}:
        assert R[n].cls == FP.OUT and R[n].tol == 0.0 and R[n].order is None
    if c.name == 'sconf_post_slots':
        B, C, Smax = c.args[3:6]
        assert outs == {'post', 'alt', 'alt_post', 'gap_post', 'gap_alt', 'gap_alt_post'}
        assert R['post'].shape == (B, Smax) and R['gap_alt'].shape == (B, Smax + 1) and R['alt'].dtype == R['gap_alt'].dtype == torch.int32
        sub = R['sub_llr'].init
        dead = torch.isnan(sub).any(-1)
        assert bool(dead.any()) and bool((~dead).any()) and bool((torch.isnan(sub).all(-1) == dead).all())          # a row is NaN throughout or not at all
        assert bool((R['post'].unspecified == dead).all()) and R['alt'].unspecified is None
        return
    B, N, C, stride, Smax = c.args[4:9]
    lp, il, tl = R['log_probs'].init, R['input_lengths'].init.tolist(), R['target_lengths'].init.tolist()
    assert R['log_probs'].strides == (N * stride, stride, 1) and stride >= C and tuple(lp.shape) == (B, N, C)
    assert 0 in tl and any(l > t for t, l in zip(il, tl)) and len(set(il)) == B and max(il) < N and max(tl) < Smax
    for b in range(B):
        assert not bool(torch.isnan(lp[b, :il[b]]).any()) and bool(torch.isnan(lp[b, il[b]:]).all())
    ws = R['workspace']
    assert ws.dtype == torch.uint8 and ws.numel == ws.extent == c.args[11] == lib.sconf_post_workspace(B, N, Smax) > 0
    if c.name == 'sconf_post_lattice':
        assert outs == {'workspace', 'loglik'} and ws.cls == FP.SCRATCH and R['loglik'].dtype == torch.float64
    else:
        assert outs == {'sub_llr', 'ins_llr'} and ws.cls == FP.IN and ws.produced and R['loglik'].cls == FP.IN and R['loglik'].produced
        assert c.before == [('sconf_post_lattice', c.args[:13])]
        assert R['sub_llr'].shape == (B, Smax, C) and R['ins_llr'].shape == (B, Smax + 1, C)
        assert bool(R['sub_llr'].unspecified.any()) and not bool(R['sub_llr'].unspecified.all())


def _cpu_launch(name, args, buf, views, leak=False):
    """The numpy restatement in the kernels' place; leak: a kernel that reads what it must not - the frame behind a sample's
    input_lengths (NaN there), or, for the summary, the row of the neighbouring slot."""
    if name == 'sconf_post_slots':
        sub = views['sub_llr'].numpy()
        out = PR.slots(np.roll(sub, 1, axis=1) if leak else sub, views['ins_llr'].numpy(), views['targets'].numpy(), args[6])
        for n, o in zip(('post', 'alt', 'alt_post', 'gap_post', 'gap_alt', 'gap_alt_post'), out):
            views[n].copy_(torch.from_numpy(o.astype(np.int32 if n.endswith('alt') else np.float32)))
        return
    il = [t + 1 if leak else t for t in views['input_lengths'].tolist()]
    ll, sub, ins = PR.neighbours_batch(views['log_probs'].numpy(), views['targets'].numpy(), il, views['target_lengths'].tolist(), args[9])
    if name == 'sconf_post_lattice':
        views['loglik'].copy_(torch.from_numpy(ll))
    else:
        views['sub_llr'].copy_(torch.from_numpy(sub.astype(np.float32))); views['ins_llr'].copy_(torch.from_numpy(ins.astype(np.float32)))


@pytest.mark.parametrize('id', list(KC.CASES))
def test_post_case_passes_with_the_restatement_as_the_kernel(lib, id):
    """The harness on a CPU arena with the restatement in the kernel's place: the case's own checks hold for a correct evaluation and
    fail for one that reads what it must not."""
    c = KC.build(id, lib)
    figures = FP.run_case(c, 'cpu', launch=_cpu_launch)
    assert len(figures['valued']) == {'sconf_post_lattice': 1, 'sconf_post_neighbours': 2, 'sconf_post_slots': 6}[c.name]
    assert all(v.endswith('=0.0e+00') for v in figures['valued'])
    with pytest.raises(FP.FootprintError):
        FP.run_case(c, 'cpu', launch=lambda *a: _cpu_launch(*a, leak=True))


def test_the_cases_cover_what_the_kernels_distinguish(lib):
    cases = {id: KC.build(id, lib) for id in KC.CASES}
    for entry in ('sconf_post_lattice', 'sconf_post_neighbours'):
        mine = [c for c in cases.values() if c.name == entry]
        classes = {c.args[6] for c in mine}
        assert min(classes) < 64 and any(64 < v <= 192 for v in classes) and max(classes) > 256          # under a wave, three waves, five
        assert {c.args[7] - c.args[6] for c in mine} == {0, 15}
        assert any(2 * c.args[8] + 1 > 4096 for c in mine) and any(2 * c.args[8] + 1 <= 64 for c in mine)   # eight states a thread, and one
    slots = [c for c in cases.values() if c.name == 'sconf_post_slots']
    assert {c.args[4] for c in slots} >= {3, 130, 257}
