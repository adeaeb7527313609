"""CPU checks of the write-footprint cases of the segmentation unit (tests/seg_footprint_cases.py): every launching entry point of
lcasr_amd.hip.seg has a case, every query is known to launch nothing, and every case is laid out on a CPU arena - regions disjoint,
aligned and guarded, the argument list as the binding types it, the declared output shapes the shapes the restatement returns, all
outputs declared OUT, the workspace of sconf_seg_align declared scratch at exactly what the query says, stars in every target row.
The library builds here as test_cabi.py builds it; the queries are host-only."""
import pytest
import torch

import footprint as FP
import seg_footprint_cases as SC
import seg_refs as SR


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from lcasr_amd.hip import seg
    return seg.load()


def test_every_seg_entry_point_has_a_case_or_launches_nothing():
    from lcasr_amd.hip import seg
    assert SC.NO_LAUNCH == set(seg.PLAIN)
    assert {entry for entry, _ in SC.CASES.values()} == set(seg.PROTOTYPES)


@pytest.mark.parametrize('id', list(SC.CASES))
def test_seg_case_layout(lib, id):
    from lcasr_amd.hip import seg
    c = SC.build(id, lib)
    assert c.name == SC.CASES[id][0]
    FP.check_layout(c, seg.PROTOTYPES)
    R = c.arena.regions
    if c.name == 'sconf_seg_align':
        B, N, C, Smax = c.args[12:16]
        ws = R['workspace']
        assert ws.cls == FP.SCRATCH and ws.dtype == torch.uint8 and ws.numel == ws.extent == c.args[11] == lib.sconf_seg_workspace(B, N, Smax, 0)
        want = {'path': ((B, N), torch.int32), 'labels': ((B, N), torch.int32), 'spans': ((B, Smax, 2), torch.int32),
                'token_logp': ((B, Smax), torch.float32), 'score': ((B,), torch.float64), 'frame_logp': ((B, N), torch.float32)}
        assert {n for n, r in R.items() if r.cls != FP.IN} == set(want) | {'workspace'}
        assert ('input_lengths' in R) == (c.args[2] is not None) and ('target_lengths' in R) == (c.args[3] is not None)
        tg = R['targets'].init
        assert Smax == 0 or bool((tg == C).any(1).all()) and int(tg.max()) == C and int(tg.min()) >= 0
        assert c.args[17] <= 0.0
    else:
        B, N, Smax, Umax = c.args[11:15]
        want = {'utt_frames': ((B, Umax, 2), torch.int32), 'utt_logp': ((B, Umax), torch.float32), 'utt_conf': ((B, Umax), torch.float32)}
        assert {n for n, r in R.items() if r.cls != FP.IN} == set(want)
        assert 1 <= c.args[7] <= lib.sconf_seg_max_window()
    for name, (shape, dtype) in want.items():
        r = R[name]
        assert r.cls == FP.OUT and r.shape == shape and r.dtype == dtype and r.unspecified is None and r.order is None


def _cpu_launch(name, args, buf, views, leak=False):
    """The restatements of tests/seg_refs.py in the kernels' place; leak: a kernel that reads what the header does not let it read."""
    if name == 'sconf_seg_align':
        lp = views['log_probs']
        if leak:                                                            # the frames behind a length, or the guard behind the log-probs
            lp = lp.clone(); lp[:, -1] = float('nan')
            il = None
        else:
            il = views.get('input_lengths')
        out = SR.align(lp, views['targets'], il, views.get('target_lengths'), args[16], args[17])
        for k, t in out._asdict().items():
            if t.numel(): views[k].copy_(t)
    else:
        g = views['frame_logp']
        if leak: g = torch.roll(g, 1, 1)                                    # the frame in front of every utterance
        out = SR.score(views['spans'], g, views['score'], views.get('input_lengths'), views['target_lengths'], views['utt'], views['utt_counts'], args[7])
        for k, t in out._asdict().items(): views[k].copy_(t)


@pytest.mark.parametrize('id', list(SC.CASES))
def test_seg_case_passes_with_the_restatement_as_the_kernel(lib, id):
    """The harness on a CPU arena with the restatement in the kernel's place: the case's own checks hold for a correct evaluation and
    fail for one that reads what it must not."""
    c = SC.build(id, lib)
    figures = FP.run_case(c, 'cpu', launch=_cpu_launch)
    assert len(figures['valued']) == (3 if c.name == 'sconf_seg_score' else 6 if c.args[15] else 4)
    if c.name == 'sconf_seg_score':
        assert all(v.endswith('=0.0e+00') for v in figures['valued'])
    with pytest.raises(FP.FootprintError):
        FP.run_case(c, 'cpu', launch=lambda *a: _cpu_launch(*a, leak=True))


def test_the_cases_cover_what_the_kernels_distinguish(lib):
    cases = {id: SC.build(id, lib) for id in SC.CASES}
    al = [c for c in cases.values() if c.name == 'sconf_seg_align']
    geo = {(lib.sconf_align_threads(c.args[15]), lib.sconf_align_states_per_thread(c.args[15])) for c in al}
    assert {(256, 1), (512, 1), (1024, 2)} <= geo and {c.args[17] for c in al} == {0.0, -1.0}
    sc = [c for c in cases.values() if c.name == 'sconf_seg_score']
    tile, W = lib.sconf_seg_score_tile(), lib.sconf_seg_max_window()
    assert {c.args[7] for c in sc} == {1, 30, W} and {c.args[3] is None for c in sc} == {True, False}
    for c in sc:
        out = c.ref({n: r.init for n, r in c.arena.regions.items() if torch.is_tensor(r.init)})['utt_frames']
        n = (out[..., 1] - out[..., 0])[out[..., 0] >= 0].tolist()
        assert {1, tile - 1, tile, tile + 1, c.args[12]} <= set(n) and c.args[12] >= c.args[7]
