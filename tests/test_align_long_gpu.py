"""The long form of CTC forced alignment on the device (csrc/align_long.hip through lcasr_amd.hip.align_long) against the numpy
restatement of the contract (tests/align_refs.py) in f64, which has no length limit.  Every comparison is EXACT: torch.equal on path,
labels, spans and token_logp, and a measured difference of 0 on score (printed before it is asserted).

Small slabs (slab_states 256 and 512) put the seams between slab launches where small lattices cross them: S = 127 | 128 | 129 at
256 states per slab is L - 1 just below, at and just above a multiple of the slab (at 128 the last slab holds the one state L - 1
and L - 2 lives in the slab below); S = 300 and 700 are 3 and 6 slabs.  Each case computes its restatement once."""
import numpy as np
import pytest
import torch

import align_long_footprint_cases as LC
import align_refs as AR
import footprint as FP

pytestmark = pytest.mark.gpu
SLABS = (256, 512, 1024, 2048, 4096, 8192)


@pytest.fixture(scope='module')
def K():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from lcasr_amd.hip import align_long
    align_long.load()
    return align_long


def _ints(v):
    return None if v is None else torch.tensor(v, dtype=torch.int32)


def restate(lp, tg, il, tl, blank):
    return AR.ctc_align(lp, tg, _ints(il), _ints(tl), blank, dtype=np.float64)


def same(got, ref, what):
    """All five outputs of a device result equal the restatement's; the score difference is printed, then asserted to be 0."""
    g = [t.cpu() for t in got]
    for name, a, b in zip(('path', 'labels', 'spans', 'token_logp'), g[:4], ref[:4]):
        if not torch.equal(a, b):
            bad = (a != b).nonzero()
            raise AssertionError(f'{what} {name}: {bad.shape[0]} element(s) differ, first at {bad[0].tolist()}: {a[tuple(bad[0])]} != {b[tuple(bad[0])]}')
    for b, (s_got, s_ref) in enumerate(zip(g[4].tolist(), ref.score.tolist())):
        if np.isnan(s_ref) or np.isinf(s_ref):
            assert (np.isnan(s_got) and np.isnan(s_ref)) or s_got == s_ref, f'{what} score[{b}]: {s_got} != {s_ref}'
        else:
            print(f'[align long gpu] {what} sample {b}: score {s_got!r} restated {s_ref!r} |d| {abs(s_got - s_ref):.3e}')
            assert s_got - s_ref == 0.0, f'{what} score[{b}]: {s_got!r} != {s_ref!r}'


def run(K, lp, tg, il, tl, blank, slab):
    dev = lambda v: None if v is None else _ints(v).cuda()
    got = K.ctc_align(lp.cuda(), tg.cuda(), dev(il), dev(tl), blank, slab_states=slab)
    torch.cuda.synchronize()
    return got


# ---- 1. seams with small slabs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S, C, slabs', [(127, 8, (256,)), (128, 16, (256,)), (129, 32, (256,)), (300, 24, (256, 512)), (700, 32, (256, 512))])
def test_seams_with_slack_and_ragged_lengths(K, S, C, slabs):
    N = S + 40
    il, tl = [N, S + 5, N - 13], [S, S, S - 3]
    lp, tg = AR.random_case(200 + S, 3, N, C, S, il, tl, repeats=4)
    assert all(AR.feasible(il[b], tg[b, :tl[b]].tolist()) for b in range(3))
    ref = restate(lp, tg, il, tl, C - 1)
    assert bool(torch.isfinite(ref.score).all())
    for w in slabs:
        assert K.slabs(S, w) == -(-(2 * S + 1) // w)
        same(run(K, lp, tg, il, tl, C - 1, w), ref, f'S={S} slab={w}')
    same(run(K, lp[:1], tg[:1], None, None, C - 1, slabs[0]), restate(lp[:1], tg[:1], None, None, C - 1), f'S={S} B=1 NULL lengths')


@pytest.mark.parametrize('S, C, slabs', [(127, 32, (256,)), (128, 32, (256,)), (129, 32, (256,)), (300, 16, (256, 512)), (700, 32, (256, 512))])
def test_no_slack_path_falls_two_states_per_frame_through_every_seam(K, S, C, slabs):
    """No two adjacent labels equal and T = S: the only path takes the s-2 step every frame, so at each seam it enters the slab's
    first label state from the state below the slab, and it ends on L - 2 (at S = 128 the top cell of the slab below the last).
    One frame fewer is infeasible.  With planted repeats T = S + repeats is feasible by exactly one frame."""
    lp, tg = AR.random_case(300 + S, 2, S + 20, C, S)
    il = [S, S - 1]
    ref = restate(lp, tg, il, None, C - 1)
    assert ref.path[0, :S].tolist() == list(range(1, 2 * S, 2)) and float(ref.score[1]) == -np.inf
    for w in slabs:
        got = run(K, lp, tg, il, None, C - 1, w)
        same(got, ref, f'T=S={S} slab={w}')
        assert float(got.score[1].cpu()) == -np.inf and bool((got.path[1] == -1).all()) and bool((got.spans[1] == -1).all())
    lp, tg = AR.random_case(400 + S, 2, S + 20, C, S, repeats=12)
    tg[1] = tg[0]
    rep = AR.repeats_of(tg[0].tolist())
    assert 3 <= rep <= 20
    il = [S + rep, S + rep - 1]
    ref = restate(lp, tg, il, None, C - 1)
    assert np.isfinite(float(ref.score[0])) and float(ref.score[1]) == -np.inf
    for w in slabs:
        same(run(K, lp, tg, il, None, C - 1, w), ref, f'T=S+repeats S={S} slab={w}')


@pytest.mark.parametrize('slab', [256, 512])
def test_a_repeated_label_across_each_seam_and_the_same_pair_broken(K, slab):
    """The skip into a slab's first label state s0 + 1 comes from s0 - 1 in the slab below and is allowed only when
    targets[s0 / 2] != targets[s0 / 2 - 1].  Row 0 repeats the label across every seam, row 1 is the same transcript with the pairs
    distinct; both with no frame to spare (the path crosses every seam on the diagonal) and with slack."""
    S, C = 700, 32
    lp, tg = AR.random_case(31, 2, S + 60, C, S)
    tg[1] = tg[0]
    seams = list(range(slab, 2 * S + 1, slab))
    assert len(seams) == (2 * S + 1 - 1) // slab >= 2
    for s0 in seams:
        tg[0, s0 // 2 - 1] = tg[0, s0 // 2]
        assert tg[1, s0 // 2 - 1] != tg[1, s0 // 2]
    rep = AR.repeats_of(tg[0].tolist())
    assert rep >= len(seams) and AR.repeats_of(tg[1].tolist()) == 0
    for il in ([S + rep, S], [S + 60, S + 47], [S + rep - 1, S - 1]):
        ref = restate(lp, tg, il, None, C - 1)
        assert bool(torch.isfinite(ref.score).all()) == (il[1] >= S)
        same(run(K, lp, tg, il, None, C - 1, slab), ref, f'seam repeats slab={slab} T={il}')


def test_long_runs_of_one_label(K):
    tg = torch.tensor([[5] * 140 + [7] * 145 + [5] * 3 + list(range(10)), [3] * 298], dtype=torch.int32)       # runs lie across the seams
    S = tg.shape[1]
    N = 2 * S + 30
    il = [N, 2 * S - 1]                                                      # 297 repeats in row 1: feasible by exactly one frame
    lp, _ = AR.random_case(15, 2, N, 32, S, il, None, targets=tg)
    ref = restate(lp, tg, il, None, 31)
    assert bool(torch.isfinite(ref.score).all())
    for w in (256, 512):
        same(run(K, lp, tg, il, None, 31, w), ref, f'runs slab={w}')


@pytest.mark.parametrize('slab, S', [(1024, 600), (2048, 1100), (4096, 2100)])
def test_a_seam_at_every_other_geometry(K, slab, S):
    """1024 x 1, 1024 x 2 and 1024 x 4 with two slabs each (1024 x 8 with three: test_past_the_old_limit)."""
    N = S + 70
    il, tl = [N, S + 9], [S, S - 2]
    lp, tg = AR.random_case(500 + S, 2, N, 16, S, il, tl, repeats=6)
    assert K.slabs(S, slab) == 2
    same(run(K, lp, tg, il, tl, 15, slab), restate(lp, tg, il, tl, 15), f'S={S} slab={slab}')


# ---- 2. ragged and poisoned batches ------------------------------------------------------------------------------------------------
def test_ragged_batch_with_a_poisoned_sample(K):
    """S = (10, 700, 0, 500) at 256 states per slab: 1, 6, 1 and 4 slabs in one batch; T = (N, short, 0, N).  Sample 3 has a label out
    of range among the labels of slab 0 and is poisoned as a whole; samples with T > N and S > Smax likewise.  The healthy samples
    are bit-equal to calls of their own."""
    Smax, N, C, w = 700, 760, 32, 256
    il, tl = [N, 704, 0, N, N + 1, N], [10, 700, 0, 500, 20, Smax + 1]
    lp, tg = AR.random_case(41, 6, N, C, Smax, [N, 704, 0, N, N, N], [10, 700, 0, 500, 20, 30])
    tg[3, 50] = C
    ref = restate(lp, tg, il, tl, C - 1)
    assert np.isfinite(ref.score[:2].numpy()).all() and float(ref.score[2]) == -np.inf and bool(torch.isnan(ref.score[3:]).all())
    got = run(K, lp, tg, il, tl, C - 1, w)
    same(got, ref, 'ragged')
    for b in (2, 3, 4, 5):
        assert bool((got.path[b] == -1).all()) and bool((got.labels[b] == -1).all()) and bool((got.spans[b] == -1).all())
        assert bool((got.token_logp[b] == 0).all())
    tg[3, 50] = -7                                                         # a negative label, and the bad label beside other slabs' work
    same(run(K, lp, tg, il, tl, C - 1, w), restate(lp, tg, il, tl, C - 1), 'ragged, negative label')
    for b in (0, 1):
        alone = run(K, lp[b:b + 1], tg[b:b + 1], il[b:b + 1], tl[b:b + 1], C - 1, w)
        for a, g in zip(alone, got):
            assert torch.equal(a[0:1].contiguous().view(torch.uint8), g[b:b + 1].contiguous().view(torch.uint8))     # (score[b] has no dimension)


# ---- 3. the two units agree --------------------------------------------------------------------------------------------------------
def test_every_slab_size_gives_the_short_units_bits(K):
    """B = 2, N = 1500, S = 600 (the short unit runs 1024 x 2 in f64): 5, 3, 2, 1, 1 and 1 slabs."""
    from lcasr_amd.hip import align
    assert align.state_bytes(600) == 8
    N, S = 1500, 600
    il, tl = [N, 1290], [S, 590]
    lp, tg = AR.random_case(51, 2, N, 32, S, il, tl, repeats=6)
    dev = [lp.cuda(), tg.cuda(), _ints(il).cuda(), _ints(tl).cuda()]
    short = align.ctc_align(*dev, 31)
    torch.cuda.synchronize()
    same(short, restate(lp, tg, il, tl, 31), 'short unit')
    for w in (0,) + SLABS:
        got = K.ctc_align(*dev, 31, slab_states=w)
        torch.cuda.synchronize()
        for name, a, b in zip(short._fields, got, short):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), f'slab_states={w}: {name} differs from sconf_align_ctc'


# ---- 4. reach ----------------------------------------------------------------------------------------------------------------------
def test_past_the_old_limit_at_the_default_geometry(K):
    """8192 labels, one more than the short unit takes, through the public interface: three slabs of 1024 x 8, the last of one state."""
    from lcasr_amd.decoding.align import ctc_forced_align
    from lcasr_amd.hip import align
    N, S, C = 9000, 8192, 64
    assert S == align.max_labels() + 1 and K.slabs(S) == 3 and K.load().sconf_lalign_states_per_thread(0) == 8
    lp, tg = AR.random_case(61, 1, N, C, S)
    got = ctc_forced_align(lp.cuda(), tg.cuda(), blank=C - 1)
    torch.cuda.synchronize()
    ref = restate(lp, tg, None, None, C - 1)
    assert np.isfinite(float(ref.score[0])) and got.path.shape == (1, N) and got.spans.shape == (1, S, 2)
    same(got, ref, 'S=8192')


def test_offsets_past_2_to_the_31(K):
    """B = 1, N = T = 33000 at Smax = 65535 (16 slab launches; the 40 labels of the sample are all in slab 0): the emission row offset
    i * (round8(Smax) + 12) and the back-pointer row offset i * round48(2 Smax + 1) pass 2^31 at i = 32762 and i = 16384."""
    N, Smax, S, C = 33000, 65535, 40, 8
    assert (N - 1) * ((Smax + 7) // 8 * 8 + 12) > 1 << 31 and (N - 1) * ((2 * Smax + 1 + 47) // 48 * 48) > 1 << 32
    lp, short = AR.random_case(71, 1, N, C, S)
    tg = torch.zeros(1, Smax, dtype=torch.int32)
    tg[:, :S] = short
    ref = restate(lp, tg, None, [S], C - 1)
    assert np.isfinite(float(ref.score[0]))
    same(run(K, lp, tg, None, [S], C - 1, 0), ref, 'offsets past 2^31')
    torch.cuda.empty_cache()                                              # 13 GB of workspace: not kept for the rest of the session


# ---- 5. refusals and footprint -----------------------------------------------------------------------------------------------------
def test_refusals_on_the_device_path(K):
    lp, tg = AR.random_case(17, 1, 8, 32, 3)
    with pytest.raises(RuntimeError, match='GPU'):
        K.ctc_align(lp, tg.cuda(), None, None, 31)
    with pytest.raises(TypeError):
        K.ctc_align(lp.cuda(), tg.cuda().long(), None, None, 31)
    with pytest.raises(ValueError, match=str(K.max_labels())):
        K.ctc_align(lp.cuda(), torch.zeros(1, K.max_labels() + 1, dtype=torch.int32).cuda(), None, None, 31)
    with pytest.raises(ValueError, match='slab_states'):
        K.ctc_align(lp.cuda(), tg.cuda(), None, None, 31, slab_states=300)
    with pytest.raises(RuntimeError, match='blank'):
        K.ctc_align(lp.cuda(), tg.cuda(), None, None, 32)


@pytest.mark.parametrize('id', list(LC.CASES))
def test_footprint(K, id):
    FP.run_on_device(LC.build(id, K.load()), K.PROTOTYPES)
