"""CTC forced alignment on the device (csrc/align.hip through lcasr_amd.hip.align) against the numpy restatement of the contract
(tests/align_refs.py) run in the state type the library reports: path, labels and spans EXACTLY, score within
T eps(state type) |score| (the restatement makes the same additions, so the difference is expected to be 0; |score| is the largest
|v| on the best path), token_logp within n 2^-24 sum|x| per token.  C = 32 unless a case says otherwise.

Launch geometry (sconf_align_threads x sconf_align_states_per_thread, asserted in test_lattice_geometry): 256 x 1 up to 127 labels,
512 x 1 up to 255, 1024 x 1 / 2 / 4 / 8 / 12 / 16 up to 511 / 1023 / 2047 / 4095 / 6143 / 8191; f32 state from 5113 labels on.  The
walk back fetches sconf_align_walk_window() = 16 frames at a time."""
import numpy as np
import pytest
import torch

import align_footprint_cases as AC
import align_refs as AR
import footprint as FP

pytestmark = pytest.mark.gpu
C32 = 32


@pytest.fixture(scope='module')
def K():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from lcasr_amd.hip import align
    align.load()
    return align


def check(K, lp, tg, il, tl, blank, what=''):
    """Run the op on the device and compare all five outputs with the restatement.  Returns (device result, restatement)."""
    B, N, C = lp.shape
    Smax = tg.shape[1]
    dev = lambda v: None if v is None else torch.tensor(v, dtype=torch.int32).cuda()
    got = K.ctc_align(lp.cuda(), tg.cuda(), dev(il), dev(tl), blank)
    torch.cuda.synchronize()
    sb = K.state_bytes(Smax)
    ref = AR.ctc_align(lp, tg, dev(il) if il is None else torch.tensor(il), dev(tl) if tl is None else torch.tensor(tl), blank,
                       dtype=AR.state_dtype(sb))
    g = [t.cpu() for t in got]
    for name, a, b in zip(('path', 'labels', 'spans'), g[:3], ref[:3]):
        bad = (a != b).nonzero()
        assert not bad.numel(), f'{what} {name}: {bad.shape[0]} element(s) differ, first at {bad[0].tolist()}: {a[tuple(bad[0])]} != {b[tuple(bad[0])]}'
    eps = 2.0 ** -52 if sb == 8 else 2.0 ** -23
    lpn = lp.numpy()
    for b in range(B):
        s_got, s_ref = float(g[4][b]), float(ref.score[b])
        T = N if il is None else il[b]
        if not np.isfinite(s_ref):
            assert (np.isnan(s_got) and np.isnan(s_ref)) or s_got == s_ref, f'{what} score[{b}]: {s_got} != {s_ref}'
        else:
            print(f'[align gpu] {what} sample {b}: score {s_got!r} restated {s_ref!r} |d| {abs(s_got - s_ref):.3e} bound {T * eps * abs(s_ref):.3e}')
            assert abs(s_got - s_ref) <= T * eps * abs(s_ref), f'{what} score[{b}]: {s_got!r} != {s_ref!r}'
        for j in range(Smax):
            f, l = ref.spans[b, j].tolist()
            bound = (l - f) * 2.0 ** -24 * float(np.abs(lpn[b, f:l, int(tg[b, j])]).sum()) if f >= 0 else 0.0
            d = abs(float(g[3][b, j]) - float(ref.token_logp[b, j]))
            assert d <= bound, f'{what} token_logp[{b}][{j}]: |d| {d:.3e} > {bound:.3e}'
    return got, ref


# ---- 7. lattice geometry --------------------------------------------------------------------------------------------------------
GEOMETRY = {0: (256, 1), 1: (256, 1), 127: (256, 1), 128: (512, 1), 255: (512, 1), 256: (1024, 1), 511: (1024, 1), 512: (1024, 2),
            1023: (1024, 2), 1024: (1024, 4), 2047: (1024, 4), 2048: (1024, 8), 4095: (1024, 8), 4096: (1024, 12), 6143: (1024, 12),
            6144: (1024, 16)}


@pytest.mark.parametrize('S', list(GEOMETRY))
def test_lattice_geometry(K, S):
    lib = K.load()
    assert (lib.sconf_align_threads(S), lib.sconf_align_states_per_thread(S)) == GEOMETRY[S]
    C = 4096 if S == 256 else C32
    N = S + 40
    il, tl = [N, S + 5, N - 13], [S, S, max(S - 3, 0)]
    lp, tg = AR.random_case(100 + S, 3, N, C, S, il, tl, repeats=4)
    for b in range(3):
        assert AR.feasible(il[b], tg[b, :tl[b]].tolist())
    got, ref = check(K, lp, tg, il, tl, C - 1, f'S={S}')
    assert bool(torch.isfinite(ref.score).all())


def test_f32_state_at_the_smallest_such_lattice(K):
    lib = K.load()
    S = next(s for s in range(1, K.max_labels() + 1) if lib.sconf_align_state_bytes(s) == 4)
    assert lib.sconf_align_state_bytes(S - 1) == 8 and S == 5113
    N = S + 64
    il, tl = [N, S + 9, N - 21], [S, S, S - 3]
    lp, tg = AR.random_case(5, 3, N, C32, S, il, tl, repeats=6)
    got, ref = check(K, lp, tg, il, tl, C32 - 1, f'f32 S={S}')
    assert bool(torch.isfinite(ref.score).all())


# ---- 8. walk-back and band extremes -------------------------------------------------------------------------------------------
def test_no_slack_path_falls_two_states_per_frame_and_one_frame_fewer_is_infeasible(K):
    """No two adjacent labels equal (all that the skip transition asks of 'distinct' labels at C = 32) and T = S: the only path takes
    the s-2 step every frame.  With planted repeats, T = S + repeats is feasible by exactly one frame; one fewer is not."""
    S, N = 300, 320
    lp, tg = AR.random_case(11, 2, N, C32, S)
    got, ref = check(K, lp, tg, [S, S - 1], [S, S], C32 - 1, 'T=S')
    assert ref.path[0, :S].tolist() == list(range(1, 2 * S, 2)) and float(ref.score[1]) == -np.inf
    assert float(got.score[1].cpu()) == -np.inf and bool((got.path[1] == -1).all()) and bool((got.spans[1] == -1).all())
    lp, tg = AR.random_case(12, 2, N, C32, S, repeats=12)
    tg[1] = tg[0]
    rep = AR.repeats_of(tg[0].tolist())
    assert rep >= 3
    got, ref = check(K, lp, tg, [S + rep, S + rep - 1], [S, S], C32 - 1, 'T=S+repeats')
    assert np.isfinite(float(ref.score[0])) and float(ref.score[1]) == -np.inf


def test_single_frame_single_label(K):
    lp, tg = AR.random_case(13, 1, 1, C32, 1)
    got, ref = check(K, lp, tg, [1], [1], C32 - 1, 'T=S=N=1')
    assert ref.path.tolist() == [[1]] and ref.spans.tolist() == [[[0, 1]]]
    got, ref = check(K, lp, tg, None, None, C32 - 1, 'T=S=N=1, NULL lengths')


def test_walk_back_windows_and_ragged_frames(K):
    W = K.load().sconf_align_walk_window()
    assert W == 16
    N = 5 * W + 3
    il = [N, 5 * W, W + 1, W - 1, 1, 2 * W + 7]                              # T = N and T < N in one batch; whole and broken windows
    tl = [20, 33, 7, 6, 0, 30]
    lp, tg = AR.random_case(14, len(il), N, C32, 41, il, tl, repeats=3)
    got, ref = check(K, lp, tg, il, tl, C32 - 1, 'windows')
    assert bool(torch.isfinite(ref.score).all())
    g = got.path.cpu()
    for b, T in enumerate(il):
        assert bool((g[b, T:] == -1).all()) and bool((got.labels[b, T:] == -1).all()) and bool((g[b, :T] >= 0).all())


def test_long_runs_of_one_label(K):
    tg = torch.tensor([[5] * 40 + [7] * 45 + [5] * 3 + list(range(10)), [3] * 98], dtype=torch.int32)
    S = tg.shape[1]
    N = 2 * S + 30
    il = [N, 2 * S - 1]                                                      # 97 repeats in row 1: feasible by exactly one frame
    lp, _ = AR.random_case(15, 2, N, C32, S, il, None, targets=tg)
    got, ref = check(K, lp, tg, il, None, C32 - 1, 'runs')
    assert bool(torch.isfinite(ref.score).all())


def test_a_poisoned_sample_leaves_its_neighbours_untouched(K):
    N, S = 70, 20
    il, tl = [N, N + 1, 60, 60, 55], [S, S, S + 1, S, S]
    lp, tg = AR.random_case(16, 5, N, C32, S, [N, N, 60, 60, 55], [S] * 5)
    tg[3, 4] = C32                                                         # a label outside [0, C)
    got, ref = check(K, lp, tg, il, tl, C32 - 1, 'poisoned')
    assert [bool(np.isnan(x)) for x in got.score.cpu().tolist()] == [False, True, True, True, False]
    for b in (1, 2, 3):
        assert bool((got.path[b] == -1).all()) and bool((got.labels[b] == -1).all()) and bool((got.spans[b] == -1).all())
        assert bool((got.token_logp[b] == 0).all())
    for b in (0, 4):                                                       # the healthy samples: bit-equal to a call of their own
        alone = K.ctc_align(lp[b:b + 1].cuda(), tg[b:b + 1].cuda(), torch.tensor(il[b:b + 1], dtype=torch.int32).cuda(),
                            torch.tensor(tl[b:b + 1], dtype=torch.int32).cuda(), C32 - 1)
        for a, w in zip(alone, got):
            assert torch.equal(a[0:1].contiguous().view(torch.uint8), w[b:b + 1].contiguous().view(torch.uint8))     # (score[b] has no dimension)


def test_refusals_on_the_device_path(K):
    lp, tg = AR.random_case(17, 1, 8, C32, 3)
    with pytest.raises(RuntimeError, match='GPU'):
        K.ctc_align(lp, tg.cuda(), None, None, 31)
    with pytest.raises(TypeError):
        K.ctc_align(lp.cuda().double(), tg.cuda(), None, None, 31)
    with pytest.raises(TypeError):
        K.ctc_align(lp.cuda(), tg.cuda().long(), None, None, 31)
    with pytest.raises(ValueError, match=str(K.max_labels())):
        K.ctc_align(lp.cuda(), torch.zeros(1, K.max_labels() + 1, dtype=torch.int32).cuda(), None, None, 31)
    with pytest.raises(RuntimeError, match='blank'):
        K.ctc_align(lp.cuda(), tg.cuda(), None, None, 32)


# ---- 9. footprint -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('id', list(AC.CASES))
def test_align_footprint(K, id):
    FP.run_on_device(AC.build(id, K.load()), K.PROTOTYPES)


# ---- 10. model level ------------------------------------------------------------------------------------------------------------
class IdTok:
    """Every token is a word: id i is spelt 't<i>'."""
    def __init__(self, V): self.V = V
    def vocab_size(self): return self.V
    def decode(self, ids): return ' '.join(f't{int(i)}' for i in ids)
    def encode(self, text): return [int(w[1:]) for w in text.split()]


CFG = dict(vocab_size=127, n_layers=2, d_model=64, n_heads=2, head_dim=32, subsampling_conv_channels=32, use_rotary=True,
           rotary_base_freq=1500000, decoder_norm=True, self_conditioning=True, bias_in_ff=False, default_norm='layer_norm')


def test_alignment_of_the_models_own_greedy_transcript(K):
    import audio_refs as AUD
    from lcasr_amd.decoding.align import ctc_forced_align
    from lcasr_amd.decoding.greedy import GreedyCTCDecoder
    from lcasr_amd.eval import run as R
    from lcasr_amd.models.sconformer_xl import SCConformerXL
    from lcasr_amd.utils import audio_tools as A
    torch.manual_seed(12345)
    model = SCConformerXL(**CFG).cuda().eval()
    wave = AUD.test_signal(3 * 16000, seed=9).cuda()
    tok, blank = IdTok(127), model.decoder.num_classes - 1
    spec = A.to_spectogram(wave[None])
    logits = R.moving_average_eval(R._Args(), model, spec, 128, 32, tok, use_tqdm=False, return_numpy=False)
    ids = GreedyCTCDecoder(tokenizer=tok, blank_id=blank)(logits, decode=False)
    assert len(ids) > 0
    text = tok.decode(ids)
    words = R.align(model, spec, text, tok, 128, 32)
    assert [w['word'] for w in words] == text.split()
    al = ctc_forced_align(logits, ids, blank=blank)
    assert np.isfinite(float(al.score))
    lab = al.labels.cpu()
    merged = [i for i in torch.unique_consecutive(lab).tolist() if i != blank]
    assert merged == ids and al.labels.shape == (logits.shape[0],)
    lg = logits.cpu()
    top2 = lg.topk(2, -1).values
    clear = top2[:, 0] > top2[:, 1]
    assert bool((lab[clear] == lg.argmax(-1)[clear].int()).all()) and int(clear.sum()) > 0
    sec = model.subsampling.subsampling_factor * A.HOP_LENGTH / A.SR
    for w, (f, l) in zip(words, al.spans.cpu().tolist()):
        assert w['startTime'] == f'{f * sec:.2f}s' and w['endTime'] == f'{l * sec:.2f}s' and 0 <= f < l <= logits.shape[0]
    assert R.align_waveform(model, wave, text, tok, 128, 32) == words
    with pytest.raises(ValueError, match='cannot be emitted'):
        R.align(model, spec, tok.decode([1, 2] * logits.shape[0]), tok, 128, 32)
