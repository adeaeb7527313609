"""CTC prefix beam search on the device (csrc/beam.hip through lcasr_amd.hip.beam) against the numpy restatement of the contract
(tests/beam_refs.py): count, tokens, lengths and token_frames EXACTLY, scores within eps = 8 T 2^-52 max|score| (a few ulp per
frame, accumulated linearly: the device's exp / log1p are not numpy's, and a run of frames without a kept token may add in another
order).  Every case first asserts ON THE CPU that the restatement's smallest decision gap on its input is at least 4 eps - then no
device total within eps of the restatement's can take another decision - and, from the restatement's counters or the library's
queries, that the input reaches what the case is named after.  C = 32 with the blank last unless a case says otherwise.

prepare(name) is the CPU half of a case (input, restatement, conditions) and needs no device."""
import math

import pytest
import torch

import beam_footprint_cases as BC
import beam_refs as BR
import footprint as FP

pytestmark = pytest.mark.gpu
C32, BL = 32, 31
INF = math.inf
DEFAULT = dict(W=16, nbest=4, thr=-5.0, prune=-10.0, K=16, L=None, il=None, blank=BL)


@pytest.fixture(scope='module')
def K():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from lcasr_amd.hip import beam
    beam.load()
    return beam


def zero_runs(kept):
    """[(first frame, length)] of the runs of frames without a kept token."""
    runs, t = [], 0
    while t < len(kept):
        if kept[t] == 0:
            s = t
            while t < len(kept) and kept[t] == 0: t += 1
            runs.append((s, t - s))
        else:
            t += 1
    return runs


RANK_LIMIT = 128


def sort_sizes(st):
    """The selection form of every frame with a kept token: 0 = ranked by counting (up to RANK_LIMIT candidates), else the keys sorted."""
    return {0 if c <= RANK_LIMIT else 1 << (c - 1).bit_length() for c in st['candidates']}


# name -> (input builder -> (lp, overrides of DEFAULT), condition(list of per-sample stats, lp, options, lib or None))
CASES = {}


def _width(W):
    def build():
        return BR.spiky_case(40 + W, 1, 200, C32, BL, every=4)[0]

    def cond(st, lp, o, lib):
        assert max(st[0]['live']) == W and (W == 1 or st[0]['folds'] > 0)
        if W > 2: assert st[0]['live'][0] < W and st[0]['live'][1] < W       # fewer live beams than W through the first frames
        if lib is not None: assert lib.sconf_beam_threads(W, 16) == {1: 64, 2: 64, 8: 128, 16: 256, 32: 512}.get(W, 1024)
    return build, cond


for _W in (1, 2, 8, 16, 32, 63, 64, 65, 100, 128):
    _b, _c = _width(_W)
    CASES[f'width-{_W}'] = (_b, dict(W=_W, nbest=min(_W, 4), cond=_c))


def _cond_cap1(st, lp, o, lib):
    assert st[0]['cap'] > 0 and max(st[0]['kept']) == 1
    if lib is not None: assert lib.sconf_beam_threads(16, 1) == 64


def _cond_cap16(st, lp, o, lib):
    assert st[0]['cap'] > 0 and max(st[0]['kept']) == 16 and max(st[0]['candidates']) == 16 * 17
    if lib is not None: assert lib.sconf_beam_max_tokens() == 16


CASES['kmax-1-cap'] = (lambda: BR.spiky_case(7, 1, 120, C32, BL, every=3, peak=4.0)[0], dict(K=1, cond=_cond_cap1))
CASES['kmax-16-cap-noise'] = (lambda: BR.noise_case(8, 1, 40, C32), dict(K=16, cond=_cond_cap16))


def _cond_argmax_alone(st, lp, o, lib):
    row_max, arg = lp[0, :, :4095].max(-1).values, lp[0].argmax(-1)
    alone = [t for t in range(64) if float(row_max[t]) < -5.0 and int(arg[t]) != 4095 and st[0]['kept'][t] == 1]
    assert len(alone) >= 8


CASES['argmax-alone-c4096'] = (lambda: BR.noise_case(9, 1, 64, 4096), dict(W=8, blank=4095, cond=_cond_argmax_alone))


def _cond_runs(st, lp, o, lib):
    G = 16 if lib is None else lib.sconf_beam_prefetch_frames()
    runs = zero_runs(st[0]['kept'])
    T = len(st[0]['kept'])
    lens = [n for _, n in runs]
    assert runs[0][0] == 0 and runs[0][1] > 2 * G and runs[-1][0] + runs[-1][1] == T and runs[-1][1] > G
    assert any(n < G for n in lens) and any(n == 1 for n in lens) and G in lens and G + 1 in lens and any(n >= 3 * G for n in lens)
    assert st[0]['folds'] > 0 and sum(k > 0 for k in st[0]['kept']) > 40


def _runs_input():
    G = 16
    quiet = [(0, 2 * G + 5), (60, 60 + G), (90, 90 + G + 1), (120, 123), (140, 140 + 3 * G + 2), (300 - G - 4, 300)]
    lp = BR.spiky_case(10, 1, 300, C32, BL, every=2, quiet=quiet)[0]
    return lp


CASES['blank-runs'] = (_runs_input, dict(W=16, cond=_cond_runs))


def _cond_one_beam(st, lp, o, lib):
    assert max(st[0]['live']) == 1 and st[0]['pruned'] > 0


def _cond_no_prune(st, lp, o, lib):
    assert st[0]['pruned'] == 0 and max(st[0]['live']) == 16


CASES['prune-to-one-beam'] = (lambda: BR.spiky_case(12, 1, 150, C32, BL, every=4)[0], dict(prune=-1e-3, cond=_cond_one_beam))
CASES['prune-off'] = (lambda: BR.spiky_case(13, 1, 150, C32, BL, every=4)[0], dict(prune=-INF, cond=_cond_no_prune))


def _recreate(W):
    def build():
        seed, scale = BR.recreation_case(W)
        return BR.noise_case(seed, 1, 24, 4, scale)

    def cond(st, lp, o, lib):
        assert st[0]['recreated'] >= 1
    return build, cond


for _W in (2, 3, 4):
    _b, _c = _recreate(_W)
    CASES[f'recreated-prefix-width-{_W}'] = (_b, dict(W=_W, nbest=_W, blank=3, cond=_c))


def _cond_sorts(st, lp, o, lib):
    got = sort_sizes(st[0]) | sort_sizes(st[1])
    assert {0, 512, 1024, 2048, 4096} <= got and max(st[0]['candidates']) == 128 * 17              # the largest sort there is, and most others
    if lib is not None: assert all(lib.sconf_beam_sort_size(c) in got for s in st for c in s['candidates'])


def _sorts_input():
    a = BR.noise_case(14, 1, 48, C32)
    b = BR.spiky_case(15, 1, 48, C32, BL, every=3, peak=5.0)[0]
    return torch.cat([a, b])


CASES['largest-sort'] = (_sorts_input, dict(W=128, nbest=8, prune=-INF, cond=_cond_sorts))


def _cond_ragged(st, lp, o, lib):
    assert [len(s['kept']) for s in st] == o['il'] and o['il'] == [90, 1, 0, 83, 90, 17]


CASES['ragged-batch'] = (lambda: BR.spiky_case(16, 6, 90, C32, BL, every=3, in_len=[90, 1, 0, 83, 90, 17])[0],
                         dict(il=[90, 1, 0, 83, 90, 17], nbest=3, cond=_cond_ragged))
CASES['lmax-shorter'] = (lambda: BR.spiky_case(17, 2, 80, C32, BL, every=3)[0], dict(L=5, cond=lambda st, lp, o, lib: None))


def _padded_input():
    g = torch.Generator().manual_seed(18)
    x = torch.randn(2, 70, 129, generator=g)
    x[:, :, 128] += 4.0
    for t in range(0, 70, 3): x[:, t, (7 * t) % 128] += 8.0
    lp = torch.log_softmax(x, -1)
    return torch.nn.functional.pad(lp, (0, 15), value=-INF).contiguous()


def _cond_padded(st, lp, o, lib):
    assert lp.shape[-1] == 144 and bool(torch.isinf(lp[..., 129:]).all()) and st[0]['folds'] > 0


CASES['padded-classes-129-to-144'] = (_padded_input, dict(blank=128, cond=_cond_padded))

_prepared = {}


def prepare(name, lib=None):
    """The CPU half: (lp, options, restatement, eps per sample); asserts the case's conditions and gap >= 4 eps."""
    if name not in _prepared:
        build, opt = CASES[name]
        o = {**DEFAULT, **{k: v for k, v in opt.items() if k != 'cond'}}
        lp = build()
        B, N, C = lp.shape
        if o['L'] is None: o['L'] = N
        st = []
        ref = BR.ctc_beam(lp, o['il'], o['blank'], o['W'], o['nbest'], o['thr'], o['prune'], o['K'], o['L'], stats=st)
        eps = []
        for b, s in enumerate(st):
            if s is None:
                eps.append(0.0)
                continue
            T = len(s['kept'])
            e = BR.eps_of(T, s['max_score'])
            print(f'[beam] {name} sample {b}: T {T} gap {s["gap"]:.3e} eps {e:.3e} cap {s["cap"]} pruned {s["pruned"]} folds {s["folds"]} '
                  f'recreated {s["recreated"]} max live {max(s["live"], default=1)} frames without a token {sum(k == 0 for k in s["kept"])}')
            assert s['gap'] >= 4 * e, f'{name} sample {b}: the smallest decision gap {s["gap"]:.3e} is below 4 eps = {4 * e:.3e}: choose another seed'
            eps.append(e)
        _prepared[name] = (lp, o, ref, eps, st)
    lp, o, ref, eps, st = _prepared[name]
    opt = CASES[name][1]
    if 'cond' in opt: opt['cond']([s for s in st], lp, o, lib)
    return lp, o, ref, eps


def run(K, lp, o):
    il = None if o['il'] is None else torch.tensor(o['il'], dtype=torch.int32).cuda()
    got = K.ctc_beam(lp.cuda(), il, o['blank'], o['W'], o['nbest'], o['thr'], o['prune'], o['K'], o['L'])
    torch.cuda.synchronize()
    return got


def compare(name, got, ref, eps):
    g = [t.cpu() for t in got]
    for what, a, b in zip(('count', 'tokens', 'lengths', 'token_frames'), g[:4], ref[:4]):
        bad = (a != b).nonzero()
        assert not bad.numel(), f'{name} {what}: {bad.shape[0]} element(s) differ, first at {bad[0].tolist()}: {a[tuple(bad[0])]} != {b[tuple(bad[0])]}'
    worst = 0.0
    for b in range(ref.scores.shape[0]):
        for r in range(ref.scores.shape[1]):
            x, y = float(g[4][b, r]), float(ref.scores[b, r])
            if not math.isfinite(y):
                assert (math.isnan(x) and math.isnan(y)) or x == y, f'{name} scores[{b}][{r}]: {x} != {y}'
            else:
                worst = max(worst, abs(x - y))
                assert abs(x - y) <= eps[b], f'{name} scores[{b}][{r}]: {x!r} != {y!r} (|d| {abs(x - y):.3e} > eps {eps[b]:.3e})'
    print(f'[beam gpu] {name}: largest |score - restated| {worst:.3e}, eps {max(eps):.3e}')


@pytest.mark.parametrize('name', list(CASES))
def test_search_against_the_restatement(K, name):
    lp, o, ref, eps = prepare(name, K.load())
    compare(name, run(K, lp, o), ref, eps)


def test_the_cases_reach_every_selection_form(K):
    """A frame of up to sconf_beam_rank_limit() candidates is ranked by counting, a larger one sorted at the next power of two: the
    cases above meet the ranked form from 2 candidates to the limit's half and beyond, and every sort size there is."""
    lib, got, cand = K.load(), set(), set()
    assert lib.sconf_beam_rank_limit() == RANK_LIMIT
    for name in CASES:
        prepare(name)
        for s in _prepared[name][4]:
            if s is not None:
                assert all(lib.sconf_beam_sort_size(c) == (0 if c <= RANK_LIMIT else 1 << (c - 1).bit_length()) for c in s['candidates'])
                got |= sort_sizes(s)
                cand |= s['candidates']
    assert got == {0, 256, 512, 1024, 2048, 4096}, sorted(got)
    assert 2 in cand and RANK_LIMIT in cand and any(RANK_LIMIT < c <= RANK_LIMIT + 64 for c in cand)      # both sides of the threshold


def test_two_calls_are_bit_equal(K):
    lp, o, ref, eps = prepare('width-100', K.load())
    a, b = run(K, lp, o), run(K, lp, o)
    assert all(torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)) for x, y in zip(a, b))


def test_a_poisoned_sample_leaves_its_neighbours_untouched(K):
    N = 60
    lp = BR.spiky_case(19, 4, N, C32, BL, every=3)[0]
    il = [N, N + 1, -1, 41]
    o = {**DEFAULT, 'il': il, 'L': N, 'nbest': 3}
    st = []
    ref = BR.ctc_beam(lp, il, BL, o['W'], o['nbest'], o['thr'], o['prune'], o['K'], N, stats=st)
    eps = [0.0 if s is None else BR.eps_of(len(s['kept']), s['max_score']) for s in st]
    assert all(s is None or s['gap'] >= 4 * e for s, e in zip(st, eps)) and [s is None for s in st] == [False, True, True, False]
    got = run(K, lp, o)
    compare('poisoned', got, ref, eps)
    assert got.count.tolist() == [3, 0, 0, 3] and bool(torch.isnan(got.scores[1:3]).all())
    assert bool((got.tokens[1:3] == -1).all()) and bool((got.token_frames[1:3] == -1).all()) and bool((got.lengths[1:3] == 0).all())
    for b in (0, 3):                                                       # the healthy samples: bit-equal to a call of their own
        alone = run(K, lp[b:b + 1], {**o, 'il': il[b:b + 1]})
        for a, w in zip(alone, got):
            assert torch.equal(a[0:1].contiguous().view(torch.uint8), w[b:b + 1].contiguous().view(torch.uint8))


def test_non_finite_log_probs_stay_in_range(K):
    lp = BR.spiky_case(20, 3, 50, C32, BL, every=3)[0].clone()
    lp[0, 7, 3] = math.nan
    lp[0, 20] = math.nan
    lp[1, 9, 5] = INF
    lp[1, 30, BL] = -INF
    lp[2, 11] = -INF
    got = run(K, lp, {**DEFAULT, 'L': 50})
    t, f = got.tokens.cpu(), got.token_frames.cpu()
    assert bool(((t >= -1) & (t < C32)).all()) and bool(((f >= -1) & (f < 50)).all())
    assert bool(((got.count >= 0) & (got.count <= 4)).all()) and bool(((got.lengths >= 0) & (got.lengths <= 50)).all())
    assert got.count[2] == 0                                               # a frame of -inf: every total is -inf, no beam is left


def _ctc_ll(lp_dev, hyps, blank):
    """Full CTC log-likelihood (f64 tensor, on the host) of each token list under lp_dev (N, C), by the loss kernel."""
    from lcasr_amd.hip import ops
    n, S = len(hyps), max(max((len(h) for h in hyps), default=0), 1)
    tg = torch.zeros(n, S, dtype=torch.int32)
    for i, h in enumerate(hyps): tg[i, :len(h)] = torch.tensor(h, dtype=torch.int32)
    N = lp_dev.shape[0]
    nll, _ = ops.ctc_fwd(lp_dev[None].expand(n, -1, -1).contiguous(), tg.cuda(), torch.full((n,), N, dtype=torch.int32).cuda(),
                         torch.tensor([len(h) for h in hyps], dtype=torch.int32).cuda(), blank)
    torch.cuda.synchronize()
    return -nll.double().cpu()


def _hyps(got, b=0):
    tok, ln = got.tokens.cpu(), got.lengths.cpu()
    return [tok[b, r, :int(ln[b, r])].tolist() for r in range(int(got.count[b]))]


@pytest.mark.parametrize('T,labels', [(1, 3), (3, 3), (4, 3), (5, 2), (6, 2)])
def test_exhaustive_search_equals_the_ctc_loss(K, T, labels):
    """Pruning off and W = 128 above the number of label sequences (at most 121 for 3 labels in 4 frames, 127 for 2 in 6): every
    score is the full CTC log-likelihood of its tokens, as the loss kernel computes it."""
    g = torch.Generator().manual_seed(100 * T + labels)
    lp = torch.log_softmax(torch.randn(1, T, labels + 1, generator=g) * 1.5, -1)
    lp = torch.nn.functional.pad(lp, (0, 4 - (labels + 1) % 4 if (labels + 1) % 4 else 0), value=-INF).contiguous()
    o = {**DEFAULT, 'W': 128, 'nbest': 128, 'thr': -INF, 'prune': -INF, 'blank': labels, 'L': T}
    got = run(K, lp, o)
    hyps = _hyps(got)
    want = BR.enumerate_paths(lp[0, :, :labels + 1].numpy(), labels)
    assert len(hyps) == len(want) <= 127 and {tuple(h) for h in hyps} == set(want)
    ll = _ctc_ll(lp[0].cuda(), hyps, labels)
    sc = got.scores[0, :len(hyps)].cpu()
    rel = ((sc - ll).abs() / ll.abs().clamp(min=1e-30)).max()
    print(f'[beam gpu] T={T} labels={labels}: {len(hyps)} hypotheses, largest relative |score + ctc_fwd| {float(rel):.2e}')
    assert float(rel) <= 1e-6


@pytest.mark.parametrize('name', ['width-16', 'width-100', 'blank-runs'])
def test_scores_do_not_exceed_the_full_likelihood(K, name):
    """Default options on the spiky inputs: the search sums a subset of the alignments of each hypothesis."""
    lp, o, ref, eps = prepare(name)
    got = run(K, lp, o)
    hyps = _hyps(got)
    ll = _ctc_ll(lp[0].cuda(), hyps, o['blank'])
    sc = got.scores[0, :len(hyps)].cpu()
    print(f'[beam gpu] {name}: score - full likelihood {[f"{float(d):.3e}" for d in sc - ll]}, eps {eps[0]:.3e}')
    assert len(hyps) >= 1 and bool((sc <= ll + eps[0]).all())


def test_refusals_on_the_device_path(K):
    lp = BR.noise_case(21, 1, 8, C32)
    with pytest.raises(RuntimeError, match='GPU'):
        K.ctc_beam(lp, None, BL, 4, 1, -5.0, -10.0, 4, 8)
    with pytest.raises(TypeError):
        K.ctc_beam(lp.cuda().double(), None, BL, 4, 1, -5.0, -10.0, 4, 8)
    with pytest.raises(TypeError):
        K.ctc_beam(lp.cuda(), torch.tensor([8]).cuda(), BL, 4, 1, -5.0, -10.0, 4, 8)
    with pytest.raises(ValueError, match=str(K.max_width())):
        K.ctc_beam(lp.cuda(), None, BL, K.max_width() + 1, 1, -5.0, -10.0, 4, 8)
    with pytest.raises(ValueError, match='nbest'):
        K.ctc_beam(lp.cuda(), None, BL, 4, 5, -5.0, -10.0, 4, 8)
    with pytest.raises(RuntimeError, match='blank'):
        K.ctc_beam(lp.cuda(), None, C32, 4, 1, -5.0, -10.0, 4, 8)


# ---- footprint ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('id', list(BC.CASES))
def test_beam_footprint(K, id):
    FP.run_on_device(BC.build(id, K.load()), K.PROTOTYPES)


# ---- model level ----------------------------------------------------------------------------------------------------------------
class IdTok:
    """Every token is a word: id i is spelt 't<i>'."""
    def __init__(self, V): self.V = V
    def vocab_size(self): return self.V
    def decode(self, ids): return ' '.join(f't{int(i)}' for i in ids)
    def encode(self, text): return [int(w[1:]) for w in text.split()]


CFG = dict(vocab_size=127, n_layers=2, d_model=64, n_heads=2, head_dim=32, subsampling_conv_channels=32, use_rotary=True,
           rotary_base_freq=1500000, decoder_norm=True, self_conditioning=True, bias_in_ff=False, default_norm='layer_norm')


def test_transcribe_with_a_beam_is_at_least_as_likely_as_greedy(K):
    import audio_refs as AUD
    from lcasr_amd.decoding.beam import BeamSearchCTCDecoder
    from lcasr_amd.eval import run as R
    from lcasr_amd.eval.utils import decode_beams_lm
    from lcasr_amd.models.sconformer_xl import SCConformerXL
    from lcasr_amd.utils import audio_tools as A
    torch.manual_seed(12345)
    model = SCConformerXL(**CFG).cuda().eval()
    wave = AUD.test_signal(3 * 16000, seed=9).cuda()
    tok, blank = IdTok(127), model.decoder.num_classes - 1
    greedy = R.transcribe(model, wave, tok, 128, 32)
    assert greedy == R.transcribe(model, wave, tok, 128, 32, beam_width=1)
    beam = R.transcribe(model, wave, tok, 128, 32, beam_width=8)
    logits = R.moving_average_eval(R._Args(), model, A.to_spectogram(wave[None]), 128, 32, tok, use_tqdm=False, return_numpy=False)
    ll = _ctc_ll(logits.float().contiguous(), [tok.encode(beam), tok.encode(greedy)], blank)
    print(f'[beam gpu] tiny model: log-likelihood of the beam transcript {float(ll[0]):.4f}, of the greedy one {float(ll[1]):.4f}')
    assert float(ll[0]) >= float(ll[1])
    dec = BeamSearchCTCDecoder(tokenizer=tok, blank_id=blank, beam_width=8)
    data, best = decode_beams_lm([logits], dec, beam_width=8, ds_factor=model.subsampling.subsampling_factor)
    assert data[0]['text'] == beam and data[0]['ngram_score'] == 0 and data[0]['am_score'] == best.logit_score <= float(ll[0]) + 1e-3
    assert [w['word'] for w in data[0]['frames']] == beam.split()
    assert all(0 <= w['start'] < w['end'] <= A.total_seconds(logits.shape[0] * model.subsampling.subsampling_factor) for w in data[0]['frames'])
