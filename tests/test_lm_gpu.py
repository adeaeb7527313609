"""CTC prefix beam search with an n-gram LM fused in, on the device (csrc/beam_lm.hip through lcasr_amd.hip.lm) against the
restatement of the contract (tests/lm_refs.py, whose LM is a dict recursion, not the image): count, tokens, lengths and token_frames
EXACTLY, scores and logit_scores within eps = 8 T 2^-52 max|score| (test_beam_gpu.py's tolerance, max|score| taken over keys, acoustic
totals and bonuses).  Every case first asserts ON THE CPU that the restatement's smallest decision gap on its input is at least 4 eps
and, from the restatement's counters or the library's queries, that the input reaches what the case is named after; a case that does
not is given another seed here, never skipped.  C = 32 with the blank last unless a case says otherwise.

prepare(name) is the CPU half of a case (input, LM, restatement, conditions) and needs no device."""
import math

import numpy as np
import pytest
import torch

import beam_refs as BR
import footprint as FP
import lm_footprint_cases as LC
import lm_refs as LR

pytestmark = pytest.mark.gpu
C32, BL = 32, 31
INF = math.inf
DEFAULT = dict(W=16, nbest=4, thr=-5.0, prune=-10.0, K=16, L=None, il=None, blank=BL, alpha=0.5, beta=1.5)
RANK_LIMIT = 128


@pytest.fixture(scope='module')
def K():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from lcasr_amd.hip import lm
    lm.load()
    return lm


# ---- language models -------------------------------------------------------------------------------------------------------------
_lms = {}


def trained(V, order, streams=(), seed=0, bos=True, use_bos=True, drop=()):
    """(image, restatement) of an order-`order` model over V tokens trained on a seeded random stream plus `streams` (the labels of
    a case's input, so that its prefixes reach long contexts); `drop`: tokens whose every gram is removed (they score <unk>)."""
    key = (V, order, tuple(map(tuple, streams)), seed, bos, use_bos, tuple(drop))
    if key not in _lms:
        rnd = np.random.default_rng(1000 + seed).integers(0, V, 20 * V).tolist()
        table = LR.train([rnd] + [list(s) for s in streams], order, V, bos=bos)
        table = {g: v for g, v in table.items() if not any(w in drop for w in g)}
        _lms[key] = LR.lm_pair(table, order, V, -4.0 if drop else None, use_bos=use_bos)
    return _lms[key]


def sort_sizes(st):
    return {0 if c <= RANK_LIMIT else 1 << (c - 1).bit_length() for c in st['candidates']}


def zero_runs(kept):
    runs, t = [], 0
    while t < len(kept):
        if kept[t] == 0:
            s = t
            while t < len(kept) and kept[t] == 0: t += 1
            runs.append((s, t - s))
        else:
            t += 1
    return runs


# name -> (builder -> (lp, (image, restatement)), overrides of DEFAULT with cond(stats, lp, options, lib or None))
CASES = {}


def _width(W):
    def build():
        lp, labels = BR.spiky_case(40 + W, 1, 200, C32, BL, every=4, peak=8.0 if W < 100 else 6.0)     # (lower peaks: W beams do get live)
        return lp, trained(31, 3, labels)

    def cond(st, lp, o, lib):
        assert max(st[0]['live']) == W and (W == 1 or st[0]['folds'] > 0) and st[0]['lookups'] > 0
        if W > 2: assert st[0]['live'][0] < W and st[0]['live'][1] < W
        if lib is not None: assert lib.sconf_lm_beam_threads(W, 16) == {1: 64, 2: 64, 8: 128, 16: 256, 32: 512}.get(W, 1024)
    return build, cond


for _W in (1, 2, 8, 16, 32, 63, 64, 65, 100, 128):
    _b, _c = _width(_W)
    CASES[f'width-{_W}'] = (_b, dict(W=_W, nbest=min(_W, 4), cond=_c))


def _order(n):
    def build():
        lp, labels = BR.spiky_case(60 + n, 1, 120, C32, BL, every=3, peak=5.0)
        return lp, trained(31, n, labels, drop=(5, 17))

    def cond(st, lp, o, lib):
        d = st[0]['depth']
        assert len(d) == n + 1 and all(d[k] > 0 for k in range(n)) and d[n] == 0, d      # every back-off depth 0 .. n - 1
        assert st[0]['unk'] > 0 and st[0]['folds'] > 0
        if lib is not None: assert n <= lib.sconf_lm_max_order()
    return build, cond


for _n in (1, 2, 3, 4, 5):
    _b, _c = _order(_n)
    CASES[f'order-{_n}'] = (_b, dict(cond=_c))


def _cond_cap1(st, lp, o, lib):
    assert st[0]['cap'] > 0 and max(st[0]['kept']) == 1
    if lib is not None: assert lib.sconf_lm_beam_threads(16, 1) == 64


def _cond_cap16(st, lp, o, lib):
    assert st[0]['cap'] > 0 and max(st[0]['kept']) == 16 and max(st[0]['candidates']) == 16 * 17


def _cap1_input():
    lp, labels = BR.spiky_case(7, 1, 120, C32, BL, every=3, peak=4.0)
    return lp, trained(31, 3, labels)


CASES['kmax-1-cap'] = (_cap1_input, dict(K=1, cond=_cond_cap1))
CASES['kmax-16-cap-noise'] = (lambda: (BR.noise_case(8, 1, 40, C32), trained(31, 3)), dict(K=16, cond=_cond_cap16))

# C = 4096: a bigram model in which token 7 has EVERY token as a child (a binary search of 12 steps), token 8 one child and token 9
# none; the planted labels walk through these contexts.
BIG_V, BIG_LABELS = 4095, [7, 100, 8, 200, 9, 300, 7, 4094, 8, 0, 9, 7, 2047, 7, 2048]


def _big_input():
    g = torch.Generator().manual_seed(9)
    x = torch.randn(1, 3 * len(BIG_LABELS), 4096, generator=g)
    for t in range(x.shape[1]):
        if t % 3 == 1:
            x[0, t, BIG_LABELS[t // 3]] += 12.0
            x[0, t, (BIG_LABELS[t // 3] * 7 + 3) % BIG_V] += 11.0          # a competitor
        else:
            x[0, t, 4095] += 12.0
    rng = np.random.default_rng(9)
    table = {(w,): (float(-rng.uniform(2.0, 5.0)), float(-rng.uniform(0.1, 1.0)) if w in (7, 8, 9) else None) for w in range(BIG_V)}
    for w in range(BIG_V): table[(7, w)] = (float(-rng.uniform(0.5, 6.0)), None)
    table[(8, 200)] = (-0.25, None)
    return torch.log_softmax(x, -1).contiguous(), LR.lm_pair(table, 2, BIG_V, use_bos=False)


def _cond_big(st, lp, o, lib):
    img = _prepared['c4096-dense-context'][5][0]
    ctx = {g: s for s, g in enumerate(img.contexts)}
    assert [int(img.states[ctx[(w,)], 1]) for w in (7, 8, 9)] == [BIG_V, 1, 0] and math.ceil(math.log2(BIG_V)) == 12
    best = _prepared['c4096-dense-context'][2].tokens[0, 0].tolist()
    after = {a: b for a, b in zip(best, best[1:]) if b >= 0}
    assert 7 in after and 8 in after and 9 in after                        # lookups from all three contexts
    assert st[0]['depth'][0] > 0 and st[0]['depth'][1] > 0


CASES['c4096-dense-context'] = (_big_input, dict(W=8, blank=4095, cond=_cond_big))


def _runs_input():
    G = 16
    quiet = [(0, 2 * G + 5), (60, 60 + G), (90, 90 + G + 1), (120, 123), (140, 140 + 3 * G + 2), (300 - G - 4, 300)]
    lp, labels = BR.spiky_case(10, 1, 300, C32, BL, every=2, quiet=quiet)
    return lp, trained(31, 3, labels)


def _cond_runs(st, lp, o, lib):
    lens = [n for _, n in zero_runs(st[0]['kept'])]
    assert 1 in lens and 16 in lens and 17 in lens and 50 in lens and st[0]['folds'] > 0 and sum(k > 0 for k in st[0]['kept']) > 40


CASES['token-less-runs'] = (_runs_input, dict(W=16, cond=_cond_runs))


RECREATE_BETA = 0.3     # (a large bonus per token favours the longer prefix so much that a prefix is hardly ever created again)


def recreation_case_lm(W, ref, alpha, beta):
    for scale in (1.0, 0.5):
        for seed in range(60):
            if LR.search_lm(BR.noise_case(seed, 1, 24, 4, scale)[0].numpy(), 3, W, ref, alpha, beta)[1]['recreated'] >= 1:
                return seed, scale
    return None


def _recreate(W):
    def build():
        lm = trained(3, 3, seed=W)
        seed, scale = recreation_case_lm(W, lm[1], 0.5, RECREATE_BETA)
        return BR.noise_case(seed, 1, 24, 4, scale), lm

    def cond(st, lp, o, lib):
        assert st[0]['recreated'] >= 1
    return build, cond


for _W in (2, 3, 4):
    _b, _c = _recreate(_W)
    CASES[f'recreated-prefix-width-{_W}'] = (_b, dict(W=_W, nbest=_W, blank=3, beta=RECREATE_BETA, cond=_c))


def _sorts_input():
    a = BR.noise_case(14, 1, 48, C32)
    b, labels = BR.spiky_case(15, 1, 48, C32, BL, every=3, peak=5.0)
    return torch.cat([a, b]), trained(31, 3, labels)


def _cond_sorts(st, lp, o, lib):
    got = sort_sizes(st[0]) | sort_sizes(st[1])
    assert {0, 512, 1024, 2048, 4096} <= got and max(st[0]['candidates']) == 128 * 17


CASES['largest-sort'] = (_sorts_input, dict(W=128, nbest=8, prune=-INF, cond=_cond_sorts))


def _ragged_input():
    lp, labels = BR.spiky_case(16, 6, 90, C32, BL, every=3, in_len=[90, 1, 0, 83, 90, 17])
    return lp, trained(31, 3, labels)


def _cond_ragged(st, lp, o, lib):
    assert [len(s['kept']) for s in st] == o['il'] == [90, 1, 0, 83, 90, 17]


def _short_input():
    lp, labels = BR.spiky_case(17, 2, 80, C32, BL, every=3)
    return lp, trained(31, 3, labels)


CASES['ragged-batch'] = (_ragged_input, dict(il=[90, 1, 0, 83, 90, 17], nbest=3, cond=_cond_ragged))
CASES['lmax-shorter'] = (_short_input, dict(L=5, cond=lambda st, lp, o, lib: None))


def _padded_input():
    g = torch.Generator().manual_seed(18)
    x = torch.randn(2, 70, 129, generator=g)
    x[:, :, 128] += 4.0
    for t in range(0, 70, 3): x[:, t, (7 * t) % 128] += 8.0
    lp = torch.log_softmax(x, -1)
    return torch.nn.functional.pad(lp, (0, 15), value=-INF).contiguous(), trained(128, 3, [[(7 * t) % 128 for t in range(0, 70, 3)]])


def _cond_padded(st, lp, o, lib):
    assert lp.shape[-1] == 144 and bool(torch.isinf(lp[..., 129:]).all()) and st[0]['folds'] > 0


CASES['padded-classes-129-to-144'] = (_padded_input, dict(blank=128, cond=_cond_padded))


def _bos(use):
    def build():
        lp, labels = BR.spiky_case(23, 1, 100, C32, BL, every=3)
        return lp, trained(31, 3, labels, use_bos=use)

    def cond(st, lp, o, lib):
        img, ref = _prepared[f'use-bos-{"on" if use else "off"}'][5]
        assert (img.start_state != 0) == use and (ref.start == (31,)) == use
    return build, cond


for _u in (True, False):
    _b, _c = _bos(_u)
    CASES[f'use-bos-{"on" if _u else "off"}'] = (_b, dict(cond=_c))


def _useful(seed):
    return lambda: (LR.usefulness_case(seed)[0], LR.lm_pair(LR.usefulness_table(), 3, 12))


for _s in LR.USEFUL_SEEDS:
    CASES[f'usefulness-seed-{_s}'] = (_useful(_s), dict(blank=15, nbest=1, alpha=1.0, beta=1.0, cond=lambda st, lp, o, lib: None))

_prepared = {}


def prepare(name, lib=None):
    """The CPU half: (lp, options, restatement, eps per sample, image); asserts the case's conditions and gap >= 4 eps."""
    if name not in _prepared:
        build, opt = CASES[name]
        o = {**DEFAULT, **{k: v for k, v in opt.items() if k != 'cond'}}
        lp, lm = build()
        B, N, C = lp.shape
        if o['L'] is None: o['L'] = N
        st = []
        ref = LR.ctc_beam_lm(lp, o['il'], lm[1], o['blank'], o['W'], o['nbest'], o['thr'], o['prune'], o['K'], o['L'], o['alpha'], o['beta'], stats=st)
        eps = []
        for b, s in enumerate(st):
            if s is None:
                eps.append(0.0)
                continue
            T = len(s['kept'])
            e = BR.eps_of(T, s['max_score'])
            print(f'[lm] {name} sample {b}: T {T} gap {s["gap"]:.3e} eps {e:.3e} cap {s["cap"]} pruned {s["pruned"]} folds {s["folds"]} '
                  f'recreated {s["recreated"]} max live {max(s["live"], default=1)} lookups {s["lookups"]} by depth {s["depth"]} unk {s["unk"]}')
            assert s['gap'] >= 4 * e, f'{name} sample {b}: the smallest decision gap {s["gap"]:.3e} is below 4 eps = {4 * e:.3e}: choose another seed'
            eps.append(e)
        _prepared[name] = (lp, o, ref, eps, st, lm)
    lp, o, ref, eps, st, lm = _prepared[name]
    opt = CASES[name][1]
    if 'cond' in opt: opt['cond']([s for s in st], lp, o, lib)
    return lp, o, ref, eps, lm[0]


def run(K, lp, o, img):
    il = None if o['il'] is None else torch.tensor(o['il'], dtype=torch.int32).cuda()
    got = K.ctc_beam_lm(lp.cuda(), il, img.device_image('cuda'), img.n_states, img.n_entries, img.num_tokens, img.order, img.start_state,
                        o['blank'], o['W'], o['nbest'], o['thr'], o['prune'], o['K'], o['L'], o['alpha'], o['beta'])
    torch.cuda.synchronize()
    return got


def compare(name, got, ref, eps):
    g = [t.cpu() for t in got]
    for what, a, b in zip(('count', 'tokens', 'lengths', 'token_frames'), g[:4], ref[:4]):
        bad = (a != b).nonzero()
        assert not bad.numel(), f'{name} {what}: {bad.shape[0]} element(s) differ, first at {bad[0].tolist()}: {a[tuple(bad[0])]} != {b[tuple(bad[0])]}'
    worst = 0.0
    for what, gs, rs in (('scores', g[4], ref.scores), ('logit_scores', g[5], ref.logit_scores)):
        for b in range(rs.shape[0]):
            for r in range(rs.shape[1]):
                x, y = float(gs[b, r]), float(rs[b, r])
                if not math.isfinite(y):
                    assert (math.isnan(x) and math.isnan(y)) or x == y, f'{name} {what}[{b}][{r}]: {x} != {y}'
                else:
                    worst = max(worst, abs(x - y))
                    assert abs(x - y) <= eps[b], f'{name} {what}[{b}][{r}]: {x!r} != {y!r} (|d| {abs(x - y):.3e} > eps {eps[b]:.3e})'
    print(f'[lm gpu] {name}: largest |score - restated| {worst:.3e}, eps {max(eps):.3e}')


@pytest.mark.parametrize('name', list(CASES))
def test_fused_search_against_the_restatement(K, name):
    lp, o, ref, eps, img = prepare(name, K.load())
    compare(name, run(K, lp, o, img), ref, eps)


def test_the_cases_reach_every_selection_form(K):
    lib, got, cand = K.load(), set(), set()
    for name in CASES:
        prepare(name)
        for s in _prepared[name][4]:
            if s is not None:
                got |= sort_sizes(s)
                cand |= s['candidates']
    assert got == {0, 256, 512, 1024, 2048, 4096}, sorted(got)
    assert 2 in cand and RANK_LIMIT in cand and any(RANK_LIMIT < c <= RANK_LIMIT + 64 for c in cand)      # both sides of the threshold


def test_the_lm_corrects_the_ambiguous_input_on_the_device(K):
    """The usefulness case: the device's LM-free search makes at least 10 token errors of 192, the fused one at most half as many."""
    from lcasr_amd.hip import beam
    free = fused = 0
    for seed in LR.USEFUL_SEEDS:
        name = f'usefulness-seed-{seed}'
        lp, o, ref, eps, img = prepare(name)
        labels = LR.usefulness_case(seed)[1]
        a = beam.ctc_beam(lp.cuda(), None, 15, 16, 1, -5.0, -10.0, 16, 96)
        b = run(K, lp, o, img)
        free += LR.edit_distance(a.tokens[0, 0, :int(a.lengths[0, 0])].tolist(), labels)
        fused += LR.edit_distance(b.tokens[0, 0, :int(b.lengths[0, 0])].tolist(), labels)
    print(f'[lm gpu] token errors of 192: LM-free {free}, with the trigram {fused}')
    assert free >= 10 and 2 * fused <= free


def test_two_calls_are_bit_equal(K):
    lp, o, ref, eps, img = prepare('width-100', K.load())
    a, b = run(K, lp, o, img), run(K, lp, o, img)
    assert all(torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)) for x, y in zip(a, b))


@pytest.mark.parametrize('W', [1, 16, 100])
def test_without_weights_the_outputs_are_those_of_the_lm_free_kernel(K, W):
    """alpha = beta = 0: the five classic outputs are bit-equal to lcasr_amd.hip.beam.ctc_beam on the same input, and logit_scores
    equals scores."""
    from lcasr_amd.hip import beam
    lp, o, ref, eps, img = prepare(f'width-{W}')
    o = {**o, 'alpha': 0.0, 'beta': 0.0}
    got = run(K, lp, o, img)
    want = beam.ctc_beam(lp.cuda(), None, o['blank'], o['W'], o['nbest'], o['thr'], o['prune'], o['K'], o['L'])
    torch.cuda.synchronize()
    for what, x, y in zip(want._fields, got[:5], want):
        assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), what
    assert torch.equal(got.logit_scores.view(torch.uint8), got.scores.view(torch.uint8))


def test_a_poisoned_sample_leaves_its_neighbours_untouched(K):
    N = 60
    lp, labels = BR.spiky_case(19, 4, N, C32, BL, every=3)
    img, ref_lm = trained(31, 3, labels)
    il = [N, N + 1, -1, 41]
    o = {**DEFAULT, 'il': il, 'L': N, 'nbest': 3}
    st = []
    ref = LR.ctc_beam_lm(lp, il, ref_lm, BL, o['W'], o['nbest'], o['thr'], o['prune'], o['K'], N, o['alpha'], o['beta'], stats=st)
    eps = [0.0 if s is None else BR.eps_of(len(s['kept']), s['max_score']) for s in st]
    assert all(s is None or s['gap'] >= 4 * e for s, e in zip(st, eps)) and [s is None for s in st] == [False, True, True, False]
    got = run(K, lp, o, img)
    compare('poisoned', got, ref, eps)
    assert got.count.tolist() == [3, 0, 0, 3] and bool(torch.isnan(got.scores[1:3]).all()) and bool(torch.isnan(got.logit_scores[1:3]).all())
    assert bool((got.tokens[1:3] == -1).all()) and bool((got.token_frames[1:3] == -1).all()) and bool((got.lengths[1:3] == 0).all())
    for b in (0, 3):                                                       # the healthy samples: bit-equal to a call of their own
        alone = run(K, lp[b:b + 1], {**o, 'il': il[b:b + 1]}, img)
        for a, w in zip(alone, got):
            assert torch.equal(a[0:1].contiguous().view(torch.uint8), w[b:b + 1].contiguous().view(torch.uint8))


def test_refusals_on_the_device_path(K):
    lp = BR.noise_case(21, 1, 8, C32)
    img, _ = trained(31, 3)
    im = img.device_image('cuda')
    sizes = (img.n_states, img.n_entries, img.num_tokens, img.order, img.start_state)
    tail = (BL, 4, 1, -5.0, -10.0, 4, 8, 0.5, 1.5)
    with pytest.raises(RuntimeError, match='GPU'):
        K.ctc_beam_lm(lp, None, im, *sizes, *tail)
    with pytest.raises(RuntimeError, match='image'):
        K.ctc_beam_lm(lp.cuda(), None, img.device_image('cpu'), *sizes, *tail)
    with pytest.raises(TypeError):
        K.ctc_beam_lm(lp.cuda(), None, im.float(), *sizes, *tail)
    with pytest.raises(ValueError, match='image'):
        K.ctc_beam_lm(lp.cuda(), None, im[:-1], *sizes, *tail)
    with pytest.raises(ValueError, match='nbest'):
        K.ctc_beam_lm(lp.cuda(), None, im, *sizes, BL, 4, 5, -5.0, -10.0, 4, 8, 0.5, 1.5)
    with pytest.raises(RuntimeError, match='finite'):
        K.ctc_beam_lm(lp.cuda(), None, im, *sizes, BL, 4, 1, -5.0, -10.0, 4, 8, math.inf, 1.5)


# ---- footprint ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('id', list(LC.CASES))
def test_lm_footprint(K, id):
    FP.run_on_device(LC.build(id, K.load()), K.PROTOTYPES)


# ---- model level ----------------------------------------------------------------------------------------------------------------
class IdTok:
    """Every token is a word: id i is spelt 't<i>'."""
    def __init__(self, V): self.V = V
    def vocab_size(self): return self.V
    def decode(self, ids): return ' '.join(f't{int(i)}' for i in ids)
    def encode(self, text): return [int(w[1:]) for w in text.split()]


CFG = dict(vocab_size=127, n_layers=2, d_model=64, n_heads=2, head_dim=32, subsampling_conv_channels=32, use_rotary=True,
           rotary_base_freq=1500000, decoder_norm=True, self_conditioning=True, bias_in_ff=False, default_norm='layer_norm')


def test_transcribe_with_an_lm_on_the_tiny_model(K):
    """The whole product path on the device: transcribe(lm=...) returns the restatement's best hypothesis of the model's log-probs, and
    decode_beams_lm's ngram_score is the LM's share."""
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
    img, ref = trained(127, 3, seed=4)
    text = R.transcribe(model, wave, tok, 128, 32, beam_width=8, lm=img.to('cuda'), alpha=0.7, beta=0.9)
    logits = R.moving_average_eval(R._Args(), model, A.to_spectogram(wave[None]), 128, 32, tok, use_tqdm=False, return_numpy=False)
    beams, st = LR.search_lm(logits.float().cpu().numpy(), blank, 8, ref, 0.7, 0.9)
    eps = BR.eps_of(logits.shape[0], st['max_score'])
    print(f'[lm gpu] tiny model: gap {st["gap"]:.3e}, eps {eps:.3e}')
    assert st['gap'] >= 4 * eps, 'the seeded model and waveform no longer give a decided search: choose another seed'
    assert text == tok.decode(beams[0][0])
    dec = BeamSearchCTCDecoder(tokenizer=tok, blank_id=blank, beam_width=8, lm=img, alpha=0.7, beta=0.9)
    data, best = decode_beams_lm([logits], dec, beam_width=8, ds_factor=model.subsampling.subsampling_factor)
    assert data[0]['text'] == text and data[0]['am_score'] == best.logit_score and data[0]['score'] == best.lm_score
    want = 0.7 * img.score(best.tokens) + 0.9 * len(best.tokens)
    assert data[0]['ngram_score'] == pytest.approx(want, abs=1e-9) and (len(best.tokens) == 0 or data[0]['ngram_score'] != 0)
