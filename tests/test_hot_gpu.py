"""CTC prefix beam search with hotword boosting on the device (csrc/beam_hot.hip through lcasr_amd.hip.hot) against the restatement of
the contract (tests/hot_refs.py, whose credits are read off the prefix, not an automaton, and whose LM is lm_refs' dict recursion):
count, tokens, lengths and token_frames EXACTLY, scores, logit_scores and hot_scores within eps = 8 T 2^-52 max|score|
(beam_refs.eps_of, the tolerance of test_beam_gpu.py and test_lm_gpu.py; max|score| over keys with and without phi, acoustic totals,
bonuses and credits).  Every case first asserts ON THE CPU that the restatement's smallest decision gap on its input - the final
re-rank included - is at least 4 eps and, from the restatement's counters, that the input reaches what the case is named after; a
case that does not is given another seed here, never skipped.  C = 32 with the blank last unless a case says otherwise.

prepare(name) is the CPU half of a case (input, LM, hotwords, restatement, conditions) and needs no device."""
import math

import numpy as np
import pytest
import torch

import beam_refs as BR
import hot_refs as HR
import lm_refs as LR

pytestmark = pytest.mark.gpu
C32, BL = 32, 31
INF = math.inf
DEFAULT = dict(W=16, nbest=4, thr=-5.0, prune=-10.0, K=16, L=None, il=None, blank=BL, alpha=0.5, beta=1.5, weight=3.0, lm=True)
RANK_LIMIT = 128


@pytest.fixture(scope='module')
def K():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from lcasr_amd.hip import hot
    hot.load()
    return hot


# ---- language models and hotword sets ------------------------------------------------------------------------------------------
_lms, _hots = {}, {}


def trained(V, order, streams=(), seed=0):
    """(image, restatement) of an order-`order` model over V tokens trained on a seeded random stream plus `streams`."""
    key = (V, order, tuple(map(tuple, streams)), seed)
    if key not in _lms:
        rnd = np.random.default_rng(1000 + seed).integers(0, V, 20 * V).tolist()
        _lms[key] = LR.lm_pair(LR.train([rnd] + [list(s) for s in streams], order, V, bos=True), order, V)
    return _lms[key]


def hotwords(V, labels, seed=0, max_len=32):
    """(HotwordSet, BruteHot): the structured set of hot_refs.phrase_set (prefix of another, suffix of another's interior, one token,
    a duplicate, a phrase of max_len tokens, random ones), plus stretches of two to four planted labels (hotwords that do end in the
    search) and such stretches with their last token replaced (hotwords that start to match and break off: phi is revoked)."""
    key = (V, tuple(map(tuple, labels)), seed, max_len)
    if key not in _hots:
        rng = np.random.default_rng(500 + seed)
        phrases, weights = HR.phrase_set(rng, V, max_len)
        for lab in labels:
            for k in range(0, max(len(lab) - 4, 0), 4):
                n = 2 + (k // 4) % 3
                p = tuple(lab[k:k + n])
                if (k // 4) % 2: p = p[:-1] + ((p[-1] + 1 + k) % V,)
                phrases.append(p)
                weights.append(float(1 + k % 7) / 4)
        _hots[key] = HR.hot_pair(phrases, weights)
    return _hots[key]


def sort_sizes(st):
    return {0 if c <= RANK_LIMIT else 1 << (c - 1).bit_length() for c in st['candidates']}


# name -> (builder -> (lp, labels per sample), overrides of DEFAULT with cond(stats, lp, options))
CASES = {}


def _width(W, lm):
    def build():
        return BR.spiky_case(151 + W, 1, 90, C32, BL, every=3, peak=8.0 if W < 100 else 6.0)

    def cond(st, lp, o):
        assert max(st[0]['live']) == W and (W == 1 or st[0]['folds'] > 0) and st[0]['boosted'] > 0
    return build, cond


for _W in (1, 2, 8, 32, 128):
    for _lm in (True, False):
        _b, _c = _width(_W, _lm)
        CASES[f'width-{_W}-{"lm" if _lm else "no-lm"}'] = (_b, dict(W=_W, nbest=min(_W, 4), lm=_lm, cond=_c))


def _cond_cap1(st, lp, o):
    assert st[0]['cap'] > 0 and max(st[0]['kept']) == 1 and 2 in st[0]['candidates']


def _cond_cap16(st, lp, o):
    assert st[0]['cap'] > 0 and max(st[0]['kept']) == 16 and max(st[0]['candidates']) == 8 * 17


CASES['kmax-1-cap'] = (lambda: BR.spiky_case(7, 1, 90, C32, BL, every=3, peak=4.0), dict(K=1, cond=_cond_cap1))
CASES['kmax-1-width-1'] = (lambda: BR.spiky_case(8, 1, 60, C32, BL, every=3, peak=4.0), dict(K=1, W=1, nbest=1, lm=False, cond=_cond_cap1))
CASES['kmax-16-cap-noise-width-8'] = (lambda: (BR.noise_case(8, 1, 40, C32), [[]]), dict(K=16, W=8, cond=_cond_cap16))


def _sorts_input():
    a = BR.noise_case(14, 1, 48, C32)
    b, labels = BR.spiky_case(15, 1, 48, C32, BL, every=3, peak=5.0)
    return torch.cat([a, b]), [[]] + labels


def _cond_sorts(st, lp, o):
    got = sort_sizes(st[0]) | sort_sizes(st[1])
    assert {0, 512, 1024, 2048, 4096} <= got and max(st[0]['candidates']) == 128 * 17


CASES['largest-sort'] = (_sorts_input, dict(W=128, nbest=8, prune=-INF, cond=_cond_sorts))
CASES['largest-sort-no-lm'] = (_sorts_input, dict(W=128, nbest=8, prune=-INF, lm=False, cond=_cond_sorts))


def _cond_mid(st, lp, o):
    assert any(RANK_LIMIT < c <= 256 for c in st[0]['candidates']) and any(c <= RANK_LIMIT for c in st[0]['candidates'])


CASES['both-sides-of-the-rank-limit-width-32'] = (lambda: BR.spiky_case(31, 1, 90, C32, BL, every=3, peak=7.0), dict(W=32, cond=_cond_mid))


def _cond_ragged(st, lp, o):
    assert [len(s['kept']) for s in st] == o['il'] == [90, 1, 0, 83, 90, 17]


CASES['ragged-batch'] = (lambda: BR.spiky_case(16, 6, 90, C32, BL, every=3, in_len=[90, 1, 0, 83, 90, 17]),
                         dict(il=[90, 1, 0, 83, 90, 17], nbest=3, cond=_cond_ragged))
CASES['ragged-batch-no-lm'] = (lambda: BR.spiky_case(16, 6, 90, C32, BL, every=3, in_len=[90, 1, 0, 83, 90, 17]),
                               dict(il=[90, 1, 0, 83, 90, 17], nbest=3, lm=False, cond=_cond_ragged))
CASES['lmax-shorter'] = (lambda: BR.spiky_case(17, 2, 80, C32, BL, every=3), dict(L=5, cond=lambda st, lp, o: None))
CASES['heavy-weight'] = (lambda: BR.spiky_case(18, 1, 90, C32, BL, every=3, peak=5.0), dict(weight=25.0, cond=lambda st, lp, o: None))


def _padded_input():
    g = torch.Generator().manual_seed(18)
    x = torch.randn(2, 70, 129, generator=g)
    x[:, :, 128] += 4.0
    for t in range(0, 70, 3): x[:, t, (7 * t) % 128] += 8.0
    lp = torch.log_softmax(x, -1)
    return torch.nn.functional.pad(lp, (0, 15), value=-INF).contiguous(), [[(7 * t) % 128 for t in range(0, 70, 3)]] * 2


def _cond_padded(st, lp, o):
    assert lp.shape[-1] == 144 and bool(torch.isinf(lp[..., 129:]).all()) and st[0]['folds'] > 0 and st[0]['boosted'] > 0


CASES['padded-classes-129-to-144'] = (_padded_input, dict(blank=128, cond=_cond_padded))
CASES['padded-classes-129-to-144-no-lm'] = (_padded_input, dict(blank=128, lm=False, cond=_cond_padded))

for _s in HR.USEFUL_SEEDS:
    CASES[f'usefulness-seed-{_s}'] = (lambda _s=_s: (HR.usefulness_case(_s)[0], None),
                                      dict(blank=15, nbest=1, lm=False, weight=HR.USEFUL_WEIGHT, cond=lambda st, lp, o: None))

_prepared = {}


def prepare(name):
    """The CPU half: (lp, options, restatement, eps per sample, LM image or None, HotwordSet); asserts the case's conditions and
    gap >= 4 eps."""
    if name not in _prepared:
        build, opt = CASES[name]
        o = {**DEFAULT, **{k: v for k, v in opt.items() if k != 'cond'}}
        lp, labels = build()
        B, N, C = lp.shape
        V = o['blank']
        if o['L'] is None: o['L'] = N
        lm = trained(V, 3, labels or ()) if o['lm'] else (None, None)
        hot = HR.hot_pair([HR.USEFUL_PHRASE]) if labels is None else hotwords(V, labels)
        st = []
        ref = HR.ctc_beam_hot(lp, o['il'], lm[1], hot[1], o['weight'], o['blank'], o['W'], o['nbest'], o['thr'], o['prune'], o['K'], o['L'],
                              o['alpha'], o['beta'], stats=st)
        eps = []
        for b, s in enumerate(st):
            if s is None:
                eps.append(0.0)
                continue
            T = len(s['kept'])
            e = BR.eps_of(T, s['max_score'])
            print(f'[hot] {name} sample {b}: T {T} gap {s["gap"]:.3e} eps {e:.3e} cap {s["cap"]} pruned {s["pruned"]} folds {s["folds"]} '
                  f'max live {max(s["live"], default=1)} boosted {s["boosted"]} revoked {s["revoked"]} reranked {s["reranked"]}')
            assert s['gap'] >= 4 * e, f'{name} sample {b}: the smallest decision gap {s["gap"]:.3e} is below 4 eps = {4 * e:.3e}: choose another seed'
            eps.append(e)
        _prepared[name] = (lp, o, ref, eps, st, lm, hot)
    lp, o, ref, eps, st, lm, hot = _prepared[name]
    CASES[name][1]['cond']([s for s in st], lp, o)
    return lp, o, ref, eps, lm[0], hot[0]


def run(K, lp, o, img, hot, weight=None, hot_image=None):
    il = None if o['il'] is None else torch.tensor(o['il'], dtype=torch.int32).cuda()
    lm_args = (None, 0, 0, 0, 0, 0) if img is None else (img.device_image('cuda'), img.n_states, img.n_entries, img.num_tokens, img.order,
                                                         img.start_state)
    got = K.ctc_beam_hot(lp.cuda(), il, *lm_args, hot.device_image('cuda'), hot.n_states, hot.n_entries, hot.max_len,
                         o['weight'] if weight is None else weight, o['blank'], o['W'], o['nbest'], o['thr'], o['prune'], o['K'], o['L'],
                         o['alpha'], o['beta'])
    torch.cuda.synchronize()
    return got


def compare(name, got, ref, eps):
    g = [t.cpu() for t in got]
    for what, a, b in zip(('count', 'tokens', 'lengths', 'token_frames'), g[:4], ref[:4]):
        bad = (a != b).nonzero()
        assert not bad.numel(), f'{name} {what}: {bad.shape[0]} element(s) differ, first at {bad[0].tolist()}: {a[tuple(bad[0])]} != {b[tuple(bad[0])]}'
    worst = 0.0
    for what, gs, rs in (('scores', g[4], ref.scores), ('logit_scores', g[5], ref.logit_scores), ('hot_scores', g[6], ref.hot_scores)):
        for b in range(rs.shape[0]):
            for r in range(rs.shape[1]):
                x, y = float(gs[b, r]), float(rs[b, r])
                if not math.isfinite(y):
                    assert (math.isnan(x) and math.isnan(y)) or x == y, f'{name} {what}[{b}][{r}]: {x} != {y}'
                else:
                    worst = max(worst, abs(x - y))
                    assert abs(x - y) <= eps[b], f'{name} {what}[{b}][{r}]: {x!r} != {y!r} (|d| {abs(x - y):.3e} > eps {eps[b]:.3e})'
    print(f'[hot gpu] {name}: largest |score - restated| {worst:.3e}, eps {max(eps):.3e}')


def bits(t):
    return t.contiguous().view(torch.uint8)


@pytest.mark.parametrize('name', list(CASES))
def test_boosted_search_against_the_restatement(K, name):
    lp, o, ref, eps, img, hot = prepare(name)
    compare(name, run(K, lp, o, img, hot), ref, eps)


def test_the_cases_reach_every_selection_form_a_revocation_and_a_rerank(K):
    lib, got, cand, revoked, reranked, boosted = K.load(), set(), set(), 0, 0, 0
    for name in CASES:
        prepare(name)
        for s in _prepared[name][4]:
            if s is not None:
                got |= sort_sizes(s)
                cand |= s['candidates']
                revoked += s['revoked'] > 0
                reranked += bool(s['reranked'])
                boosted += s['boosted'] > 0
    from lcasr_amd.hip import beam
    assert beam.load().sconf_beam_rank_limit() == RANK_LIMIT
    assert got == {0, 256, 512, 1024, 2048, 4096}, sorted(got)
    assert 2 in cand and RANK_LIMIT in cand and any(RANK_LIMIT < c <= RANK_LIMIT + 64 for c in cand)      # both sides of the threshold
    assert revoked > 0 and reranked > 0 and boosted > 0, (revoked, reranked, boosted)
    assert {lib.sconf_hot_beam_threads(W, k) for W in (1, 2, 8, 32, 128) for k in (1, 16)} == {64, 128, 512, 1024}


@pytest.mark.parametrize('name', ['width-1-lm', 'width-32-lm', 'width-128-lm', 'ragged-batch', 'padded-classes-129-to-144'])
@pytest.mark.parametrize('how', ['weight-0', 'root-only'])
def test_without_a_boost_the_outputs_are_those_of_the_lm_kernel(K, name, how):
    """weight = 0, or an image that holds only the root: the six outputs of sconf_lm_beam_ctc bit for bit, hot_scores 0."""
    from lcasr_amd.decoding.hotwords import HotwordSet
    from lcasr_amd.hip import lm
    lp, o, ref, eps, img, hot = prepare(name)
    got = run(K, lp, o, img, hot, weight=0.0) if how == 'weight-0' else run(K, lp, o, img, HotwordSet([]))
    il = None if o['il'] is None else torch.tensor(o['il'], dtype=torch.int32).cuda()
    want = lm.ctc_beam_lm(lp.cuda(), il, img.device_image('cuda'), img.n_states, img.n_entries, img.num_tokens, img.order, img.start_state,
                          o['blank'], o['W'], o['nbest'], o['thr'], o['prune'], o['K'], o['L'], o['alpha'], o['beta'])
    torch.cuda.synchronize()
    for what, x, y in zip(want._fields, got[:6], want):
        assert torch.equal(bits(x), bits(y)), what
    assert bool((got.hot_scores[torch.isfinite(got.scores)] == 0).all())


@pytest.mark.parametrize('name', ['width-1-no-lm', 'width-32-no-lm', 'width-128-no-lm', 'ragged-batch-no-lm', 'padded-classes-129-to-144-no-lm'])
@pytest.mark.parametrize('how', ['weight-0', 'root-only'])
def test_without_a_boost_and_an_lm_the_outputs_are_those_of_the_lm_free_kernel(K, name, how):
    """No LM and weight = 0 (or the root alone): the five outputs of sconf_beam_ctc bit for bit, logit_scores equals scores."""
    from lcasr_amd.decoding.hotwords import HotwordSet
    from lcasr_amd.hip import beam
    lp, o, ref, eps, img, hot = prepare(name)
    assert img is None
    got = run(K, lp, o, None, hot, weight=0.0) if how == 'weight-0' else run(K, lp, o, None, HotwordSet([]))
    il = None if o['il'] is None else torch.tensor(o['il'], dtype=torch.int32).cuda()
    want = beam.ctc_beam(lp.cuda(), il, o['blank'], o['W'], o['nbest'], o['thr'], o['prune'], o['K'], o['L'])
    torch.cuda.synchronize()
    for what, x, y in zip(want._fields, got[:5], want):
        assert torch.equal(bits(x), bits(y)), what
    assert torch.equal(bits(got.logit_scores), bits(got.scores))


def test_two_calls_are_bit_equal(K):
    lp, o, ref, eps, img, hot = prepare('width-128-lm')
    a, b = run(K, lp, o, img, hot), run(K, lp, o, img, hot)
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def test_a_poisoned_sample_leaves_its_neighbours_untouched(K):
    N = 60
    lp, labels = BR.spiky_case(19, 4, N, C32, BL, every=3)
    img, ref_lm = trained(31, 3, labels)
    hot, brute = hotwords(31, labels)
    il = [N, N + 1, -1, 41]
    o = {**DEFAULT, 'il': il, 'L': N, 'nbest': 3}
    st = []
    ref = HR.ctc_beam_hot(lp, il, ref_lm, brute, o['weight'], BL, o['W'], o['nbest'], o['thr'], o['prune'], o['K'], N, o['alpha'], o['beta'], stats=st)
    eps = [0.0 if s is None else BR.eps_of(len(s['kept']), s['max_score']) for s in st]
    assert all(s is None or s['gap'] >= 4 * e for s, e in zip(st, eps)) and [s is None for s in st] == [False, True, True, False]
    got = run(K, lp, o, img, hot)
    compare('poisoned', got, ref, eps)
    assert got.count.tolist() == [3, 0, 0, 3]
    assert all(bool(torch.isnan(t[1:3]).all()) for t in (got.scores, got.logit_scores, got.hot_scores))
    assert bool((got.tokens[1:3] == -1).all()) and bool((got.token_frames[1:3] == -1).all()) and bool((got.lengths[1:3] == 0).all())
    for b in (0, 3):                                                       # the healthy samples: bit-equal to a call of their own
        alone = run(K, lp[b:b + 1], {**o, 'il': il[b:b + 1]}, img, hot)
        for a, w in zip(alone, got):
            assert torch.equal(bits(a[0:1]), bits(w[b:b + 1]))


def test_refusals_on_the_device_path(K):
    from lcasr_amd.decoding.beam import ctc_beam_search_hot
    lp = BR.noise_case(21, 1, 8, C32)
    img, _ = trained(31, 3)
    hot, _ = hotwords(31, [[1, 2, 3, 4, 5, 6, 7, 8, 9]])
    im, hi = img.device_image('cuda'), hot.device_image('cuda')
    lm_sizes = (img.n_states, img.n_entries, img.num_tokens, img.order, img.start_state)
    hs = (hot.n_states, hot.n_entries, hot.max_len)
    tail = (BL, 4, 1, -5.0, -10.0, 4, 8, 0.5, 1.5)
    with pytest.raises(RuntimeError, match='GPU'):
        K.ctc_beam_hot(lp, None, im, *lm_sizes, hi, *hs, 3.0, *tail)
    with pytest.raises(RuntimeError, match='hotword image'):
        K.ctc_beam_hot(lp.cuda(), None, im, *lm_sizes, hot.device_image('cpu'), *hs, 3.0, *tail)
    with pytest.raises(RuntimeError, match='LM image'):
        K.ctc_beam_hot(lp.cuda(), None, img.device_image('cpu'), *lm_sizes, hi, *hs, 3.0, *tail)
    with pytest.raises(TypeError):
        K.ctc_beam_hot(lp.cuda(), None, im, *lm_sizes, hi.float(), *hs, 3.0, *tail)
    with pytest.raises(ValueError, match='image'):
        K.ctc_beam_hot(lp.cuda(), None, im, *lm_sizes, hi[:-1], *hs, 3.0, *tail)
    with pytest.raises(ValueError, match='no LM image'):
        K.ctc_beam_hot(lp.cuda(), None, None, *lm_sizes, hi, *hs, 3.0, *tail)
    with pytest.raises(ValueError, match='nbest'):
        K.ctc_beam_hot(lp.cuda(), None, im, *lm_sizes, hi, *hs, 3.0, BL, 4, 5, -5.0, -10.0, 4, 8, 0.5, 1.5)
    with pytest.raises(RuntimeError, match='weight'):
        K.ctc_beam_hot(lp.cuda(), None, im, *lm_sizes, hi, *hs, -1.0, *tail)
    with pytest.raises(RuntimeError, match='hot_max_len'):
        K.ctc_beam_hot(lp.cuda(), None, im, *lm_sizes, hi, hot.n_states, hot.n_entries, 33, 3.0, *tail)
    with pytest.raises(ValueError, match='blank'):
        ctc_beam_search_hot(lp.cuda(), hot, blank=int(hot.entries[0, 0]))
    with pytest.raises(ValueError, match='hotword_weight'):
        ctc_beam_search_hot(lp.cuda(), hot, -2.0, blank=BL)


def test_the_hotword_is_found_on_the_device(K):
    """The usefulness case: the device's plain search misses every plant of the phrase, the boosted one returns them all, and the
    edit distance to the intended sequence at least halves - with the counts of the restatement."""
    from lcasr_amd.hip import beam
    contains = lambda seq: sum(tuple(seq[k:k + 3]) == HR.USEFUL_PHRASE for k in range(len(seq)))
    free = boosted = found_free = found = want_free = want_boosted = 0
    for seed in HR.USEFUL_SEEDS:
        lp, o, ref, eps, img, hot = prepare(f'usefulness-seed-{seed}')
        labels = HR.usefulness_case(seed)[1]
        st = BR.search(lp[0].numpy(), 15, 16)
        assert st[1]['gap'] >= 4 * BR.eps_of(96, st[1]['max_score'])
        want_free += LR.edit_distance(list(st[0][0][0]), labels)
        want_boosted += LR.edit_distance(ref.tokens[0, 0, :int(ref.lengths[0, 0])].tolist(), labels)
        a = beam.ctc_beam(lp.cuda(), None, 15, 16, 1, -5.0, -10.0, 16, 96)
        b = run(K, lp, o, None, hot)
        ta, tb = a.tokens[0, 0, :int(a.lengths[0, 0])].tolist(), b.tokens[0, 0, :int(b.lengths[0, 0])].tolist()
        free += LR.edit_distance(ta, labels)
        boosted += LR.edit_distance(tb, labels)
        found_free += contains(ta)
        found += contains(tb)
        assert float(b.hot_scores[0, 0]) == HR.USEFUL_WEIGHT * contains(tb)
    print(f'[hot gpu] token errors of 128: plain {free}, boosted {boosted}; the phrase found {found_free} / {found} times of 16')
    assert (free, boosted) == (want_free, want_boosted) and found_free == 0 and found == 16 and free >= 40 and 2 * boosted <= free


# ---- model level ----------------------------------------------------------------------------------------------------------------
class IdTok:
    """Every token is a word: id i is spelt 't<i>'."""
    def __init__(self, V): self.V = V
    def vocab_size(self): return self.V
    def decode(self, ids): return ' '.join(f't{int(i)}' for i in ids)
    def encode(self, text): return [int(w[1:]) for w in text.split()]


CFG = dict(vocab_size=127, n_layers=2, d_model=64, n_heads=2, head_dim=32, subsampling_conv_channels=32, use_rotary=True,
           rotary_base_freq=1500000, decoder_norm=True, self_conditioning=True, bias_in_ff=False, default_norm='layer_norm')


def deciding_hotword(lp, blank, W, free):
    """The hotword of the model-level test: the first stretch of a runner-up of the plain search `free` (ranks 1, 2, ..; three, two
    or one token) that the best hypothesis does not hold and that, weighted by twice that runner-up's distance from the top plus
    one, changes the restated search's best hypothesis with every decision at least 4 eps wide.  Returns (phrase, weight, restated
    beams, statistics, eps)."""
    top = free[0][0]
    has = lambda seq, p: any(tuple(seq[k:k + len(p)]) == tuple(p) for k in range(len(seq)))
    for rank in range(1, len(free)):
        other = free[rank][0]
        for n in (3, 2, 1):
            for k in range(len(other) - n + 1):
                p = other[k:k + n]
                if has(top, p): continue
                weight = 2.0 * (free[0][2] - free[rank][2]) + 1.0
                beams, st = HR.search_hot(lp, blank, W, HR.BruteHot([p]), weight)
                eps = BR.eps_of(lp.shape[0], st['max_score'])
                if beams[0][0] != top and has(beams[0][0], p) and st['gap'] >= 4 * eps:
                    return p, weight, beams, st, eps
    raise AssertionError('no runner-up of the seeded model and waveform holds a stretch that decides the boosted search: choose another seed')


def test_transcribe_with_hotwords_on_the_tiny_model(K):
    """The whole product path on the device: the hotword is a stretch of the restatement's own runner-up that the best hypothesis
    does not hold, heavy enough to win: transcribe(hotwords=[...]) returns what the restatement of the boosted search returns, which
    is not the plain transcript, and decode_beams reports the credit in lm_score."""
    import audio_refs as AUD
    from lcasr_amd.decoding.beam import BeamSearchCTCDecoder
    from lcasr_amd.eval import run as R
    from lcasr_amd.models.sconformer_xl import SCConformerXL
    from lcasr_amd.utils import audio_tools as A
    torch.manual_seed(12345)
    model = SCConformerXL(**CFG).cuda().eval()
    wave = AUD.test_signal(3 * 16000, seed=9).cuda()
    tok, blank = IdTok(127), model.decoder.num_classes - 1
    logits = R.moving_average_eval(R._Args(), model, A.to_spectogram(wave[None]), 128, 32, tok, use_tqdm=False, return_numpy=False)
    lp = logits.float().cpu().numpy()
    free, st0 = BR.search(lp, blank, 8)
    assert len(free) > 1 and st0['gap'] >= 4 * BR.eps_of(lp.shape[0], st0['max_score']), 'choose another seed'
    top = free[0][0]
    phrase, weight, beams, st, eps = deciding_hotword(lp, blank, 8, free)
    words = [tok.decode(phrase)]
    print(f'[hot gpu] tiny model: phrase {phrase} weight {weight:.3f} gap {st["gap"]:.3e} eps {eps:.3e}')
    text = R.transcribe(model, wave, tok, 128, 32, beam_width=8, hotwords=words, hotword_weight=weight)
    assert text == tok.decode(beams[0][0]) != R.transcribe(model, wave, tok, 128, 32, beam_width=8) == tok.decode(top)
    dec = BeamSearchCTCDecoder(tokenizer=tok, blank_id=blank, beam_width=8)
    best = dec.decode_beams(logits, hotwords=words, hotword_weight=weight)[0]
    assert best.tokens == list(beams[0][0]) and best.lm_score - best.logit_score == pytest.approx(beams[0][4], abs=1e-9) and beams[0][4] >= weight
