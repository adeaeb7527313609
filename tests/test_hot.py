"""CPU tests of hotword boosting: the Aho-Corasick image of lcasr_amd.decoding.hotwords.HotwordSet against the automaton-free credits
of tests/hot_refs.py (BruteHot), its refusals and save / load, the restatement of the boosted search (hot_refs.search_hot) against the
enumeration of every frame path, against lm_refs.search_lm / beam_refs.search at weight 0 and on hand cases, the usefulness case,
the eleventh ABI unit's header / binding / queries / refusals, and BeamSearchCTCDecoder(hotwords=...) / decode_beams(hotwords=...) /
transcribe(hotwords=...) on the tiny fixture model with the op replaced by the restatement.  The HIP kernels themselves are tested in
test_hot_gpu.py."""
import ctypes
import math
import os
import types

import numpy as np
import pytest
import torch

import audio_refs as AR
import beam_refs as BR
import eval_refs as E
import hot_refs as HR
import lm_refs as LR
from cabi_header import assert_binding_is_header, header_abi
from common_model import build_from_fixture
from conftest import ROOT, load_golden

INF = math.inf


def HS():
    from lcasr_amd.decoding.hotwords import HotwordSet
    return HotwordSet


def MAX_LEN():
    from lcasr_amd.hip import hot
    return hot.MAX_LEN


# ---- 1. the image against the definition --------------------------------------------------------------------------------------
@pytest.mark.parametrize('V', [4, 5, 6])
def test_image_equals_the_brute_force_on_every_sequence(V):
    """Random phrase sets over V tokens with a phrase that is a prefix of another, one that is a suffix of another's interior, a
    one-token phrase, a duplicate and a phrase of max_len tokens: for every token sequence up to length 6 (7 at V = 4), and on long
    random walks that run through the longest phrase, each step of the image gives the emit and phi that the brute force reads off
    the prefix, and score() the summed credit of every occurrence."""
    rng = np.random.default_rng(40 + V)
    depth = 7 if V == 4 else 6
    for _ in range(2):
        phrases, weights = HR.phrase_set(rng, V, MAX_LEN())
        img, ref = HR.hot_pair(phrases, weights)
        assert img.max_len == MAX_LEN() == max(len(p) for p in phrases) and img.n_entries == img.n_states - 1
        assert len(img.phrases) == len(set(phrases)) < len(phrases)           # the duplicate was merged ...
        dup = phrases[0]
        assert phrases.count(dup) >= 2                                     # ... with the summed weight
        assert img.weights[img.phrases.index(dup)] == sum(w for p, w in zip(phrases, weights) if p == dup) >= weights[0] + weights[5]
        assert img.paths[0] == () and any(p[:2] == dup and len(p) == 3 for p in phrases) and any(len(p) == 1 for p in phrases)
        stack, seen = [((), 0, 0.0)], 0
        while stack:
            seq, s, total = stack.pop()
            if seq:
                seen += 1
                assert img.paths[s] == next(seq[k:] for k in range(len(seq) + 1) if seq[k:] in set(img.paths))   # the longest suffix that is a node
            if len(seq) == depth: continue
            for c in range(V):
                s2, e, p = img.step(s, c)
                assert e == ref.emit(seq + (c,)) and p == ref.phi(seq + (c,)), (seq, c, e, p)
                stack.append((seq + (c,), s2, total + e))
        assert seen == sum(V ** n for n in range(1, depth + 1))
        longest = max(phrases, key=len)
        for walk in (list(longest), list(rng.integers(0, V, 40)) + list(longest) + list(rng.integers(0, V, 40)),
                     list(longest[:-1]) + [int((longest[-1] + 1) % V)] + list(longest)):
            perm, phi = img.score(walk)
            assert perm == ref.permanent(tuple(walk)) and phi == ref.phi(tuple(walk))
            assert perm >= ref.table[longest]
        assert img.step(3, V + 7) == (0, 0.0, 0.0)                             # a class no phrase holds falls to the root


def test_the_credits_by_hand():
    """"a b" (1), "a b c" (2), "b c" (0.5), "c" (0.25), over a = 0, b = 1, c = 2."""
    img, ref = HR.hot_pair([(0, 1), (0, 1, 2), (1, 2), (2,)], [1.0, 2.0, 0.5, 0.25])
    s, e, p = img.step(0, 0)
    assert (e, p) == (0.0, HR.f32(2.0 / 3))                                # inside "a b c": a third of 2 beats half of 1
    s, e, p = img.step(s, 1)
    assert (e, p) == (1.0, HR.f32(4.0 / 3))                                # "a b" ends; two thirds of "a b c" beats half of "b c"
    s, e, p = img.step(s, 2)
    assert (e, p) == (2.0 + 0.5 + 0.25, 0.0)                               # "a b c", "b c" and "c" all end here
    assert img.score([0, 1, 2]) == (3.75, 0.0) and img.score([0, 1]) == (1.0, HR.f32(4.0 / 3)) and img.score([1]) == (0.0, 0.25)
    assert img.score([0, 0, 1, 1, 2]) == (1.0 + 0.75, 0.0) and ref.permanent((0, 0, 1, 1, 2)) == 1.75


class Tok:
    """A sentencepiece-like stub: a word is spelt by its '▁' piece and letters."""
    PIECES = ['▁', 'a', 'b', 'c', '▁ab', '▁c']

    def encode(self, text):
        out = []
        for w in text.split():
            w = '▁' + w
            while w:
                k = max((p for p in self.PIECES if w.startswith(p)), key=len)
                out.append(self.PIECES.index(k))
                w = w[len(k):]
        return out

    def id_to_piece(self, i): return self.PIECES[i]
    def decode(self, ids): return ''.join(self.PIECES[i] for i in ids).replace('▁', ' ').strip()


def test_from_text_encodes_with_the_tokenizer():
    hs = HS().from_text(['abc', 'cab', 'abc'], Tok(), [1.0, 2.0, 0.5])
    assert hs.phrases == [(4, 3), (5, 1, 2)] and hs.weights == [1.5, 2.0]   # a word starts with its '▁' piece
    with pytest.raises(ValueError, match='no token'):
        HS().from_text(['abc', ' '], Tok())
    with pytest.raises(TypeError):
        HS().from_text('abc', Tok())


def test_refusals_of_the_set(tmp_path):
    with pytest.raises(ValueError, match='empty phrase'):
        HS()([(1, 2), ()])
    with pytest.raises(ValueError, match='at most'):
        HS()([tuple(range(MAX_LEN() + 1))])
    for w in (0.0, -1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match='weight'):
            HS()([(1, 2)], [w])
    with pytest.raises(ValueError, match='weights'):
        HS()([(1, 2)], [1.0, 2.0])
    with pytest.raises(ValueError, match='negative'):
        HS()([(1, -2)])
    hs = HS()([(1, 2), (3,)])
    hs.validate(blank=0, num_classes=4)
    with pytest.raises(ValueError, match='blank'):
        hs.validate(blank=2, num_classes=4)
    with pytest.raises(ValueError, match='classes'):
        hs.validate(blank=0, num_classes=3)
    S = hs.n_states
    damage = {'children outside the entries': (1, 9), 'a failure state out of range': (4 * 1 + 2, S), 'a next state out of range': (6 * S + 1, -1),
              'a failure cycle': (4 * 2 + 2, 2), 'a non-finite credit': (4 * S + 2, int(np.array([np.inf], dtype=np.float32).view(np.int32)[0])),
              'a negative credit': (4 * S + 3, int(np.array([-1.0], dtype=np.float32).view(np.int32)[0])),
              'unsorted children': (6 * S, 7)}
    for what, (at, v) in damage.items():
        im = hs.image.copy()
        im[at] = v
        with pytest.raises(ValueError, match='hotword image'):
            HS().from_image(im, S, hs.n_entries, hs.max_len)
        print(f'[hot] validate refuses {what}')
    with pytest.raises(ValueError, match='hotword image'):
        HS().from_image(hs.image[:-1], S, hs.n_entries, hs.max_len)
    with pytest.raises(ValueError, match='hotword image'):
        HS().from_image(hs.image, S, hs.n_entries, MAX_LEN() + 1)
    with pytest.raises(ValueError, match='hotword image'):
        HS().from_image(hs.image, S, hs.n_entries, 0)                      # failure arcs under a bound of none


def test_save_and_load_round_trip_bit_equal(tmp_path):
    phrases, weights = HR.phrase_set(np.random.default_rng(3), 6, 9)
    hs = HS()(phrases, weights)
    p = str(tmp_path / 'hot.npz')
    hs.save(p)
    back = HS().load(p)
    assert back.image.dtype == np.int32 and back.image.tobytes() == hs.image.tobytes() and back.phrases is None
    assert (back.n_states, back.n_entries, back.max_len) == (hs.n_states, hs.n_entries, 9)
    assert back.score([0, 1, 2, 3, 4, 5] * 3) == hs.score([0, 1, 2, 3, 4, 5] * 3)
    assert hs.to('cpu') is hs and hs.device_image('cpu').dtype == torch.int32 and hs.device_image('cpu') is hs.device_image('cpu')
    root = HS()([])
    assert (root.n_states, root.n_entries, root.max_len, root.image.size) == (1, 0, 0, 6) and root.step(0, 3) == (0, 0.0, 0.0)


# ---- 2. the restatement of the boosted search -------------------------------------------------------------------------------------
def _lm7():
    return LR.lm_pair(LR.train([[0, 1, 2, 3, 4, 5, 6] * 5], 3, 7), 3, 7)[1]


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_search_hot_at_weight_zero_is_search_lm_and_the_lm_free_search(seed):
    ref = _lm7()
    hot = HR.BruteHot([(0, 1), (2,), (3, 4, 5)])
    lp = BR.noise_case(seed, 1, 40, 8)[0].numpy()
    for h, w in ((hot, 0.0), (HR.BruteHot([]), 10.0)):                      # weight 0, and a set with the root alone
        want, st0 = LR.search_lm(lp, 7, 8, ref, 0.5, 1.5)
        got, st1 = HR.search_hot(lp, 7, 8, h, w, ref, 0.5, 1.5)
        assert [b[:4] for b in got] == want and all(b[4] == 0.0 for b in got)
        for k in ('gap', 'cap', 'pruned', 'folds', 'recreated', 'kept', 'live', 'max_score', 'candidates', 'depth', 'unk', 'lookups'):
            assert st0[k] == st1[k], k
        assert st1['revoked'] == 0 and not st1['reranked'] and st1['boosted'] == 0
        free, st2 = BR.search(lp, 7, 8)
        got, st3 = HR.search_hot(lp, 7, 8, h, w, None, 0.5, 1.5)               # no LM: alpha and beta do nothing
        assert [b[:3] for b in got] == free and all(b[2] == b[3] and b[4] == 0.0 for b in got)
        for k in ('gap', 'cap', 'pruned', 'folds', 'recreated', 'kept', 'live', 'max_score', 'candidates'):
            assert st2[k] == st3[k], k


def _lp(probs):
    with np.errstate(divide='ignore'):
        return np.log(np.asarray(probs, dtype=np.float64)).astype(np.float32)


def test_a_hotword_turns_b_into_a_and_a_fold_keeps_one_credit():
    """Classes: 0 = a, 1 = b, 2 = blank; P(a) = 0.45, P(b) = 0.55 in one frame.  Then two frames of a alone: the fold of the empty
    prefix's extension into the live beam "a" adds mass, not a second credit."""
    hot = HR.BruteHot([(0,)])
    lp = _lp([[0.45, 0.55, 0.0]])
    assert BR.search(lp, 2, 4)[0][0][0] == (1,)
    beams, st = HR.search_hot(lp, 2, 4, hot, 1.0)
    assert [b[0] for b in beams] == [(0,), (1,)] and st['boosted'] == 1
    assert beams[0][2] == beams[0][3] + 1.0 and beams[0][4] == 1.0 and beams[1][2] == beams[1][3] and beams[1][4] == 0.0
    beams, st = HR.search_hot(_lp([[0.6, 0.4]] * 2), 1, 4, hot, 2.5)
    got = {b[0]: b for b in beams}
    assert st['folds'] >= 1 and got[(0,)][3] == pytest.approx(math.log(0.84), abs=1e-7) and got[(0,)][2] - got[(0,)][3] == 2.5
    got = {b[0]: b for b in HR.search_hot(_lp([[0.6, 0.4]] * 3), 1, 4, hot, 2.5)[0]}
    assert got[(0, 0)][4] == 5.0 and got[(0,)][4] == 2.5 and got[()][4] == 0.0                    # a a: the hotword twice


def test_partial_credit_is_held_while_matching_revoked_after_and_dropped_at_the_end():
    """Classes 0 = a, 1 = b, 2 = c, 3 = blank; the hotword is "a b c", weight 3.  At W = 1: frame 0 offers a (0.4) or c (0.5): the third
    of the credit that "a" holds (1.0) beats ln(0.5 / 0.4).  The recording ends there: the final score of "a" has no credit, and
    with W = 2 the re-rank puts "c" first again.  Going on with b then a: the credit grows to 2, then falls to 1 ("a b a" is inside
    the hotword again, one token deep) - a revocation - and nothing permanent was ever added."""
    hot = HR.BruteHot([(0, 1, 2)])
    f0 = [0.4, 0.0, 0.5, 0.1]
    assert BR.search(_lp([f0]), 3, 1)[0][0][0] == (2,)
    one, st = HR.search_hot(_lp([f0]), 3, 1, hot, 3.0)
    assert one[0][0] == (0,) and one[0][2] == one[0][3] == pytest.approx(math.log(0.4), abs=1e-7) and one[0][4] == 0.0
    two, st = HR.search_hot(_lp([f0]), 3, 2, hot, 3.0)
    assert [b[0] for b in two] == [(2,), (0,)] and st['reranked']          # phi ranked "a" first during the search; the end drops it
    lp = _lp([f0, [0.0, 0.9, 0.0, 0.1], [0.9, 0.0, 0.0, 0.1]])
    beams, st = HR.search_hot(lp, 3, 1, hot, 3.0, beam_prune_logp=-INF)
    assert beams[0][0] == (0, 1, 0) and beams[0][4] == 0.0 and beams[0][2] == beams[0][3] and st['revoked'] == 1 and st['boosted'] == 0
    done, st = HR.search_hot(_lp([f0, [0.0, 0.9, 0.0, 0.1], [0.0, 0.0, 0.9, 0.1]]), 3, 1, hot, 3.0)
    assert done[0][0] == (0, 1, 2) and done[0][4] == 3.0 and done[0][2] == done[0][3] + 3.0 and st['boosted'] == 1


@pytest.mark.parametrize('with_lm', [False, True])
def test_restatement_against_the_enumeration_of_every_frame_path(with_lm):
    """Token pruning off, W above the number of prefixes, T <= 6, C <= 4: every label sequence is a hypothesis, its logit score the
    log-sum of all its alignments, its hot score weight times the summed weights of every phrase occurrence in it, and its score
    the sum of both plus alpha ln P_LM(tokens) + beta per token; the ranking is by that score."""
    rng = np.random.default_rng(2027)
    worst, sets = 0.0, 0
    for C in (2, 3, 4):
        V = C - 1
        img = ref = None
        if with_lm:
            table, unk = LR.random_table(rng, V, min(3, C), True)
            img, ref = LR.lm_pair(table, max(len(g) for g in table), V, unk)
        phrases = [(0,), (0, 0)] if V == 1 else [(0, 1), (0, 1, 0), (1,), (1, 0, 1, 0)] + ([(2, 0), (1, 2)] if V == 3 else [])
        weights = [0.5 + 0.25 * k for k in range(len(phrases))]
        hot = HR.BruteHot(phrases, weights)
        for T in range(1, 7 if C < 4 else 6):
            for weight, alpha, beta in ((10.0, 0.5, 1.5), (0.75, 1.3, -0.4)):
                x = rng.normal(size=(T, C)) * 2
                lp = (x - np.log(np.exp(x).sum(-1, keepdims=True))).astype(np.float32)
                beams, st = HR.search_hot(lp, C - 1, 2000, hot, weight, ref, alpha, beta, -INF, -INF, 16)
                want = BR.enumerate_paths(lp, C - 1)
                assert {b[0] for b in beams} == set(want) and len(beams) == len(want)
                assert [b[2] for b in beams] == sorted((b[2] for b in beams), reverse=True)
                for pre, frames, keyv, a, h in beams:
                    lm_part = alpha * img.score(pre) + beta * len(pre) if with_lm else 0.0
                    worst = max(worst, abs(a - want[pre]), abs(h - weight * hot.permanent(pre)), abs(keyv - (want[pre] + lm_part + weight * hot.permanent(pre))))
                sets += 1
    print(f'[hot] {sets} emission sets, largest |score - (log-sum of the alignments + LM part + weight permanent)| = {worst:.2e}')
    assert worst <= 1e-11


def test_the_hotword_is_found_in_the_ambiguous_input():
    """The usefulness case on the restatement: four seeds, 128 tokens, 16 plants of the phrase."""
    hot = HR.BruteHot([HR.USEFUL_PHRASE])
    free = boosted = found_free = found = 0
    contains = lambda seq: sum(tuple(seq[k:k + 3]) == HR.USEFUL_PHRASE for k in range(len(seq)))
    for seed in HR.USEFUL_SEEDS:
        lp, labels = HR.usefulness_case(seed)
        assert len(labels) == 32 and contains(labels) == 4
        a = list(BR.search(lp[0].numpy(), 15, 16)[0][0][0])
        beams, st = HR.search_hot(lp[0].numpy(), 15, 16, hot, HR.USEFUL_WEIGHT)
        b = list(beams[0][0])
        free += LR.edit_distance(a, labels)
        boosted += LR.edit_distance(b, labels)
        found_free += contains(a)
        found += contains(b)
        assert beams[0][4] == HR.USEFUL_WEIGHT * contains(b)
    print(f'[hot] token errors of 128: plain {free}, boosted {boosted}; the phrase found {found_free} / {found} times of 16')
    assert found_free == 0 and found == 16 and free >= 40 and 2 * boosted <= free


# ---- 3. the eleventh ABI unit -------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from lcasr_amd.hip import hot
    return hot.load()


def test_header_binding_and_exports_agree(lib):
    from lcasr_amd.hip import _lib, hot
    funcs, enums = header_abi('sconf_hot.h', 'sconf_hot_')
    assert not enums and set(funcs) == {'sconf_hot_max_len', 'sconf_hot_max_width', 'sconf_hot_max_tokens', 'sconf_hot_beam_threads',
                                        'sconf_hot_beam_workspace', 'sconf_hot_beam_ctc'}
    assert_binding_is_header(funcs, hot.PROTOTYPES, hot.PLAIN, 'hip/hot.py')
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(raw, n) for n in funcs)
    for n, (args, res) in {**{k: (v, ctypes.c_int) for k, v in hot.PROTOTYPES.items()}, **hot.PLAIN}.items():
        assert _lib.bound()[n] == (args, res)
    assert not any(n.startswith('sconf_hot_') for n in list(_lib.PROTOTYPES) + list(_lib.PLAIN))
    for f in ('include/sconf.h', 'include/sconf_beam.h', 'include/sconf_lm.h', 'long-context-asr_amd/hip/_lib.py', 'long-context-asr_amd/hip/beam.py',
              'long-context-asr_amd/hip/lm.py', 'long-context-asr_amd/hip/__init__.py', 'long-context-asr_amd/decoding/lm.py'):
        assert 'sconf_hot_' not in open(os.path.join(ROOT, f)).read() and 'import hot' not in open(os.path.join(ROOT, f)).read(), f


def test_hot_queries(lib):
    from lcasr_amd.hip import beam, hot
    assert lib.sconf_hot_max_len() == 32 == hot.MAX_LEN == hot.max_len()
    blib = beam.load()
    assert lib.sconf_hot_max_width() == blib.sconf_beam_max_width() == 128 and lib.sconf_hot_max_tokens() == blib.sconf_beam_max_tokens() == 16
    for W, K in ((1, 1), (8, 16), (16, 16), (32, 16), (100, 16), (128, 16), (0, 1), (129, 1), (1, 17)):
        assert lib.sconf_hot_beam_threads(W, K) == blib.sconf_beam_threads(W, K)
    ws = lib.sconf_hot_beam_workspace
    assert ws(1, 16384, 100, 16) == 28446208 == hot.beam_workspace(1, 16384, 100, 16)               # the figure in the header
    r256 = lambda n: (n + 255) // 256 * 256
    for B, N, W, K in ((1, 1, 1, 1), (2, 100, 7, 3), (3, 2048, 64, 16), (16, 2048, 100, 16)):
        assert ws(B, N, W, K) == r256(B * N * (8 + 8 * K)) + r256(16 * B * N * W) + r256(32 * B * W) + r256(4 * B)
    assert ws(0, 10, 4, 4) == -1 and ws(1, 0, 4, 4) == -1 and ws(1, 10, 129, 4) == -1 and ws(1, 10, 4, 17) == -1 and ws(1 << 20, 1 << 20, 4, 4) == -1
    with pytest.raises(ValueError, match='beam_width'):
        hot.beam_workspace(1, 10, 129, 4)


def test_hot_refusals_launch_nothing(lib):
    one = ctypes.c_void_p(16)                                              # never dereferenced: every call below is refused on the host
    need = lib.sconf_hot_beam_workspace(1, 10, 8, 4)

    def call(lp=one, image=one, S=3, E=2, V=12, order=3, start=0, himage=one, HS=4, HE=3, hlen=3, weight=10.0, ws=need, B=1, N=10, C=32,
             blank=31, W=8, nbest=2, prune=-10.0, K=4, L=10, alpha=0.5, beta=1.5):
        return lib.sconf_hot_beam_ctc(lp, None, image, S, E, V, order, start, himage, HS, HE, hlen, weight, one, one, one, one, one, one, one,
                                      one, ws, B, N, C, blank, W, nbest, -5.0, prune, K, L, alpha, beta, None)

    for kw, word in ((dict(blank=32), b'blank'), (dict(ws=need - 1), b'workspace'), (dict(W=0), b'beam_width'), (dict(W=129, ws=1 << 40), b'128'),
                     (dict(nbest=9), b'nbest'), (dict(K=0), b'max_tokens_per_frame'), (dict(prune=0.5), b'beam_prune_logp'),
                     (dict(prune=math.nan), b'beam_prune_logp'), (dict(C=30), b'multiple of 4'), (dict(N=0), b'sizes'), (dict(L=0), b'sizes'),
                     (dict(lp=None), b'null'), (dict(image=None), b'null'), (dict(order=0), b'order'), (dict(order=6), b'order'),
                     (dict(V=0), b'num_tokens'), (dict(V=33), b'num_tokens'), (dict(E=-1), b'image sizes'),
                     (dict(S=1 << 30, E=1 << 30), b'image sizes'), (dict(start=3), b'start_state'), (dict(start=-1), b'start_state'),
                     (dict(alpha=math.inf), b'finite'), (dict(beta=math.nan), b'finite'), (dict(image=ctypes.c_void_p(24)), b'aligned'),
                     (dict(image=None, S=0, E=1, V=0), b'image sizes'), (dict(image=None, S=0, E=0, V=3), b'image sizes'),
                     (dict(himage=None), b'null'), (dict(himage=ctypes.c_void_p(24)), b'aligned'), (dict(HS=0), b'hotword image sizes'),
                     (dict(HE=-1), b'hotword image sizes'), (dict(HS=1 << 30, HE=0), b'hotword image sizes'), (dict(hlen=-1), b'hot_max_len'),
                     (dict(hlen=33), b'hot_max_len'), (dict(weight=-1.0), b'weight'), (dict(weight=math.inf), b'weight'),
                     (dict(weight=math.nan), b'weight')):
        assert call(**kw) != 0 and word in lib.sconf_last_error(), (kw, lib.sconf_last_error())
    assert call(B=0) == 0                                                  # nothing to do, nothing launched


def test_a_cpu_tensor_is_refused_by_the_product_path():
    from lcasr_amd.decoding.beam import ctc_beam_search_hot
    hs = HS()([(0, 1), (2,)])
    lp = BR.noise_case(1, 1, 8, 8)
    with pytest.raises(RuntimeError, match='GPU'):
        ctc_beam_search_hot(lp[0], hs, blank=7)
    with pytest.raises(ValueError, match='HotwordSet'):
        ctc_beam_search_hot(lp[0], None, blank=7)
    with pytest.raises(ValueError, match='blank'):
        ctc_beam_search_hot(lp[0], hs, blank=2)
    with pytest.raises(ValueError, match='classes'):
        ctc_beam_search_hot(lp[0, :, :2], HS()([(2,)]), blank=0)
    for w in (-1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match='hotword_weight'):
            ctc_beam_search_hot(lp[0], hs, w, blank=7)


# ---- 4. the Python layers on the restatement ------------------------------------------------------------------------------------
@pytest.fixture
def emulated_hot(monkeypatch):
    """lcasr_amd.hip.hot.ctc_beam_hot replaced by the restatement: the hotword image is read back into its phrases (every state's
    own weight is emit(s) - emit(fail(s))), `use(ref)` names the DictLM that stands for an LM image.  The LM-free and the LM ops are
    replaced too, and count their calls."""
    from lcasr_amd.decoding import beam as D
    from lcasr_amd.hip import hot as hot_kernels
    from lcasr_amd.hip import lm as lm_kernels
    box, calls, other = {'ref': None}, [], []

    def phrases_of(image, S, E):
        st, cr, en = image[:4 * S].reshape(-1, 4), image[4 * S:6 * S].reshape(-1, 2).contiguous().view(torch.float32), image[6 * S:].reshape(-1, 2)
        path = {0: ()}
        for s in range(S):                                                 # states are in order of depth: a parent comes first
            for e in range(int(st[s, 0]), int(st[s, 0]) + int(st[s, 1])):
                path[int(en[e, 1])] = path[s] + (int(en[e, 0]),)
        own = {path[s]: float(cr[s, 0]) - float(cr[int(st[s, 2]), 0]) for s in range(1, S)}
        return [p for p, w in own.items() if w > 0], [w for w in own.values() if w > 0]

    def op(lp, il, lm_image, S, E, V, order, start, hot_image, HS_, HE, hlen, weight, *rest):
        assert hot_image.dtype == torch.int32 and hot_image.numel() == 6 * HS_ + 2 * HE
        assert (lm_image is None) == (box['ref'] is None) and (lm_image is not None or (S, E, V, order, start) == (0, 0, 0, 0, 0))
        ph, w = phrases_of(hot_image, HS_, HE)
        assert hlen == max((len(p) for p in ph), default=0)
        calls.append((tuple(ph), weight) + rest)
        return HR.ctc_beam_hot(lp, il, box['ref'], HR.BruteHot(ph, w), weight, *rest)

    def lm_op(lp, il, image, S, E, V, order, start, *rest):
        other.append('lm')
        return LR.ctc_beam_lm(lp, il, box['ref'], *rest)

    def free_op(*a):
        other.append('free')
        return BR.ctc_beam(*a)

    monkeypatch.setattr(hot_kernels, 'ctc_beam_hot', op)
    monkeypatch.setattr(lm_kernels, 'ctc_beam_lm', lm_op)
    monkeypatch.setattr(D.beam_kernels, 'ctc_beam', free_op)
    return types.SimpleNamespace(D=D, use=lambda ref: box.__setitem__('ref', ref), calls=calls, other=other)


def _cat_emission():
    """20 frames over the 7 pieces of PieceTok + blank: 'on the cats sat' with frame 1 ambiguous between 'on' (5, 0.4) and 'sat' (4, 0.5)."""
    ids = [5, 0, 1, 2, 3, 4]
    p = np.full((20, 8), 0.001)
    p[:, 7] = 1 - 0.007
    for j, c in enumerate(ids):
        p[3 * j + 1, c] = 0.9
        p[3 * j + 1, 7] = 0.1 - 0.006
    p[1, 5], p[1, 4], p[1, 7] = 0.4, 0.5, 0.1 - 0.005
    return torch.from_numpy(np.log(p).astype(np.float32)), ids


class PieceTok:
    """A sentencepiece-like stub."""
    PIECES = ['▁the', '▁c', 'at', 's', '▁sat', 'on', '▁']
    WORDS = {'on the': [5, 0], 'cats': [1, 2, 3], 'the': [0]}

    def id_to_piece(self, i): return self.PIECES[i]
    def decode(self, ids): return ''.join(self.PIECES[i] for i in ids).replace('▁', ' ').strip()
    def encode(self, text): return list(self.WORDS[text])


def test_beam_decoder_and_decode_beams_with_hotwords(emulated_hot):
    D, calls, other = emulated_hot.D, emulated_hot.calls, emulated_hot.other
    lp, ids = _cat_emission()
    free = D.BeamSearchCTCDecoder(tokenizer=PieceTok(), blank_id=7, beam_width=16, nbest=4)
    assert free(lp, decode=False)[0] == 4 and not calls and other == ['free']
    beams = free.decode_beams(lp, hotwords=['on the'], hotword_weight=2.0)          # pyctcdecode's call
    assert calls[-1][:2] == (((5, 0),), 2.0) and calls[-1][3:5] == (16, 4) and beams[0].tokens == ids and beams[0].text == 'on the cats sat'
    assert beams[0].lm_score == beams[0].logit_score + 2.0 and [b.lm_score for b in beams] == sorted((b.lm_score for b in beams), reverse=True)
    assert free.decode_beams(lp, hotwords=['on the'])[0].lm_score == beams[0].logit_score + 10.0 and calls[-1][1] == 10.0
    assert len(free._hotword_sets) == 1 and free.decode_beams(lp, hotwords=['cats', 'the']) and len(free._hotword_sets) == 2
    assert calls[-1][0] == ((0,), (1, 2, 3))
    assert free(lp, hotwords=['on the']) == 'on the cats sat' and free(lp) == 'sat the cats sat'
    from lcasr_amd.decoding.hotwords import HotwordSet
    hs = HotwordSet([(5,)], [0.5])
    n = len(calls)
    assert free.decode_beams(lp, hotwords=hs, hotword_weight=1.0)[0].tokens == ids and calls[-1][:2] == (((5,),), 1.0) and len(calls) == n + 1
    assert free.decode_beams(lp, hotwords=hs, hotword_weight=0.25)[0].tokens[0] == 4                 # 0.125 < ln(0.5 / 0.4)
    assert free.decode_beams(lp, hotwords=[])[0].tokens[0] == 4 and len(calls) == n + 2               # no hotword: the search of today
    dec = D.BeamSearchCTCDecoder(tokenizer=PieceTok(), blank_id=7, beam_width=16, nbest=4, hotwords=['on the'], hotword_weight=3.0)
    assert dec(lp, decode=False) == ids and calls[-1][1] == 3.0 and dec.decode_beams(lp, hotword_weight=0.0)[0].tokens[0] == 4
    with pytest.raises(ValueError, match='tokenizer'):
        D.BeamSearchCTCDecoder(blank_id=7).decode_beams(lp, hotwords=['on the'])
    with pytest.raises(TypeError):
        free.decode_beams(lp, hotwords='on the')
    with pytest.raises(TypeError):
        free.decode_beams(lp, hotwords=[(5, 0)])
    a = D.ctc_beam_search_hot(lp, hs, 1.0, blank=7, beam_width=5, nbest=3)
    assert isinstance(a, D.CTCBeamsHot) and a.tokens.shape == (3, 20) and a.hot_scores.shape == (3,) and a.count.shape == ()
    assert D.CTCBeamsHot._fields == D.CTCBeamsLM._fields + ('hot_scores',)
    b = D.ctc_beam_search_hot(torch.stack([lp, lp]), hs, 1.0, input_lengths=[20, 9], blank=7, beam_width=5, nbest=3, max_len=4)
    assert b.tokens.shape == (2, 3, 4) and torch.equal(b.scores[0], a.scores) and torch.equal(b.hot_scores[0], a.hot_scores)
    assert float(a.hot_scores[0]) == 0.5 and float(a.scores[0]) == float(a.logit_scores[0]) + 0.5
    assert D.OutputBeam._fields == ('text', 'tokens', 'logit_score', 'lm_score', 'text_frames')


def test_hotwords_beside_an_lm_and_none_is_the_path_of_today(emulated_hot):
    D, calls, other = emulated_hot.D, emulated_hot.calls, emulated_hot.other
    lp, ids = _cat_emission()
    img, ref = LR.lm_pair(LR.train([[4, 0, 1, 2, 3, 4] * 8], 3, 7), 3, 7)      # an LM that has only seen the sentence start with 'sat'
    emulated_hot.use(ref)
    dec = D.BeamSearchCTCDecoder(tokenizer=PieceTok(), blank_id=7, beam_width=16, nbest=4, lm=img, alpha=1.0, beta=0.5)
    plain = dec.decode_beams(lp)
    assert other == ['lm'] and not calls and plain[0].tokens[0] == 4
    want = LR.ctc_beam_lm(lp[None], None, ref, 7, 16, 4, -5.0, -10.0, 16, 20, 1.0, 0.5)
    assert [b.lm_score for b in plain] == want.scores[0, :len(plain)].tolist() and [b.logit_score for b in plain] == want.logit_scores[0, :len(plain)].tolist()
    assert [b.tokens for b in plain] == [want.tokens[0, r, :int(want.lengths[0, r])].tolist() for r in range(len(plain))]
    zero = dec.decode_beams(lp, hotwords=['on the'], hotword_weight=0.0)
    assert zero == plain and len(calls) == 1                               # weight 0 through the hotword unit: the LM search's output, bit for bit
    hot = dec.decode_beams(lp, hotwords=['on the'], hotword_weight=12.0)
    assert hot[0].tokens == ids and calls[-1][-2:] == (1.0, 0.5)
    assert hot[0].lm_score - hot[0].logit_score == pytest.approx(1.0 * img.score(ids) + 0.5 * len(ids) + 12.0, abs=1e-9)


class WordTok:
    """Toy tokenizer: id i decodes to the word 'w<i % 7>'; 't<i>' encodes to id i."""
    def __init__(self, V): self.V = V
    def vocab_size(self): return self.V
    def decode(self, ids): return ' '.join(f'w{int(i) % 7}' for i in ids)
    def encode(self, text): return [int(w[1:]) for w in text.split()]


def test_transcribe_and_evaluate_with_hotwords_on_the_tiny_model(emulated_ops, emulated_hot, monkeypatch):
    from lcasr_amd.eval import run as R
    from lcasr_amd.utils import audio_tools
    monkeypatch.setattr(audio_tools.audio, 'melspec', AR.melspec)
    E.attach(monkeypatch, emulated_ops)
    fx = load_golden('infer_tiny')
    m = build_from_fixture(fx).eval()
    V = int(fx['cfg.vocab_size'])
    tok, blank = WordTok(V), m.decoder.num_classes - 1
    wave = AR.test_signal(3 * 16000, seed=3)
    logits = R.moving_average_eval(R._Args(), m, audio_tools.to_spectogram(wave[None]), 128, 32, tok, use_tqdm=False, return_numpy=False)
    free, _ = BR.search(logits.float().numpy(), blank, 4)
    assert len(free) > 1 and free[1][0] != free[0][0]
    runner_up = free[1][0]
    phrase = next(runner_up[k:k + 2] for k in range(len(runner_up)) if not any(free[0][0][j:j + 2] == runner_up[k:k + 2] for j in range(len(free[0][0]))))
    words = [' '.join(f't{c}' for c in phrase)]
    weight = 2.0 * (free[0][2] - free[1][2]) + 1.0
    text = R.transcribe(m, wave, tok, 128, 32, beam_width=4, hotwords=words, hotword_weight=weight)
    assert emulated_hot.calls[-1][:2] == ((tuple(phrase),), weight) and emulated_hot.calls[-1][3] == 4
    best = HR.search_hot(logits.float().numpy(), blank, 4, HR.BruteHot([phrase]), weight)[0][0]
    assert text == tok.decode(best[0]) and best[4] >= weight and best[0] != free[0][0]
    assert R.transcribe(m, wave, tok, 128, 32, beam_width=4) == tok.decode(free[0][0])
    spec = torch.from_numpy(fx['spec'].copy())
    n = len(emulated_hot.calls)
    data = R.evaluate(m, [('r0', spec, 'w1 w2 w3 w4')], tok, 256, 64, beam_width=4, hotwords=words)
    assert len(emulated_hot.calls) == n + 1 and emulated_hot.calls[-1][1] == 10.0 and data[-1]['recording'] == 'all'
    with pytest.raises(ValueError, match='greedy'):
        R.transcribe(m, wave, tok, 128, 32, beam_width=1, hotwords=words)
    with pytest.raises(ValueError, match='greedy'):
        R.evaluate(m, [('r0', spec, 'w1')], tok, 256, 64, hotwords=words)
    d = R._decoder(m, tok, 4)
    assert type(d).__name__ == 'BeamSearchCTCDecoder' and d.hotwords is None and d.lm is None


def test_the_cache_of_compiled_sets_keeps_the_most_recently_used(emulated_hot):
    D = emulated_hot.D
    lp, ids = _cat_emission()
    dec = D.BeamSearchCTCDecoder(tokenizer=PieceTok(), blank_id=7, beam_width=4)
    dec.HOTWORD_SETS_KEPT = 2
    lists = (['on the'], ['cats'], ['the'])
    first = dec._hotword_set(lists[0])
    assert dec._hotword_set(lists[1]) is not first and dec._hotword_set(lists[0]) is first         # used again: now the most recent
    dec._hotword_set(lists[2])
    assert list(dec._hotword_sets) == [('on the',), ('the',)] and dec._hotword_set(lists[0]) is first
    assert dec.decode_beams(lp, hotwords=lists[1])[0].tokens[1:] == ids[1:] and len(dec._hotword_sets) == 2
    assert D.BeamSearchCTCDecoder.HOTWORD_SETS_KEPT == 16
