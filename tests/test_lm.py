"""CPU tests of the n-gram LM and of the beam search fused with it: the automaton image of lcasr_amd.decoding.lm.NGramLM against the
dict-keyed ARPA recursion of tests/lm_refs.py, ARPA parsing and its refusals, validate / save / load, the restatement of the fused
search (lm_refs.search_lm) against beam_refs.search, hand cases and the enumeration of every frame path, the usefulness case, the
fifth ABI unit's header / binding / queries / refusals, and BeamSearchCTCDecoder(lm=...) / decode_beams_lm / transcribe(lm=...) on
the tiny fixture model with the op replaced by the restatement.  The HIP kernels themselves are tested in test_lm_gpu.py."""
import ctypes
import itertools
import math
import os
import types

import numpy as np
import pytest
import torch

import audio_refs as AR
import beam_refs as BR
import eval_refs as E
import lm_refs as LR
from cabi_header import assert_binding_is_header, header_abi
from common_model import build_from_fixture
from conftest import ROOT, load_golden

INF = math.inf


def NG():
    from lcasr_amd.decoding.lm import NGramLM
    return NGramLM


# ---- 1. the image against the definition --------------------------------------------------------------------------------------
@pytest.mark.parametrize('order', [1, 2, 3, 4, 5])
@pytest.mark.parametrize('bos', [False, True])
def test_image_equals_the_dict_recursion_on_every_sequence(order, bos):
    """Random prefix-closed tables over 5 tokens (leaves, contexts without children, missing back-off columns, a token without a
    unigram): for every token sequence up to length 6, each step of the image gives the conditional of the recursion over the FULL
    history, and lands in the state of the longest known suffix."""
    V = 5
    rng = np.random.default_rng(100 * order + bos)
    worst, leaves, childless, unk_tables = 0.0, 0, 0, 0
    for _ in range(2):
        table, unk = LR.random_table(rng, V, order, bos)
        img, ref = LR.lm_pair(table, order, V, unk, use_bos=bos)
        assert img.order == max(len(g) for g in table) and img.num_tokens == V and img.n_states == 1 + sum(len(g) < img.order for g in table)
        assert img.contexts[img.start_state] == ref.start
        unk_tables += unk is not None
        leaves += sum(len(g) < order and not any(g + (w,) in table for w in range(V)) for g in table)
        childless += int((img.states[1:, 1] == 0).sum())
        # every sequence of 1 .. 6 tokens, all 19 530 of them, depth first: a sequence shares the steps of its prefix, which were
        # checked when the prefix was visited; frame = (sequence, image state, full history, sum of the image's q, of the recursion's)
        stack, seen = [((), img.start_state, ref.start, 0.0, 0.0)], 0
        while stack:
            seq, s, hist, total, want = stack.pop()
            if seq:
                seen += 1
                worst = max(worst, abs(total - want), abs(img.score(seq) - want))
            if len(seq) == 6: continue
            for c in range(V):
                q, s2 = img.step(s, c)
                w = ref.cond(hist, c)
                assert abs(q - w) <= 1e-12, (seq, c, q, w)
                assert img.contexts[s2] == ref.state_of(hist + (c,)), (seq, c, img.contexts[s2], ref.state_of(hist + (c,)))
                stack.append((seq + (c,), s2, hist + (c,), total + q, want + w))
        assert seen == sum(V ** n for n in range(1, 7))
    print(f'[lm] order {order} bos {bos}: largest |score - recursion| {worst:.2e}; {leaves} leaf grams, {childless} states without children')
    assert worst <= 1e-12 and (order == 1 or (leaves > 0 and childless > 0))


def test_an_unknown_class_scores_nothing_and_resets_the_context():
    img, ref = LR.lm_pair(LR.usefulness_table(), 3, 12)
    q, s = img.step(img.step(0, 3)[1], 12)
    assert (q, s) == (0.0, 0) and ref.step((3,), 12) == (0.0, ())


# ---- 2. ARPA parsing ------------------------------------------------------------------------------------------------------------
ARPA = '''
\\data\\
ngram 1=6
ngram 2=4
ngram 3=1

\\1-grams:
-99\t<s>\t-0.5
-1.0\t</s>
-2.0\t<unk>
-0.5\t0\t-0.25
-0.75\t1
-1.25\t2\t-0.125

\\2-grams:
-0.3\t<s> 0\t-0.2
-0.4\t0 1
-0.6\t0 </s>
-0.7\t2 <unk>

\\3-grams:
-0.1\t<s> 0 1

\\end\\
'''.split('\n')


def test_arpa_parsing_by_hand():
    lm = NG().from_arpa(ARPA, 4)
    n = lambda v: float(np.float32(v * math.log(10.0)))
    assert lm.order == 3 and lm.num_tokens == 4 and lm.n_states == 7 and lm.n_entries == 3
    assert lm.contexts == [(), (0,), (1,), (2,), (4,), (0, 1), (4, 0)]
    ctx = {g: s for s, g in enumerate(lm.contexts)}
    assert lm.start_state == ctx[(4,)] and NG().from_arpa(ARPA, 4, use_bos=False).start_state == 0
    assert lm.step(0, 0) == (n(-0.5), ctx[(0,)])                           # log10 -> natural log, f32
    assert lm.step(0, 3) == (n(-2.0), 0)                                   # no unigram: <unk>
    assert lm.step(ctx[(1,)], 2) == (0.0 + n(-1.25), ctx[(2,)])            # a missing back-off column is 0
    assert lm.step(ctx[(0,)], 2) == (n(-0.25) + n(-1.25), ctx[(2,)])       # back-off, then the unigram
    assert lm.step(ctx[(4,)], 0) == (n(-0.3), ctx[(4, 0)])
    assert lm.step(ctx[(4, 0)], 1) == (n(-0.1), ctx[(0, 1)])               # the trigram; next: its longest suffix that is a state
    assert lm.step(ctx[(4, 0)], 2) == (n(-0.2) + n(-0.25) + n(-1.25), ctx[(2,)])
    assert all(4 not in g[1:] for g in lm.contexts) and lm.entries[:, 0].max() < 4                 # </s> and <unk> grams are gone
    assert lm.score([0, 1]) == n(-0.3) + n(-0.1)
    shifted = NG().from_arpa(ARPA, 4, token_of=lambda w: {'0': 1, '1': 0, '2': 2}[w])           # a mapping of its own
    assert shifted.step(0, 1)[0] == n(-0.5) and shifted.step(0, 0)[0] == n(-0.75)

    class Tok:
        def piece_to_id(self, w): return int(w) + 0
    assert np.array_equal(NG().from_arpa(ARPA, 4, tokenizer=Tok()).image, lm.image)
    assert NG().from_arpa(ARPA, 4, unk_logp=-7.0).step(0, 3) == (float(np.float32(-7.0)), 0)


def test_arpa_refusals(tmp_path):
    lines = lambda grams, order, **kw: LR.write_arpa(grams, order, 4, **kw)
    ok = {(0,): (-0.5, -0.1), (1,): (-0.6, None), (2,): (-0.7, None), (3,): (-0.8, None), (0, 1): (-0.2, None)}
    NG().from_arpa(lines(ok, 2), 4)
    with pytest.raises(ValueError, match='prefix-closed'):
        NG().from_arpa(lines({**ok, (1, 2, 3): (-0.3, None)}, 3), 4)
    with pytest.raises(ValueError, match='outside'):
        NG().from_arpa(lines({**ok, (7,): (-0.3, None)}, 2), 4)
    with pytest.raises(ValueError, match='outside'):
        NG().from_arpa(lines(ok, 2), 3)
    six = {tuple(range(k)) if k <= 4 else (0, 1, 2, 3) + (0,) * (k - 4): (-0.3, -0.1) for k in range(1, 7)}
    with pytest.raises(ValueError, match='order'):
        NG().from_arpa(lines({**ok, **six}, 6), 4)
    missing = {g: v for g, v in ok.items() if g != (3,)}
    with pytest.raises(ValueError, match='unk_logp'):
        NG().from_arpa(lines(missing, 2), 4)
    assert NG().from_arpa(lines(missing, 2, unk_log10=-3.0), 4).step(0, 3)[0] == LR.nat32(-3.0)
    assert NG().from_arpa(lines(missing, 2), 4, unk_logp=-5.0).step(0, 3)[0] == -5.0
    p = tmp_path / 'lm.arpa'
    p.write_text('\n'.join(lines(ok, 2, with_eos=True)))
    assert np.array_equal(NG().from_arpa(str(p), 4).image, NG().from_arpa(lines(ok, 2), 4).image)        # from a path; </s> dropped


def _damaged(lm, change):
    image = lm.image.copy()
    change(image, lm)
    return image, lm.n_states, lm.n_entries, lm.num_tokens, lm.order, lm.start_state


def test_validate_refuses_each_kind_of_damage(tmp_path):
    lm, _ = LR.lm_pair(LR.train([np.random.default_rng(3).integers(0, 6, 200).tolist()], 3, 6), 3, 6)
    S, E = lm.n_states, lm.n_entries
    lm.validate()
    two = int(np.flatnonzero(lm.states[:, 1] >= 2)[0])                     # a state with two children
    deep = int(np.flatnonzero(lm.states[:, 3] != 0)[0])                    # a state of two words
    damage = {
        'children outside the entries': lambda im, m: im.__setitem__(4 * two + 1, E + 1),
        'a negative first child': lambda im, m: im.__setitem__(4 * two, -1),
        'a back-off state out of range': lambda im, m: im.__setitem__(4 * deep + 3, S),
        'a next state out of range': lambda im, m: im.__setitem__(4 * S + 2, S + 5),
        'a dense next state out of range': lambda im, m: im.__setitem__(4 * (S + E) + 1, -2),
        'a token out of range': lambda im, m: im.__setitem__(4 * S, 6),
        'unsorted children': lambda im, m: im.__setitem__(4 * (S + int(m.states[two, 0]) + 1), int(m.entries[int(m.states[two, 0]), 0])),
        'a back-off cycle': lambda im, m: im.__setitem__(4 * deep + 3, deep),
        'a back-off chain that is too long': lambda im, m: (im.__setitem__(4 * 1 + 3, deep)),
        'a non-finite value': lambda im, m: im.__setitem__(4 * S + 1, int(np.array([np.inf], dtype=np.float32).view(np.int32)[0])),
    }
    for what, change in damage.items():
        with pytest.raises(ValueError, match='LM image'):
            NG()(*_damaged(lm, change))
        print(f'[lm] validate refuses {what}')
    with pytest.raises(ValueError, match='LM image'):
        NG()(lm.image[:-1], S, E, 6, 3, 0)
    with pytest.raises(ValueError, match='start state'):
        NG()(lm.image, S, E, 6, 3, S)
    bad = tmp_path / 'bad.npz'                                             # load validates too
    im = _damaged(lm, damage['a back-off cycle'])
    with open(bad, 'wb') as f:
        np.savez(f, image=im[0], sizes=np.asarray(im[1:], dtype=np.int64))
    with pytest.raises(ValueError, match='LM image'):
        NG().load(str(bad))


def test_save_and_load_round_trip_bit_equal(tmp_path):
    rng = np.random.default_rng(7)
    table, unk = LR.random_table(rng, 5, 4, True)
    lm, _ = LR.lm_pair(table, 4, 5, unk)
    p = str(tmp_path / 'lm.npz')
    lm.save(p)
    back = NG().load(p)
    assert back.image.dtype == np.int32 and back.image.tobytes() == lm.image.tobytes()
    assert (back.n_states, back.n_entries, back.num_tokens, back.order, back.start_state) == (lm.n_states, lm.n_entries, 5, 4, lm.start_state)
    assert back.score([0, 1, 2, 3, 4, 0]) == lm.score([0, 1, 2, 3, 4, 0])
    assert lm.to('cpu') is lm and lm.device_image('cpu').dtype == torch.int32 and lm.device_image('cpu') is lm.device_image('cpu')


# ---- 3. the restatement of the fused search ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_search_lm_without_weights_is_the_lm_free_search(seed):
    _, ref = LR.lm_pair(LR.train([[0, 1, 2, 3, 4, 5, 6] * 5], 3, 7), 3, 7)
    lp = BR.noise_case(seed, 1, 40, 8)[0].numpy()
    want, st0 = BR.search(lp, 7, 8)
    got, st1 = LR.search_lm(lp, 7, 8, ref, 0.0, 0.0)
    assert [(p, f, k) for p, f, k, _ in got] == want and all(k == a for _, _, k, a in got)
    for k in ('gap', 'cap', 'pruned', 'folds', 'recreated', 'kept', 'live', 'max_score', 'candidates'):
        assert st0[k] == st1[k], k
    assert st1['lookups'] > 0 and sum(st1['depth']) == st1['lookups']


def _lp(probs):
    with np.errstate(divide='ignore'):
        return np.log(np.asarray(probs, dtype=np.float64)).astype(np.float32)


def _unigram_ab(pa=0.9, pb=0.1):
    return LR.lm_pair({(0,): (math.log10(pa), None), (1,): (math.log10(pb), None)}, 1, 2)


def test_one_frame_where_the_lm_turns_b_into_a():
    """Classes: 0 = a, 1 = b, 2 = blank.  P(a) = 0.45, P(b) = 0.55; the unigram LM says P(a) = 0.9, P(b) = 0.1."""
    img, ref = _unigram_ab()
    lp = _lp([[0.45, 0.55, 0.0]])
    assert BR.search(lp, 2, 4)[0][0][0] == (1,)
    beams, _ = LR.search_lm(lp, 2, 4, ref, 1.0, 0.0)
    assert [b[0] for b in beams] == [(0,), (1,)]
    assert beams[0][2] == pytest.approx(math.log(0.45) + math.log(0.9), abs=1e-6) and beams[0][3] == pytest.approx(math.log(0.45), abs=1e-7)
    assert beams[0][2] == beams[0][3] + 1.0 * img.score([0])


def test_a_fold_with_the_lm_on_keeps_one_bonus():
    """Classes: 0 = a, 1 = blank; P(a) = 0.6 in both frames.  In frame 1 the empty prefix extended by a IS the live beam "a": its
    mass is folded in and the beam keeps the one bonus it got when it was created."""
    img, ref = LR.lm_pair({(0,): (math.log10(0.5), None)}, 1, 1)
    beams, st = LR.search_lm(_lp([[0.6, 0.4]] * 2), 1, 4, ref, 0.7, 1.25)
    assert st['folds'] >= 1 and st['lookups'] == 1                         # one lookup: the fold took no step
    got = {b[0]: b for b in beams}
    assert got[(0,)][3] == pytest.approx(math.log(0.84), abs=1e-7)
    assert got[(0,)][2] - got[(0,)][3] == pytest.approx(0.7 * img.score([0]) + 1.25, abs=1e-12)
    assert got[()][2] == got[()][3] == pytest.approx(math.log(0.16), abs=1e-7)


def test_restatement_against_the_enumeration_of_every_frame_path():
    """Token pruning off, W above the number of prefixes, T <= 5, C <= 4: every label sequence is a hypothesis, its logit score the
    log-sum of all its alignments and its score that plus alpha ln P_LM(tokens) + beta per token."""
    rng = np.random.default_rng(2026)
    worst, sets = 0.0, 0
    for C in (2, 3, 4):
        table, unk = LR.random_table(rng, C - 1, min(3, C), True)
        img, ref = LR.lm_pair(table, max(len(g) for g in table), C - 1, unk)
        for T in range(1, 6):
            for alpha, beta in ((0.5, 1.5), (1.3, -0.4)):
                x = rng.normal(size=(T, C)) * 2
                lp = (x - np.log(np.exp(x).sum(-1, keepdims=True))).astype(np.float32)
                beams, st = LR.search_lm(lp, C - 1, 2000, ref, alpha, beta, -INF, -INF, 16)
                want = BR.enumerate_paths(lp, C - 1)
                assert {b[0] for b in beams} == set(want) and len(beams) == len(want)
                assert [b[2] for b in beams] == sorted((b[2] for b in beams), reverse=True)
                for pre, frames, keyv, a in beams:
                    worst = max(worst, abs(a - want[pre]), abs(keyv - (want[pre] + alpha * img.score(pre) + beta * len(pre))))
                sets += 1
    print(f'[lm] {sets} emission sets, largest |score - (log-sum of the alignments + alpha ln P + beta len)| = {worst:.2e}')
    assert worst <= 1e-12


def test_the_lm_corrects_the_ambiguous_spiky_input():
    """The usefulness case on the restatement: six seeds, 192 tokens."""
    img, ref = LR.lm_pair(LR.usefulness_table(), 3, 12)
    free, fused, gap = 0, 0, INF
    for seed in LR.USEFUL_SEEDS:
        lp, labels = LR.usefulness_case(seed)
        assert len(labels) == 32
        free += LR.edit_distance(list(BR.search(lp[0].numpy(), 15, 16)[0][0][0]), labels)
        beams, st = LR.search_lm(lp[0].numpy(), 15, 16, ref, 1.0, 1.0)
        fused += LR.edit_distance(list(beams[0][0]), labels)
        gap = min(gap, st['gap'])
    print(f'[lm] token errors of 192: LM-free {free}, with the trigram {fused}; smallest decision gap {gap:.2e}')
    assert free >= 10 and 2 * fused <= free


# ---- 4. the fifth ABI unit --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from lcasr_amd.hip import lm
    return lm.load()


def test_header_binding_and_exports_agree(lib):
    from lcasr_amd.hip import _lib, lm
    funcs, enums = header_abi('sconf_lm.h', 'sconf_lm_')
    assert not enums and set(funcs) == {'sconf_lm_max_order', 'sconf_lm_beam_threads', 'sconf_lm_beam_workspace', 'sconf_lm_beam_ctc'}
    assert_binding_is_header(funcs, lm.PROTOTYPES, lm.PLAIN, 'hip/lm.py')
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(raw, n) for n in funcs)
    for n, (args, res) in {**{k: (v, ctypes.c_int) for k, v in lm.PROTOTYPES.items()}, **lm.PLAIN}.items():
        assert _lib.bound()[n] == (args, res)
    assert not any(n.startswith('sconf_lm_') for n in list(_lib.PROTOTYPES) + list(_lib.PLAIN))
    for f in ('include/sconf.h', 'include/sconf_beam.h', 'long-context-asr_amd/hip/_lib.py', 'long-context-asr_amd/hip/beam.py',
              'long-context-asr_amd/hip/__init__.py', 'long-context-asr_amd/hip/audio.py', 'long-context-asr_amd/hip/align.py'):
        assert 'sconf_lm_' not in open(os.path.join(ROOT, f)).read() and 'import lm' not in open(os.path.join(ROOT, f)).read(), f
    lib.sconf_version.restype = ctypes.c_int
    assert lib.sconf_version() == 220


def test_lm_queries(lib):
    from lcasr_amd.hip import beam, lm
    assert lib.sconf_lm_max_order() == 5 == lm.MAX_ORDER == lm.max_order()
    blib = beam.load()
    for W, K in ((1, 1), (8, 16), (16, 16), (32, 16), (100, 16), (128, 16), (0, 1), (129, 1), (1, 17)):
        assert lib.sconf_lm_beam_threads(W, K) == blib.sconf_beam_threads(W, K)
    ws = lib.sconf_lm_beam_workspace
    assert ws(1, 16384, 100, 16) == 28445440 == lm.beam_workspace(1, 16384, 100, 16)               # the figure in the header
    r256 = lambda n: (n + 255) // 256 * 256
    for B, N, W, K in ((1, 1, 1, 1), (2, 100, 7, 3), (3, 2048, 64, 16), (16, 2048, 100, 16)):
        assert ws(B, N, W, K) == r256(B * N * (8 + 8 * K)) + r256(16 * B * N * W) + r256(24 * B * W) + r256(4 * B)
    assert ws(0, 10, 4, 4) == -1 and ws(1, 0, 4, 4) == -1 and ws(1, 10, 129, 4) == -1 and ws(1, 10, 4, 17) == -1 and ws(1 << 20, 1 << 20, 4, 4) == -1
    with pytest.raises(ValueError, match='beam_width'):
        lm.beam_workspace(1, 10, 129, 4)


def test_lm_refusals_launch_nothing(lib):
    one = ctypes.c_void_p(16)                                              # never dereferenced: every call below is refused on the host
    need = lib.sconf_lm_beam_workspace(1, 10, 8, 4)

    def call(lp=one, image=one, S=3, E=2, V=12, order=3, start=0, ws=need, B=1, N=10, C=32, blank=31, W=8, nbest=2, prune=-10.0, K=4, L=10,
             alpha=0.5, beta=1.5):
        return lib.sconf_lm_beam_ctc(lp, None, image, S, E, V, order, start, one, one, one, one, one, one, one, ws, B, N, C, blank, W, nbest,
                                     -5.0, prune, K, L, alpha, beta, None)

    for kw, word in ((dict(blank=32), b'blank'), (dict(ws=need - 1), b'workspace'), (dict(W=0), b'beam_width'), (dict(W=129, ws=1 << 40), b'128'),
                     (dict(nbest=9), b'nbest'), (dict(K=0), b'max_tokens_per_frame'), (dict(prune=0.5), b'beam_prune_logp'),
                     (dict(prune=math.nan), b'beam_prune_logp'), (dict(C=30), b'multiple of 4'), (dict(N=0), b'sizes'), (dict(L=0), b'sizes'),
                     (dict(lp=None), b'null'), (dict(image=None), b'null'), (dict(order=0), b'order'), (dict(order=6), b'order'),
                     (dict(V=0), b'num_tokens'), (dict(V=33), b'num_tokens'), (dict(S=0), b'image sizes'), (dict(E=-1), b'image sizes'),
                     (dict(S=1 << 30, E=1 << 30), b'image sizes'), (dict(start=3), b'start_state'), (dict(start=-1), b'start_state'),
                     (dict(alpha=math.inf), b'finite'), (dict(beta=math.nan), b'finite'), (dict(image=ctypes.c_void_p(24)), b'aligned')):
        assert call(**kw) != 0 and word in lib.sconf_last_error(), (kw, lib.sconf_last_error())
    assert call(B=0) == 0                                                  # nothing to do, nothing launched


def test_a_cpu_tensor_is_refused_by_the_product_path():
    from lcasr_amd.decoding.beam import ctc_beam_search_lm
    img, _ = _unigram_ab()
    lp = BR.noise_case(1, 1, 8, 8)
    with pytest.raises(RuntimeError, match='GPU'):
        ctc_beam_search_lm(lp[0], img, blank=7)
    with pytest.raises(ValueError, match='language model'):
        ctc_beam_search_lm(lp[0], None, blank=7)
    with pytest.raises(ValueError, match='tokens'):
        ctc_beam_search_lm(lp[0, :, :1], img, blank=0)


# ---- 5. the Python layers on the restatement ------------------------------------------------------------------------------------
@pytest.fixture
def emulated_lm(monkeypatch):
    """lcasr_amd.hip.lm.ctc_beam_lm replaced by the restatement; `use(ref)` names the DictLM that stands for the image."""
    from lcasr_amd.decoding import beam as D
    from lcasr_amd.hip import lm as lm_kernels
    box, calls = {}, []

    def op(lp, il, image, S, E, V, order, start, *rest):
        assert image.dtype == torch.int32 and image.numel() == 4 * S + 4 * E + 2 * V and V == box['ref'].num_tokens and order == box['ref'].order
        calls.append(rest)
        return LR.ctc_beam_lm(lp, il, box['ref'], *rest)

    monkeypatch.setattr(lm_kernels, 'ctc_beam_lm', op)
    return types.SimpleNamespace(D=D, use=lambda ref: box.__setitem__('ref', ref), calls=calls)


class PieceTok:
    """A sentencepiece-like stub."""
    PIECES = ['▁the', '▁c', 'at', 's', '▁sat', 'on', '▁']

    def id_to_piece(self, i): return self.PIECES[i]
    def decode(self, ids): return ''.join(self.PIECES[i] for i in ids).replace('▁', ' ').strip()


def test_beam_decoder_and_decode_beams_lm_with_an_lm(emulated_lm, monkeypatch):
    from lcasr_amd.eval.utils import decode_beams_lm
    D, calls = emulated_lm.D, emulated_lm.calls
    monkeypatch.setattr(D.beam_kernels, 'ctc_beam', BR.ctc_beam)
    ids = [5, 0, 1, 2, 3, 4]
    img, ref = LR.lm_pair(LR.train([ids * 8], 3, 7), 3, 7)
    emulated_lm.use(ref)
    # frame 1 is ambiguous between 'on' (5) and 'sat' (4), acoustically 0.4 : 0.5; the LM has seen the sentence starting with 'on'
    p = np.full((20, 8), 0.001)
    p[:, 7] = 1 - 0.007
    for j, c in enumerate(ids):
        p[3 * j + 1, c] = 0.9
        p[3 * j + 1, 7] = 0.1 - 0.006
    p[1, 5], p[1, 4], p[1, 7] = 0.4, 0.5, 0.1 - 0.005
    lp = torch.from_numpy(np.log(p).astype(np.float32))
    free = D.BeamSearchCTCDecoder(tokenizer=PieceTok(), blank_id=7, beam_width=16, nbest=4)
    assert free(lp, decode=False)[0] == 4 and free.decode_beams(lp)[0].lm_score == free.decode_beams(lp)[0].logit_score and not calls
    dec = D.BeamSearchCTCDecoder(tokenizer=PieceTok(), blank_id=7, beam_width=16, nbest=4, lm=img, alpha=1.0, beta=0.5)
    assert dec(lp, decode=False) == ids and dec(lp) == 'on the cats sat'
    assert calls[-1][-2:] == (1.0, 0.5) and calls[-1][1:3] == (16, 1)
    beams = dec.decode_beams(lp)
    assert 1 < len(beams) <= 4 and beams[0].tokens == ids
    assert [b.lm_score for b in beams] == sorted((b.lm_score for b in beams), reverse=True)
    for b in beams:
        assert b.lm_score - b.logit_score == pytest.approx(1.0 * img.score(b.tokens) + 0.5 * len(b.tokens), abs=1e-9)
    data, best = decode_beams_lm([lp], dec, beam_width=8, ds_factor=4)
    d = data[0]
    assert d['text'] == 'on the cats sat' and d['ngram_score'] != 0 and d['am_score'] + d['ngram_score'] == pytest.approx(d['score'], abs=1e-12)
    assert d['am_score'] == best.logit_score < 0 and d['score'] == best.lm_score
    a = D.ctc_beam_search_lm(lp, img, 1.0, 0.5, blank=7, beam_width=5, nbest=3)
    assert isinstance(a, D.CTCBeamsLM) and a.tokens.shape == (3, 20) and a.logit_scores.shape == (3,) and a.count.shape == ()
    b = D.ctc_beam_search_lm(torch.stack([lp, lp]), img, 1.0, 0.5, input_lengths=[20, 9], blank=7, beam_width=5, nbest=3, max_len=4)
    assert b.tokens.shape == (2, 3, 4) and torch.equal(b.scores[0], a.scores) and torch.equal(b.logit_scores[0], a.logit_scores)
    assert D.CTCBeams._fields == ('count', 'tokens', 'lengths', 'token_frames', 'scores')          # the LM-free tuple is what it was


class WordTok:
    """Toy tokenizer: id i decodes to the word 'w<i % 7>'."""
    def __init__(self, V): self.V = V
    def vocab_size(self): return self.V
    def decode(self, ids): return ' '.join(f'w{int(i) % 7}' for i in ids)


def test_transcribe_and_evaluate_with_an_lm_on_the_tiny_model(emulated_ops, emulated_lm, monkeypatch):
    from lcasr_amd.eval import run as R
    from lcasr_amd.utils import audio_tools
    monkeypatch.setattr(audio_tools.audio, 'melspec', AR.melspec)
    E.attach(monkeypatch, emulated_ops)
    fx = load_golden('infer_tiny')
    m = build_from_fixture(fx).eval()
    V = int(fx['cfg.vocab_size'])
    tok, blank = WordTok(V), m.decoder.num_classes - 1
    assert blank == V
    rng = np.random.default_rng(5)
    img, ref = LR.lm_pair(LR.train([rng.integers(0, V, 400).tolist()], 2, V), 2, V)
    emulated_lm.use(ref)
    wave = AR.test_signal(3 * 16000, seed=3)
    text = R.transcribe(m, wave, tok, 128, 32, beam_width=4, lm=img, alpha=0.8, beta=0.3)
    assert emulated_lm.calls[-1][1] == 4 and emulated_lm.calls[-1][-2:] == (0.8, 0.3)
    logits = R.moving_average_eval(R._Args(), m, audio_tools.to_spectogram(wave[None]), 128, 32, tok, use_tqdm=False, return_numpy=False)
    best = LR.search_lm(logits.float().numpy(), blank, 4, ref, 0.8, 0.3)[0][0]
    assert isinstance(text, str) and text == tok.decode(best[0])
    spec = torch.from_numpy(fx['spec'].copy())
    n = len(emulated_lm.calls)
    data = R.evaluate(m, [('r0', spec, 'w1 w2 w3 w4')], tok, 256, 64, beam_width=4, lm=img)
    assert len(emulated_lm.calls) == n + 1 and emulated_lm.calls[-1][-2:] == (0.5, 1.5) and data[-1]['recording'] == 'all'
    with pytest.raises(ValueError, match='beam_width'):
        R.transcribe(m, wave, tok, 128, 32, beam_width=1, lm=img)
    with pytest.raises(ValueError, match='beam_width'):
        R.evaluate(m, [('r0', spec, 'w1')], tok, 256, 64, lm=img)
    assert type(R._decoder(m, tok, 4)).__name__ == 'BeamSearchCTCDecoder' and R._decoder(m, tok, 4).lm is None
