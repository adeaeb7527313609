"""The posterior unit without a GPU (include/sconf_post.h, lcasr_amd.hip.post, lcasr_amd.decoding.posterior): the two numpy
restatements of tests/post_refs.py against torch's CTC loss and against each other, the invariants of the reported ratios, that the
inputs of the GPU parity tests see every rule of the recurrences, the long form's cut rule and its exactness where the scores pin
the cuts, the binding against the header, the host-side queries and refusals, and the glue of eval.run on the tiny fixture model
with the restatements in the kernels' place."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import eval_refs as E
import post_refs as PR
from cabi_header import assert_binding_is_header, header_abi
from common_model import build_from_fixture
from conftest import ROOT, load_golden

HEADER = 'sconf_post.h'
NAMES = {'sconf_post_max_labels', 'sconf_post_workspace', 'sconf_post_step_error', 'sconf_post_lattice', 'sconf_post_neighbours',
         'sconf_post_slots'}


def random_case(rng, T=None, L=None, C=None, holes=0.15):
    T = int(rng.integers(1, 13)) if T is None else T
    C = int(rng.integers(3, 7)) if C is None else C
    blank = int(rng.integers(0, C))
    L = int(rng.integers(0, min(T, 5) + 1)) if L is None else L
    labels = [c for c in range(C) if c != blank]
    y = rng.choice(labels, size=L)
    if L >= 2 and rng.random() < 0.5:                                       # a repeated label
        k = int(rng.integers(1, L))
        y[k] = y[k - 1]
    lp = np.log(rng.dirichlet(np.ones(C), size=T)) if T else np.zeros((0, C))
    lp = np.where(rng.random(lp.shape) < holes, -np.inf, lp)
    return lp, y, blank


def same_pattern(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a == -np.inf, b == -np.inf) and not (a == np.inf).any()


def close(a, b, tol):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    f = np.isfinite(a)
    return same_pattern(a, b) and (not f.any() or float(np.abs(a[f] - b[f]).max()) <= tol)


# ---- 1. the yardsticks ------------------------------------------------------------------------------------------------------------
def torch_loglik(lp, strings, blank):
    """-ctc_loss in float64 of every string (K, L') over lp (T, C)."""
    K, L = strings.shape
    T = lp.shape[0]
    x = torch.from_numpy(lp)[:, None, :].expand(T, K, lp.shape[1]).contiguous()
    tg = torch.from_numpy(np.concatenate([strings, np.zeros((K, 1), dtype=np.int64)], axis=1))
    nll = torch.nn.functional.ctc_loss(x, tg, torch.full((K,), T, dtype=torch.long), torch.full((K,), L, dtype=torch.long), blank=blank,
                                       reduction='none', zero_infinity=False)
    return -nll.numpy()


def test_plain_form_against_torch_ctc_loss():
    rng = np.random.default_rng(11)
    checked = 0
    for trial in range(40):
        lp, y, blank = random_case(rng, holes=0.1 if trial % 2 else 0.0)
        C, L = lp.shape[1], len(y)
        ll, sub, ins = PR.neighbours_plain(lp, y, blank)
        want = float(torch_loglik(lp, y[None], blank)[0])
        assert (ll == want == -np.inf) or abs(ll - want) <= 1e-10
        if not np.isfinite(ll):
            assert np.isnan(sub).all() and np.isnan(ins).all()
            continue
        subs, inss, dels = PR.edited_strings(y, C, blank)
        real = np.arange(C) != blank
        assert close(ins[:, real] + ll, torch_loglik(lp, inss[:, real].reshape((L + 1) * (C - 1), L + 1), blank).reshape(L + 1, C - 1), 1e-10)
        if L:
            assert close(sub[:, real] + ll, torch_loglik(lp, subs[:, real].reshape(L * (C - 1), L), blank).reshape(L, C - 1), 1e-10)
            assert close(sub[:, blank] + ll, torch_loglik(lp, dels, blank), 1e-10)
        assert (ins[:, blank] == 0.0).all()
        checked += 1
    assert checked >= 24


def test_bridge_form_against_plain_form():
    rng = np.random.default_rng(12)
    kinds = {'empty': 0, 'infeasible': 0, 'repeat': 0, 'holes': 0, 'ends': 0}
    for trial in range(300):
        if trial % 10 == 0:                                                  # L > T, or a repeat that needs one frame more than there are
            T = int(rng.integers(1, 5))
            lp, y, blank = random_case(rng, T=T, L=T + 1 if trial % 20 else T, holes=0.0)
            if len(y) == T and T >= 2:
                y[1] = y[0]
        else:
            lp, y, blank = random_case(rng, L=0 if trial % 10 == 1 else None, holes=0.2 if trial % 3 else 0.0)
        a, b = PR.neighbours_plain(lp, y, blank), PR.neighbours_bridge(lp, y, blank)
        for u, v, what in zip(a, b, ('ll', 'sub_llr', 'ins_llr')):
            assert close(u, v, 1e-10), (trial, what, lp.shape, y, blank)
        kinds['empty'] += len(y) == 0
        kinds['infeasible'] += a[0] == -np.inf and not np.isinf(lp).any()
        kinds['repeat'] += len(y) >= 2 and bool((y[1:] == y[:-1]).any()) and np.isfinite(a[0])
        kinds['holes'] += bool(np.isinf(lp).any()) and np.isfinite(a[0]) and bool((a[1] == -np.inf).any())
        kinds['ends'] += len(y) >= 1 and np.isfinite(a[0])
        if a[0] == -np.inf:
            assert np.isnan(a[1]).all() and np.isnan(a[2]).all() and np.isnan(b[2]).all()
    assert all(v >= 10 for v in kinds.values()), kinds
    # no frames at all: the empty transcript has probability 1 and nothing can be inserted
    ll, sub, ins = PR.neighbours_bridge(np.zeros((0, 4)), np.zeros(0, dtype=np.int64), 1)
    assert ll == 0.0 and sub.shape == (0, 4) and ins.tolist() == [[-np.inf, 0.0, -np.inf, -np.inf]]
    assert close(ins, PR.neighbours_plain(np.zeros((0, 4)), np.zeros(0, dtype=np.int64), 1)[2], 0.0)
    # poisoned: a NaN, a +inf, a label out of range or equal to the blank
    lp, y, blank = random_case(np.random.default_rng(5), T=6, L=3, C=5, holes=0.0)
    for bad_lp, bad_y in ((np.where(np.arange(30).reshape(6, 5) == 7, np.nan, lp), y), (np.where(np.arange(30).reshape(6, 5) == 9, np.inf, lp), y),
                          (lp, np.array([y[0], 5, y[2]])), (lp, np.array([-1, y[1], y[2]])), (lp, np.array([y[0], y[1], blank]))):
        for form in (PR.neighbours_plain, PR.neighbours_bridge):
            ll, sub, ins = form(bad_lp, bad_y, blank)
            assert math.isnan(ll) and np.isnan(sub).all() and np.isnan(ins).all() and sub.shape == (3, 5) and ins.shape == (4, 5)


def test_invariants_of_the_ratios():
    rng = np.random.default_rng(13)
    seen = 0
    for trial in range(60):
        lp, y, blank = random_case(rng, holes=0.1 if trial % 2 else 0.0)
        ll, sub, ins = PR.neighbours_bridge(lp, y, blank)
        if not np.isfinite(ll):
            continue
        seen += 1
        L = len(y)
        assert np.abs(sub[np.arange(L), y]).max(initial=0.0) <= 1e-10           # y_i -> y_i is y itself
        assert (ins[:, blank] == 0.0).all()
        post, alt, alt_post, gap_post, gap_alt, gap_alt_post = PR.slots(sub[None], ins[None], y[None], blank)
        for rows in (sub, ins):
            assert np.allclose(np.exp(rows - PR._lse(rows, axis=1)[:, None]).sum(1), 1.0, atol=1e-12)
        assert ((post > 0) & (post <= 1)).all() and ((gap_post > 0) & (gap_post <= 1)).all()
        assert (alt[0] != y).all() and (gap_alt[0] != blank).all() and (alt_post <= 1 - post + 1e-12).all()
        shifted = lp + rng.normal(size=(lp.shape[0], 1)) * 5.0                  # a constant per frame moves ll and no ratio
        ll2, sub2, ins2 = PR.neighbours_bridge(shifted, y, blank)
        assert close(sub, sub2, 1e-9) and close(ins, ins2, 1e-9) and (lp.shape[0] == 0 or ll2 != ll)
    assert seen >= 30
    # first index on ties, and a row whose alternatives are all impossible
    rows = np.array([[0.0, -1.0, -1.0, -3.0], [-np.inf, 0.0, -np.inf, -np.inf], [np.nan] * 4])
    post, alt, alt_post = PR._summary(rows, np.array([0, 1, 2]))
    assert alt.tolist() == [1, 0, -1] and post[1] == 1.0 and alt_post[1] == 0.0 and math.isnan(post[2]) and math.isnan(alt_post[2])
    assert post[0] == pytest.approx(1 / (1 + 2 * math.exp(-1) + math.exp(-3)), abs=1e-15)


# ---- 2. the inputs of the GPU parity tests see every rule ---------------------------------------------------------------------------
def test_the_parity_inputs_see_every_rule_of_the_recurrences():
    """With each rule of the bridge switched off in turn, some reported llr of the GPU parity inputs (the batches of up to 65 frames
    are enough) moves by more than 100 times that entry's llr tolerance at the largest step error the header may state.  The batches
    also are what tests/test_post_gpu.py says they are: B = 3 and ragged, a sample without labels, one without an alignment, the
    sizes, class counts and strides of its list, and at most 2 % of the rows tied."""
    moved = {r: 0.0 for r in PR.RULES}
    Ts, Cs, strides, widths, tied, rows = set(), set(), set(), set(), 0, 0
    for k, (samples, C, pad, pad_labels, seed) in enumerate(PR.PARITY):
        lp, tg, il, tl, blank, C = PR.parity_inputs(k)
        assert lp.shape[0] == 3 and (len(set(il.tolist())) == 3 or il[0] < 3) and len(set(tl.tolist())) >= 2 and 0 in tl.tolist() and lp.shape[2] == C + pad and np.isnan(lp[:, :, C:]).all()
        assert tg.shape[1] == max(tl) + pad_labels and lp.shape[1] == max(il) + 2
        Ts.add(int(il[0])); Cs.add(C); strides.add(pad); widths.add(int(tg.shape[1]))
        if il[0] > 65:
            continue
        ll, sub, ins = PR.neighbours_batch(lp, tg, il, tl, blank, C)
        assert np.isfinite(ll[0]) and np.isfinite(ll[1]) and ll[2] == -np.inf and il[2] < tl[2]
        T = il.astype(np.float64)[:, None, None]
        tol = [PR.llr_tol(np.broadcast_to(T, v.shape), v, PR.STEP_ERROR_CAP) for v in (sub, ins)]
        for r in PR.RULES:
            _, sub2, ins2 = PR.neighbours_batch(lp, tg, il, tl, blank, C, off=(r,))
            for a, b, t in ((sub, sub2, tol[0]), (ins, ins2, tol[1])):
                f = np.isfinite(a) & np.isfinite(b)
                if f.any():
                    moved[r] = max(moved[r], float((np.abs(a[f] - b[f]) / t[f]).max()))
        for v, own, t in ((sub, tg.astype(np.int64), tol[0]), (ins, np.full(ins.shape[:2], blank), tol[1])):
            flat = v.reshape(-1, C)
            live = ~np.isnan(flat).any(1)
            tied += int(PR.tied_rows(flat, own.reshape(-1), t.reshape(-1, C).max(1))[live].sum())
            rows += int(live.sum())
    assert all(v > 100.0 for v in moved.values()), moved
    assert Ts == {1, 2, 3, 63, 64, 65, 130, 256} and Cs == {3, 5, 129, 130, 257} and strides == {0, 15}
    assert any(w <= 31 for w in widths) and any(32 <= w <= 63 for w in widths) and any(64 <= w <= 1023 for w in widths) and any(w > 2048 for w in widths)
    for C in Cs:
        assert {p[2] for p in PR.PARITY if p[1] == C} == {0, 15}
    assert rows > 300 and tied <= 0.02 * rows, (tied, rows)


# ---- 3. the long form ---------------------------------------------------------------------------------------------------------------
def test_cut_rule_by_hand():
    from lcasr_amd.decoding import posterior as D
    spans = [(2, 4), (10, 11), (11, 13), (30, 31), (40, 44)]
    for cut in (PR.cut_pieces, D.cut_pieces):
        assert cut(spans, 50, 100, 100) == [(0, 5, 0, 50)]
        # midpoints behind the tokens: 7, 11, 21, 35, and 50 behind the last
        assert cut(spans, 50, 100, 2) == [(0, 2, 0, 11), (2, 4, 11, 35), (4, 5, 35, 50)]
        assert cut(spans, 50, 21, 100) == [(0, 3, 0, 21), (3, 4, 21, 35), (4, 5, 35, 50)]      # token 3 would end the piece at frame 35 > 21
        assert cut(spans, 50, 20, 100) == [(0, 2, 0, 11), (2, 3, 11, 21), (3, 4, 21, 35), (4, 5, 35, 50)]
        assert cut(spans, 50, 3, 100) == [(0, 1, 0, 7), (1, 2, 7, 11), (2, 3, 11, 21), (3, 4, 21, 35), (4, 5, 35, 50)]   # a piece takes its first token whatever its length
        assert cut([], 9, 4, 4) == [(0, 0, 0, 9)]
        assert cut([(0, 9)], 9, 4, 4) == [(0, 1, 0, 9)]


def pinned_recording(rng, groups, C):
    """Scores whose cuts are exact.  groups: label sets, disjoint, none with the blank C - 1.  Group g owns a run of frames: free
    frames that admit the labels of the group but its first and last one, and the blank; in front of them one frame that admits
    the group's first label alone, behind them one that admits its last label alone.  Everything else is -inf.  The transcript
    takes, per group, the first label, labels of the free frames, the last label.  A string that moves a label across the border of
    two groups has no alignment, with or without a cut there, so cutting between the groups changes no ratio."""
    blank = C - 1
    rows, tokens, spans = [], [], []
    for labels in groups:
        first, last, inner = labels[0], labels[-1], labels[1:-1]
        f0 = len(rows)
        rows.append(np.where(np.arange(C) == first, rng.normal(), -np.inf))
        tokens.append(first); spans.append((f0, f0 + 1))
        n_inner = 3                                                           # every group has five tokens: a label cap cuts at the groups
        for k in range(n_inner):
            for _ in range(int(rng.integers(2, 5))):
                r = np.full(C, -np.inf)
                r[list(inner) + [blank]] = rng.normal(size=len(inner) + 1)
                rows.append(r)
            tokens.append(int(inner[k % len(inner)])); spans.append((len(rows) - 2, len(rows) - 1))
        rows.append(np.where(np.arange(C) == last, rng.normal(), -np.inf))
        tokens.append(last); spans.append((len(rows) - 1, len(rows)))
    return np.array(rows), tokens, spans, blank


def test_long_form_is_exact_where_the_scores_pin_the_cuts():
    """Frames left of a cut admit only labels of one set and the blank, frames right of it only labels of a disjoint set and the
    blank, everything else is -inf.  That alone does not make the pieces exact: the last token left of a cut could still be
    replaced by a label that the frames right of it emit.  The frame on either side of a cut therefore admits one label only, which
    rules those strings out on both sides (pinned_recording); then the pieces' figures are the whole recording's to 1e-9."""
    rng = np.random.default_rng(21)
    groups = [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9, 10], [11, 12, 13, 14, 15]]
    lp, tokens, spans, blank = pinned_recording(rng, groups, 17)
    n = len(tokens)
    per_group = [sum(1 for t in tokens if t in g) for g in groups]
    whole = PR.long_form(lp, tokens, spans, blank, 10 ** 6, 10 ** 6)
    assert PR.cut_pieces(spans, len(lp), 10 ** 6, 10 ** 6) == [(0, n, 0, len(lp))]
    ll, sub, ins = PR.neighbours_bridge(lp, np.array(tokens), blank)
    assert np.isfinite(ll) and np.isfinite(sub).sum() > 2 * n and whole[0].shape == (n,) and whole[3].shape == (n + 1,)
    assert (whole[0] < 1 - 1e-6).sum() >= n // 2                              # the free frames leave real competition
    # cuts in front of the first token of the second and of the third group: by the label count of the longest group ...
    pieces = PR.cut_pieces(spans, len(lp), 10 ** 6, max(per_group))
    bounds = np.cumsum([0] + per_group)
    if [p[:2] for p in pieces] != [(int(a), int(b)) for a, b in zip(bounds[:-1], bounds[1:])]:
        pytest.fail(f'the cuts {pieces} are not the groups {bounds.tolist()}: change the recording, not the rule')
    assert [p[2] for p in pieces[1:]] == [spans[b][0] for b in bounds[1:-1]]     # ... at the first frame of each group
    cut = PR.long_form(lp, tokens, spans, blank, 10 ** 6, max(per_group))
    for a, b, what in zip(whole, cut, ('post', 'alt', 'alt_post', 'gap_post', 'gap_alt', 'gap_alt_post')):
        assert close(a, b, 1e-9), what
    # and a recording without such borders is an approximation: the same cuts move some figure
    free = np.log(rng.dirichlet(np.ones(17), size=len(lp)))
    assert not close(PR.long_form(free, tokens, spans, blank, 10 ** 6, 10 ** 6)[0], PR.long_form(free, tokens, spans, blank, 10 ** 6, max(per_group))[0], 1e-9)


# ---- 4. host side of the unit -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from lcasr_amd.hip import post
    return post.load()


def _declared():
    src = open(os.path.join(ROOT, 'include', HEADER)).read()
    return sorted(set(re.findall(r'\b(sconf_[a-z0-9_]+) ?\(', re.sub(r'/\*.*?\*/', '', src, flags=re.S))))


def test_binding_is_the_header_and_the_core_does_not_name_it(lib):
    from lcasr_amd.hip import _lib, post
    funcs, enums = header_abi(HEADER, 'sconf_post_')
    assert sorted(funcs) == _declared() and set(funcs) == NAMES and not enums
    assert_binding_is_header(funcs, post.PROTOTYPES, post.PLAIN, 'hip/post.py')
    assert not any(n in _lib.PROTOTYPES or n in _lib.PLAIN for n in NAMES)
    for n in NAMES:
        assert hasattr(lib, n) and n in _lib.bound()
    for path in (os.path.join(ROOT, 'long-context-asr_amd', 'hip', '_lib.py'), os.path.join(ROOT, 'include', 'sconf.h'),
                 os.path.join(ROOT, 'long-context-asr_amd', 'hip', '__init__.py')):
        assert 'sconf_post_' not in open(path).read(), path
    hip = os.path.join(ROOT, 'long-context-asr_amd', 'hip')
    for f in sorted(os.listdir(hip)):                                        # nothing under hip/ imports this unit
        if f.endswith('.py') and f != 'post.py':
            assert not re.search(r'import post\b|from \.post\b|from \. import [^\n]*\bpost\b', open(os.path.join(hip, f)).read()), f
    assert lib.sconf_version() == 220


def test_queries_answer_on_the_host(lib):
    from lcasr_amd.hip import post
    cap = post.max_labels()
    assert cap >= 2047 and 2 * (2 * cap + 1 + 4) * 8 <= 160 * 1024            # two f64 rows of the lattice fit the LDS
    e = post.step_error()
    assert 0.0 < e <= PR.STEP_ERROR_CAP
    assert lib.sconf_post_step_error(None) != 0 and b'null' in lib.sconf_last_error()
    ws = lib.sconf_post_workspace
    for B, N, S in ((0, 5, 3), (1, 0, 0), (1, 1, 0), (3, 130, 7), (8, 2048, 600), (2, 9, cap)):
        assert ws(B, N, S) == post.workspace_bytes(B, N, S) == 16 * B * N * (2 * S + 1)
    for bad in ((-1, 5, 3), (1, -5, 3), (1, 5, -1), (1, 5, cap + 1), (2 ** 31, 5, 3), (2 ** 30, 2 ** 30, cap)):
        assert ws(*bad) == -1
    with pytest.raises(ValueError, match='at most'):
        post.workspace_bytes(1, 5, cap + 1)


def test_refusals_launch_nothing(lib):
    """Every refusal happens before a kernel is enqueued, so none needs a GPU: the pointers are host addresses that are never read."""
    one, err, cap = ctypes.c_void_p(16), lib.sconf_last_error, lib.sconf_post_max_labels()

    def lattice(lp=one, tg=one, il=one, tl=one, B=2, N=9, C=5, stride=5, Smax=3, blank=4, ws=one, ws_bytes=1 << 40, ll=one):
        return lib.sconf_post_lattice(lp, tg, il, tl, B, N, C, stride, Smax, blank, ws, ws_bytes, ll, None)

    def neighbours(lp=one, tg=one, il=one, tl=one, B=2, N=9, C=5, stride=5, Smax=3, blank=4, ws=one, ws_bytes=1 << 40, ll=one, sub=one, ins=one):
        return lib.sconf_post_neighbours(lp, tg, il, tl, B, N, C, stride, Smax, blank, ws, ws_bytes, ll, sub, ins, None)

    def slots(sub=one, ins=one, tg=one, B=2, C=5, Smax=3, blank=4, post=one, alt=one, alt_post=one, gp=one, ga=one, gap=one):
        return lib.sconf_post_slots(sub, ins, tg, B, C, Smax, blank, post, alt, alt_post, gp, ga, gap, None)

    for fn in (lattice, neighbours):
        assert fn(B=0) == 0                                                   # no samples: nothing to launch
        assert fn(Smax=cap + 1) != 0 and b'Smax' in err()
        assert fn(Smax=-1) != 0 and b'Smax' in err()
        assert fn(C=1) != 0 and b'classes' in err()
        assert fn(blank=5) != 0 and b'blank' in err()
        assert fn(blank=-1) != 0 and b'blank' in err()
        assert fn(stride=4) != 0 and b'stride' in err()
        assert fn(B=-1) != 0 and b'out of range' in err()
        assert fn(ws_bytes=16 * 2 * 9 * 7 - 1) != 0 and b'workspace' in err()
        assert fn(ws=None) != 0 and b'workspace' in err()
        assert fn(ws=ctypes.c_void_p(24)) != 0 and b'aligned' in err()
        for null in ('lp', 'tg', 'il', 'tl', 'll'):
            assert fn(**{null: None}) != 0 and b'null' in err(), null
    assert neighbours(sub=None) != 0 and b'null' in err()
    assert neighbours(ins=None) != 0 and b'null' in err()
    assert slots(B=0) == 0
    assert slots(Smax=cap + 1) != 0 and b'Smax' in err()
    assert slots(C=1) != 0 and b'classes' in err()
    assert slots(blank=5) != 0 and b'blank' in err()
    for null in ('sub', 'ins', 'tg', 'post', 'alt', 'alt_post', 'gp', 'ga', 'gap'):
        assert slots(**{null: None}) != 0 and b'null' in err(), null


def test_a_cpu_tensor_is_refused_by_the_product_path():
    from lcasr_amd.decoding import posterior as D
    from lcasr_amd.hip import post
    lp, tg, n = torch.zeros(1, 4, 5), torch.ones(1, 2, dtype=torch.int32), torch.tensor([2], dtype=torch.int32)
    with pytest.raises(RuntimeError, match='GPU'):
        post.lattice(lp, tg, torch.tensor([4], dtype=torch.int32), n, 4)
    with pytest.raises(RuntimeError, match='GPU'):
        post.neighbours(lp, tg, torch.tensor([4], dtype=torch.int32), n, 4, post.Lattice(torch.zeros(1, dtype=torch.float64), torch.zeros(0, dtype=torch.uint8)))
    with pytest.raises(RuntimeError, match='GPU'):
        post.slots(torch.zeros(1, 2, 5), torch.zeros(1, 3, 5), tg, 4)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='GPU'):
            D.posterior_confidence(lp[0], [1, 2], 4)


# ---- 5. the Python surface, with the restatements in the kernels' place -------------------------------------------------------------
@pytest.fixture
def emulated(monkeypatch):
    """lcasr_amd.hip.post's three ops, and the confidence and calibration ops the callers in eval.run use beside them, replaced by
    the numpy restatements: host logic without a GPU.  The host-only queries stay the library's."""
    import __graft_entry__ as g
    g.build()
    import calib_refs as AR
    import confid_refs as CR
    from lcasr_amd.decoding import calibration as K
    from lcasr_amd.decoding import confidence as F
    from lcasr_amd.decoding import posterior as D
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    monkeypatch.setattr(D.post_kernels, 'lattice', PR.op_lattice)
    monkeypatch.setattr(D.post_kernels, 'neighbours', PR.op_neighbours)
    monkeypatch.setattr(D.post_kernels, 'slots', PR.op_slots)
    monkeypatch.setattr(K.calib_kernels, 'edit_align', AR.op_edit_align)
    monkeypatch.setattr(K.calib_kernels, 'frames_sweep', AR.op_frames_sweep)
    monkeypatch.setattr(F.confid_kernels, 'frames', CR.op_frames)
    monkeypatch.setattr(F.confid_kernels, 'runs', CR.op_runs)
    monkeypatch.setattr(F.confid_kernels, 'aggregate', CR.op_aggregate)
    return D


def test_the_tensor_functions(emulated):
    D = emulated
    rng = np.random.default_rng(31)
    lp, y, blank = random_case(rng, T=9, L=3, C=6, holes=0.0)
    lp32 = lp.astype(np.float32)
    ll, sub, ins = PR.neighbours_bridge(lp32.astype(np.float64), y, blank)
    s = D.neighbour_scores(torch.from_numpy(lp32), [int(v) for v in y], blank)
    assert s.loglik.shape == () and float(s.loglik) == pytest.approx(ll, abs=1e-12)
    assert s.sub_llr.dtype == torch.float32 and close(s.sub_llr.numpy(), sub.astype(np.float32), 0.0) and close(s.ins_llr.numpy(), ins.astype(np.float32), 0.0)
    # a batch, ragged in both lengths, from lists of lists; the padded slots and gaps are NaN
    sb = D.neighbour_scores(torch.from_numpy(np.stack([lp32, lp32])), [[int(v) for v in y], [int(y[0])]], blank, input_lengths=[9, 4])
    assert tuple(sb.sub_llr.shape) == (2, 3, 6) and tuple(sb.ins_llr.shape) == (2, 4, 6) and torch.equal(sb.sub_llr[0], s.sub_llr)
    ll1, sub1, ins1 = PR.neighbours_bridge(lp32[:4].astype(np.float64), y[:1], blank)
    assert close(sb.sub_llr[1, :1].numpy(), sub1.astype(np.float32), 0.0) and bool(torch.isnan(sb.sub_llr[1, 1:]).all()) and bool(torch.isnan(sb.ins_llr[1, 2:]).all())
    # the temperature scales the scores first
    st = D.neighbour_scores(torch.from_numpy(lp32), torch.tensor(y, dtype=torch.int64), blank, temperature=2.0)
    _, sub_t, _ = PR.neighbours_bridge((lp32 * np.float32(0.5)).astype(np.float64), y, blank)
    assert close(st.sub_llr.numpy(), sub_t.astype(np.float32), 0.0) and not close(st.sub_llr.numpy(), s.sub_llr.numpy(), 1e-3)
    with pytest.raises(ValueError, match='temperature'):
        D.neighbour_scores(torch.from_numpy(lp32), [1], blank, temperature=0.0)
    pc = D.posterior_confidence(torch.from_numpy(lp32), [int(v) for v in y], blank)
    want = PR.slots(sub.astype(np.float32)[None], ins.astype(np.float32)[None], y[None], blank)
    for got, w in zip(pc, want):
        assert close(got.numpy(), w[0].astype(got.numpy().dtype), 0.0)
    assert pc.token_posterior.dtype == torch.float32 and pc.alternative.dtype == torch.int32 and tuple(pc.gap_posterior.shape) == (4,)
    p, idx = D.alternatives(s, 3)
    soft = torch.softmax(s.sub_llr, -1)
    assert tuple(p.shape) == (3, 3) and torch.equal(p, soft.gather(-1, idx)) and bool((p[:, 0] >= p[:, 1]).all())
    assert all(int(idx[i, 0]) in (int(y[i]), int(pc.alternative[i])) for i in range(3))
    with pytest.raises(ValueError, match='k = 7'):
        D.alternatives(s, 7)
    # the long form: the product function against the float64 restatement of the same cuts, and its argument checks
    lp, tokens, spans, blank = pinned_recording(np.random.default_rng(32), [[0, 1, 2, 3], [4, 5, 6, 7]], 9)
    lp32 = lp.astype(np.float32)
    for max_frames, max_labels in ((2048, None), (2048, 3), (7, None)):
        got = D.posterior_confidence_long(torch.from_numpy(lp32), tokens, spans, blank, max_frames=max_frames, max_labels=max_labels)
        want = PR.long_form(lp32.astype(np.float64), tokens, spans, blank, max_frames, max_labels or 10 ** 6)
        for g, w, tol in zip(got, want, (1e-6, 0, 1e-6, 1e-6, 0, 1e-6)):
            assert tuple(g.shape) == w.shape and close(g.numpy(), w, tol)
    assert len(PR.cut_pieces(spans, len(lp), 7, 10 ** 6)) > 2
    empty = D.posterior_confidence_long(torch.from_numpy(lp32), [], [], blank)
    assert tuple(empty.token_posterior.shape) == (0,) and tuple(empty.gap_posterior.shape) == (1,)
    with pytest.raises(ValueError, match='spans'):
        D.posterior_confidence_long(torch.from_numpy(lp32), tokens, spans[:-1], blank)
    with pytest.raises(ValueError, match='span 1'):
        D.posterior_confidence_long(torch.from_numpy(lp32), tokens[:2], [(3, 5), (4, 6)], blank)
    with pytest.raises(ValueError, match='max_labels'):
        D.posterior_confidence_long(torch.from_numpy(lp32), tokens, spans, blank, max_labels=0)


class IdTok:
    """Every token is a word: id i is spelt 't<i>'."""
    def __init__(self, V): self.V = V
    def vocab_size(self): return self.V
    def decode(self, ids): return ' '.join(f't{int(i)}' for i in ids)
    def encode(self, text): return [int(w[1:]) for w in text.split()]


def test_transcribe_detail_and_calibrate_on_the_tiny_model(emulated_ops, emulated, monkeypatch):
    import audio_refs as AUD
    import confid_refs as CR
    from lcasr_amd.decoding.calibration import calibration_metrics
    from lcasr_amd.eval import run as R
    from lcasr_amd.utils import audio_tools
    monkeypatch.setattr(audio_tools.audio, 'melspec', AUD.melspec)
    E.attach(monkeypatch, emulated_ops)
    fx = load_golden('infer_tiny')
    m = build_from_fixture(fx).eval()
    tok = IdTok(int(fx['cfg.vocab_size']))
    blank = m.decoder.num_classes - 1
    wave = AUD.test_signal(3 * 16000, seed=3)
    d0 = R.transcribe_detail(m, wave, tok, 128, 32)
    assert R.transcribe_detail(m, wave, tok, 128, 32, posterior=False) == d0 and set(d0) == {'text', 'tokens', 'token_confidence', 'words'}
    d1 = R.transcribe_detail(m, wave, tok, 128, 32, posterior=True)
    assert set(d1) == set(d0) | {'token_posterior', 'token_alternative'}
    assert {k: d1[k] for k in ('text', 'tokens', 'token_confidence')} == {k: d0[k] for k in ('text', 'tokens', 'token_confidence')}
    assert [{k: v for k, v in w.items() if k != 'posterior'} for w in d1['words']] == d0['words'] and all('posterior' in w for w in d1['words'])
    n = len(d0['tokens'])
    assert n >= 3 and len(d1['token_posterior']) == n == len(d1['token_alternative'])
    # the same figures from the restatements, step by step: the logits, the greedy spans, the long form
    spec = audio_tools.to_spectogram(wave[None])
    logits = R.moving_average_eval(R._Args(), m, spec, 128, 32, tok, use_tqdm=False, return_numpy=False)
    (want,), _ = CR.greedy(logits.float().numpy()[None], blank, 'tsallis', 'exp', 1 / 3, 'min', True)
    assert want[0] == d0['tokens']
    spans = [s[:2] for s in want[1]]
    post, alt, alt_post, _, _, _ = PR.long_form(logits.float().numpy().astype(np.float64), d0['tokens'], spans, blank, 2048, 10 ** 6)
    assert d1['token_posterior'] == pytest.approx(post.tolist(), abs=1e-6) and all(0 < p <= 1 for p in d1['token_posterior'])
    assert [a['token'] for a in d1['token_alternative']] == [None if a == blank else int(a) for a in alt]
    assert [a['posterior'] for a in d1['token_alternative']] == pytest.approx(alt_post.tolist(), abs=1e-6)
    assert [w['posterior'] for w in d1['words']] == pytest.approx(post.tolist(), abs=1e-6)             # every token is a word here

    recs = []
    for seed in (3, 4):
        spec = audio_tools.to_spectogram(AUD.test_signal(3 * 16000, seed=seed)[None])
        logits = R.moving_average_eval(R._Args(), m, spec, 128, 32, tok, use_tqdm=False, return_numpy=False)
        greedy = [int(c) for c in logits.argmax(-1).tolist()]
        runs = [c for i, c in enumerate(greedy) if c != blank and (i == 0 or greedy[i - 1] != c)]
        gold = [r for k, r in enumerate(runs) if k % 5 != 2]
        gold = [(r + 1) % blank if k % 4 == 1 else r for k, r in enumerate(gold)] + [1, 2]
        recs.append((f'rec{seed}', spec, tok.decode(gold).upper(), logits))
    temps = [0.5, 1.0, 2.0]
    c0 = R.calibrate(m, [r[:3] for r in recs], tok, 128, 32, temperatures=temps)
    assert set(c0) == {'temperatures', 'metrics', 'temperature', 'labels', 'confusion_pairs', 'words'}
    assert _same_with_nan(R.calibrate(m, [r[:3] for r in recs], tok, 128, 32, temperatures=temps, posterior=False), c0)
    c1 = R.calibrate(m, [r[:3] for r in recs], tok, 128, 32, temperatures=temps, posterior=True)
    assert set(c1) == set(c0) | {'posterior_metrics'} and _same_with_nan({k: v for k, v in c1.items() if k != 'posterior_metrics'}, c0)
    pooled = []
    for _, _, _, logits in recs:
        (want,), _ = CR.greedy(logits.float().numpy()[None], blank, 'tsallis', 'exp', 1 / 3, 'min', True)
        pooled += PR.long_form(logits.float().numpy().astype(np.float64), want[0], [s[:2] for s in want[1]], blank, 2048, 10 ** 6)[0].tolist()
    assert len(pooled) == c0['words']
    want = calibration_metrics(torch.tensor(pooled, dtype=torch.float32), c0['labels'])
    assert set(c1['posterior_metrics']) == set(want) == set(c0['metrics'][0])
    for key, v in c1['posterior_metrics'].items():
        assert v == pytest.approx(want[key], abs=1e-5, nan_ok=True), key


def _same_with_nan(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(_same_with_nan(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same_with_nan(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    return a == b
