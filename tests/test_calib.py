"""CPU tests of the calibration unit: the numpy restatements (tests/calib_refs.py) against an exhaustive enumeration and against each
other, the tie rule by hand, the host side of the fifteenth ABI unit (include/sconf_calib.h: header against binding against the
library's exports, queries, refusals), the Python surface (eval/wer.py's alignment listing, decoding/calibration.py's metrics and
temperature fit, the temperature keyword of decoding/confidence.py), and eval.run.calibrate on the tiny fixture model with the
binding replaced by the restatements."""
import ctypes
import itertools
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import calib_refs as AR
import confid_refs as CR
import eval_refs as E
from cabi_header import assert_binding_is_header, header_abi
from common_model import build_from_fixture
from conftest import ROOT, load_golden

HEADER = 'sconf_calib.h'
NAMES = {'sconf_edit_align_strip_cols', 'sconf_edit_align_pass_cols', 'sconf_edit_align_block_rows', 'sconf_edit_align_cells_per_word',
         'sconf_edit_align_tile_bytes', 'sconf_edit_align_max_len', 'sconf_edit_align_pair_bytes', 'sconf_edit_align',
         'sconf_calib_max_temps', 'sconf_calib_frames_sweep'}
NAN = math.nan


@pytest.fixture
def emulated(monkeypatch):
    """The binding layers (lcasr_amd.hip.calib's two ops, lcasr_amd.hip.confid's three) replaced by the numpy restatements: host
    logic without a GPU.  The host-only queries stay the library's."""
    import __graft_entry__ as g
    g.build()
    from lcasr_amd.decoding import calibration as D
    from lcasr_amd.decoding import confidence as F
    # the surface moves CPU input to the device wherever one is present (confidence._on_device, calibration, wer._device, the
    # decoders); the restatements are numpy, so the move is pinned to the CPU: the same run with and without a GPU
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    monkeypatch.setattr(D.calib_kernels, 'edit_align', AR.op_edit_align)
    monkeypatch.setattr(D.calib_kernels, 'frames_sweep', AR.op_frames_sweep)
    monkeypatch.setattr(F.confid_kernels, 'frames', CR.op_frames)
    monkeypatch.setattr(F.confid_kernels, 'runs', CR.op_runs)
    monkeypatch.setattr(F.confid_kernels, 'aggregate', CR.op_aggregate)
    return D


# ---- 1. the yardstick -----------------------------------------------------------------------------------------------------------
def _same(a, b):
    return all(np.array_equal(p, q) and p.dtype == q.dtype for p, q in zip(a, b))


def test_plain_form_against_every_alignment_of_short_pairs():
    """Every pair of sequences of length <= 4 over 2 symbols: the cell-by-cell form gives the smallest (errors, substitutions) of
    all alignments, and of the alignments that reach it the one the backtrace's order names; the fast form agrees."""
    n = 0
    for H, R in itertools.product(range(5), repeat=2):
        for h in itertools.product((0, 1), repeat=H):
            for r in itertools.product((0, 1), repeat=R):
                want = AR.align_brute(h, r)
                assert _same(AR.align_plain(h, r), want) and _same(AR.align_fast(h, r), want), (h, r)
                n += 1
    assert n == 31 * 31


def test_fast_form_against_plain_form_on_random_pairs():
    rng = np.random.default_rng(0)
    with_ties = 0
    for _ in range(80):
        H, R = (int(v) for v in rng.integers(0, 61, 2))
        vocab = int(rng.choice([2, 3, 10, 1000]))
        h, r = rng.integers(0, vocab, H), rng.integers(0, vocab, R)
        a, b = AR.align_plain(h, r), AR.align_fast(h, r)
        assert _same(a, b), (h, r)
        e, s, d, i = (int(v) for v in a[2])
        assert e == s + d + i and i - d == H - R and (a[0] >= 0).sum() == (a[1] >= 0).sum() == H - i == R - d
        assert np.array_equal(E.edit_counts(*[torch.from_numpy(np.asarray(v)) for v in
                                                        (h.astype(np.int32), [0, H], r.astype(np.int32), [0, R])])[0].numpy(), a[2])
        with_ties += vocab == 2
    assert with_ties > 5


def test_the_tie_rule_by_hand():
    a, b, c = 0, 1, 2
    h2r, r2h, counts = AR.align_plain([a, b], [b, c])                       # insertion, hit, deletion: not two substitutions
    assert h2r.tolist() == [-1, 0] and r2h.tolist() == [1, -1] and counts.tolist() == [2, 0, 1, 1]
    h2r, r2h, counts = AR.align_plain([a, a, a], [a, a])                    # the backtrace takes diagonals first: the FIRST a is inserted
    assert h2r.tolist() == [-1, 0, 1] and r2h.tolist() == [1, 2] and counts.tolist() == [1, 0, 0, 1]
    h2r, r2h, counts = AR.align_plain([a, a], [a, a, a])
    assert h2r.tolist() == [1, 2] and r2h.tolist() == [-1, 0, 1] and counts.tolist() == [1, 0, 1, 0]
    h2r, r2h, counts = AR.align_plain([], [a, b])
    assert h2r.tolist() == [] and r2h.tolist() == [-1, -1] and counts.tolist() == [2, 0, 2, 0]
    h2r, r2h, counts = AR.align_plain([a, b, c], [])
    assert h2r.tolist() == [-1, -1, -1] and r2h.tolist() == [] and counts.tolist() == [3, 0, 0, 3]
    h2r, r2h, counts = AR.align_plain([], [])
    assert h2r.tolist() == [] and r2h.tolist() == [] and counts.tolist() == [0, 0, 0, 0]
    h2r, r2h, counts = AR.align_plain([a, b, c, a], [a, b, c, a])
    assert h2r.tolist() == [0, 1, 2, 3] == r2h.tolist() and counts.tolist() == [0, 0, 0, 0]
    h2r, r2h, counts = AR.align_plain([a, b], [c, c])                       # one substitution costs what an insertion costs, a pair of them less than both
    assert h2r.tolist() == [0, 1] and counts.tolist() == [2, 2, 0, 0]


def test_batch_counts_are_the_edit_counts_and_short_slices_are_refused():
    rng = np.random.default_rng(3)
    pairs = [(rng.integers(0, 4, int(rng.integers(0, 40))).astype(np.int32), rng.integers(0, 4, int(rng.integers(0, 40))).astype(np.int32))
             for _ in range(12)]
    hyp, ref = np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])
    ho, ro = np.cumsum([0] + [len(p[0]) for p in pairs]), np.cumsum([0] + [len(p[1]) for p in pairs])
    h2r, r2h, counts = AR.align_batch(hyp, ho, ref, ro)
    want = E.edit_counts(torch.from_numpy(hyp), torch.from_numpy(ho), torch.from_numpy(ref), torch.from_numpy(ro))
    assert np.array_equal(counts, want.numpy()) and counts.dtype == np.int64
    sizes = [AR.pair_bytes(len(h), len(r)) for h, r in pairs]
    k = next(p for p, n in enumerate(sizes) if n > 0)
    short = list(sizes)
    short[k] -= 16
    a, b, c = AR.align_batch(hyp, ho, ref, ro, np.cumsum([0] + short))
    assert (c[k] == -1).all() and (a[ho[k]:ho[k + 1]] == -1).all() and (b[ro[k]:ro[k + 1]] == -1).all()
    keep = np.arange(len(pairs)) != k
    assert np.array_equal(c[keep], counts[keep]) and np.array_equal(a[:ho[k]], h2r[:ho[k]]) and np.array_equal(a[ho[k + 1]:], h2r[ho[k + 1]:])


def test_sweep_restatements():
    """The column at temperature 1 is confid_refs.frames; a lower temperature sharpens every measure; float32 is near float64."""
    x = CR.planted()[0][:30]
    for method, norm in CR.MEASURES:
        idx, conf = AR.sweep(x, [1.0, 2.0, 0.5, math.inf, 0.0, -1.0, NAN], None, method, norm, 1 / 3)
        i1, c1 = CR.frames(x, None, method, norm, 1 / 3)
        assert np.array_equal(idx, i1) and np.array_equal(conf[0], c1) and np.isnan(conf[3:]).all()
        assert (conf[1] >= conf[0] - 1e-12).all() and (conf[0] >= conf[2] - 1e-12).all() and (conf[1] > conf[2]).any()
        c32 = AR.sweep32(x, [1.0, 2.0, 0.5], None, method, norm, 1 / 3)
        assert c32.dtype == np.float32 and float(np.abs(c32 - conf[:3]).max()) < 1e-5
        tol, d32 = AR.sweep_tolerance(x, 2.0, None, method, norm, 1 / 3)
        assert tol == 4 * d32 + 1e-6 and d32 == float(np.abs(c32[1].astype(np.float64) - conf[1]).max())
    bad = x.copy()
    bad[3, 2] = NAN
    idx, conf = AR.sweep(bad, [1.0, 2.0])
    assert idx[3] == -1 and np.isnan(conf[:, 3]).all() and not np.isnan(np.delete(conf, 3, axis=1)).any()


# ---- 2. host side of the unit -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from lcasr_amd.hip import calib
    return calib.load()


def _declared():
    src = open(os.path.join(ROOT, 'include', HEADER)).read()
    return sorted(set(re.findall(r'\b(sconf_[a-z0-9_]+) ?\(', re.sub(r'/\*.*?\*/', '', src, flags=re.S))))


def test_binding_is_the_header_and_the_core_does_not_name_it(lib):
    from lcasr_amd.hip import _lib, calib, confid
    funcs, enums = header_abi(HEADER, 'sconf_')
    assert sorted(funcs) == _declared() and set(funcs) == NAMES and not enums
    assert all(n.startswith(('sconf_edit_align', 'sconf_calib_')) for n in funcs)
    assert_binding_is_header(funcs, calib.PROTOTYPES, calib.PLAIN, 'hip/calib.py')
    assert not any(n in _lib.PROTOTYPES or n in _lib.PLAIN for n in NAMES)
    for n in NAMES:
        assert hasattr(lib, n) and n in _lib.bound()
    for path in (os.path.join(ROOT, 'long-context-asr_amd', 'hip', '_lib.py'), os.path.join(ROOT, 'include', 'sconf.h'),
                 os.path.join(ROOT, 'long-context-asr_amd', 'hip', '__init__.py')):
        text = open(path).read()
        assert 'sconf_edit_align' not in text and 'sconf_calib_' not in text and not re.search(r'\bcalib\b', text), path
    hip = os.path.join(ROOT, 'long-context-asr_amd', 'hip')
    for f in sorted(os.listdir(hip)):                                        # nothing under hip/ imports this unit
        if f.endswith('.py') and f != 'calib.py':
            assert not re.search(r'import calib\b|from \.calib\b|from \. import [^\n]*\bcalib\b', open(os.path.join(hip, f)).read()), f
    assert (calib.METHOD, calib.NORM) == (confid.METHOD, confid.NORM)        # the sweep takes sconf_confid.h's enumerators
    assert lib.sconf_version() == 220


def test_queries_answer_on_the_host(lib):
    from lcasr_amd.hip import calib
    strip, pas, rows, cpw = calib.strip_cols(), calib.pass_cols(), calib.block_rows(), calib.cells_per_word()
    assert (strip, pas, rows, cpw) == (AR.STRIP, AR.PASS, AR.ROWS, AR.CPL) and lib.sconf_edit_align_tile_bytes() == AR.TILE_BYTES
    assert pas % strip == 0 and strip % cpw == 0 and 16 % cpw == 0
    assert calib.max_len() == AR.MAX_LEN >= 32767 and calib.max_temps() >= 16
    pb = lib.sconf_edit_align_pair_bytes
    cap = calib.max_len()
    for H, R in ((0, 0), (0, 9), (9, 0), (1, 1), (rows, strip), (rows + 1, strip), (rows, strip + 1), (300, pas), (300, pas + 1), (10000, 10000),
                 (30000, 30000), (cap, cap)):
        assert pb(H, R) == AR.pair_bytes(H, R) == calib.pair_bytes(H, R) and pb(H, R) % 16 == 0
    assert pb(1, 1) == AR.TILE_BYTES and pb(300, pas + 1) - pb(300, pas) == 2 * AR.TILE_BYTES + 8 * 301 + 8
    for a, b in itertools.product((1, 7, rows - 1, rows, rows + 1, 3000), (1, 9, strip, strip + 1, pas, pas + 1, 5000)):     # monotone in both
        assert pb(a, b) <= pb(a + 1, b) and pb(a, b) <= pb(a, b + 1)
    for bad in ((-1, 5), (5, -1), (cap + 1, 5), (5, cap + 1)):
        assert pb(*bad) == -1
    with pytest.raises(ValueError, match='at most'):
        calib.pair_bytes(cap + 1, 3)
    assert calib.workspace_offsets([3, 0, rows + 1], [4, 5, pas + 1]) == [0, pb(3, 4), pb(3, 4), pb(3, 4) + pb(rows + 1, pas + 1)]


def test_refusals_launch_nothing(lib):
    """Every refusal happens before a kernel is enqueued, so none needs a GPU: the pointers are host addresses that are never read."""
    one, err = ctypes.c_void_p(16), lib.sconf_last_error
    assert lib.sconf_edit_align(None, None, None, None, 0, None, None, None, None, None, None) == 0           # P == 0 launches nothing
    assert lib.sconf_edit_align(one, one, one, one, -1, one, one, one, one, one, None) != 0 and b'out of range' in err()
    for null in range(4):
        args = [one, one, one, one, 2, one, one, one, one, one, None]
        args[(1, 3, 7, 9)[null]] = None
        assert lib.sconf_edit_align(*args) != 0 and b'null' in err()
    assert lib.sconf_edit_align(one, one, one, one, 2, one, one, one, ctypes.c_void_p(24), one, None) != 0 and b'aligned' in err()

    def sweep(x=one, it=one, idx=one, conf=one, M=4, classes=8, stride=8, method=2, norm=1, alpha=0.5, K=3):
        return lib.sconf_calib_frames_sweep(x, M, classes, stride, method, norm, alpha, it, K, idx, conf, None)

    for null in ('x', 'it', 'idx', 'conf'):
        assert sweep(**{null: None}) != 0 and b'null' in err(), null
    assert sweep(K=0) != 0 and b'temperatures' in err()
    assert sweep(K=lib.sconf_calib_max_temps() + 1) != 0 and b'temperatures' in err()
    assert sweep(classes=1) != 0 and b'classes' in err()
    assert sweep(stride=7) != 0 and b'stride' in err()
    assert sweep(method=4) != 0 and b'method' in err()
    assert sweep(norm=2) != 0 and b'norm' in err()
    assert sweep(method=0, norm=1) != 0 and b'max_prob' in err()
    assert sweep(alpha=5.0) != 0 and b'alpha' in err()
    assert sweep(M=-1) != 0 and b'M=' in err()
    assert sweep(M=0) == 0                                                    # no rows: nothing to launch


# ---- 3. the Python surface --------------------------------------------------------------------------------------------------------
def test_edit_alignment_of_ids_and_the_listing(emulated):
    from lcasr_amd.eval import wer as W
    out = W.edit_alignment_of_ids([[5, 6], [], [1, 2, 3]], [[6, 7], [4], [1, 2, 3]])
    assert out == [([-1, 0], [1, -1], [2, 0, 1, 1]), ([], [-1], [1, 0, 1, 0]), ([0, 1, 2], [0, 1, 2], [0, 0, 0, 0])]
    assert W.edit_alignment_of_ids([], []) == []
    with pytest.raises(ValueError, match='as many'):
        W.edit_alignment_of_ids([[1]], [])
    hyp, ref = 'the cat sat on on the mat', 'a cat sat on the big mat'
    (ops,) = W.word_error_alignment([hyp], [ref])
    assert [(o['op'], o['hyp'], o['ref'], o['hyp_index'], o['ref_index']) for o in ops] == [
        ('sub', 'the', 'a', 0, 0), ('hit', 'cat', 'cat', 1, 1), ('hit', 'sat', 'sat', 2, 2), ('ins', 'on', None, 3, None),
        ('hit', 'on', 'on', 4, 3), ('hit', 'the', 'the', 5, 4), ('del', None, 'big', None, 5), ('hit', 'mat', 'mat', 6, 6)]
    wer, words, ins, dele, sub = E_detail(hyp, ref)
    assert (sum(o['op'] == 'ins' for o in ops), sum(o['op'] == 'del' for o in ops), sum(o['op'] == 'sub' for o in ops)) == \
        (round(ins * words), round(dele * words), round(sub * words))
    both = W.word_error_alignment(['b c', ''], ['a b', 'x y'])
    assert [[o['op'] for o in ops] for ops in both] == [['del', 'hit', 'ins'], ['del', 'del']]
    (tail,) = W.word_error_alignment(['a b c'], ['a'])                      # insertions behind the last reference word
    assert [(o['op'], o['hyp_index']) for o in tail] == [('hit', 0), ('ins', 1), ('ins', 2)]
    (chars,) = W.word_error_alignment([' abd '], ['abcd'], use_cer=True)
    assert [(o['op'], o['hyp'], o['ref']) for o in chars] == [('hit', 'a', 'a'), ('hit', 'b', 'b'), ('del', None, 'c'), ('hit', 'd', 'd')]
    (spaces,) = W.word_error_alignment(['a b'], ['a  b'], use_cer=True)     # inner spaces are tokens, as in word_error_rate_detail
    assert [o['op'] for o in spaces].count('del') == 1 and spaces[1]['ref'] == ' '
    (empty_ref,) = W.word_error_alignment([' x'], [''], use_cer=True)       # an empty reference keeps the hypothesis unstripped
    assert [(o['op'], o['hyp']) for o in empty_ref] == [('ins', ' '), ('ins', 'x')]
    with pytest.raises(ValueError, match='as many'):
        W.word_error_alignment(['a'], [])


def E_detail(hyp, ref):
    """word_error_rate_detail through the CPU restatement of the edit counts."""
    from lcasr_amd import functional as Fn
    from lcasr_amd.eval import wer as W
    saved = Fn.ops
    Fn.ops = types.SimpleNamespace(edit_counts=E.edit_counts)
    try:
        return W.word_error_rate_detail([hyp], [ref])
    finally:
        Fn.ops = saved


def test_confusion_pairs(emulated):
    from lcasr_amd.eval import wer as W
    hyps = ['the cat sat', 'the dog sat', 'a cat', 'the bat sat down']
    refs = ['a cat sat', 'a cat sat', 'a cat', 'a cat sat']
    want = [('a', 'the', 3), ('cat', 'bat', 1), ('cat', 'dog', 1)]
    assert W.confusion_pairs(W.word_error_alignment(hyps, refs)) == want == W.confusion_pairs(hyps, refs)
    assert W.confusion_pairs([]) == [] and W.confusion_pairs(['ab'], ['ax'], use_cer=True) == [('x', 'b', 1)]


def test_calibration_metrics_in_closed_form():
    from lcasr_amd.decoding.calibration import METRICS, calibration_metrics
    m = calibration_metrics([0.9, 0.8, 0.7, 0.2, 0.1], [1, 1, 1, 0, 0])     # perfectly separated
    assert set(m) == set(METRICS) and (m['n'], m['n_nan']) == (5, 0) and m['accuracy'] == 0.6
    assert m['auroc'] == 1.0 and m['aupr'] == pytest.approx(1.0) and m['aupr_errors'] == pytest.approx(1.0) and 0 < m['nce'] < 1
    assert m['ece'] == pytest.approx((abs(1 - 0.9) + abs(1 - 0.8) + abs(1 - 0.7) + 0.2 + 0.1) / 5)            # one sample a bin
    m = calibration_metrics([0.1, 0.2, 0.8, 0.9], [1, 1, 0, 0])             # perfectly wrong
    assert m['auroc'] == 0.0 and m['nce'] < 0
    for c, y in ((0.7, [1, 0, 1, 1]), (0.25, [1, 0, 0, 0, 1, 0, 0, 0])):    # constant confidence
        m = calibration_metrics([c] * len(y), y)
        acc = sum(y) / len(y)
        assert m['auroc'] == 0.5 and m['ece'] == pytest.approx(abs(acc - c)) and m['aupr'] == pytest.approx(acc) and m['aupr_errors'] == pytest.approx(1 - acc)
    m = calibration_metrics([0.75] * 4, [1, 1, 1, 0])                       # the base rate itself: no information, NCE 0
    assert m['nce'] == pytest.approx(0.0, abs=1e-12) and m['ece'] == pytest.approx(0.0, abs=1e-12)
    m = calibration_metrics([1.0, 1.0, 0.0, 0.0], [1, 1, 0, 0])             # certain and right: the clamp keeps NCE just under 1
    assert 1 - 1e-4 < m['nce'] < 1 and m['ece'] == 0.0
    m = calibration_metrics([0.5, 0.5, 0.9, 0.1], [1, 0, 1, 0])             # a tie between a correct and a wrong sample counts a half
    assert m['auroc'] == pytest.approx((1 + 1 + 0.5 + 1) / 4)
    m = calibration_metrics([0.9, NAN, 0.2, NAN, 0.6], [1, 0, 0, 1, 1])     # NaN confidences are dropped and counted
    assert (m['n'], m['n_nan']) == (3, 2) and m['accuracy'] == pytest.approx(2 / 3) and m['auroc'] == 1.0
    for y in ([1, 1, 1], [0, 0, 0]):                                        # one class
        m = calibration_metrics([0.9, 0.5, 0.7], y)
        assert all(math.isnan(m[k]) for k in ('nce', 'auroc', 'aupr', 'aupr_errors')) and m['accuracy'] == y[0]
        assert m['ece'] == pytest.approx(abs(y[0] - 0.7))
    m = calibration_metrics([], [])
    assert m['n'] == 0 and all(math.isnan(m[k]) for k in METRICS if k not in ('n', 'n_nan'))
    rng = np.random.default_rng(0)                                          # against the definitions, pair by pair
    c, y = np.round(rng.random(60), 1), rng.integers(0, 2, 60)
    m = calibration_metrics(torch.from_numpy(c), torch.from_numpy(y), n_bins=4)
    pos, neg = c[y == 1], c[y == 0]
    assert m['auroc'] == pytest.approx(np.mean([(p > q) + 0.5 * (p == q) for p in pos for q in neg]))
    b = np.minimum((c * 4).astype(int), 3)
    assert m['ece'] == pytest.approx(sum(abs(y[b == k].mean() - c[b == k].mean()) * (b == k).sum() for k in range(4) if (b == k).any()) / 60)
    ap = sum((y[c >= t].sum() - y[c > t].sum()) / y.sum() * y[c >= t].mean() for t in np.unique(c))
    assert m['aupr'] == pytest.approx(ap)
    with pytest.raises(ValueError):
        calibration_metrics([0.5], [1, 0])


def test_fit_temperature_and_its_tie_rule():
    from lcasr_amd.decoding.calibration import fit_temperature
    nce = lambda *v: [{'nce': x} for x in v]
    assert fit_temperature(None, None, [0.5, 1.0, 2.0], metrics=nce(0.1, 0.3, 0.2)) == 1.0
    assert fit_temperature(None, None, [0.5, 1.0, 2.0], metrics=nce(0.4, 0.3, 0.2)) == 0.5
    assert fit_temperature(None, None, [0.5, 1.0, 2.0], metrics=nce(0.3, 0.3, 0.3)) == 1.0            # a tie: nearest 1
    assert fit_temperature(None, None, [2.0, 0.8, 1.2, 0.5], metrics=nce(0.3, 0.3, 0.3, 0.3)) == 0.8   # then the lower one
    assert fit_temperature(None, None, [1.5, 0.5], metrics=nce(0.3, 0.3)) == 0.5
    assert fit_temperature(None, None, [0.5, 2.0, 3.0], metrics=nce(NAN, -0.5, NAN)) == 2.0          # NaN loses to any number
    assert fit_temperature(None, None, [3.0, 2.0], metrics=nce(NAN, NAN)) == 2.0
    conf = torch.tensor([[0.6, 0.6, 0.4, 0.4], [0.9, 0.9, 0.1, 0.1], [0.4, 0.4, 0.6, 0.6]])
    assert fit_temperature(conf, [1, 1, 0, 0], [2.0, 1.0, 0.5]) == 1.0
    with pytest.raises(ValueError):
        fit_temperature(conf, [1, 1, 0, 0], [1.0, 2.0])
    with pytest.raises(ValueError):
        fit_temperature(conf, [1, 1, 0, 0], [])


def test_error_labels_and_the_sweep_wrapper(emulated):
    D = emulated
    assert D.error_labels([5, 6, 7, 9], [6, 8, 9]).tolist() == [0, 1, 0, 1] and D.error_labels([5, 6, 7, 9], [6, 8, 9]).dtype == torch.int32
    assert D.error_labels([], [1]).tolist() == [] and D.error_labels([1, 2], []).tolist() == [0, 0]
    lp = torch.from_numpy(CR.planted()[0][:24])
    cfg = D.ConfidenceConfig(entropy_type='renyi', alpha=0.5, entropy_norm='lin')
    temps = [0.5 + 0.1 * k for k in range(20)]                              # more than one launch takes
    idx, conf = D.frame_confidence_sweep(lp, temps, cfg)
    want_i, want = AR.sweep(lp.numpy(), [float(np.float32(1.0 / t)) for t in temps], None, 'renyi', 'lin', 0.5)
    assert idx.tolist() == want_i.tolist() and tuple(conf.shape) == (20, 24) and np.array_equal(conf.numpy(), want.astype(np.float32))
    idx3, conf3 = D.frame_confidence_sweep(lp.reshape(2, 12, -1), [1.0, 2.0], cfg)
    assert tuple(idx3.shape) == (2, 12) and tuple(conf3.shape) == (2, 2, 12)
    for bad in ([], [0.0], [-1.0], [math.inf], [NAN]):
        with pytest.raises(ValueError):
            D.frame_confidence_sweep(lp, bad, cfg)
    with pytest.raises(ValueError):
        D.frame_confidence_sweep(lp[0], [1.0], cfg)


def test_the_temperature_keyword_of_the_confidence_functions(emulated):
    from lcasr_amd.decoding import confidence as F
    lp = torch.from_numpy(CR.planted()[0])
    cfg = F.ConfidenceConfig()
    idx, conf = F.frame_confidence(lp, cfg)
    i1, c1 = F.frame_confidence(lp, cfg, temperature=1.0)
    i2, c2 = F.frame_confidence(lp, cfg, temperature=2.0)
    assert torch.equal(idx, i1) and torch.equal(idx, i2) and torch.equal(conf, c1) and bool((c2 < conf).all())
    g, g2 = F.greedy_confidence(lp, 31, cfg), F.greedy_confidence(lp, 31, cfg, temperature=2.0)
    assert g2.tokens == g.tokens and g2.spans == g.spans and all(a < b for a, b in zip(g2.token_confidence, g.token_confidence))
    assert F.greedy_confidence(lp, 31, cfg, temperature=None).token_confidence == g.token_confidence
    for bad in (0.0, -2.0, math.inf, NAN):
        with pytest.raises(ValueError, match='temperature'):
            F.frame_confidence(lp, cfg, temperature=bad)


def test_a_cpu_tensor_is_refused_by_the_product_path():
    from lcasr_amd.hip import calib
    off = torch.tensor([0, 2], dtype=torch.int64)
    with pytest.raises(RuntimeError, match='GPU'):
        calib.edit_align(torch.tensor([1, 2], dtype=torch.int32), off, torch.tensor([1, 3], dtype=torch.int32), off, off, None)
    with pytest.raises(RuntimeError, match='GPU'):
        calib.frames_sweep(torch.zeros(4, 8), torch.ones(1))


# ---- 4. eval.run.calibrate on the tiny fixture model ------------------------------------------------------------------------------
class IdTok:
    """Every token is a word: id i is spelt 't<i>'."""
    def __init__(self, V): self.V = V
    def vocab_size(self): return self.V
    def decode(self, ids): return ' '.join(f't{int(i)}' for i in ids)
    def encode(self, text): return [int(w[1:]) for w in text.split()]


def test_calibrate_on_the_tiny_model(emulated_ops, emulated, monkeypatch):
    import audio_refs as AUD
    from lcasr_amd.eval import run as R
    from lcasr_amd.utils import audio_tools
    monkeypatch.setattr(audio_tools.audio, 'melspec', AUD.melspec)
    E.attach(monkeypatch, emulated_ops)
    fx = load_golden('infer_tiny')
    m = build_from_fixture(fx).eval()
    tok = IdTok(int(fx['cfg.vocab_size']))
    blank = m.decoder.num_classes - 1
    temps = [0.5, 1.0, 2.0]
    recs = []
    for seed in (3, 4):
        spec = audio_tools.to_spectogram(AUD.test_signal(3 * 16000, seed=seed)[None])
        logits = R.moving_average_eval(R._Args(), m, spec, 128, 32, tok, use_tqdm=False, return_numpy=False)
        greedy = [int(c) for c in logits.argmax(-1).tolist()]
        runs = [c for i, c in enumerate(greedy) if c != blank and (i == 0 or greedy[i - 1] != c)]
        gold = [r for k, r in enumerate(runs) if k % 5 != 2]                # a reference that drops every fifth word of the hypothesis,
        gold = [(r + 1) % blank if k % 4 == 1 else r for k, r in enumerate(gold)] + [1, 2]        # replaces every fourth and adds two
        recs.append((f'rec{seed}', spec, tok.decode(gold).upper(), runs, logits))
    out = R.calibrate(m, [r[:3] for r in recs], tok, 128, 32, temperatures=temps)
    assert set(out) == {'temperatures', 'metrics', 'temperature', 'labels', 'confusion_pairs', 'words'}
    assert out['temperatures'] == temps and len(out['metrics']) == 3 and out['temperature'] in temps
    assert out['words'] == len(out['labels']) == sum(len(r[3]) for r in recs) > 6
    labels, conf, pairs = [], [[] for _ in temps], {}
    for _, _, gold, runs, logits in recs:                                    # the same figures from the restatements, step by step
        h2r, _, _ = AR.align_plain(runs, tok.encode(gold.lower()))
        ref = tok.encode(gold.lower())
        labels += [int(j >= 0 and ref[j] == runs[i]) for i, j in enumerate(h2r)]
        for i, j in enumerate(h2r):
            if j >= 0 and ref[j] != runs[i]:
                pairs[(f't{ref[j]}', f't{runs[i]}')] = pairs.get((f't{ref[j]}', f't{runs[i]}'), 0) + 1
        for k, t in enumerate(temps):
            (want,), _ = CR.greedy(AR.scaled(logits.float().numpy(), None, 1.0 / t)[None], blank, 'tsallis', 'exp', 1 / 3, 'min', True)
            assert want[0] == runs
            conf[k] += list(want[2])
    assert out['labels'] == labels and 0 < sum(labels) < len(labels)
    assert out['confusion_pairs'] == sorted(((r, h, n) for (r, h), n in pairs.items()), key=lambda v: (-v[2], v[0], v[1])) and pairs
    from lcasr_amd.decoding.calibration import calibration_metrics, fit_temperature
    for k in range(3):
        want = calibration_metrics(conf[k], labels)
        for key, v in out['metrics'][k].items():
            assert v == pytest.approx(want[key], abs=1e-5, nan_ok=True), (k, key)
    assert out['temperature'] == fit_temperature(None, None, temps, metrics=out['metrics'])
    with pytest.raises(ValueError, match='no recordings'):
        R.calibrate(m, [], tok, 128, 32)
    d0 = R.transcribe_detail(m, AUD.test_signal(3 * 16000, seed=3), tok, 128, 32)
    d2 = R.transcribe_detail(m, AUD.test_signal(3 * 16000, seed=3), tok, 128, 32, temperature=2.0)
    assert d2['tokens'] == d0['tokens'] and all(a <= b for a, b in zip(d2['token_confidence'], d0['token_confidence']))
    assert R.transcribe_detail(m, AUD.test_signal(3 * 16000, seed=3), tok, 128, 32, temperature=None) == d0
