"""CPU tests of context attribution (include/sconf_ctxattr.h, lcasr_amd.hip.ctxattr, lcasr_amd.eval.context_attribution): the header
against the binding and the exports, the typing in both import orders, the host-side queries and refusals, and the driver with the
unit's ops replaced by the naive numpy restatement (tests/ctxattr_refs.py) and the model on the emulated op layer.  The kernels
themselves are tested in test_ctxattr_gpu.py."""
import ctypes
import importlib
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import ctxattr_refs as CR
import eval_refs as E
from cabi_header import assert_binding_is_header, header_abi
from common_model import build_from_fixture
from conftest import ROOT, load_golden

HEADER, PREFIX = 'sconf_ctxattr.h', 'sconf_ctxattr_'
NAMES = {'sconf_ctxattr_max_ref', 'sconf_ctxattr_max_window_frames', 'sconf_ctxattr_threads', 'sconf_ctxattr_cells_per_thread',
         'sconf_ctxattr_score_workspace', 'sconf_ctxattr_window_means', 'sconf_ctxattr_mask_fill', 'sconf_ctxattr_score'}


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from lcasr_amd.hip import ctxattr
    return ctxattr.load()


def _declared():
    src = open(os.path.join(ROOT, 'include', HEADER)).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(sconf_[a-z0-9_]+)\s*\(', src)))


# ---- 1. the unit: header, binding, exports, typing ---------------------------------------------------------------------------------
def test_binding_is_the_header_and_the_other_units_do_not_name_it(lib):
    from lcasr_amd.hip import _lib, ctxattr
    funcs, enums = header_abi(HEADER, PREFIX)
    assert sorted(funcs) == _declared() and not enums and set(funcs) == NAMES
    assert_binding_is_header(funcs, ctxattr.PROTOTYPES, ctxattr.PLAIN, 'hip/ctxattr.py')
    assert not any(n.startswith(PREFIX) for n in list(_lib.PROTOTYPES) + list(_lib.PLAIN))
    mine = {os.path.join('include', HEADER), os.path.join('long-context-asr_amd', 'hip', 'ctxattr.py')}
    others = [os.path.join('include', f) for f in os.listdir(os.path.join(ROOT, 'include'))]
    others += [os.path.join('long-context-asr_amd', 'hip', f) for f in os.listdir(os.path.join(ROOT, 'long-context-asr_amd', 'hip')) if f.endswith('.py')]
    assert len(others) >= 14
    for f in sorted(set(others) - mine):
        assert 'ctxattr' not in open(os.path.join(ROOT, f)).read(), f
    assert lib.sconf_version() == 220


def test_every_declared_name_is_exported(lib):
    from lcasr_amd.hip import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert len(_declared()) == 8
    for n in _declared():
        assert hasattr(raw, n), f'{n} declared in include/{HEADER} but not exported'


_ORDER_CHILD = '''
import ctypes, sys
from lcasr_amd.hip import _lib
if sys.argv[1] == 'load-first': _lib.load()
from lcasr_amd.hip import ctxattr
lib = _lib.load()
for name, args in ctxattr.PROTOTYPES.items():
    assert list(getattr(lib, name).argtypes) == args and getattr(lib, name).restype is ctypes.c_int, name
    assert _lib.bound()[name] == (args, ctypes.c_int), name
for name, (args, res) in ctxattr.PLAIN.items():
    assert list(getattr(lib, name).argtypes) == args and getattr(lib, name).restype is res, name
    assert _lib.bound()[name] == (args, res), name
assert lib.sconf_ctxattr_score_workspace.restype is ctypes.c_int64 and lib.sconf_ctxattr_score_workspace(100, 65535, 1, 65535) > 1 << 32
print('typed', sys.argv[1])
'''


def test_the_unit_is_typed_in_both_import_orders(lib):
    for order in ('import-first', 'load-first'):
        r = subprocess.run([sys.executable, '-c', _ORDER_CHILD, order], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True)
        assert r.returncode == 0 and f'typed {order}' in r.stdout, r.stdout + r.stderr


_LAZY_CHILD = '''
import sys
import lcasr_amd.eval
import lcasr_amd.eval.run
from lcasr_amd.hip import _lib
assert 'lcasr_amd.hip.ctxattr' not in sys.modules and _lib._lib is None
assert not any(n.startswith('sconf_ctxattr_') for u in _lib._units for t in u for n in t)
from lcasr_amd.eval import context_attribution, ContextAttribution
assert callable(context_attribution) and 'lcasr_amd.hip.ctxattr' in sys.modules
assert sys.modules['lcasr_amd.eval.context_attribution'].context_attribution is context_attribution is lcasr_amd.eval.context_attribution
print('exported')
'''


def test_the_driver_is_exported_and_the_package_binds_the_unit_on_first_use_only():
    r = subprocess.run([sys.executable, '-c', _LAZY_CHILD], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True)
    assert r.returncode == 0 and 'exported' in r.stdout, r.stdout + r.stderr


# ---- 2. queries ------------------------------------------------------------------------------------------------------------------
def test_geometry_queries(lib):
    from lcasr_amd.hip import ctxattr
    M = lib.sconf_ctxattr_max_ref()
    assert M == 65535 == ctxattr.max_ref() == ctxattr.MAX_REF
    assert lib.sconf_ctxattr_max_window_frames() == ctxattr.MAX_WINDOW_FRAMES == ctxattr.max_window_frames() >= 4096
    assert 4 * lib.sconf_ctxattr_max_window_frames() <= 64 * 1024                          # the middle in static LDS
    steps = [0, 1, 62, 63, 64, 65, 127, 128, 255, 256, 511, 512, 1022, 1023, 1024, 1025, 2047, 2048, 4095, 4096, 8191, 8192, 13000, 16383, 16384,
             32767, 32768, 50000, M - 1, M]
    last = (0, 0)
    for R in steps:
        nt, cpt = lib.sconf_ctxattr_threads(R), lib.sconf_ctxattr_cells_per_thread(R)
        assert nt in (64, 128, 256, 512, 1024) and cpt in (1, 2, 4, 8, 16, 32, 64) and (cpt == 1 or nt == 1024)
        assert nt * cpt >= R + 1, R                                                        # covers the row
        assert nt >= last[0] and cpt >= last[1], R                                         # monotone
        assert nt * cpt < 2 * (R + 1) or nt == 64                                          # and no wider than it must be
        last = (nt, cpt)
    assert (lib.sconf_ctxattr_threads(63), lib.sconf_ctxattr_threads(64), lib.sconf_ctxattr_threads(1023)) == (64, 128, 1024)
    assert [lib.sconf_ctxattr_cells_per_thread(R) for R in (1023, 1024, 2047, 2048, 32767, 32768, M)] == [1, 2, 2, 4, 32, 64, 64]
    for bad in (-1, M + 1, 1 << 40):
        assert lib.sconf_ctxattr_threads(bad) == -1 and lib.sconf_ctxattr_cells_per_thread(bad) == -1


def test_workspace_query(lib):
    from lcasr_amd.hip import ctxattr
    ws = lib.sconf_ctxattr_score_workspace
    r256 = lambda n: (n + 255) // 256 * 256

    def formula(I, R):
        P = lib.sconf_ctxattr_threads(R) * lib.sconf_ctxattr_cells_per_thread(R)
        return r256(16 * I) + r256(8 * P) + 2 * r256(4 * I * P)

    assert ws(45000, 176, 176, 13000) == 23202560 == formula(176, 13000)                   # the figure in the header
    for N, I, J, R in ((1, 1, 1, 0), (300, 3, 3, 65535), (16384, 64, 64, 4096), (100, 7, 2, 1024), (50, 65535, 1, 10)):
        assert ws(N, I, J, R) == formula(I, R) == ctxattr.score_workspace(N, I, J, R)
        assert ws(N, I, J, R) <= ws(N, I + 1, J, R) if I < 65535 else True
    for bad in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, -1), (1, 1, 1, 65536), (1, 65536, 1, 1), (1 << 20, 1, 1 << 20, 1)):
        assert ws(*bad) == -1, bad
    with pytest.raises(ValueError, match='65535'):
        ctxattr.score_workspace(10, 1, 1, 65536)


# ---- 3. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_name_their_cause(lib):
    one = ctypes.c_void_p(16)                                              # never dereferenced: every call below is refused on the host
    bound = lib.sconf_ctxattr_max_window_frames()

    def call(windows=((0, 5), (5, 10)), N=10, J=2, R=3, ws=None, cap=8, tokens=None, blank=31, **null):
        I = len(windows)
        fw = (ctypes.c_int32 * (2 * I))(*[v for w in windows for v in w]) if I else None
        need = lib.sconf_ctxattr_score_workspace(N, I, J, R)
        ptr = {k: one for k in ('clean', 'masked', 'ref', 'errors', 'clean_errors', 'clean_len', 'mid_len', 'workspace')}
        ptr.update(null)
        return lib.sconf_ctxattr_score(ptr['clean'], ptr['masked'], ptr['ref'], fw, ptr['errors'], ptr['clean_errors'], ptr['clean_len'],
                                       ptr['mid_len'], tokens, ptr['workspace'], need if ws is None else ws, N, I, J, R, cap, blank, None)

    assert call(R=65536, ws=1 << 40) != 0 and b'65535' in lib.sconf_last_error()
    assert call(R=-1, ws=1 << 40) != 0 and b'65535' in lib.sconf_last_error()
    assert call(windows=((0, 5), (7, 6))) != 0 and b'frame window 1' in lib.sconf_last_error() and b'f <= g' in lib.sconf_last_error()     # g < f
    assert call(windows=((0, 5), (5, 11))) != 0 and b'frame window 1' in lib.sconf_last_error()                                             # g > N
    assert call(windows=((-1, 5),)) != 0 and b'frame window 0' in lib.sconf_last_error()
    assert call(windows=((0, bound),), N=bound + 5) != 0 and b'wider than the bound' in lib.sconf_last_error()                             # g - f + 1 over it
    assert call(windows=(), ws=1 << 20) != 0 and b'sizes' in lib.sconf_last_error()
    assert call(N=0, windows=((0, 0),), ws=1 << 20) != 0 and b'sizes' in lib.sconf_last_error()
    assert call(J=0, ws=1 << 20) != 0 and b'sizes' in lib.sconf_last_error()
    assert call(ws=lib.sconf_ctxattr_score_workspace(10, 2, 2, 3) - 1) != 0 and b'workspace' in lib.sconf_last_error()
    assert call(tokens=one, cap=5) != 0 and b'mid_cap' in lib.sconf_last_error()           # the middle of [0, 5) has 6 frames
    for missing in ('clean', 'masked', 'ref', 'errors', 'clean_errors', 'clean_len', 'mid_len', 'workspace'):
        assert call(**{missing: None}) != 0 and b'null' in lib.sconf_last_error(), missing
    # the two streaming entry points
    assert lib.sconf_ctxattr_window_means(None, None, None, 80, 100, 0, None) == 0         # nothing to do, nothing launched
    assert lib.sconf_ctxattr_window_means(one, one, one, 0, 100, 3, None) != 0 and b'sizes' in lib.sconf_last_error()
    assert lib.sconf_ctxattr_window_means(one, None, one, 80, 100, 3, None) != 0 and b'null' in lib.sconf_last_error()
    assert lib.sconf_ctxattr_mask_fill(None, None, None, None, 80, 100, 3, 0, 0, None) == 0
    assert lib.sconf_ctxattr_mask_fill(one, one, one, one, 80, 100, 3, 2, 2, None) != 0 and b'batch' in lib.sconf_last_error()
    assert lib.sconf_ctxattr_mask_fill(one, one, one, one, 80, 100, 3, -1, 1, None) != 0 and b'batch' in lib.sconf_last_error()
    assert lib.sconf_ctxattr_mask_fill(one, one, one, one, 80, 100, 2000, 0, 1000, None) != 0 and b'batch' in lib.sconf_last_error()
    assert lib.sconf_ctxattr_mask_fill(one, one, one, None, 80, 100, 3, 0, 1, None) != 0 and b'null' in lib.sconf_last_error()


def test_cpu_tensors_are_refused_by_the_ops(lib):
    from lcasr_amd.hip import ctxattr
    with pytest.raises(RuntimeError, match='GPU'):
        ctxattr.window_means(torch.zeros(4, 8), torch.zeros(1, 2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match='GPU'):
        ctxattr.score(torch.zeros(8, dtype=torch.int32), torch.zeros(1, 8, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), [(0, 8)], 3)


# ---- 4. the restatement against the identity's pieces ------------------------------------------------------------------------------
def test_restatement_rows_and_middles_compose_to_the_spliced_hypothesis():
    """pre_i ++ mid_ij ++ suf_i is the collapse of the spliced labels, for ragged, empty and unordered windows with repeats across
    both seams (what the driver's word level composes on the host)."""
    rng = np.random.default_rng(5)
    for trial in range(60):
        N, J, blank = int(rng.integers(1, 40)), 2, 3
        clean, masked = CR.random_labels(rng, J, N, 3, blank)
        cuts = sorted(int(c) for c in rng.integers(0, N + 1, 4))
        windows = [(cuts[0], cuts[1]), (cuts[1], cuts[1]), (cuts[2], cuts[3]), (0, N)]
        sc = CR.score(torch.from_numpy(clean), torch.from_numpy(masked), torch.zeros(0, dtype=torch.int32), windows, blank, with_tokens=True)
        for i, (f, g) in enumerate(windows):
            ge = min(g + 1, N)
            pre = CR.collapse(clean[:f], blank)
            suf = CR.collapse(clean[ge:], blank, int(clean[ge - 1]) if ge > 0 else None)
            for j in range(J):
                mid = sc.mid_tokens[i, j, :int(sc.mid_len[i, j])].tolist()
                hyp = CR.collapse(CR.spliced(clean, masked[j], f, g), blank)
                assert pre + mid + suf == hyp and int(sc.errors[i, j]) == len(hyp)      # against an empty reference: all insertions
        assert int(sc.clean_len) == len(CR.collapse(clean, blank)) == int(sc.clean_errors)


# ---- 5. the driver -----------------------------------------------------------------------------------------------------------------
T_TINY, WINDOW = 403, 96                      # five windows, the last of 19 frames; N = 51, so T / N is no integer


class Tok:
    """Toy tokenizer: 'w<i>' encodes to id i; id i decodes to the word 'w<i % 7>', so several ids share a word."""
    def vocab_size(self): return 127
    def encode(self, text): return [int(w[1:]) for w in text.split()]
    def decode(self, ids): return ' '.join(f'w{int(i) % 7}' for i in ids)


@pytest.fixture
def driver(emulated_ops, monkeypatch):
    """eval.context_attribution with the unit's three ops replaced by the naive restatement and the model's ops emulated."""
    E.attach(monkeypatch, emulated_ops)
    from lcasr_amd.hip import ctxattr
    for name in ('window_means', 'mask_fill', 'score'):
        monkeypatch.setattr(ctxattr, name, getattr(CR, name))
    return importlib.import_module('lcasr_amd.eval.context_attribution')


@pytest.fixture(scope='module')
def tiny():
    fx = load_golden('infer_tiny')
    return fx, torch.from_numpy(fx['spec'].copy())[:, :, :T_TINY].contiguous()


def _count_forwards(m):
    calls = []
    inner = m.forward

    def forward(x, *a, **kw):
        calls.append(tuple(x.shape))
        return inner(x, *a, **kw)

    m.forward = forward
    return calls


def test_window_arithmetic_is_the_references(driver, tiny):
    fx, spec = tiny
    m = build_from_fixture(fx).eval()
    res = driver.context_attribution(m, spec, 'w1 w2 w3', Tok(), seq_len=256, window_size=WINDOW, batch_size=2)
    N = res.frame_labels.shape[1]
    assert N == 51 and T_TINY % WINDOW != 0 and (T_TINY / N) != T_TINY // N
    table = [(0, 96), (96, 192), (192, 288), (288, 384), (384, 403)]
    assert res.windows == table
    ds = T_TINY / N
    frames = [(int(s / ds), int(e / ds)) for s, e in table]                # the reference's expression, lines 86-87
    assert res.frame_windows == frames == driver.attribution_windows(T_TINY, N, WINDOW)[1]
    assert frames == [(0, 12), (12, 24), (24, 36), (36, 48), (48, 51)]     # worked by hand: 96 k * 51 / 403 = 12.149 k
    assert res.frame_labels.shape == (6, N) and res.frame_labels.dtype == torch.int32
    assert res.wer_matrix.shape == (5, 6) and res.wer_matrix.dtype == torch.float32 and res.errors.shape == (5, 6) and res.units == 3
    # a rounding case of the float expression: the last edge of an exact division may fall one short of N; the table is still the float one
    for Tn, Nn, w in ((400, 50, 96), (1000, 125, 96), (16384, 2048, 2048), (131072, 16384, 2048), (299, 38, 50)):
        wins, fw = driver.attribution_windows(Tn, Nn, w)
        assert fw == [(int(s / (Tn / Nn)), int(e / (Tn / Nn))) for s, e in wins] and all(0 <= f <= g <= Nn for f, g in fw)


@pytest.mark.parametrize('batch_size', [1, 2, 4, 8])
def test_the_model_runs_once_clean_and_once_per_batch(driver, tiny, batch_size):
    fx, spec = tiny
    m = build_from_fixture(fx).eval()
    calls = _count_forwards(m)
    res = driver.context_attribution(m, spec, 'w1 w2 w3', Tok(), seq_len=256, window_size=WINDOW, batch_size=batch_size)
    W = len(res.windows)
    assert W == 5 and len(calls) == 1 + math.ceil(W / batch_size)
    assert calls[0] == (1, 80, T_TINY) and sum(c[0] for c in calls[1:]) == W and all(c[0] <= batch_size for c in calls[1:])


def test_token_level_is_the_naive_procedure(driver, tiny):
    """batch_size = 1: mask, forward, splice the LOG-PROBS, argmax, collapse, eval_refs.edit_counts, pair by pair as the reference."""
    from lcasr_amd.eval import run as R
    fx, spec = tiny
    m = build_from_fixture(fx).eval()
    blank, tok = m.decoder.num_classes - 1, Tok()
    att = R._windowed_modules(m)
    for a in att: a.left_window = a.right_window = 256 // 8 // 2
    with torch.no_grad():
        clean_lp = m(spec)['final_posteriors'].float()[0]
        hyp = CR.collapse(clean_lp.argmax(-1).tolist(), blank)
        assert len(hyp) >= 6
        gold = CR.gold_of(hyp)
        windows = [(s, min(s + WINDOW, T_TINY)) for s in range(0, T_TINY, WINDOW)]
        ds = T_TINY / clean_lp.shape[0]
        want = torch.zeros(5, 6, dtype=torch.int64)
        for j, (s, e) in enumerate(windows):
            x = spec.clone()
            x[:, :, s:e] = float(CR.window_means(spec[0], torch.tensor([[s, e]], dtype=torch.int32))[0])
            lp_j = m(x)['final_posteriors'].float()[0]
            for i, (s2, e2) in enumerate(windows):
                f, g = int(s2 / ds), int(e2 / ds)
                cur = clean_lp.clone()
                cur[f:g] = lp_j[f:g]
                want[i, j] = CR.distance(CR.collapse(cur.argmax(-1).tolist(), blank), gold)
        want[:, 5] = CR.distance(hyp, gold)
    for a in att: a.left_window = a.right_window = -1
    res = driver.context_attribution(m, spec, ' '.join(f'w{i}' for i in gold), tok, seq_len=256, window_size=WINDOW, batch_size=1)
    assert res.units == len(gold) and torch.equal(res.errors, want)
    assert torch.equal(res.wer_matrix, (want.double() / len(gold) * 100).float())
    assert res.unharmed == tok.decode(hyp) and res.transcripts is None
    assert all(a.left_window == -1 and a.right_window == -1 for a in att)
    print('[ctxattr cpu] errors', want.tolist())
    assert CR.condition(want)


def test_the_end_to_end_case_of_the_gpu_test_meets_its_condition_under_emulation(driver, tiny):
    """test_ctxattr_gpu.py compares the matrix of this input on the device; here, on the emulated ops: the clean hypothesis is not
    empty and masking a window moves the errors of another one."""
    fx, _ = tiny
    spec = torch.from_numpy(fx['spec'].copy())[:, :, :CR.E2E_T].contiguous()
    m = build_from_fixture(fx).eval()
    tok = Tok()
    first = driver.context_attribution(m, spec, 'w1', tok, seq_len=256, window_size=CR.E2E_WINDOW, batch_size=1)
    hyp = CR.collapse(first.frame_labels[5].tolist(), m.decoder.num_classes - 1)
    res = driver.context_attribution(m, spec, ' '.join(f'w{i}' for i in CR.gold_of(hyp)), tok, seq_len=256, window_size=CR.E2E_WINDOW, batch_size=1)
    print('[ctxattr cpu] end-to-end errors', res.errors.tolist())
    assert len(res.windows) == 5 and res.windows[-1] == (384, 400) and res.frame_labels.shape == (6, 50)
    assert len(hyp) > 0 and CR.condition(res.errors)


def test_word_level_is_word_error_rate_detail_of_the_naive_transcripts(driver, tiny):
    from lcasr_amd.eval.wer import word_error_rate_detail
    fx, spec = tiny
    m = build_from_fixture(fx).eval()
    blank, tok = m.decoder.num_classes - 1, Tok()
    gold_text = 'W3 w1 w4 w1 w5 w2 w6 w5 w3 w5 w0'
    normalize = lambda s: s.replace('w6', 'w0')
    res = driver.context_attribution(m, spec, gold_text, tok, seq_len=256, window_size=WINDOW, level='word', batch_size=3, normalize=normalize,
                                     return_transcripts=True)
    labels = res.frame_labels.numpy()
    clean = labels[5]
    assert res.units == 11 and res.unharmed == normalize(tok.decode(CR.collapse(clean, blank))).lower()
    for i, (f, g) in enumerate(res.frame_windows):
        for j in range(5):
            text = normalize(tok.decode(CR.collapse(CR.spliced(clean, labels[j], f, g), blank))).lower()
            assert res.transcripts[i][j] == text
            wer = word_error_rate_detail(hypotheses=[text], references=[gold_text])[0]
            assert float(res.wer_matrix[i, j]) == float(np.float32(wer * 100)), (i, j)
    clean_wer = word_error_rate_detail(hypotheses=[res.unharmed], references=[gold_text])[0]
    assert all(float(v) == float(np.float32(clean_wer * 100)) for v in res.wer_matrix[:, 5])
    # the token level of the same call scores ids, the restatement applied to the returned labels
    tok_res = driver.context_attribution(m, spec, 'w3 w1 w4', tok, seq_len=256, window_size=WINDOW, batch_size=3)
    sc = CR.score(tok_res.frame_labels[5], tok_res.frame_labels[:5], torch.tensor([3, 1, 4], dtype=torch.int32), tok_res.frame_windows, blank)
    assert torch.equal(tok_res.errors[:, :5], sc.errors.long()) and bool((tok_res.errors[:, 5] == int(sc.clean_errors)).all())


def test_modes_set_and_restore_the_module_windows(driver, tiny):
    from lcasr_amd.eval import run as R
    fx, spec = tiny
    m = build_from_fixture(fx).eval()
    att = R._windowed_modules(m)
    seen = []
    inner = att[0].forward_prenorm
    att[0].forward_prenorm = lambda *a, **kw: (seen.append((att[0].left_window, att[0].right_window)), inner(*a, **kw))[1]
    driver.context_attribution(m, spec, 'w1', Tok(), seq_len=256, window_size=200, batch_size=4)
    assert set(seen) == {(16, 16)} and len(seen) == 2
    del seen[:]
    driver.context_attribution(m, spec, 'w1', Tok(), seq_len=256, window_size=200, batch_size=4, evaluation_mode='full')
    assert set(seen) == {(-1, -1)}
    att[0].left_window, att[0].right_window = 5, 7
    calls = []

    def boom(*a, **kw):
        calls.append((att[1].left_window, att[1].right_window))
        if len(calls) == 2: raise RuntimeError('injected failure')          # the first masked batch
        return inner2(*a, **kw)

    inner2 = att[1].forward_prenorm
    att[1].forward_prenorm = boom
    with pytest.raises(RuntimeError, match='injected failure'):
        driver.context_attribution(m, spec, 'w1', Tok(), seq_len=200, window_size=200, batch_size=4)
    assert calls == [(12, 12), (12, 12)]
    assert (att[0].left_window, att[0].right_window) == (5, 7) and (att[1].left_window, att[1].right_window) == (-1, -1)


def test_the_driver_refuses_what_the_unit_cannot_score(driver, tiny, monkeypatch):
    fx, spec = tiny
    m = build_from_fixture(fx).eval()
    calls = _count_forwards(m)
    with pytest.raises(ValueError, match='empty'):
        driver.context_attribution(m, spec, '  ', Tok(), seq_len=256, window_size=WINDOW)

    class Long(Tok):
        def encode(self, text): return [1] * 65536

    with pytest.raises(ValueError, match='65535'):
        driver.context_attribution(m, spec, 'w1', Long(), seq_len=256, window_size=WINDOW)
    for bad in (dict(level='char'), dict(evaluation_mode='buffered'), dict(batch_size=0), dict(window_size=0)):
        with pytest.raises(ValueError):
            driver.context_attribution(m, spec, 'w1', Tok(), seq_len=256, **bad)
    with pytest.raises(ValueError, match='features, time'):
        driver.context_attribution(m, spec[0], 'w1', Tok(), seq_len=256)
    assert not calls                                                       # all refused before the first forward
    from lcasr_amd.hip import ctxattr
    monkeypatch.setattr(ctxattr, 'MAX_WINDOW_FRAMES', 12)
    with pytest.raises(ValueError, match='window of 12 model frames'):
        driver.context_attribution(m, spec, 'w1', Tok(), seq_len=256, window_size=WINDOW)
