"""Context attribution on the device (csrc/ctxattr.hip through lcasr_amd.hip.ctxattr and lcasr_amd.eval.context_attribution) against
the naive numpy restatement (tests/ctxattr_refs.py: splice, collapse, eval_refs.edit_counts per pair).  Every integer output is
compared EXACTLY.

The scan seams are sizes of the reference: R + 1 cells are spread over 64 .. 1024 threads of 1 .. 64 cells, so R + 1 either side of a
wave (64), of the widest workgroup (1024) and of every step of cells_per_thread moves a cell across a lane, a wave or a thread's
chunk.  The splice seams are frames: the edges f and g of a window, where a repeat or a blank on one side decides whether the other
side emits.  Alphabets of 2 and 3 symbols make ties everywhere.  Each case computes its restatement once."""
import numpy as np
import pytest
import torch

import ctxattr_footprint_cases as XC
import ctxattr_refs as CR
import footprint as FP
from common_model import build_from_fixture
from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def K():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from lcasr_amd.hip import ctxattr
    ctxattr.load()
    return ctxattr


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def run(K, clean, masked, ref, windows, blank, with_tokens=True):
    got = K.score(_dev(clean), _dev(masked), _dev(ref), windows, blank, with_tokens=with_tokens)
    torch.cuda.synchronize()
    return got


def same(got, want, what):
    for name, a, b in zip(got._fields, got, want):
        if a is None and b is None: continue
        a, b = a.cpu(), b.cpu()
        assert a.dtype == torch.int32 and a.shape == b.shape, f'{what} {name}: {a.dtype} {tuple(a.shape)}, restated {tuple(b.shape)}'
        if not torch.equal(a, b):
            bad = (a != b).nonzero()
            raise AssertionError(f'{what} {name}: {bad.shape[0]} element(s) differ, first at {bad[0].tolist()}: {int(a[tuple(bad[0])])} != {int(b[tuple(bad[0])])}')


def check(K, clean, masked, ref, windows, blank, what, with_tokens=True):
    want = CR.score(torch.from_numpy(clean), torch.from_numpy(masked), torch.from_numpy(np.asarray(ref, dtype=np.int32)), windows, blank, with_tokens)
    got = run(K, clean, masked, ref, windows, blank, with_tokens)
    same(got, want, what)
    return got, want


# ---- 1. scan seams -----------------------------------------------------------------------------------------------------------------
STEPS = (1024, 2048, 4096, 8192, 16384, 32768)          # R + 1 at which cells_per_thread doubles (1024: 1 -> 2 cells)
CELLS = sorted({1, 2, 63, 64, 65, 1023, 1024, 1025} | {c + d for c in STEPS for d in (0, 1)})


@pytest.mark.parametrize('cells', CELLS)
def test_reference_sizes_either_side_of_every_seam(K, cells):
    R = cells - 1
    lib = K.load()
    nt, cpt = lib.sconf_ctxattr_threads(R), lib.sconf_ctxattr_cells_per_thread(R)
    if cells in STEPS: assert lib.sconf_ctxattr_cells_per_thread(R + 1) == 2 * cpt and nt == 1024
    if cells - 1 in STEPS: assert lib.sconf_ctxattr_cells_per_thread(R - 1) * 2 == cpt
    for alphabet in (2, 3):
        rng = np.random.default_rng(cells * 7 + alphabet)
        N, J = 56, 3
        clean, masked = CR.random_labels(rng, J, N, alphabet, alphabet)
        ref = rng.integers(0, alphabet, R).astype(np.int32)
        check(K, clean, masked, ref, [(0, 19), (19, 37), (37, 56)], alphabet, f'R+1={cells} ({nt}x{cpt}) alphabet={alphabet}')


def test_the_widest_reference(K):
    R, N = 65535, 300
    assert K.load().sconf_ctxattr_cells_per_thread(R) == 64 and R == K.max_ref()
    rng = np.random.default_rng(11)
    clean, masked = CR.random_labels(rng, 3, N, 3, 3, p_blank=0.3)
    ref = rng.integers(0, 3, R).astype(np.int32)
    check(K, clean, masked, ref, CR.even_windows(N, 3), 3, 'R=65535')
    with pytest.raises(ValueError, match='65535'):
        K.score(_dev(clean), _dev(masked), torch.zeros(R + 1, dtype=torch.int32).cuda(), [(0, N)], 3)


def test_a_planted_pair_with_long_matches(K):
    """The reference is the clean hypothesis after 40 random edits: long diagonal runs of matches, the optimal path far from both axes."""
    rng = np.random.default_rng(21)
    N, J, blank = 4000, 4, 50
    clean, masked = CR.random_labels(rng, J, N, 50, blank, p_change=0.05)
    hyp = CR.collapse(clean, blank)
    ref = list(hyp)
    for _ in range(40):
        kind, at = int(rng.integers(0, 3)), int(rng.integers(0, len(ref)))
        if kind == 0: ref[at] = int(rng.integers(0, 50))
        elif kind == 1: del ref[at]
        else: ref.insert(at, int(rng.integers(0, 50)))
    assert 1100 < len(ref) < 2048 and K.load().sconf_ctxattr_cells_per_thread(len(ref)) == 2
    got, want = check(K, clean, masked, ref, CR.even_windows(N, 4), blank, 'planted', with_tokens=False)
    assert 0 < int(want.clean_errors) <= 40 and int(want.clean_len) == len(hyp)


# ---- 2. splice seams ---------------------------------------------------------------------------------------------------------------
def test_splice_seams(K):
    """blank = 9.  One clean row, hand-made masked rows, windows that put each seam where the rule can go wrong."""
    b = 9
    clean = np.array([1, 1, 2, b, 2, 3, 3, b, 1, 2, 2, 3, b, b, 1, 1], dtype=np.int32)       # N = 16
    N = len(clean)
    windows = [(0, 4), (4, 8), (8, 8), (8, 12), (12, 15), (15, 16), (3, 12), (0, 16), (16, 16), (0, 0)]
    rows = {
        'clean': clean.copy(),                                                     # row j = clean reproduces clean_errors in every i
        'repeat across f': np.array([1, 1, 2, b, b, 3, 3, b, 2, 2, 2, 3, 3, b, 1, 1]),       # aj[4] = a0[3] (blank), aj[8] = 2 != a0[7]; aj[12] = a0[11] = 3
        'repeat across g': np.array([1, 1, 2, 2, 2, 3, 3, 1, 1, 2, 2, 2, b, b, 1, 1]),       # aj[7] = 1 = a0[8] != a0[7]; aj[3] = 2 = a0[4] != a0[3]
        'all blank': np.full(N, b),
        'alternating': np.array([1, 2, 1, 2, 1, 2, 1, 2, 3, 1, 3, 1, 3, 2, 3, 2]),           # every frame emits
    }
    masked = np.stack([np.asarray(r, dtype=np.int32) for r in rows.values()])
    names = list(rows)
    a = masked[names.index('repeat across f')]
    assert a[4] == clean[3] and a[12] == clean[11]
    a = masked[names.index('repeat across g')]
    assert a[7] == clean[8] != clean[7] and a[3] == clean[4] != clean[3]
    ref = np.array([1, 2, 2, 3, 1, 2, 3, 1], dtype=np.int32)
    got, want = check(K, clean, masked, ref, windows, b, 'hand-made')
    # what the cases were made for, on the restatement
    ml = want.mid_len.numpy()
    alt = names.index('alternating')
    assert ml[1, alt] == 8 - 4 + 1                                                 # a middle of exactly g - f + 1 tokens (frame g emits too)
    assert ml[6, alt] == 12 - 3 - 1                                                # aj[3] repeats a0[2] across f, and a0[12] is blank
    assert ml[7, alt] == N and ml[5, alt] == 1                                     # g = N: no frame behind the window; a last window of one frame
    ab = names.index('all blank')
    assert ml[7, ab] == 0 and ml[0, ab] == 1 and ml[3, ab] == 0                    # all-blank windows: only frame g can emit (a0[4] does, a0[12] is blank)
    assert int(want.clean_len) == 8
    e = got.errors.cpu()
    assert bool((e[:, 0] == int(got.clean_errors)).all())                          # row j = clean
    assert bool((e[[2, 8, 9]] == int(got.clean_errors)).all())                     # empty windows score as the clean hypothesis, whatever the row
    # R = 0 and an all-blank clean run (H = 0), with the same masked rows
    check(K, clean, masked, np.zeros(0, dtype=np.int32), windows, b, 'R=0')
    got0, want0 = check(K, np.full(N, b, dtype=np.int32), masked, ref, windows, b, 'H=0')
    assert int(want0.clean_len) == 0 and int(want0.clean_errors) == len(ref)
    check(K, np.full(N, b, dtype=np.int32), masked, np.zeros(0, dtype=np.int32), windows, b, 'H=0 R=0')


def test_random_windows_unordered_and_overlapping(K):
    rng = np.random.default_rng(31)
    for trial, (N, R, alphabet) in enumerate(((1, 3, 2), (2, 0, 2), (37, 20, 2), (130, 90, 3), (200, 300, 3))):
        clean, masked = CR.random_labels(rng, 3, N, alphabet, alphabet)
        masked[2] = clean
        windows = [tuple(sorted(int(c) for c in rng.integers(0, N + 1, 2))) for _ in range(6)] + [(0, N), (N, N), (0, 0)]
        ref = rng.integers(0, alphabet, R).astype(np.int32)
        got, _ = check(K, clean, masked, ref, windows, alphabet, f'random windows {trial}')
        assert bool((got.errors[:, 2] == got.clean_errors).all())


def test_many_windows_take_more_than_one_staging_launch(K):
    """300 windows: the windows reach the device 224 per launch."""
    rng = np.random.default_rng(41)
    N, I = 640, 300
    clean, masked = CR.random_labels(rng, 1, N, 3, 3)
    windows = [(2 * i, 2 * i + 3) for i in range(I)]
    ref = rng.integers(0, 3, 70).astype(np.int32)
    check(K, clean, masked, ref, windows, 3, '300 windows', with_tokens=False)


def test_two_launches_are_bit_equal_and_tokens_are_optional(K):
    rng = np.random.default_rng(51)
    clean, masked = CR.random_labels(rng, 4, 500, 3, 3)
    ref = rng.integers(0, 3, 1500).astype(np.int32)
    windows = CR.even_windows(500, 5)
    a, b, c = (run(K, clean, masked, ref, windows, 3, t) for t in (True, True, False))
    for name, x, y in zip(a._fields, a, b):
        assert torch.equal(x, y), name
    assert c.mid_tokens is None and all(torch.equal(x, y) for x, y in zip(a[:4], c[:4]))


# ---- 3. means and the masked batch ---------------------------------------------------------------------------------------------------
def test_window_means_within_one_ulp_of_the_f64_mean(K):
    g = torch.Generator().manual_seed(61)
    F, T = 80, 1003
    spec = torch.randn(F, T, generator=g) * 4 + 2.5
    windows = [(s, min(s + 96, T)) for s in range(0, T, 96)] + [(17, 18), (0, T), (40, 40), (1002, 1003)]     # T is no multiple of the window
    wd = torch.tensor(windows, dtype=torch.int32).cuda()
    got = K.window_means(spec.cuda(), wd)
    again = K.window_means(spec.cuda(), wd)
    torch.cuda.synchronize()
    assert torch.equal(got, again) and got.dtype == torch.float32 and got.shape == (len(windows),)
    x = spec.numpy().astype(np.float64)
    for (s, e), m in zip(windows, got.cpu().numpy()):
        exact = x[:, s:e].mean() if e > s else 0.0
        d = abs(float(m) - exact)
        print(f'[ctxattr gpu] mean of [{s}, {e}): {m!r} f64 {exact!r} |d| {d:.3e} ulp {np.spacing(np.float32(exact)):.3e}')
        assert d <= np.spacing(np.float32(abs(exact))), (s, e)
    assert float(got[windows.index((40, 40))]) == 0.0
    assert torch.equal(got.cpu(), CR.window_means(spec, wd.cpu()))                 # rounded once: the f64 mean cast to f32


@pytest.mark.parametrize('F, T, w', [(80, 1000, 96), (5, 203, 48)])
def test_mask_fill_is_bit_equal_outside_the_window(K, F, T, w):
    """T = 1000: 16 bytes per thread; T = 203: one element per thread.  b in {1, 3}, j0 = 0 and j0 > 0, the short last window."""
    g = torch.Generator().manual_seed(71)
    spec = torch.randn(F, T, generator=g)
    windows = [(s, min(s + w, T)) for s in range(0, T, w)]
    assert len(windows) >= 5 and windows[-1][1] - windows[-1][0] < w
    wd = torch.tensor(windows, dtype=torch.int32).cuda()
    means = K.window_means(spec.cuda(), wd)
    for j0, b in ((0, 1), (1, 3), (len(windows) - 1, 1)):
        dst = K.mask_fill(spec.cuda(), wd, means, j0, b).cpu()
        assert dst.shape == (b, F, T)
        for k in range(b):
            s, e = windows[j0 + k]
            want = spec.clone()
            want[:, s:e] = means[j0 + k].cpu()
            assert torch.equal(dst[k].view(torch.int32), want.view(torch.int32)), (j0, k)
    with pytest.raises(ValueError):
        K.mask_fill(spec.cuda(), wd, means, len(windows) - 1, 2)


# ---- 4. end to end -----------------------------------------------------------------------------------------------------------------
class Tok:
    def vocab_size(self): return 127
    def encode(self, text): return [int(w[1:]) for w in text.split()]
    def decode(self, ids): return ' '.join(f'w{int(i) % 7}' for i in ids)


def test_end_to_end_matrix_is_the_naive_procedure(K):
    """The tiny golden model, T = 400, window_size = 96: five windows, the last one short.  batch_size = 1 against the reference's own
    procedure through the public pieces (one B = 1 forward per j, the LOG-PROBS spliced in torch, argmax, collapse, eval_refs.edit_counts);
    batch_size = 3 against the restatement applied to the returned frame labels (a batched forward may take another GEMM path)."""
    from lcasr_amd.eval import context_attribution
    from lcasr_amd.eval import run as R
    fx = load_golden('infer_tiny')
    spec = torch.from_numpy(fx['spec'].copy())[:, :, :CR.E2E_T].contiguous().cuda()
    m = build_from_fixture(fx, 'cuda').eval()
    blank, tok, T, Wn = m.decoder.num_classes - 1, Tok(), CR.E2E_T, CR.E2E_WINDOW
    windows = [(s, min(s + Wn, T)) for s in range(0, T, Wn)]
    assert len(windows) == 5 and windows[-1] == (384, 400)
    att = R._windowed_modules(m)
    for a in att: a.left_window = a.right_window = 256 // 8 // 2
    with torch.no_grad():
        means = K.window_means(spec[0], torch.tensor(windows, dtype=torch.int32).cuda())
        clean_lp = m(spec)['final_posteriors'].float()[0]
        N = clean_lp.shape[0]
        hyp = CR.collapse(clean_lp.argmax(-1).tolist(), blank)
        gold = CR.gold_of(hyp)
        ds = T / N
        want = torch.zeros(5, 6, dtype=torch.int64)
        for j, (s, e) in enumerate(windows):
            x = spec.clone()
            x[:, :, s:e] = means[j]
            lp_j = m(x)['final_posteriors'].float()[0]
            for i, (s2, e2) in enumerate(windows):
                f, g = int(s2 / ds), int(e2 / ds)
                cur = clean_lp.clone()
                cur[f:g] = lp_j[f:g]
                want[i, j] = CR.distance(CR.collapse(cur.argmax(-1).tolist(), blank), gold)
        want[:, 5] = CR.distance(hyp, gold)
    for a in att: a.left_window = a.right_window = -1
    print('[ctxattr gpu] end-to-end errors', want.tolist(), 'clean tokens', len(hyp))
    assert len(hyp) > 0 and CR.condition(want)                                     # the condition of the case, not a measurement
    gold_text = ' '.join(f'w{i}' for i in gold)
    res = context_attribution(m, spec, gold_text, tok, seq_len=256, window_size=Wn, batch_size=1)
    assert res.units == len(gold) and res.windows == windows and res.frame_labels.shape == (6, N)
    assert torch.equal(res.errors, want)
    assert torch.equal(res.wer_matrix, (want.double() / len(gold) * 100).float())
    assert all(a.left_window == -1 and a.right_window == -1 for a in att)
    res3 = context_attribution(m, spec, gold_text, tok, seq_len=256, window_size=Wn, batch_size=3, return_transcripts=True)
    labels = res3.frame_labels.cpu()
    sc = CR.score(labels[5], labels[:5], torch.tensor(gold, dtype=torch.int32), res3.frame_windows, blank)
    assert torch.equal(res3.errors[:, :5], sc.errors.long()) and bool((res3.errors[:, 5] == int(sc.clean_errors)).all())
    for i, (f, g) in enumerate(res3.frame_windows):
        for j in range(5):
            assert res3.transcripts[i][j] == tok.decode(CR.collapse(CR.spliced(labels[5].numpy(), labels[j].numpy(), f, g), blank)).lower()
    word = context_attribution(m, spec, 'w1 w2 w3 w4 w5 w6 w0 w1', tok, seq_len=256, window_size=Wn, batch_size=3, level='word')
    assert word.units == 8 and word.errors.shape == (5, 6) and bool((word.errors >= 0).all())


# ---- 5. refusals and footprint -----------------------------------------------------------------------------------------------------
def test_refusals_on_the_device_path(K):
    clean, masked = torch.zeros(8, dtype=torch.int32).cuda(), torch.zeros(2, 8, dtype=torch.int32).cuda()
    ref = torch.zeros(3, dtype=torch.int32).cuda()
    with pytest.raises(RuntimeError, match='GPU'):
        K.score(clean.cpu(), masked, ref, [(0, 8)], 3)
    with pytest.raises(TypeError):
        K.score(clean.long(), masked, ref, [(0, 8)], 3)
    for bad in ((5, 4), (0, 9), (-1, 3)):
        with pytest.raises(ValueError, match='frame window'):
            K.score(clean, masked, ref, [(0, 8), bad], 3)
    with pytest.raises(ValueError):
        K.score(clean, masked[:, :7].contiguous(), ref, [(0, 8)], 3)


@pytest.mark.parametrize('id', list(XC.CASES))
def test_footprint(K, id):
    FP.run_on_device(XC.build(id, K.load()), K.PROTOTYPES)
