"""The posterior kernels on the device (csrc/post.hip through lcasr_amd.hip.post) against the float64 restatement of the header's
recurrences (tests/post_refs.neighbours_bridge, itself held to brute force and to torch's CTC loss in tests/test_post.py), within the
tolerances of the header's contract, every one computed from sconf_post_step_error() and from nothing else:
    log-likelihoods  E(T) = (T + 1) step_error        finite llr  2 E(T) + 2^-22 max(1, |llr|)        posteriors  4 E(T) + 2^-22
with exact agreement on which entries are -inf and which are NaN.  The batches are post_refs.PARITY: the smallest shapes at which the
launch geometry can go wrong, B = 3 and ragged, one sample without labels and one without an alignment in each.  Then poisoning,
determinism, and the product path (posterior_confidence_long, eval.run.transcribe_detail) against the same calls with the
restatements in the kernels' place."""
import functools

import numpy as np
import pytest
import torch

import post_refs as PR

pytestmark = pytest.mark.gpu
OBSERVED = {'loglik': (0.0, 0.0), 'llr': (0.0, 0.0), 'posterior': (0.0, 0.0)}      # largest error seen, and its tolerance


@pytest.fixture(scope='module')
def K():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from lcasr_amd.hip import post
    post.load()
    assert 0.0 < post.step_error() <= PR.STEP_ERROR_CAP
    return post


@functools.lru_cache(maxsize=None)
def reference(k):
    """Batch k and its restatement, computed once: (inputs, (loglik, sub_llr, ins_llr), slots)."""
    inputs = PR.parity_inputs(k)
    lp, tg, il, tl, blank, C = inputs
    ll, sub, ins = PR.neighbours_batch(lp, tg, il, tl, blank, C)
    return inputs, (ll, sub, ins), PR.slots(sub, ins, tg, blank)


def on_device(K, lp, tg, il, tl, blank, C):
    wide = torch.from_numpy(lp).cuda()
    view = wide[:, :, :C]                                                    # the row stride is the batch's, NaN behind column C
    tg_d, il_d, tl_d = (torch.from_numpy(v).cuda() for v in (tg, il, tl))
    lat = K.lattice(view, tg_d, il_d, tl_d, blank)
    sub, ins = K.neighbours(view, tg_d, il_d, tl_d, blank, lat)
    out = K.slots(sub, ins, tg_d, blank)
    torch.cuda.synchronize()
    return lat.loglik.cpu().numpy(), sub.cpu().numpy(), ins.cpu().numpy(), tuple(v.cpu().numpy() for v in out)


def same_pattern(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), f'{what}: NaN at {np.argwhere(np.isnan(got) != np.isnan(want))[:3].tolist()}'
    assert np.array_equal(got == -np.inf, want == -np.inf), f'{what}: -inf at {np.argwhere((got == -np.inf) != (want == -np.inf))[:3].tolist()}'
    assert not (got == np.inf).any(), what


def within(got, want, tol, what, key):
    """Exact agreement on NaN and -inf, the finite entries within tol (an array like want); records the largest error."""
    same_pattern(got, want, what)
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    f = np.isfinite(want)
    if not f.any():
        return 0.0
    err = np.abs(got[f] - want[f])
    tol = np.broadcast_to(tol, want.shape)[f]
    worst = int(np.argmax(err / tol))
    if err.max() > OBSERVED[key][0]:
        OBSERVED[key] = (float(err.max()), float(tol[int(np.argmax(err))]))
    assert (err <= tol).all(), f'{what}: error {err[worst]:.3e} against a tolerance of {tol[worst]:.3e}'
    return float(err.max())


def check_alternatives(alt, rows, own, tol, what):
    """Where the restatement's best and second-best llr of a row (the column `own` left out) differ by more than the llr tolerance,
    alt is the restatement's; elsewhere it is one of the tied columns.  Rows with a NaN give -1.  Returns (tied rows, live rows)."""
    R, C = rows.shape
    tied = PR.tied_rows(rows, own, tol)
    want = PR._summary(rows, own)[1]
    live = ~np.isnan(rows).any(1)
    for r in range(R):
        if not live[r] or not tied[r]:
            assert alt[r] == want[r], f'{what} row {r}: alternative {alt[r]}, the restatement gives {want[r]}'
        else:
            v = np.where(np.arange(C) == own[r], -np.inf, rows[r])
            assert alt[r] != own[r] and 0 <= alt[r] < C and v.max() - v[alt[r]] <= tol[r], f'{what} row {r}: {alt[r]} is not among the tied columns'
    return int(tied[live].sum()), int(live.sum())


@pytest.mark.parametrize('k', range(len(PR.PARITY)))
def test_parity(K, k):
    (lp, tg, il, tl, blank, C), (ll, sub, ins), summary = reference(k)
    step = K.step_error()
    got_ll, got_sub, got_ins, got = on_device(K, lp, tg, il, tl, blank, C)
    assert got_sub.dtype == np.float32 and got_ll.dtype == np.float64 and got[1].dtype == np.int32
    T = il.astype(np.float64)
    e_ll = within(got_ll, ll, PR.loglik_tol(T, step), 'loglik', 'loglik')
    T3 = T[:, None, None]
    e_llr = max(within(got_sub, sub, PR.llr_tol(T3, sub, step), 'sub_llr', 'llr'), within(got_ins, ins, PR.llr_tol(T3, ins, step), 'ins_llr', 'llr'))
    assert (got_ins[:, :, blank][~np.isnan(ins[:, :, blank])] == 0.0).all()
    e_post = 0.0
    for i in (0, 2, 3, 5):
        e_post = max(e_post, within(got[i], summary[i], PR.post_tol(T[:, None], step), ('post', '', 'alt_post', 'gap_post', '', 'gap_alt_post')[i], 'posterior'))
    tol_sub, tol_ins = PR.llr_tol(T3, sub, step).max(-1).reshape(-1), PR.llr_tol(T3, ins, step).max(-1).reshape(-1)
    t1, n1 = check_alternatives(got[1].reshape(-1), sub.reshape(-1, C), tg.astype(np.int64).reshape(-1), tol_sub, 'alt')
    t2, n2 = check_alternatives(got[4].reshape(-1), ins.reshape(-1, C), np.full(tol_ins.shape, blank), tol_ins, 'gap_alt')
    samples, _, pad, pad_labels, _ = PR.PARITY[k]
    print(f'[post gpu] batch {k}: (T, L) {samples} C {C} stride {C + pad} Smax {tg.shape[1]}: |ll - ref| {e_ll:.2e} (budget {PR.loglik_tol(T.max(), step):.2e}), '
          f'llr {e_llr:.2e} (budget {2 * PR.loglik_tol(T.max(), step) + 2.0 ** -22:.2e}), posterior {e_post:.2e} (budget {PR.post_tol(T.max(), step):.2e}), '
          f'tied rows {t1 + t2} of {n1 + n2}')


def test_few_rows_are_tied_and_the_observed_errors():
    """The restatement alone: over all batches at most 2 % of the rows have a best and a second-best alternative within the llr
    tolerance of each other, so `alt` is pinned nearly everywhere.  Prints the largest errors test_parity saw, beside their
    tolerances."""
    tied = rows = 0
    for k in range(len(PR.PARITY)):
        (lp, tg, il, tl, blank, C), (ll, sub, ins), _ = reference(k)
        T3 = il.astype(np.float64)[:, None, None]
        for v, own in ((sub, tg.astype(np.int64).reshape(-1)), (ins, np.full(ins.shape[0] * ins.shape[1], blank))):
            flat = v.reshape(-1, C)
            live = ~np.isnan(flat).any(1)
            tied += int(PR.tied_rows(flat, own, PR.llr_tol(T3, v, PR.STEP_ERROR_CAP).max(-1).reshape(-1))[live].sum())
            rows += int(live.sum())
    print(f'[post gpu] tied rows: {tied} of {rows}')
    for key, (err, tol) in OBSERVED.items():
        print(f'[post gpu] largest {key} error over the parity batches: {err:.3e} (its tolerance {tol:.3e})')
    assert rows > 1000 and tied <= 0.02 * rows


def test_poisoning_stays_inside_the_sample(K):
    k = next(i for i, p in enumerate(PR.PARITY) if p[0][0] == (63, 2) and p[2] == 15)
    (lp, tg, il, tl, blank, C), _, _ = reference(k)
    clean = on_device(K, lp, tg, il, tl, blank, C)
    assert np.isfinite(clean[0][:2]).all()
    label, nan_row, inf_row, beyond = tg.copy(), lp.copy(), lp.copy(), lp.copy()
    label[0, 1] = C                                                          # out of range, inside the transcript
    nan_row[1, 5, 1] = np.nan                                                # inside the sample's frames and classes
    inf_row[0, il[0] - 1, C - 1] = np.inf
    beyond[0, il[0]:, :C] = np.nan                                             # behind input_lengths: never read
    beyond[1, :, C:] = np.inf                                                # behind the classes: never read
    long_t, long_l = il.copy(), tl.copy()
    long_t[1] = lp.shape[1] + 1                                              # T > N
    long_l[0] = tg.shape[1] + 1                                              # L > Smax
    for what, args, bad in (('label', (lp, label, il, tl), 0), ('nan', (nan_row, tg, il, tl), 1), ('+inf', (inf_row, tg, il, tl), 0),
                            ('T > N', (lp, tg, long_t, tl), 1), ('L > Smax', (lp, tg, il, long_l), 0)):
        got = on_device(K, *args, blank, C)
        assert np.isnan(got[0][bad]) and np.isnan(got[1][bad]).all() and np.isnan(got[2][bad]).all(), what
        assert all(np.isnan(v[bad]).all() for v in (got[3][0], got[3][2], got[3][3], got[3][5])) and (got[3][1][bad] == -1).all() and (got[3][4][bad] == -1).all(), what
        for b in range(3):
            if b != bad:
                for u, v in zip(got[:3] + got[3], clean[:3] + clean[3]):
                    assert u[b].tobytes() == v[b].tobytes(), (what, b)
    got = on_device(K, beyond, tg, il, tl, blank, C)
    for u, v in zip(got[:3] + got[3], clean[:3] + clean[3]):
        assert u.tobytes() == v.tobytes()


def test_two_launches_give_the_same_bits(K):
    k = next(i for i, p in enumerate(PR.PARITY) if p[0][0] == (130, 130))
    (lp, tg, il, tl, blank, C), _, _ = reference(k)
    a, b = on_device(K, lp, tg, il, tl, blank, C), on_device(K, lp, tg, il, tl, blank, C)
    for u, v in zip(a[:3] + a[3], b[:3] + b[3]):
        assert u.tobytes() == v.tobytes()


# ---- the product path ---------------------------------------------------------------------------------------------------------------
def on_host(fn):
    def call(*args, **kw):
        out = fn(*[PR.Lattice(*(t.cpu() for t in a)) if isinstance(a, tuple) else a.cpu() if torch.is_tensor(a) else a for a in args], **kw)
        return type(out)(*(o.cuda() for o in out)) if hasattr(out, '_fields') else tuple(o.cuda() for o in out)
    return call


def patch_restatements(monkeypatch, K):
    monkeypatch.setattr(K, 'lattice', on_host(PR.op_lattice))
    monkeypatch.setattr(K, 'neighbours', on_host(PR.op_neighbours))
    monkeypatch.setattr(K, 'slots', on_host(PR.op_slots))


def compare_confidences(got, want, T, step, what):
    """Two PosteriorConfidence-like sextuples of lists: posteriors within the contract's tolerance, alternatives equal unless tied
    (then their posteriors agree within it)."""
    tol = float(PR.post_tol(T, step))
    for i in (0, 2, 3, 5):
        a, b = np.asarray(got[i], dtype=np.float64), np.asarray(want[i], dtype=np.float64)
        assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and (np.abs(a - b)[~np.isnan(a)] <= tol).all(), (what, i)
    for i in (1, 4):
        assert all(x == y or abs(p - q) <= tol for x, y, p, q in zip(got[i], want[i], got[i + 1], want[i + 1])), (what, i)


def test_long_form_against_the_restatements(K, monkeypatch):
    from lcasr_amd.decoding import posterior as D
    rng = np.random.default_rng(41)
    N, C, blank = 300, 40, 39
    spans, f = [], 3
    while f + 6 < N:
        run = int(rng.integers(1, 3))
        spans.append((f, f + run))
        f += run + int(rng.integers(0, 9))
    tokens = [int(v) for v in rng.integers(0, C - 1, size=len(spans))]
    x = rng.normal(size=(N, C))
    x[:, blank] += 3.0
    for (s, e), t in zip(spans, tokens):
        x[s:e, t] += 7.0
    lp = torch.from_numpy(x.astype(np.float32)).cuda()
    pieces = D.cut_pieces(spans, N, 64, K.max_labels())
    assert len(pieces) >= 4 and pieces == PR.cut_pieces(spans, N, 64, K.max_labels())
    got = [v.cpu().tolist() for v in D.posterior_confidence_long(lp, tokens, spans, blank, max_frames=64)]
    assert len(got[0]) == len(tokens) and len(got[3]) == len(tokens) + 1 and not np.isnan(got[0]).any()
    patch_restatements(monkeypatch, K)
    want = [v.cpu().tolist() for v in D.posterior_confidence_long(lp, tokens, spans, blank, max_frames=64)]
    compare_confidences(got, want, max(p[3] - p[2] for p in pieces), K.step_error(), 'long form')
    assert 0.05 < np.mean(np.asarray(got[0]) < 0.999)                        # not every token is certain: the figures are not trivial


class IdTok:
    """Every token is a word: id i is spelt 't<i>'."""
    def __init__(self, V): self.V = V
    def vocab_size(self): return self.V
    def decode(self, ids): return ' '.join(f't{int(i)}' for i in ids)
    def encode(self, text): return [int(w[1:]) for w in text.split()]


CFG = dict(vocab_size=127, n_layers=2, d_model=64, n_heads=2, head_dim=32, subsampling_conv_channels=32, use_rotary=True,
           rotary_base_freq=1500000, decoder_norm=True, self_conditioning=True, bias_in_ff=False, default_norm='layer_norm')


def test_transcribe_detail_on_the_tiny_model_against_the_restatements(K, monkeypatch):
    import audio_refs as AUD
    from lcasr_amd.eval import run as R
    from lcasr_amd.models.sconformer_xl import SCConformerXL
    torch.manual_seed(12345)
    model = SCConformerXL(**CFG).cuda().eval()
    tok = IdTok(127)
    wave = AUD.test_signal(3 * 16000, seed=9).cuda()
    plain = R.transcribe_detail(model, wave, tok, 128, 32)
    results = {}
    for width in (1, 4):
        results[width] = R.transcribe_detail(model, wave, tok, 128, 32, beam_width=width, posterior=True)
    assert {k: results[1][k] for k in plain if k != 'words'} == {k: plain[k] for k in plain if k != 'words'}
    assert [{k: v for k, v in w.items() if k != 'posterior'} for w in results[1]['words']] == plain['words']
    patch_restatements(monkeypatch, K)
    for width, got in results.items():
        want = R.transcribe_detail(model, wave, tok, 128, 32, beam_width=width, posterior=True)
        n = len(got['tokens'])
        assert n >= 1 and got['tokens'] == want['tokens'] and len(got['token_posterior']) == n == len(got['token_alternative'])
        g = (got['token_posterior'], [a['token'] for a in got['token_alternative']], [a['posterior'] for a in got['token_alternative']])
        w = (want['token_posterior'], [a['token'] for a in want['token_alternative']], [a['posterior'] for a in want['token_alternative']])
        compare_confidences(g + g, w + w, 2048, K.step_error(), f'beam width {width}')
        assert all(0.0 < p <= 1.0 for p in got['token_posterior'])
        assert [x['posterior'] for x in got['words']] == pytest.approx([x['posterior'] for x in want['words']], abs=float(PR.post_tol(2048, K.step_error())))
