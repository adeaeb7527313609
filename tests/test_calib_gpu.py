"""The calibration kernels on the device (csrc/calib.hip through lcasr_amd.hip.calib): the edit alignment bit-equal to the numpy
restatement (tests/calib_refs.py) with counts bit-equal to sconf_edit_counts on the same buffers, at the sizes the geometry queries
name; the temperature sweep bit-equal to sconf_confid_frames in its column at temperature 1, and within the confidence unit's own
tolerance (confid_refs.tolerance on the scaled input: 4 d32 + 1e-6) of the float64 restatement everywhere else; and eval.run.calibrate
on a tiny random-weight model against the same call with the restatements in the kernels' place."""
import math

import numpy as np
import pytest
import torch

import calib_refs as AR
import confid_refs as CR
from test_confid_gpu import rows_of_every_kind

pytestmark = pytest.mark.gpu
KINDS = ('identical', 'edits', 'disjoint', 'two')


@pytest.fixture(scope='module')
def K():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from lcasr_amd.hip import calib
    calib.load()
    return calib


def run_pairs(K, pairs, short=(), compare_counts=True):
    """One launch over `pairs` [(hyp, ref)], each slice of the workspace exactly what its pair needs (16 bytes less for the pairs in
    `short`), against the restatement; the counts against sconf_edit_counts on the same device buffers."""
    from lcasr_amd.hip import ops
    hyp = np.concatenate([p[0] for p in pairs] + [np.zeros(0, np.int32)]).astype(np.int32)
    ref = np.concatenate([p[1] for p in pairs] + [np.zeros(0, np.int32)]).astype(np.int32)
    ho = np.cumsum([0] + [len(p[0]) for p in pairs]).astype(np.int64)
    ro = np.cumsum([0] + [len(p[1]) for p in pairs]).astype(np.int64)
    sizes = [AR.pair_bytes(len(h), len(r)) for h, r in pairs]
    for n, (h, r) in zip(sizes, pairs):
        assert n == K.load().sconf_edit_align_pair_bytes(len(h), len(r))
    sizes = [max(n, 0) - (16 if p in short else 0) for p, n in enumerate(sizes)]
    assert min(sizes) >= 0
    wo = np.cumsum([0] + sizes).astype(np.int64)
    dev = [torch.from_numpy(a).cuda() for a in (hyp, ho, ref, ro, wo)]
    ws = torch.empty(max(int(wo[-1]), 16), dtype=torch.uint8, device='cuda')
    h2r, r2h, counts = K.edit_align(*dev, ws)
    want = AR.align_batch(hyp, ho, ref, ro, wo)
    for got, ref_, name in zip((h2r, r2h, counts), want, ('hyp_to_ref', 'ref_to_hyp', 'counts')):
        got = got.cpu().numpy()
        assert got.dtype == ref_.dtype and got.shape == ref_.shape, name
        assert (got == ref_).all(), f'{name}: first difference at {np.argwhere(got != ref_)[:3].tolist()}'
    if compare_counts:
        assert torch.equal(counts, ops.edit_counts(dev[0], dev[1], dev[2], dev[3]))
    return want


def geometry_sizes(K):
    """(H, R) at the sizes where the kernel's path changes, all from the queries."""
    strip, pas, rows, cpw = K.strip_cols(), K.pass_cols(), K.block_rows(), K.cells_per_word()
    sizes = []
    for q in (strip, rows):
        sizes += [(v, v) for v in (q - 1, q, q + 1)]
    sizes += [(v, 70) for v in (cpw - 1, cpw, cpw + 1, 2 * cpw - 1, 2 * cpw + 1)]           # H around the packing
    sizes += [(70, v) for v in (cpw - 1, cpw, cpw + 1, 2 * cpw - 1, 2 * cpw + 1)]           # R likewise: the cells of a word are columns
    sizes += [(20, pas - 1), (20, pas), (300, pas + 1), (rows + 1, pas + strip + 1), (1, 1), (1, strip + 1), (rows + 1, 1)]
    sizes += [(0, 5), (5, 0), (0, 0)]
    return sizes


@pytest.mark.parametrize('kind', KINDS)
def test_alignment_at_the_sizes_of_the_geometry(K, kind):
    sizes = geometry_sizes(K)
    pairs = [AR.pair_case(kind, H, R, seed=n) for n, (H, R) in enumerate(sizes)]
    h2r, r2h, counts = run_pairs(K, pairs)
    if kind == 'identical':
        assert all(int(counts[n, 0]) == 0 for n, (H, R) in enumerate(sizes) if H == R)
    if kind == 'disjoint':
        assert all(int(counts[n, 0]) == max(H, R) for n, (H, R) in enumerate(sizes))
    print(f'[calib gpu] {kind}: {len(pairs)} pairs, {int((counts[:, 0] > 0).sum())} with errors, errors {int(counts[:, 0].sum())}')


def test_alignment_of_no_pairs_launches_nothing(K):
    e32, e64 = torch.zeros(0, dtype=torch.int32, device='cuda'), torch.zeros(1, dtype=torch.int64, device='cuda')
    h2r, r2h, counts = K.edit_align(e32, e64, e32, e64, e64, None)
    assert h2r.numel() == 0 and r2h.numel() == 0 and tuple(counts.shape) == (0, 4)


def test_an_undersized_slice_and_an_overlong_pair_are_refused_alone(K):
    rows, strip, cap = K.block_rows(), K.strip_cols(), K.max_len()
    sizes = [(40, 50), (rows + 5, strip + 9), (33, 20), (cap + 1, 1), (7, 9), (1, cap + 1), (12, 12), (cap, 3), (3, cap)]
    pairs = [AR.pair_case('edits' if max(s) < cap else 'two', *s, seed=n) for n, s in enumerate(sizes)]
    h2r, r2h, counts = run_pairs(K, pairs, short=(1,), compare_counts=False)
    assert counts[:, 0].tolist()[1] == -1 and counts[3].tolist() == [-1] * 4 and counts[5].tolist() == [-1] * 4
    assert all(int(counts[p, 0]) >= 0 for p in (0, 2, 4, 6)) and counts[7, 0] >= cap - 3 and counts[8, 0] >= cap - 3       # the longest pairs taken
    ho = np.cumsum([0] + [s[0] for s in sizes])
    assert (h2r[ho[1]:ho[2]] == -1).all() and (h2r[ho[3]:ho[4]] == -1).all() and (h2r[ho[2]:ho[3]] >= 0).any()


def test_one_large_pair(K):
    hyp, ref = AR.pair_case('edits', 3001, 2999, seed=77)
    _, _, counts = run_pairs(K, [(hyp, ref)])
    assert 150 < int(counts[0, 0]) < 600


# ---- the sweep ------------------------------------------------------------------------------------------------------------------
def sweep_classes(K):
    from lcasr_amd.hip import confid
    return [(8, 8), (129, 144), (257, 257), (confid.row_capacity() + 1, confid.row_capacity() + 1),
            (confid.block_capacity() + 1, confid.block_capacity() + 1)]


@pytest.mark.parametrize('geometry', range(5))
@pytest.mark.parametrize('method, norm', CR.MEASURES)
def test_sweep(K, geometry, method, norm):
    """K in {1, 3, max}: the column at temperature 1 is sconf_confid_frames bit for bit, idx is its idx, every column is within the
    confidence unit's tolerance on the scaled input, a factor that is not finite and positive gives a NaN column."""
    from lcasr_amd.hip import confid
    classes, stride = sweep_classes(K)[geometry]
    M = 14 if classes <= 1025 else 7                                         # every kind of row of rows_of_every_kind, invalid ones included
    alpha = 1 / 3
    x = rows_of_every_kind(M, classes, stride, seed=geometry)
    dev = torch.from_numpy(x).cuda()
    view = dev[:, :classes] if stride > classes else dev
    idx1, conf1 = confid.frames(view, classes, method, norm, alpha)
    kmax = K.max_temps()
    grids = {1: [1.0], 3: [0.5, 1.0, 1.7], kmax: [1.0] + [1.0 / t for t in np.linspace(0.4, 3.0, kmax - 1)]}
    assert kmax >= 16 and len(grids[kmax]) == kmax
    tol_of = {}
    for Kn, inv in grids.items():
        it = torch.tensor(inv, dtype=torch.float32, device='cuda')
        idx, conf = K.frames_sweep(view, it, classes, method, norm, alpha)
        assert tuple(conf.shape) == (Kn, M) and torch.equal(idx, idx1)
        one = inv.index(1.0)
        assert torch.equal(conf[one].view(torch.int32), conf1.view(torch.int32)), f'K {Kn}: the column at temperature 1 is not sconf_confid_frames'
        want_i, want = AR.sweep(x, inv, classes, method, norm, alpha)
        got = conf.cpu().numpy().astype(np.float64)
        assert (idx.cpu().numpy() == want_i).all() and (np.isnan(got) == np.isnan(want)).all()
        for k, v in enumerate(inv):
            if v not in tol_of:
                tol_of[v] = AR.sweep_tolerance(x, v, classes, method, norm, alpha)
            tol, d32 = tol_of[v]
            ok = ~np.isnan(want[k])
            err = float(np.abs(got[k][ok] - want[k][ok]).max())
            print(f'[calib gpu] sweep {method}/{norm} classes {classes}/{stride} K {Kn} 1/T {v:.3f}: d32 {d32:.2e}, device err {err:.2e}')
            assert err <= tol, f'1/T {v}: max err {err:.3e} > 4 * {d32:.3e} + 1e-6'
    bad = torch.tensor([1.0, 0.0, -2.0, math.inf, math.nan, 2.0], dtype=torch.float32, device='cuda')
    idx, conf = K.frames_sweep(view, bad, classes, method, norm, alpha)
    assert torch.equal(idx, idx1) and torch.equal(conf[0].view(torch.int32), conf1.view(torch.int32))
    assert bool(torch.isnan(conf[1:5]).all()) and torch.equal(torch.isnan(conf[5]), torch.isnan(conf1))
    with pytest.raises(RuntimeError, match='temperatures'):
        K.frames_sweep(view, torch.ones(kmax + 1, device='cuda'), classes, method, norm, alpha)
    with pytest.raises(RuntimeError, match='temperatures'):
        K.frames_sweep(view, torch.ones(0, device='cuda'), classes, method, norm, alpha)


# ---- end to end -----------------------------------------------------------------------------------------------------------------
class IdTok:
    """Every token is a word: id i is spelt 't<i>'."""
    def __init__(self, V): self.V = V
    def vocab_size(self): return self.V
    def decode(self, ids): return ' '.join(f't{int(i)}' for i in ids)
    def encode(self, text): return [int(w[1:]) for w in text.split()]


CFG = dict(vocab_size=127, n_layers=2, d_model=64, n_heads=2, head_dim=32, subsampling_conv_channels=32, use_rotary=True,
           rotary_base_freq=1500000, decoder_norm=True, self_conditioning=True, bias_in_ff=False, default_norm='layer_norm')


def test_calibrate_on_the_tiny_model_against_the_restatements(K, monkeypatch):
    """eval.run.calibrate on a tiny random-weight model, then the same call with the unit's two ops replaced by the numpy
    restatements (fed from the device's log-scores, through CPU copies): the same labels, confusion pairs and chosen temperature,
    the metrics within 1e-9."""
    import audio_refs as AUD
    from lcasr_amd.eval import run as R
    from lcasr_amd.models.sconformer_xl import SCConformerXL
    from lcasr_amd.utils import audio_tools as A
    torch.manual_seed(12345)
    model = SCConformerXL(**CFG).cuda().eval()
    tok, blank = IdTok(127), model.decoder.num_classes - 1
    temps = [0.5, 0.8, 1.0, 1.25, 2.0]
    recs = []
    for seed in (9, 10):
        spec = A.to_spectogram(AUD.test_signal(3 * 16000, seed=seed).cuda()[None])
        ids = tok.encode(R._decoder(model, tok, 1)(R.moving_average_eval(R._Args(), model, spec, 128, 32, tok, use_tqdm=False, return_numpy=False)))
        gold = [r for k, r in enumerate(ids) if k % 5 != 2]
        gold = [(r + 1) % blank if k % 4 == 1 else r for k, r in enumerate(gold)] + [1, 2]
        recs.append((f'rec{seed}', spec, tok.decode(gold)))
    got = R.calibrate(model, recs, tok, 128, 32, temperatures=temps)
    assert got['words'] > 6 and 0 < sum(got['labels']) < got['words'] and got['temperature'] in temps

    def on_host(fn):
        def call(*args, **kw):
            out = fn(*[a.cpu() if torch.is_tensor(a) else a for a in args], **kw)
            return tuple(o.cuda() for o in out)
        return call
    monkeypatch.setattr(K, 'edit_align', on_host(AR.op_edit_align))
    monkeypatch.setattr(K, 'frames_sweep', on_host(AR.op_frames_sweep))
    want = R.calibrate(model, recs, tok, 128, 32, temperatures=temps)
    assert got['labels'] == want['labels'] and got['confusion_pairs'] == want['confusion_pairs'] and got['temperature'] == want['temperature']
    for k, (a, b) in enumerate(zip(got['metrics'], want['metrics'])):
        for key in a:
            print(f'[calib gpu] calibrate T {temps[k]} {key}: device {a[key]!r} restatement {b[key]!r}')
    for a, b in zip(got['metrics'], want['metrics']):
        for key in a:
            assert a[key] == pytest.approx(b[key], abs=1e-9, nan_ok=True), key
