"""The confidence kernels on the device (csrc/confid.hip through lcasr_amd.hip.confid) against the float64 restatement of the contract
(tests/confid_refs.py): idx, targets, spans and target_lengths EXACTLY, min / max aggregates bit for bit, confidences within
4 d32 + 1e-6 with d32 = max |float32 restatement - float64 restatement| ON THE SAME INPUT (confid_refs.tolerance), mean and prod
aggregates within the rounding of n float32 operations.  Each case prints d32 and the device's largest error."""
import math

import numpy as np
import pytest
import torch

import confid_refs as CR

pytestmark = pytest.mark.gpu
NAN, INF = math.nan, math.inf
ALPHAS = (1 / 3, 1 / 2, 1.0, 2.0)
SWEEP = [('max_prob', 'lin', 1 / 3), ('shannon', 'lin', 1 / 3), ('shannon', 'exp', 1 / 3)] + \
        [(m, n, a) for m in ('tsallis', 'renyi') for n in CR.NORMS for a in ALPHAS]


@pytest.fixture(scope='module')
def K():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from lcasr_amd.hip import confid
    confid.load()
    return confid


def rows_of_every_kind(M, classes, stride, seed):
    """(M, stride) f32: rows cycle through random, peaky (x 20), one-hot via -inf, uniform, an exact tie (the first index wins; the
    two maxima sit in different lanes), a NaN, all -inf; the columns behind `classes` hold NaN."""
    rng = np.random.default_rng(seed)
    x = np.full((M, stride), NAN, dtype=np.float32)
    body = rng.normal(size=(M, classes)).astype(np.float32)
    for r in range(M):
        kind = r % 7
        if kind == 1: body[r] *= 20
        elif kind == 2: body[r] = -INF; body[r, (3 * r) % classes] = 0.5
        elif kind == 3: body[r] = -2.25
        elif kind == 4: body[r, classes - 1] = body[r, 1 % classes] = body[r].max() + 1
        elif kind == 5: body[r, (5 * r) % classes] = NAN
        elif kind == 6: body[r] = -INF
    x[:, :classes] = body
    return x


def class_counts(K):
    cap = K.row_capacity()
    issue = [2, 3, 129, 144, 256, 257, cap - 1, cap, cap + 1, 4 * cap + 3]
    block = K.block_capacity()                                             # and both sides of every other change of geometry
    return issue + [64, 65, 128, 192, 193, 512, 513, block, block + 1]


def check_frames(K, x, dev, M, classes, method, norm, alpha, tag):
    idx, conf = K.frames(dev[:M, :classes] if dev.shape[1] > classes else dev[:M], classes, method, norm, alpha)
    want_i, want_c = CR.frames(x[:M], classes, method, norm, alpha)
    tol, d32 = CR.tolerance(x[:M], classes, method, norm, alpha)
    got_i, got_c = idx.cpu().numpy(), conf.cpu().numpy().astype(np.float64)
    assert got_i.dtype == np.int32 and (got_i == want_i).all(), f'{tag}: idx differs at rows {np.nonzero(got_i != want_i)[0][:5]}'
    bad = np.isnan(want_c)
    assert (np.isnan(got_c) == bad).all() and (got_i[bad] == -1).all()
    err = float(np.abs(got_c[~bad] - want_c[~bad]).max()) if (~bad).any() else 0.0
    assert err <= tol, f'{tag}: max err {err:.3e} > 4 * {d32:.3e} + 1e-6'
    return idx, conf, d32, err


@pytest.mark.parametrize('which', range(19))
def test_frames_at_every_row_count_and_stride(K, which):
    from lcasr_amd.hip import ops
    classes = class_counts(K)[which]
    for stride in (classes, classes + 15):
        x = rows_of_every_kind(257, classes, stride, seed=which)
        dev = torch.from_numpy(x).cuda()
        worst = (0.0, 0.0)
        for M in (1, 3, 4, 5, 257):
            idx, conf, d32, err = check_frames(K, x, dev, M, classes, 'tsallis', 'exp', 1 / 3, f'classes {classes} stride {stride} M {M}')
            worst = max(worst, (err, d32))
            again = K.frames(dev[:M, :classes] if stride > classes else dev[:M], classes, 'tsallis', 'exp', 1 / 3)
            assert torch.equal(again[0], idx) and torch.equal(again[1].view(torch.int32), conf.view(torch.int32))     # two calls: the same bits
            if classes % 4 == 0 and stride == classes:
                ok = idx >= 0
                assert torch.equal(ops.argmax_rows(dev[:M])[ok], idx[ok])
        print(f'[confid gpu] classes {classes} stride {stride}: d32 {worst[1]:.2e}, device err {worst[0]:.2e}')


@pytest.mark.parametrize('which', range(19))
def test_every_measure_and_alpha(K, which):
    classes = class_counts(K)[which]
    for stride in (classes, classes + 15):
        x = rows_of_every_kind(16, classes, stride, seed=100 + which)
        dev = torch.from_numpy(x).cuda()
        for method, norm, alpha in SWEEP:
            _, _, d32, err = check_frames(K, x, dev, 16, classes, method, norm, alpha, f'{method}/{norm}/{alpha:.3f} classes {classes} stride {stride}')
            print(f'[confid gpu] {method}/{norm} alpha {alpha:.3f} classes {classes} stride {stride}: d32 {d32:.2e}, device err {err:.2e}')
    with pytest.raises(RuntimeError, match='max_prob has no exp'):
        K.frames(dev, classes, 'max_prob', 'exp')
    with pytest.raises(RuntimeError, match='alpha'):
        K.frames(dev, classes, 'renyi', 'lin', 5.0)


def sequences(chunk, N, seed):
    """(3, N) int32, lengths [0, 1, N], blank 0: row 2 holds a run across the first chunk boundary, alternating labels, a stretch of
    blanks, and an invalid frame inside a run."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, 4, size=(3, N)).astype(np.int32)                 # short random runs with blanks
    r = idx[2]
    r[max(chunk - 4, 0):chunk + 3] = 5                                     # straddles the boundary (where N reaches it)
    r[10:40] = np.tile([6, 7], 15)                                         # alternating: a label per frame
    r[50:90] = 0
    r[100:110] = 9; r[104] = -1                                            # two runs of 9
    return idx, [0, 1, N]


@pytest.mark.parametrize('span', ['chunk-1', 'chunk', '2chunk+1'])
def test_runs(K, span):
    chunk = K.scan_chunk()
    N = {'chunk-1': chunk - 1, 'chunk': chunk, '2chunk+1': 2 * chunk + 1}[span]
    idx, lengths = sequences(chunk, N, seed=N)
    dev, il = torch.from_numpy(idx).cuda(), torch.tensor(lengths, dtype=torch.int32).cuda()
    count = int(CR.runs(idx, lengths, 0)[2][2])
    assert 100 < count < N
    for s_cap, lens in ((None, lengths), (count, lengths), (count - 1, lengths), (7, None), (0, lengths)):
        tg, sp, tl = K.runs(dev, None if lens is None else il, 0, s_cap)
        want = CR.runs(idx, lens, 0, s_cap)
        for got, ref, name in zip((tg, sp, tl), want, ('targets', 'spans', 'target_lengths')):
            assert got.dtype == torch.int32 and got.shape == ref.shape and (got.cpu().numpy() == ref).all(), f'{name} at S_cap {s_cap}'
        if s_cap == count: assert tl.tolist() == [0, 1 if idx[1, 0] > 0 else 0, count]
        if s_cap == count - 1: assert int(tl[2]) == -1
    blank = np.full((2, N), 3, dtype=np.int32)                              # all blank; and all one label
    for b in (3, 4):
        got = K.runs(torch.from_numpy(blank).cuda(), None, b, 5)
        for g, ref in zip(got, CR.runs(blank, None, b, 5)):
            assert (g.cpu().numpy() == ref).all()


def test_aggregate(K):
    x = np.random.default_rng(5).normal(size=(1200, 16)).astype(np.float32) * 2
    x[700, 3] = NAN                                                         # one invalid frame: a NaN among the values
    idx, conf = K.frames(torch.from_numpy(x).cuda(), 16, 'shannon', 'lin')
    values = conf.cpu().numpy()
    blank = 2
    idx = idx.clone(); idx[300:320] = blank; idx[5] = -1
    spans = [[0, 0], [7, 8], [10, 73], [10, 74], [10, 75], [100, 1100], [20, 60], [300, 320], [5, 6], [-1, 4], [1190, 1201], [9, 3],
             [650, 750], [0, 1200], [1199, 1200], [1200, 1200]]
    sp = torch.tensor(spans, dtype=torch.int32).cuda()
    for exclude in (False, True):
        ia, ih = (idx, idx.cpu().numpy()) if exclude else (None, None)
        for agg in CR.AGGS:
            got = K.aggregate(conf, sp, agg, ia, blank).cpu().numpy()
            want = CR.aggregate(values, spans, agg, ih, blank)
            assert (np.isnan(got) == np.isnan(want)).all(), (agg, exclude)
            through_700 = [] if exclude else [5, 12, 13]                  # the invalid frame is skipped with its idx of -1
            assert np.isnan(want[[0, 9, 10, 11, 15] + through_700]).all() and int(np.isnan(want).sum()) == 5 + len(through_700)
            ok = ~np.isnan(want)
            if agg in ('min', 'max'):
                assert (got[ok] == want[ok].astype(np.float32)).all()     # one of the values, bit for bit
                continue
            n = np.array([b - a for a, b in spans])[ok]
            # n float32 operations, each within 2^-24 of a partial result no larger than the final bound: |values| <= 1
            bound = (n + 2) * 2.0 ** -24 * (np.abs(want[ok]) if agg == 'prod' else 1.0) * 1.01 + 1e-37
            err = np.abs(got[ok].astype(np.float64) - want[ok])
            assert (err <= bound).all(), (agg, exclude, err.max())
            print(f'[confid gpu] aggregate {agg} exclude_blank {exclude}: max err / bound {float((err / bound).max()):.3f}')
    assert torch.equal(K.aggregate(conf, sp, 'mean').view(torch.int32), K.aggregate(conf, sp, 'mean').view(torch.int32))


def test_greedy_confidence_end_to_end(K):
    from lcasr_amd.decoding import confidence as D
    rng = np.random.default_rng(8)
    x = np.full((2, 300, 144), NAN, dtype=np.float32)
    x[:, :, :129] = rng.normal(size=(2, 300, 129)).astype(np.float32) * 4
    x[:, :, 128] += 4                                                       # the blank is often the argmax
    x[1, 200:, :129] = x[1, 199:200, :129]                                  # a long run
    dev = torch.from_numpy(x).cuda()[:, :, :129]                           # a row stride of 144
    for cfg in (D.ConfidenceConfig(), D.ConfidenceConfig(entropy_type='renyi', alpha=0.5, entropy_norm='lin', aggregation='mean', exclude_blank=False)):
        method, norm = cfg.measure
        g = D.greedy_confidence(dev, 128, cfg, lengths=[300, 250])
        want, fc = CR.greedy(x[:, :, :129], 128, method, norm, cfg.alpha, cfg.aggregation, cfg.exclude_blank, [300, 250])
        tol, d32 = CR.tolerance(x.reshape(600, 144), 129, method, norm, cfg.alpha)
        assert float(np.abs(g.frame_confidence.cpu().numpy() - fc).max()) <= tol
        for b in range(2):
            assert g.tokens[b] == want[b][0] and g.spans[b] == want[b][1] and len(g.tokens[b]) > 20
            assert float(np.abs(np.array(g.token_confidence[b]) - want[b][2]).max()) <= tol + 300 * 2.0 ** -24      # (the mean's own rounding)
        one = D.greedy_confidence(dev[0], 128, cfg)
        assert one.tokens == g.tokens[0] and one.token_confidence == g.token_confidence[0]


@pytest.mark.parametrize('method, norm', CR.MEASURES)
def test_corrupted_tokens_score_below_clean_ones_on_the_device(K, method, norm):
    from lcasr_amd.decoding import confidence as D
    lp, labels, bad = CR.planted()
    dev = torch.from_numpy(lp).cuda()
    for agg in CR.AGGS:
        if (method, agg) == ('max_prob', 'mean'):
            continue
        (ref,), _ = CR.greedy(lp[None], 31, method, norm, 1 / 3, agg, True)
        assert ref[0] == labels and max(c for k, c in enumerate(ref[2]) if k in bad) < min(c for k, c in enumerate(ref[2]) if k not in bad)
        cfg = D.ConfidenceConfig(method='max_prob') if method == 'max_prob' else D.ConfidenceConfig(entropy_type=method, entropy_norm=norm)
        g = D.greedy_confidence(dev, 31, D.ConfidenceConfig(**{**cfg.__dict__, 'aggregation': agg}))
        assert g.tokens == labels
        assert max(c for k, c in enumerate(g.token_confidence) if k in bad) < min(c for k, c in enumerate(g.token_confidence) if k not in bad)


class IdTok:
    """Every token is a word: id i is spelt 't<i>'."""
    def __init__(self, V): self.V = V
    def vocab_size(self): return self.V
    def decode(self, ids): return ' '.join(f't{int(i)}' for i in ids)
    def encode(self, text): return [int(w[1:]) for w in text.split()]


CFG = dict(vocab_size=127, n_layers=2, d_model=64, n_heads=2, head_dim=32, subsampling_conv_channels=32, use_rotary=True,
           rotary_base_freq=1500000, decoder_norm=True, self_conditioning=True, bias_in_ff=False, default_norm='layer_norm')


def test_transcribe_detail_on_the_tiny_model(K):
    import audio_refs as AUD
    from lcasr_amd.eval import run as R
    from lcasr_amd.models.sconformer_xl import SCConformerXL
    from lcasr_amd.utils import audio_tools as A
    torch.manual_seed(12345)
    model = SCConformerXL(**CFG).cuda().eval()
    wave = AUD.test_signal(3 * 16000, seed=9).cuda()
    tok, blank = IdTok(127), model.decoder.num_classes - 1
    sec = model.subsampling.subsampling_factor * A.HOP_LENGTH / A.SR
    logits = R.moving_average_eval(R._Args(), model, A.to_spectogram(wave[None]), 128, 32, tok, use_tqdm=False, return_numpy=False)
    lp = logits.float().cpu().numpy()
    tol, d32 = CR.tolerance(lp, None, 'tsallis', 'exp', 1 / 3)
    d = R.transcribe_detail(model, wave, tok, 128, 32)
    (want,), fc = CR.greedy(lp[None], blank, 'tsallis', 'exp', 1 / 3, 'min', True)
    assert d['tokens'] == want[0] and d['text'] == R.transcribe(model, wave, tok, 128, 32) == tok.decode(want[0]) and len(want[0]) > 0
    assert float(np.abs(np.array(d['token_confidence']) - want[2]).max()) <= tol
    assert [(w['word'], w['startTime'], w['endTime']) for w in d['words']] == \
        [(f't{i}', f'{s[0] * sec:.2f}s', f'{s[1] * sec:.2f}s') for i, s in zip(want[0], want[1])]
    assert [w['confidence'] for w in d['words']] == d['token_confidence']
    b = R.transcribe_detail(model, wave, tok, 128, 32, beam_width=4)
    assert b['text'] == R.transcribe(model, wave, tok, 128, 32, beam_width=4) == tok.decode(b['tokens']) and len(b['tokens']) > 0
    starts = [round(float(w['startTime'][:-1]) / sec) for w in b['words']]
    assert starts == sorted(starts) and len(starts) == len(b['tokens'])
    wi, wc = CR.frames(lp, None, 'tsallis', 'exp', 1 / 3)
    # the frames are read back from the times only where 0.01 s resolves a frame; the spans come from the search itself
    from lcasr_amd.decoding.beam import BeamSearchCTCDecoder
    out = BeamSearchCTCDecoder(tokenizer=tok, blank_id=blank, beam_width=4)._search(logits, nbest=1)
    fr = out.token_frames[0, :int(out.lengths[0])].tolist()
    spans = [[f, g] for f, g in zip(fr, fr[1:] + [lp.shape[0]])]
    assert float(np.abs(np.array(b['token_confidence']) - CR.aggregate(wc, spans, 'min', wi, blank)).max()) <= tol
    print(f'[confid gpu] tiny model: {len(want[0])} greedy tokens, {len(fr)} beam tokens, d32 {d32:.2e}')
