"""CPU tests of the confidence scores: the properties of the restatement (tests/confid_refs.py), hand cases of the runs and of the
aggregation, the twelfth ABI unit's header, binding, queries and refusals (host-only calls), and the Python surface -
decoding.confidence, GreedyCTCDecoder(confidence=), eval.run.transcribe_detail and align(confidence=) - with the unit's three ops
replaced by the restatement.  The HIP kernels themselves are tested in test_confid_gpu.py."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import align_refs as AR
import audio_refs as AUD
import beam_refs as BR
import confid_refs as CR
import eval_refs as E
from cabi_header import assert_binding_is_header, header_abi
from common_model import build_from_fixture
from conftest import ROOT, load_golden

HEADER, PREFIX = 'sconf_confid.h', 'sconf_confid_'
NAMES = {'sconf_confid_row_capacity', 'sconf_confid_block_capacity', 'sconf_confid_scan_chunk', 'sconf_confid_frames', 'sconf_confid_runs', 'sconf_confid_aggregate'}
NAN = math.nan


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from lcasr_amd.hip import confid
    return confid.load()


@pytest.fixture
def emulated(monkeypatch):
    """The unit's three ops (lcasr_amd.hip.confid) replaced by their restatements: host logic without a GPU."""
    from lcasr_amd.decoding import confidence as K
    # the surface moves CPU input to the device wherever one is present (confidence._on_device, calibration, wer._device, the
    # decoders); the restatements are numpy, so the move is pinned to the CPU: the same run with and without a GPU
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    monkeypatch.setattr(K.confid_kernels, 'frames', CR.op_frames)
    monkeypatch.setattr(K.confid_kernels, 'runs', CR.op_runs)
    monkeypatch.setattr(K.confid_kernels, 'aggregate', CR.op_aggregate)
    return K


# ---- 1. properties of the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('V', [2, 3, 129])
@pytest.mark.parametrize('method, norm', CR.MEASURES)
def test_one_hot_is_1_uniform_is_0_and_the_path_between_is_monotone(V, method, norm):
    for alpha in (1 / 3, 0.5, 2.0):
        one_hot = np.full(V, -np.inf); one_hot[V // 2] = 3.0
        assert CR.frame_row(one_hot, method, norm, alpha) == (V // 2, pytest.approx(1.0, abs=1e-12))
        assert CR.frame_row(np.full(V, -1.5), method, norm, alpha) == (0, pytest.approx(0.0, abs=1e-12))
        path = []
        for lam in np.linspace(0.0, 1.0, 41)[:-1]:                         # p = (1 - lam) uniform + lam one-hot
            p = np.full(V, (1 - lam) / V); p[1] += lam
            path.append(CR.frame_row(np.log(p), method, norm, alpha)[1])
        assert all(b > a for a, b in zip(path, path[1:])) and path[0] == pytest.approx(0.0, abs=1e-12) and path[-1] < 1.0


@pytest.mark.parametrize('norm', CR.NORMS)
def test_tsallis_and_renyi_meet_shannon_at_alpha_1(norm):
    rng = np.random.default_rng(1)
    for V in (2, 7, 129):
        row = rng.normal(size=V) * 3
        want = CR.frame_row(row, 'shannon', norm, 1.0)[1]
        for method in ('tsallis', 'renyi'):
            assert CR.frame_row(row, method, norm, 1.0)[1] == want
            for alpha in (1 - 1e-6, 1 + 1e-6):
                assert abs(CR.frame_row(row, method, norm, alpha)[1] - want) < 1e-5


@pytest.mark.parametrize('method, norm', CR.MEASURES)
def test_minus_inf_entries_count_as_zero_probability(method, norm):
    """-inf entries add 0 to every sum: the entropy is that of the row without them; only the normalisation knows V."""
    rng = np.random.default_rng(2)
    row = rng.normal(size=9)
    wide = np.concatenate([row[:4], [-np.inf, -np.inf], row[4:], [-np.inf]])
    i, c = CR.frame_row(wide, method, norm, 0.5)
    j, small = CR.frame_row(row, method, norm, 0.5)
    assert i == (j if j < 4 else j + 2)
    p = np.exp(row - row.max()); p /= p.sum()
    V = 12
    H = {'shannon': -(p * np.log(p)).sum(), 'tsallis': (1 - (p ** 0.5).sum()) / -0.5, 'renyi': math.log((p ** 0.5).sum()) / 0.5, 'max_prob': 0}[method]
    if method == 'max_prob':
        want = (V * p.max() - 1) / (V - 1)
    elif norm == 'lin':
        want = 1 - H / ((1 - V ** 0.5) / -0.5 if method == 'tsallis' else math.log(V))
    elif method == 'tsallis':
        hm = (1 - V ** 0.5) / -0.5
        want = (math.exp(-H) - math.exp(-hm)) / (1 - math.exp(-hm))
    else:
        want = (V * math.exp(-H) - 1) / (V - 1)
    assert c == pytest.approx(want, abs=1e-12) and c != pytest.approx(small, abs=1e-6)


def test_invalid_rows_and_refused_measures():
    for row in ([0.0, NAN, 1.0], [-np.inf] * 3, [0.0, np.inf, 1.0]):
        i, c = CR.frame_row(row, 'shannon', 'lin', 1.0)
        assert i == -1 and math.isnan(c)
    assert CR.frame_row([1.0, 2.0, 2.0, -np.inf], 'max_prob', 'lin', 1.0)[0] == 1          # the first index on a tie
    with pytest.raises(ValueError):
        CR.frame_row([0.0, 1.0], 'max_prob', 'exp', 1.0)
    for alpha in (0.0, -1.0, 4.5, NAN):
        with pytest.raises(ValueError):
            CR.frame_row([0.0, 1.0], 'tsallis', 'lin', alpha)
    x = np.random.default_rng(3).normal(size=(5, 20)).astype(np.float32)
    x[1, 3] = NAN
    tol, d32 = CR.tolerance(x, 17, 'tsallis', 'exp', 1 / 3)
    assert 0 < d32 < 1e-5 and tol == 4 * d32 + 1e-6 and math.isnan(CR.frames32(x, 17)[1])


def test_runs_by_hand():
    a, b, _ = 1, 2, 0
    tg, sp, n = CR.runs_row([a, a, _, a, b, b, _], 7, _, 7)
    assert n == 3 and tg.tolist() == [a, a, b, 0, 0, 0, 0]
    assert sp.tolist() == [[0, 2, 3], [3, 4, 4], [4, 6, 7]] + [[0, 0, 0]] * 4
    assert CR.runs_row([_, _, _], 3, _, 3)[2] == 0 and not CR.runs_row([_, _, _], 3, _, 3)[1].any()
    tg, sp, n = CR.runs_row([a, b, a], 3, _, 3)                            # no blanks
    assert n == 3 and tg.tolist() == [a, b, a] and sp.tolist() == [[0, 1, 1], [1, 2, 2], [2, 3, 3]]
    assert CR.runs_row([a, b], 0, _, 2)[2] == 0 and CR.runs_row([a, b], 1, _, 2)[1].tolist() == [[0, 1, 1], [0, 0, 0]]
    tg, sp, n = CR.runs_row([a, a, -1, a, _, b], 5, _, 4)                  # an invalid frame breaks the run; frame 5 is past the length
    assert n == 2 and tg.tolist() == [a, a, 0, 0] and sp.tolist() == [[0, 2, 3], [3, 4, 5], [0, 0, 0], [0, 0, 0]]
    tg, sp, n = CR.runs_row([a, b, a, b], 4, _, 3)                         # one label too many: the first S_cap are written
    assert n == -1 and tg.tolist() == [a, b, a] and sp.tolist() == [[0, 1, 1], [1, 2, 2], [2, 3, 3]]
    assert CR.runs_row([a, b, a], 3, _, 3)[2] == 3                         # S_cap exactly reached
    tg, sp, n = CR.runs([[a, a, _], [b, _, b]], [3, 1], _, 2)
    assert n.tolist() == [1, 1] and tg.tolist() == [[a, 0], [b, 0]] and sp[1, 0].tolist() == [0, 1, 1]


def test_aggregation_by_hand():
    v = [0.5, 0.25, 1.0, 0.125, NAN, 0.75]
    idx = [3, 0, 0, 3, 3, -1]                                              # blank 0
    spans = [[0, 4], [1, 3], [2, 2], [3, 2], [-1, 2], [4, 7], [3, 5], [5, 6], [1, 4]]
    for agg, f in (('mean', np.mean), ('min', np.min), ('max', np.max), ('prod', np.prod)):
        out = CR.aggregate(v, spans, agg)
        assert out[0] == f(v[0:4]) and out[1] == f(v[1:3]) and out[7] == 0.75
        assert all(math.isnan(out[k]) for k in (2, 3, 4, 5, 6))            # empty, reversed, out of range twice, a NaN inside
        out = CR.aggregate(v, spans, agg, idx, 0)
        assert out[0] == f([0.5, 0.125]) and out[8] == 0.125
        assert out[1] == f(v[1:3])                                         # nothing but blanks: all frames of the span
        assert out[7] == 0.75                                              # nothing but an invalid frame: the same
    assert CR.word_groups([5, 6, 7, 8], lambda i: i in (5, 7)) == [[0, 1], [2, 3]] and CR.word_groups([6, 5], lambda i: i == 5) == [[0], [1]]


# ---- 2. the ABI unit ------------------------------------------------------------------------------------------------------------
def _declared():
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', HEADER)).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(sconf_[a-z0-9_]+)\s*\(', src)))


def test_binding_is_the_header_and_the_core_does_not_name_it(lib):
    from lcasr_amd.hip import _lib, confid
    funcs, enums = header_abi(HEADER, PREFIX)
    assert sorted(funcs) == _declared() and set(funcs) == NAMES
    assert_binding_is_header(funcs, confid.PROTOTYPES, confid.PLAIN, 'hip/confid.py')
    for table, stem in ((confid.METHOD, 'SCONF_CONFID_'), (confid.NORM, 'SCONF_CONFID_'), (confid.AGGREGATION, 'SCONF_CONFID_')):
        assert all(enums[stem + k.upper()] == v for k, v in table.items())
    assert len(enums) == len(confid.METHOD) + len(confid.NORM) + len(confid.AGGREGATION)
    assert not any(n.startswith(PREFIX) for n in list(_lib.PROTOTYPES) + list(_lib.PLAIN))
    for n in NAMES:
        assert hasattr(lib, n) and n in _lib.bound()
    for path in (os.path.join(ROOT, 'long-context-asr_amd', 'hip', '_lib.py'), os.path.join(ROOT, 'include', 'sconf.h')):
        assert PREFIX not in open(path).read(), path
    lib.sconf_version.restype = ctypes.c_int
    assert lib.sconf_version() == 220


def test_queries_answer_on_the_host(lib):
    from lcasr_amd.hip import confid
    cap, chunk = lib.sconf_confid_row_capacity(), lib.sconf_confid_scan_chunk()
    assert cap == confid.row_capacity() and cap >= 256 and cap % 256 == 0          # whole quads for every lane of a wave
    block = lib.sconf_confid_block_capacity()
    assert block == confid.block_capacity() and block >= 4 * cap and block % 1024 == 0      # whole quads for every thread of a workgroup
    assert chunk == confid.scan_chunk() and chunk >= 256 and chunk % 256 == 0


def test_host_side_validation_sets_the_error_before_any_launch(lib):
    """Every refusal happens before a kernel is enqueued, so none needs a GPU: the pointers are host addresses that are never read."""
    one = ctypes.c_void_p(16)
    err = lib.sconf_last_error
    third = ctypes.c_float(1 / 3)

    def frames(**kw):
        a = dict(dict(x=one, M=4, C=129, rs=144, method=2, norm=1, alpha=third, idx=one, conf=one), **kw)
        return lib.sconf_confid_frames(a['x'], a['M'], a['C'], a['rs'], a['method'], a['norm'], a['alpha'], a['idx'], a['conf'], None)
    assert frames(method=0, norm=1) != 0 and b'max_prob has no exp' in err()
    for alpha in (0.0, -0.5, 4.0001, math.nan, math.inf):
        for method in (2, 3):
            assert frames(method=method, alpha=ctypes.c_float(alpha)) != 0 and b'alpha' in err() and b'(1, 4]' in err()
    assert frames(C=1, rs=1) != 0 and b'classes' in err()
    assert frames(rs=128) != 0 and b'stride' in err()
    assert frames(M=-1) != 0 and b'M=' in err()
    assert frames(method=4) != 0 and b'method' in err() and frames(method=-1) != 0
    assert frames(norm=2) != 0 and b'norm' in err()
    for name in ('x', 'idx', 'conf'):
        assert frames(**{name: None}) != 0 and b'null' in err()
    assert frames(M=0) == 0 and frames(M=0, method=1, alpha=ctypes.c_float(9.0)) == 0      # shannon and max_prob do not read alpha

    def runs(**kw):
        a = dict(dict(idx=one, lens=None, B=2, N=100, blank=0, tg=one, sp=one, tl=one, cap=100), **kw)
        return lib.sconf_confid_runs(a['idx'], a['lens'], a['B'], a['N'], a['blank'], a['tg'], a['sp'], a['tl'], a['cap'], None)
    assert runs(B=-1) != 0 and b'B=' in err()
    assert runs(N=-1) != 0 and b'N=' in err() and runs(N=2 ** 31) != 0 and b'N=' in err()
    assert runs(cap=-1) != 0 and b'S_cap' in err() and runs(cap=2 ** 31 // 3 + 1) != 0 and b'S_cap' in err()
    for name in ('idx', 'tg', 'sp', 'tl'):
        assert runs(**{name: None}) != 0 and b'null' in err()
    assert runs(B=0) == 0

    def agg(**kw):
        a = dict(dict(v=one, idx=None, blank=0, M=10, sp=one, S=3, agg=1, out=one), **kw)
        return lib.sconf_confid_aggregate(a['v'], a['idx'], a['blank'], a['M'], a['sp'], a['S'], a['agg'], a['out'], None)
    assert agg(agg=4) != 0 and b'aggregation' in err() and agg(agg=-1) != 0
    assert agg(M=-1) != 0 and b'M=' in err() and agg(M=2 ** 31) != 0
    assert agg(S=-1) != 0 and b'S=' in err()
    for name in ('v', 'sp', 'out'):
        assert agg(**{name: None}) != 0 and b'null' in err()
    assert agg(S=0) == 0


def test_a_cpu_tensor_is_refused_by_the_product_path(lib):
    from lcasr_amd.decoding import confidence as K
    from lcasr_amd.decoding.greedy import GreedyCTCDecoder
    from lcasr_amd.hip import confid
    lp = torch.zeros(5, 8)
    calls = [lambda: confid.frames(lp), lambda: confid.runs(torch.zeros(1, 5, dtype=torch.int32), None, 0),
             lambda: confid.aggregate(torch.zeros(5), torch.zeros(1, 2, dtype=torch.int32))]
    if not torch.cuda.is_available():                                      # (where there is a device the surface moves CPU input to it)
        calls += [lambda: K.frame_confidence(lp), lambda: K.greedy_confidence(lp, 7),
                  lambda: GreedyCTCDecoder(blank_id=7)(lp, confidence=K.ConfidenceConfig())]
    for call in calls:
        with pytest.raises(RuntimeError, match='GPU'):
            call()


# ---- 3. the Python surface on the restatement -----------------------------------------------------------------------------------
def test_config_validation_has_the_messages_of_the_c_refusals():
    from lcasr_amd.decoding.confidence import ConfidenceConfig as Cfg
    c = Cfg()
    assert (c.method, c.entropy_type, c.alpha, c.entropy_norm, c.aggregation, c.exclude_blank, c.word_aggregation) == \
        ('entropy', 'tsallis', 1 / 3, 'exp', 'min', True, None)
    assert c.measure == ('tsallis', 'exp') and c.words == 'min' and Cfg(word_aggregation='mean').words == 'mean'
    assert Cfg(method='max_prob').measure == ('max_prob', 'lin') and Cfg(entropy_type='shannon', entropy_norm='lin').measure == ('shannon', 'lin')
    for bad in (0.0, -1.0, 4.5, math.nan):
        for kind in ('tsallis', 'renyi'):
            with pytest.raises(ValueError, match=r'alpha=.* must be in \(0, 1\), 1 or \(1, 4\]'):
                Cfg(entropy_type=kind, alpha=bad)
    assert Cfg(alpha=1.0).alpha == 1.0 and Cfg(entropy_type='shannon', alpha=9.0) and Cfg(method='max_prob', alpha=9.0)
    for kw, word in ((dict(method='margin'), 'method'), (dict(entropy_type='gibbs'), 'entropy_type'), (dict(entropy_norm='log'), 'norm'),
                     (dict(aggregation='median'), 'aggregation'), (dict(word_aggregation='median'), 'aggregation')):
        with pytest.raises(ValueError, match='unknown ' + word):
            Cfg(**kw)


def _emission(seed=0):
    """30 frames over 7 labels + blank 7 with repeats, blanks and one invalid frame."""
    rng = np.random.default_rng(seed)
    lp = torch.from_numpy(rng.normal(size=(30, 8)).astype(np.float32) * 3)
    lp[4] = lp[3]; lp[5] = lp[3]; lp[10, 7] = 20.0; lp[11, 7] = 20.0; lp[17, 2] = NAN
    return lp


class PieceTok:
    PIECES = ['▁the', '▁c', 'at', 's', '▁sat', 'on', '▁']
    def id_to_piece(self, i): return self.PIECES[i]
    def decode(self, ids): return ''.join(self.PIECES[i] for i in ids).replace('▁', ' ').strip()


def test_greedy_decoder_with_and_without_confidence(emulated, emulated_ops):
    from lcasr_amd.decoding.greedy import GreedyCTCDecoder
    K = emulated
    lp = _emission()
    clean = torch.nan_to_num(lp, nan=0.0)
    dec = GreedyCTCDecoder(tokenizer=None, blank_id=7)
    idx = clean.argmax(-1)
    today = [i for i in torch.unique_consecutive(idx).tolist() if i != 7]
    assert dec(clean) == today and dec(clean, decode=False) == today and dec(clean, confidence=None) == today
    for cfg in (K.ConfidenceConfig(), K.ConfidenceConfig(method='max_prob', aggregation='mean', exclude_blank=False),
                K.ConfidenceConfig(entropy_type='renyi', alpha=2.0, entropy_norm='lin', aggregation='prod')):
        ids, conf = dec(clean, confidence=cfg)
        assert ids == today and len(conf) == len(ids) and all(0.0 <= c <= 1.0 for c in conf)
        method, norm = cfg.measure
        (want,), fc = CR.greedy(clean.numpy()[None], 7, method, norm, cfg.alpha, cfg.aggregation, cfg.exclude_blank)
        assert want[0] == ids and np.allclose(conf, want[2], atol=1e-6)
    ids, conf = dec(lp, confidence=K.ConfidenceConfig())                   # the invalid frame 17 breaks a run and is dropped
    g = K.greedy_confidence(lp, 7, K.ConfidenceConfig())
    assert g.tokens == ids and g.token_confidence == conf and math.isnan(float(g.frame_confidence[17])) and g.frame_confidence.shape == (30,)
    assert all(s[0] < s[1] <= s[2] for s in g.spans) and all(a[2] == b[0] for a, b in zip(g.spans, g.spans[1:])) and g.spans[-1][2] == 30
    assert not any(s[0] <= 17 < s[1] for s in g.spans)
    text, conf2 = GreedyCTCDecoder(tokenizer=PieceTok(), blank_id=7)(lp, confidence=K.ConfidenceConfig())
    assert text == PieceTok().decode(ids) and conf2 == conf
    both = K.greedy_confidence(torch.stack([lp, clean]), 7, K.ConfidenceConfig(), lengths=[30, 12])
    assert both.tokens[0] == ids and both.token_confidence[0] == conf and both.frame_confidence.shape == (2, 30)
    assert both.tokens[1] == K.greedy_confidence(clean[:12], 7).tokens and both.spans[1][-1][2] == 12


def test_frame_token_and_word_confidence(emulated):
    K = emulated
    lp = torch.nan_to_num(_emission(1), nan=0.0)
    cfg = K.ConfidenceConfig(entropy_type='shannon', aggregation='mean', word_aggregation='min')
    idx, conf = K.frame_confidence(lp, cfg)
    want_i, want_c = CR.frames(lp.numpy(), 8, 'shannon', 'exp', 1 / 3)
    assert idx.tolist() == want_i.tolist() and idx.dtype == torch.int32 and np.allclose(conf.numpy(), want_c, atol=1e-6)
    wide = torch.cat([lp, torch.full((30, 8), NAN)], dim=1)                # guard columns behind `classes`
    i2, c2 = K.frame_confidence(wide, cfg, classes=8)
    assert torch.equal(i2, idx) and torch.equal(c2, conf)
    i3, c3 = K.frame_confidence(torch.stack([lp, lp]), cfg)
    assert i3.shape == (2, 30) and torch.equal(i3[1], idx) and torch.equal(c3[0], conf)
    with pytest.raises(ValueError):
        K.frame_confidence(lp[0], cfg)
    frames = torch.tensor([2, 3, 9, 20])
    spans = K.spans_from_token_frames(frames, 30)
    assert spans.tolist() == [[2, 3], [3, 9], [9, 20], [20, 30]] and spans.dtype == torch.int32
    tc = K.token_confidence(conf, idx, spans, cfg, blank=7)
    assert np.allclose(tc.numpy(), CR.aggregate(want_c, spans.tolist(), 'mean', want_i, 7), atol=1e-6)
    off = K.ConfidenceConfig(aggregation='mean', exclude_blank=False)
    assert np.allclose(K.token_confidence(conf, None, spans, off).numpy(), CR.aggregate(want_c, spans.tolist(), 'mean'), atol=1e-6)
    with pytest.raises(ValueError, match='exclude_blank'):
        K.token_confidence(conf, None, spans, cfg)
    ids, t = [0, 1, 2, 3, 4, 5], [0.9, 0.8, 0.3, 0.7, 0.6, 0.5]            # 'the', 'c' 'at' 's', 'sat' 'on'
    assert K.word_confidence(ids, t, PieceTok(), cfg) == pytest.approx([0.9, 0.3, 0.5])
    assert K.word_confidence(ids, torch.tensor(t), PieceTok(), K.ConfidenceConfig(aggregation='max')) == pytest.approx([0.9, 0.8, 0.6])
    assert K.word_confidence(ids, t, PieceTok(), K.ConfidenceConfig(aggregation='prod'), word_start=lambda i: i % 2 == 0) == \
        pytest.approx([0.72, 0.21, 0.3])
    assert K.word_confidence(ids[:2], t[:2], object(), cfg) == pytest.approx([0.9, 0.8])       # no id_to_piece: every token a word
    assert K.word_confidence([], [], PieceTok(), cfg) == []
    from lcasr_amd.decoding import beam
    assert K._word_groups is beam._word_groups                             # shared, not copied


class IdTok:
    """Every token is a word: id i is spelt 't<i>'."""
    def __init__(self, V): self.V = V
    def vocab_size(self): return self.V
    def decode(self, ids): return ' '.join(f't{int(i)}' for i in ids)
    def encode(self, text): return [int(w[1:]) for w in text.split()]


@pytest.fixture
def tiny(emulated, emulated_ops, monkeypatch):
    from lcasr_amd.decoding import align as A
    from lcasr_amd.decoding import beam as D
    from lcasr_amd.eval import run as R
    from lcasr_amd.utils import audio_tools
    monkeypatch.setattr(audio_tools.audio, 'melspec', AUD.melspec)
    monkeypatch.setattr(A.align_kernels, 'ctc_align', AR.ctc_align)
    monkeypatch.setattr(D.beam_kernels, 'ctc_beam', BR.ctc_beam)
    E.attach(monkeypatch, emulated_ops)
    fx = load_golden('infer_tiny')
    m = build_from_fixture(fx).eval()
    return R, m, IdTok(int(fx['cfg.vocab_size'])), AUD.test_signal(3 * 16000, seed=3), audio_tools


def test_transcribe_detail_on_the_tiny_model(tiny, emulated):
    R, m, tok, wave, audio_tools = tiny
    K = emulated
    blank = m.decoder.num_classes - 1
    sec = m.subsampling.subsampling_factor * audio_tools.HOP_LENGTH / audio_tools.SR
    logits = R.moving_average_eval(R._Args(), m, audio_tools.to_spectogram(wave[None]), 128, 32, tok, use_tqdm=False, return_numpy=False)
    text = R.transcribe(m, wave, tok, 128, 32)
    assert isinstance(text, str)
    d = R.transcribe_detail(m, wave, tok, 128, 32)
    assert set(d) == {'text', 'tokens', 'token_confidence', 'words'} and d['text'] == text == tok.decode(d['tokens'])
    (want,), _ = CR.greedy(logits.float().numpy()[None], blank, 'tsallis', 'exp', 1 / 3, 'min', True)
    assert d['tokens'] == want[0] and np.allclose(d['token_confidence'], want[2], atol=1e-6) and len(d['tokens']) > 0
    assert [w['word'] for w in d['words']] == text.split() and all(set(w) == {'word', 'startTime', 'endTime', 'confidence'} for w in d['words'])
    assert [(w['startTime'], w['endTime']) for w in d['words']] == [(f'{s[0] * sec:.2f}s', f'{s[1] * sec:.2f}s') for s in want[1]]
    assert [w['confidence'] for w in d['words']] == pytest.approx(d['token_confidence'])      # every token a word
    cfg = K.ConfidenceConfig(method='max_prob', aggregation='mean', exclude_blank=False)
    d2 = R.transcribe_detail(m, wave, tok, 128, 32, confidence=cfg)
    assert d2['tokens'] == d['tokens'] and d2['token_confidence'] != d['token_confidence']
    # beam_width > 1: the best beam's token frames
    best = BR.search(logits.float().numpy(), blank, 4)[0][0]
    b = R.transcribe_detail(m, wave, tok, 128, 32, beam_width=4)
    assert b['tokens'] == list(best[0]) and b['text'] == R.transcribe(m, wave, tok, 128, 32, beam_width=4)
    fr = list(best[1])
    wi, wc = CR.frames(logits.float().numpy(), None, 'tsallis', 'exp', 1 / 3)
    spans = [[f, g] for f, g in zip(fr, fr[1:] + [logits.shape[0]])]
    assert np.allclose(b['token_confidence'], CR.aggregate(wc, spans, 'min', wi, blank), atol=1e-6)
    assert [(w['startTime'], w['endTime']) for w in b['words']] == [(f'{f * sec:.2f}s', f'{(f + 1) * sec:.2f}s') for f in fr]
    with pytest.raises(ValueError, match='greedy'):
        R.transcribe_detail(m, wave, tok, 128, 32, hotwords=['t1'])


def test_align_with_confidence_on_the_tiny_model(tiny, emulated):
    R, m, tok, wave, audio_tools = tiny
    K = emulated
    spec = audio_tools.to_spectogram(wave[None])
    text = 't3 t1 t4 t1 t5 t9 t2 t6'
    today = R.align(m, spec, text, tok, 128, 32)
    assert all(set(w) == {'word', 'startTime', 'endTime', 'logp'} for w in today) and R.align(m, spec, text, tok, 128, 32, confidence=None) == today
    cfg = K.ConfidenceConfig(entropy_type='shannon', aggregation='mean')
    got = R.align(m, spec, text, tok, 128, 32, confidence=cfg)
    assert [{k: v for k, v in w.items() if k != 'confidence'} for w in got] == today
    logits = R.moving_average_eval(R._Args(), m, spec, 128, 32, tok, use_tqdm=False, return_numpy=False)
    ref = AR.ctc_align(logits.float()[None], torch.tensor([tok.encode(text)], dtype=torch.int32), None, None, m.decoder.num_classes - 1)
    _, wc = CR.frames(logits.float().numpy(), None, 'shannon', 'exp', 1 / 3)
    assert [w['confidence'] for w in got] == pytest.approx(CR.aggregate(wc, ref.spans[0].tolist(), 'mean').tolist(), abs=1e-6)
    assert R.align_waveform(m, wave, text, tok, 128, 32, confidence=cfg) == got and R.align_waveform(m, wave, text, tok, 128, 32) == today


# ---- 4. the usefulness case -----------------------------------------------------------------------------------------------------
def usefulness_measures():
    return [(m, n, a) for m, n in CR.MEASURES for a in CR.AGGS if (m, a) != ('max_prob', 'mean')]


@pytest.mark.parametrize('method, norm, agg', usefulness_measures())
def test_corrupted_tokens_score_below_clean_ones_in_the_restatement(method, norm, agg):
    lp, labels, bad = CR.planted()
    assert lp.shape == (120, 32) and len(labels) == 40 and len(bad) == 8
    (out,), _ = CR.greedy(lp[None], 31, method, norm, 1 / 3, agg, True)
    tokens, _, conf = out
    assert tokens == labels
    worst_clean = min(c for k, c in enumerate(conf) if k not in bad)
    best_bad = max(c for k, c in enumerate(conf) if k in bad)
    print(f'[confid] {method}/{norm}/{agg}: corrupted <= {best_bad:.4f} < {worst_clean:.4f} <= clean')
    assert best_bad < worst_clean
