"""CPU tests of the resampler: the restatement (tests/resample_refs.py) against the values torchaudio's algorithm gives, the
product's compact table against the restatement's f32 kernel, the ninth ABI unit's header, queries and refusals (host-only calls),
and the host logic of lcasr_amd.utils.audio_tools.resample / processing_chain and of eval.run.transcribe / spectrograms_of with
the unit's op replaced by the restatement.  The HIP kernel itself is tested in test_resample_gpu.py."""
import ctypes
import math
import os
import re

import pytest
import torch

import audio_refs as AR
import eval_refs as E
import resample_refs as RR
from cabi_header import assert_binding_is_header, header_abi
from common_model import build_from_fixture
from conftest import ROOT, load_golden

HEADER, PREFIX = 'sconf_resample.h', 'sconf_resample_'
NAMES = {'sconf_resample_tile', 'sconf_resample_max_table', 'sconf_resample_out_length', 'sconf_resample_rows'}


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from lcasr_amd.hip import resample
    return resample.load()


@pytest.fixture
def emulated(monkeypatch):
    """The new unit's op (lcasr_amd.hip.resample.resample_rows) and the mel op replaced by their f32 restatements: host logic
    without a GPU."""
    from lcasr_amd.utils import audio_tools
    monkeypatch.setattr(audio_tools.resampler, 'resample_rows', RR.resample_rows)
    monkeypatch.setattr(audio_tools.audio, 'melspec', AR.melspec)
    return audio_tools


# ---- the yardstick ------------------------------------------------------------------------------------------------------------
def test_restatement_anchors_of_44100_to_16000():
    k, raw, width = RR.kernel(44100, 16000, torch.float32)
    assert RR.ratio(44100, 16000) == (441, 160) and width == 17 and tuple(k.shape) == (160, 475) and k.dtype == torch.float32
    assert float(k[0, 17]) == 0.359183669090271 and float(k[1, 20]) == 0.3544856309890747 and float(k[80, 100]) == 0.0
    k64 = RR.kernel(44100, 16000)[0]
    assert k64.dtype == torch.float64 and float(k64[(raw.abs() >= 6)].abs().max()) < 2e-49


@pytest.mark.parametrize('L, want', [(1, 1), (5, 2), (440, 160), (441, 160), (442, 161), (882, 320), (883, 321)])
def test_restatement_output_lengths(L, want):
    y = RR.resample(RR.test_signal(L, 44100), 44100, 16000)
    assert y.shape == (want,) and RR.out_length(L, 44100, 16000) == want == math.ceil(160 * L / 441)


def test_restatement_resamples_a_tone():
    orig, new = 44100, 16000
    L = orig // 2 + 37
    w = torch.sin(2 * math.pi * 1000 * torch.arange(L, dtype=torch.float64) / orig)
    y = RR.resample(w, orig, new)
    ref = torch.sin(2 * math.pi * 1000 * torch.arange(y.shape[0], dtype=torch.float64) / new)
    err = float((y - ref)[200:-200].abs().max())
    print(f'[resample] 1 kHz tone 44100 -> 16000, {y.shape[0]} outputs: max |y - sin| inside = {err:.2e}')
    assert y.shape[0] == math.ceil(new * L / orig) and err <= 8e-4


@pytest.mark.parametrize('pair', list(RR.PAIRS), ids=lambda p: f'{p[0]}-{p[1]}')
def test_f32_restatement_is_inside_the_bound_and_lengths_mean_alone(pair):
    orig, new = pair
    O, P, K = RR.PAIRS[pair]
    L = 3 * O + (O * 7) // 3 + 11 if O > 50 else 4001
    w = torch.stack([RR.test_signal(L, orig, seed=1), RR.test_signal(L, orig, seed=2)])
    lens = [L, L // 2 + 3]
    y64, y32, bd = RR.resample(w, orig, new, lens), RR.resample(w, orig, new, lens, dtype=torch.float32), RR.bound(w, orig, new, lens)
    assert y64.shape == y32.shape == bd.shape == (2, RR.out_length(L, orig, new))
    n1 = RR.out_length(lens[1], orig, new)
    assert torch.equal(y64[1, :n1], RR.resample(w[1, :lens[1]], orig, new)) and not bool(y64[1, n1:].any()) and not bool(bd[1, n1:].any())
    r = float(((y32.double() - y64).abs() / bd.clamp(min=1e-300)).max())
    print(f'[resample] {orig} -> {new}: f32 restatement err / bound = {r:.3f}')
    assert r <= 1.0
    taps, first, k = RR.compact(orig, new)
    assert k == K and RR.ratio(orig, new) == (O, P)
    via_table = RR.rows_from_table(w, lens, taps, first, O, P)            # f32 taps, f64 sums: one rounding per tap
    assert via_table.shape == y64.shape and bool(((via_table - y64).abs() <= bd).all())


def test_bound_holds_where_a_signal_follows_silence():
    """The outputs just before the signal have every live tap on exact zeros and clamped taps (1e-49 in f64, 0 in f32) on samples:
    the f64 yardstick is not 0 there, an f32 evaluation is, and the bound has to say so."""
    w = torch.zeros(3000)
    w[1500:] = RR.test_signal(1500, 44100, seed=90)
    y64, y32, bd = RR.resample(w, 44100, 16000), RR.resample(w, 44100, 16000, dtype=torch.float32), RR.bound(w, 44100, 16000)
    lead = (y32 == 0) & (y64 != 0)
    assert int(lead.sum()) > 0 and float(y64[lead].abs().max()) < 1e-48
    assert bool(((y32.double() - y64).abs() <= bd).all()) and not bool(bd[:300].any())


# ---- the product's table ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pair', list(RR.PAIRS), ids=lambda p: f'{p[0]}-{p[1]}')
def test_product_table_is_the_f32_kernel_on_its_support(lib, pair):
    from lcasr_amd.utils import audio_tools as A
    orig, new = pair
    O, P, K = RR.PAIRS[pair]
    taps, first, o, p = A.resample_table(orig, new)
    assert (o, p) == (O, P) and tuple(taps.shape) == (P, K) and taps.dtype == torch.float32 and taps.is_contiguous()
    assert tuple(first.shape) == (P,) and first.dtype == torch.int32
    dense, raw, width = RR.kernel(orig, new, torch.float32)
    rebuilt = torch.zeros_like(dense)
    for ph in range(P):
        a = int(first[ph]) + width
        assert a >= 0
        n = min(K, dense.shape[1] - a)
        rebuilt[ph, a:a + n] = taps[ph, :n]
        assert not bool(taps[ph, n:].any())                                # padding that hangs over the dense kernel's end is 0
    live = raw.abs() < 6
    assert torch.equal(rebuilt.view(torch.int32)[live], dense.view(torch.int32)[live])      # bit for bit on the support
    assert torch.equal(rebuilt, dense) and not bool(dense[~live].any())   # and 0 outside it (the reference's clamped taps are -0.0)
    rt, rf, rk = RR.compact(orig, new)
    assert rk == K and torch.equal(rf, first) and torch.equal(rt.view(torch.int32), taps.view(torch.int32))
    s = torch.cat([first.long(), first[:1].long() + O])                   # q O + first[p] over one period and the next phase 0
    assert bool((s[1:] >= s[:-1]).all()) and int((s[1:] - s[:-1]).max()) <= -(-O // P)      # forward only, ceil(O / P) at most
    assert P * K <= 8320
    # the span a tile stages, (Q - 1) O / P + K + 3 samples from the first sample of its first output on, holds every output's taps
    Q = lib.sconf_resample_tile()
    j = torch.arange(P + Q)
    pos = (j // P) * O + first.long()[j % P]
    reach = pos[Q - 1:Q - 1 + P] - pos[:P]                                  # last output of a tile against its first, every phase p0
    assert int(reach.max()) + K <= (Q - 1) * O // P + K + 3 and int(reach.min()) >= 0


def test_table_is_cached_per_device_and_rates(lib):
    from lcasr_amd.utils import audio_tools as A
    a = A._device_resample_table(torch.device('cpu'), 44100, 16000)
    assert a is A._device_resample_table(torch.device('cpu'), 44100, 16000) and a[2:] == (441, 160)
    assert A._device_resample_table(torch.device('cpu'), 48000, 16000) is not a
    assert ('cpu', 44100, 16000) in A._resample_tables


# ---- the ABI unit ---------------------------------------------------------------------------------------------------------------
def _declared():
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', HEADER)).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(sconf_[a-z0-9_]+)\s*\(', src)))


def test_binding_is_the_header_and_the_core_does_not_name_it(lib):
    from lcasr_amd.hip import _lib, resample
    funcs, enums = header_abi(HEADER, PREFIX)
    assert sorted(funcs) == _declared() and set(funcs) == NAMES and not enums
    assert_binding_is_header(funcs, resample.PROTOTYPES, resample.PLAIN, 'hip/resample.py')
    assert not any(n.startswith(PREFIX) for n in list(_lib.PROTOTYPES) + list(_lib.PLAIN))
    for n in NAMES:
        assert hasattr(lib, n) and n in _lib.bound()
    hip = os.path.join(ROOT, 'long-context-asr_amd', 'hip')
    for path in [os.path.join(hip, f) for f in ('_lib.py', 'audio.py', 'align.py', 'beam.py')] + [os.path.join(ROOT, 'include', 'sconf.h')]:
        assert 'resample' not in open(path).read(), path
    lib.sconf_version.restype = ctypes.c_int
    assert lib.sconf_version() == 220


def test_queries_answer_on_the_host(lib):
    from lcasr_amd.hip import resample
    Q = lib.sconf_resample_tile()
    assert Q == resample.tile() and Q >= 64
    assert lib.sconf_resample_max_table() == resample.max_table() >= 8320
    f = lib.sconf_resample_out_length
    for L in (0, 1, 5, 440, 441, 442, 882, 883, 2 ** 31 + 3 * 441 + 7, 2 ** 40, 2 ** 40 + 1):
        for O, P in ((441, 160), (3, 1), (1, 2), (441, 640), (147, 160)):
            assert f(L, O, P) == -(-(P * L) // O) == resample.out_length(L, O, P), (L, O, P)
    assert f(-1, 3, 1) == -1 and f(5, 0, 1) == -1 and f(5, 3, 0) == -1 and f(2 ** 62, 1, 4) == -1
    with pytest.raises(ValueError, match='invalid'):
        resample.out_length(-1, 3, 1)


def test_host_side_validation_sets_the_error_before_any_launch(lib):
    """Every refusal happens before a kernel is enqueued, so none needs a GPU: the pointers are host addresses that are never read."""
    one = ctypes.c_void_p(16)
    ok = dict(wave=one, cs=1000, rs=1000, ch=1, mix=0, lens=None, L=1000, taps=one, first=one, O=3, P=1, K=37, out=one, os=334, Lo=334, B=1)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.sconf_resample_rows(a['wave'], a['cs'], a['rs'], a['ch'], a['mix'], a['lens'], a['L'], a['taps'], a['first'], a['O'], a['P'],
                                       a['K'], a['out'], a['os'], a['Lo'], a['B'], None)
    assert call(wave=None) != 0 and b'null' in lib.sconf_last_error()
    assert call(out=None) != 0 and b'null' in lib.sconf_last_error()
    assert call(O=0) != 0 and b'bad O' in lib.sconf_last_error()
    assert call(K=0) != 0 and b'bad O' in lib.sconf_last_error()
    M = lib.sconf_resample_max_table()
    assert call(P=M // 37 + 1, Lo=-(-(1000 * (M // 37 + 1)) // 3), os=1 << 40) != 0 and b'kept in LDS' in lib.sconf_last_error()
    assert call(ch=0) != 0 and b'channels' in lib.sconf_last_error()
    assert call(ch=65) != 0 and b'channels' in lib.sconf_last_error()
    assert call(mix=2) != 0 and b'mix' in lib.sconf_last_error()
    assert call(L=0, Lo=0) != 0 and b'length' in lib.sconf_last_error()
    assert call(Lo=333) != 0 and b'ceil(P L / O)' in lib.sconf_last_error()
    assert call(os=333) != 0 and b'stride' in lib.sconf_last_error()
    assert call(B=2, rs=999) != 0 and b'stride' in lib.sconf_last_error()
    assert call(ch=2, mix=1, cs=999) != 0 and b'stride' in lib.sconf_last_error()
    assert call(B=0) != 0 and b'batch' in lib.sconf_last_error()
    assert call(O=200000, P=1, K=37, Lo=1) != 0 and b'LDS' in lib.sconf_last_error()               # a span of 200 M samples per tile
    assert call(B=1 << 30, L=15000, rs=15000, cs=15000, Lo=5000, os=5000) != 0 and b'too many' in lib.sconf_last_error()


# ---- host logic -----------------------------------------------------------------------------------------------------------------
def test_resample_host_logic_equals_the_restatement(emulated):
    A = emulated
    L = 2000
    lens = [2000, 5, 1077]
    w = torch.full((3, L + 40), float('nan'))
    for b, n in enumerate(lens): w[b, :n] = RR.test_signal(n, 44100, seed=b)
    view = w[:, :L]                                                        # a row stride larger than L
    got = A.resample(view, 44100, 16000, lengths=lens)
    want = RR.resample(view, 44100, 16000, lens, dtype=torch.float32)
    assert got.shape == (3, 726) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    assert float((got.double() - RR.resample(view, 44100, 16000, lens)).abs().max()) <= float(RR.bound(view.nan_to_num(), 44100, 16000, lens).max())
    assert got.shape == want.shape
    nl = A.resampled_lengths(torch.tensor(lens), 44100, 16000)
    assert nl.tolist() == [726, 2, 391] == [A.resampled_lengths(n, 44100, 16000) for n in lens]
    hour = A.resampled_lengths(torch.tensor([3600 * 44100], dtype=torch.int32), 44100, 16000)          # 160 L is past int32
    assert hour.tolist() == [57600000] and A.resampled_lengths(3600 * 44100 + 1, 44100, 16000) == 57600001
    for b, n in enumerate(lens):
        alone = A.resample(w[b, :n].clone(), 44100, 16000)
        assert alone.shape == (int(nl[b]),) and torch.equal(got[b, :int(nl[b])], alone) and not bool(got[b, int(nl[b]):].any())
    assert torch.equal(got, A.resample(view, 44100, 16000, lengths=torch.tensor(lens, dtype=torch.int32)))
    one = A.resample(w[0, :L], 8000, 16000)
    assert one.shape == (2 * L,) and A.resample(w[0:1, :L], 8000, 16000).shape == (1, 2 * L)
    # channels of one recording
    st = torch.stack([w[0, :L], w[0, :L].flip(0)])
    left, mean = A.resample(st, 44100, 16000, mix='left'), A.resample(st, 44100, 16000, mix='mean')
    assert left.shape == mean.shape == (1, 726)
    assert torch.equal(left, A.resample(A.grab_left_channel(st), 44100, 16000)) and torch.equal(mean, A.resample(A.take_mean_channel(st), 44100, 16000))
    assert torch.equal(A.resample(st[0], 44100, 16000, mix='left'), left)
    strided = torch.stack([w[0, :L], w[2, :L]], 1)                         # (L, 2): channel-last storage, transposed view
    assert torch.equal(A.resample(strided.T, 44100, 16000, mix='left'), left)
    assert torch.equal(A.resample(st, 44100, 16000, lengths=[1000], mix='left')[:, :363], A.resample(st[0, :1000].clone(), 44100, 16000)[None])
    # equal rates: the input, or the mixed channel
    assert A.resample(st, 16000, 16000) is st
    assert torch.equal(A.resample(st, 16000, 16000, mix='left'), st[0:1]) and torch.equal(A.resample(st, 16000, 16000, mix='mean'), st.mean(0, keepdim=True))


def test_resample_refusals(emulated, lib):
    A = emulated
    w = torch.zeros(2, 100)
    for bad in ((44100.0, 16000), (44100, 0), (-1, 16000), (True, 16000), ('44100', 16000)):
        with pytest.raises(ValueError, match='positive integers'):
            A.resample(w, *bad)
    with pytest.raises(ValueError, match='positive integers'):
        A.resampled_lengths(5, 0, 16000)
    with pytest.raises(TypeError, match='float32'):
        A.resample(w.double(), 44100, 16000)
    with pytest.raises(ValueError, match='1D or 2D'):
        A.resample(torch.zeros(1, 2, 100), 44100, 16000)
    with pytest.raises(ValueError, match='mix'):
        A.resample(w, 44100, 16000, mix='right')
    with pytest.raises(ValueError, match='lengths'):
        A.resample(w, 44100, 16000, lengths=[100])
    with pytest.raises(ValueError, match='length'):
        A.resample(w, 44100, 16000, lengths=[100, 101])
    with pytest.raises(ValueError, match='empty'):
        A.resample(torch.zeros(2, 0), 44100, 16000)
    for orig, new in ((44101, 16000), (16000, 7), (11025, 32000)):         # tables far past the limit, and one (1280 x 13) just past it
        with pytest.raises(ValueError, match='sconf_resample_max_table'):
            A.resample(w, orig, new)


def test_a_cpu_tensor_is_refused_by_the_product_path(lib):
    from lcasr_amd.hip import resample
    from lcasr_amd.utils import audio_tools as A
    w = RR.test_signal(1000, 44100)
    with pytest.raises(RuntimeError, match='GPU'):
        A.resample(w, 44100, 16000)
    with pytest.raises(RuntimeError, match='GPU'):
        A.processing_chain(w[None], 44100, resample_input=True)
    taps, first, O, P = A.resample_table(44100, 16000)
    with pytest.raises(RuntimeError, match='GPU'):
        resample.resample_rows(w[None], None, taps, first, O, P)


def test_processing_chain_default_still_refuses_and_the_keyword_resamples(emulated):
    A = emulated
    w = torch.stack([RR.test_signal(4410, 44100, seed=3), RR.test_signal(4410, 44100, seed=4)])
    with pytest.raises(NotImplementedError, match='44100'):
        A.processing_chain(w, 44100)
    with pytest.raises(NotImplementedError, match='resample_input'):
        A.processing_chain(w, 44100, normalise=False)
    got = A.processing_chain(w, 44100, resample_input=True)
    at16 = RR.resample(w[0:1], 44100, 16000, dtype=torch.float32)
    assert at16.shape == (1, 1600) and got.shape == (1, 80, 11)
    assert torch.equal(got, A.to_spectogram(A.resample(A.grab_left_channel(w), 44100, 16000)))
    raw = A.processing_chain(w, 44100, normalise=False, resample_input=True)
    assert torch.equal(raw, A.to_spectogram(A.resample(w[0:1], 44100, 16000), global_normalisation=False))
    same = A.processing_chain(w[:, :1600], 16000, resample_input=True)                      # 16 kHz: nothing to resample
    assert torch.equal(same, A.processing_chain(w[:, :1600], 16000))


class WordTok:
    """Toy tokenizer: id i decodes to the word 'w<i % 7>'."""
    def __init__(self, V): self.V = V
    def vocab_size(self): return self.V
    def decode(self, ids): return ' '.join(f'w{int(i) % 7}' for i in ids)


def test_transcribe_and_spectrograms_of_at_44100(emulated_ops, emulated, monkeypatch):
    from lcasr_amd.eval import run as R
    E.attach(monkeypatch, emulated_ops)
    fx = load_golden('infer_tiny')
    m = build_from_fixture(fx).eval()
    tok = WordTok(int(fx['cfg.vocab_size']))
    wave = torch.stack([RR.test_signal(2 * 44100, 44100, seed=3), RR.test_signal(2 * 44100, 44100, seed=4)])
    at16 = emulated.resample(wave, 44100, 16000, mix='left')
    assert at16.shape == (1, 32000)
    text = R.transcribe(m, wave, tok, 128, 32, sample_rate=44100)
    assert isinstance(text, str) and len(text) > 0 and text == R.transcribe(m, at16, tok, 128, 32) == R.transcribe(m, at16[0], tok, 128, 32, sample_rate=16000)
    recs = [('r0', wave, 'w1 w2 w3'), ('r1', wave[0, :30000], 'w5 w6')]
    specs = list(R.spectrograms_of(recs, sample_rate=44100))
    assert [(i, g) for i, _, g in specs] == [('r0', 'w1 w2 w3'), ('r1', 'w5 w6')]
    assert torch.equal(specs[0][1], emulated.to_spectogram(at16)) and specs[1][1].shape == (1, 80, 1 + RR.out_length(30000, 44100, 16000) // 160)
    assert torch.equal(list(R.spectrograms_of([('r', at16, '')]))[0][1], specs[0][1])       # the default rate: as before
