"""CPU tests of the noise corruption: the restatement (tests/noise_refs.py) against the Random123 known answers and the moments of
a normal, the tenth ABI unit's header, queries and refusals (host-only calls), and the host logic of
lcasr_amd.utils.audio_tools.wave_power / add_gaussian_snr / add_background_noise, utils.augmentation.AddGaussianSNR /
AddBackgroundNoise and processing_chain(corrupt=) with the unit's ops replaced by the restatement.  The HIP kernels themselves are
tested in test_noise_gpu.py."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import audio_refs as AR
import noise_refs as NR
from cabi_header import assert_binding_is_header, header_abi
from conftest import ROOT

HEADER, PREFIX = 'sconf_noise.h', 'sconf_noise_'
NAMES = {'sconf_noise_tile', 'sconf_noise_max_levels', 'sconf_noise_workspace', 'sconf_noise_power', 'sconf_noise_add_gaussian',
         'sconf_noise_add_background'}


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from lcasr_amd.hip import noise
    return noise.load()


@pytest.fixture
def emulated(lib, monkeypatch):
    """The unit's three ops (lcasr_amd.hip.noise) and the mel op replaced by their restatements: host logic without a GPU."""
    from lcasr_amd.utils import audio_tools
    monkeypatch.setattr(audio_tools.noiser, 'power', NR.op_power)
    monkeypatch.setattr(audio_tools.noiser, 'add_gaussian', NR.op_add_gaussian)
    monkeypatch.setattr(audio_tools.noiser, 'add_background', NR.op_add_background)
    monkeypatch.setattr(audio_tools.audio, 'melspec', AR.melspec)
    return audio_tools


# ---- the yardstick ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('counter, key, want', [
    ([0, 0, 0, 0], (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
    ([0xffffffff] * 4, (0xffffffff, 0xffffffff), '408f276d 41c83b0e a20bc7c6 6d5451fd'),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], (0xa4093822, 0x299f31d0), 'd16cfe09 94fdcceb 5001e420 24126ea1')])
def test_philox_known_answers(counter, key, want):
    assert ' '.join(f'{v:08x}' for v in NR.philox4x32_10(np.array([counter]), key)[0]) == want


def test_moments_of_the_first_normals():
    n = 2 ** 22
    z, r = NR.normals(17925, 0, 0, n)
    mean, var, m4 = float(z.mean()), float((z * z).mean()), float((z ** 4).mean())
    print(f'[noise] seed 17925, row 0, first {n} normals: mean {mean:.2e}  variance {var:.5f}  fourth moment {m4:.4f}  max |z| {float(z.abs().max()):.3f}')
    assert abs(mean) < 4 / math.sqrt(n) and abs(var - 1) < 4 * math.sqrt(2 / n) and abs(m4 - 3) < 4 * math.sqrt(96 / n)
    assert float(z.abs().max()) <= math.sqrt(48 * math.log(2)) and bool((z.abs() <= r).all())


@pytest.mark.parametrize('cut', [4096, 4097, 3, 9998])
def test_a_row_in_pieces_equals_the_row_in_one_pass(cut):
    first, n = 2 ** 34 + 3, 10000
    whole = NR.normals(5, 7, first, n)[0]
    a, b = NR.normals(5, 7, first, cut)[0], NR.normals(5, 7, first + cut, n - cut)[0]
    assert torch.equal(torch.cat([a, b]), whole)
    assert not torch.equal(NR.normals(5, 8, first, n)[0], whole) and not torch.equal(NR.normals(6, 7, first, n)[0], whole)
    assert not torch.equal(NR.normals(5, 7 + 2 ** 32, first, n)[0], whole) and not torch.equal(NR.normals(5 + 2 ** 32, 7, first, n)[0], whole)
    assert not torch.equal(NR.normals(5, 7, first - 2 ** 34, n)[0], whole)                 # the high word of the sample counter


def test_restated_mixes_reach_the_requested_snr():
    x = NR.test_signal(20000, seed=1)[None]
    y, bd, sigma = NR.gaussian(x, [20.0, 0.0])
    for k, snr in enumerate((20.0, 0.0)):
        got = 10 * math.log10(float(NR.power(x)) / float(((y[0, k] - x[0].double()) ** 2).mean()))
        assert abs(got - snr) < 0.1                                          # sample variance of 20000 normals
    clip = NR.test_signal(777, seed=2)[None]
    y, bd, g = NR.background(x, clip, [10.0], offsets=[5])
    got = 10 * math.log10(float(NR.power(x)) / float(((y[0, 0] - x[0].double()) ** 2).mean()))
    assert abs(got - 10.0) < 1e-9 and float(bd.max()) < 1e-6
    silent = torch.full((1, 50), 1e-10)
    assert torch.equal(NR.background(x, silent, [10.0])[0][0, 0], x[0].double()) and float(NR.background(x, silent, [10.0])[2]) == 0.0


# ---- the ABI unit ---------------------------------------------------------------------------------------------------------------
def _declared():
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', HEADER)).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(sconf_[a-z0-9_]+)\s*\(', src)))


def test_binding_is_the_header_and_the_core_does_not_name_it(lib):
    from lcasr_amd.hip import _lib, noise
    funcs, enums = header_abi(HEADER, PREFIX)
    assert sorted(funcs) == _declared() and set(funcs) == NAMES and not enums
    assert_binding_is_header(funcs, noise.PROTOTYPES, noise.PLAIN, 'hip/noise.py')
    assert not any(n.startswith(PREFIX) for n in list(_lib.PROTOTYPES) + list(_lib.PLAIN))
    for n in NAMES:
        assert hasattr(lib, n) and n in _lib.bound()
    for path in (os.path.join(ROOT, 'long-context-asr_amd', 'hip', '_lib.py'), os.path.join(ROOT, 'include', 'sconf.h')):
        assert PREFIX not in open(path).read(), path
    lib.sconf_version.restype = ctypes.c_int
    assert lib.sconf_version() == 220


def test_queries_answer_on_the_host(lib):
    from lcasr_amd.hip import noise
    Q = lib.sconf_noise_tile()
    assert Q == noise.tile() and Q >= 256 and Q % 4 == 0
    assert lib.sconf_noise_max_levels() == noise.max_levels() >= 16
    f = lib.sconf_noise_workspace
    for B in (0, 1, 3, 128):
        for L in (0, 1, Q - 1, Q, Q + 1, 2 * Q + 1, 57_600_000, 2 ** 31 + 7):
            assert f(B, L) == 8 * B * -(-L // Q) == noise.workspace(B, L), (B, L)
    assert f(-1, 5) == -1 and f(5, -1) == -1
    assert f(2 ** 31 - 1, Q) == 8 * (2 ** 31 - 1) and f(2 ** 31, Q) == -1 and f(2 ** 30, Q + 1) == -1        # B ceil(L / tile) >= 2^31
    with pytest.raises(ValueError, match='invalid'):
        noise.workspace(-1, 3)


def test_host_side_validation_sets_the_error_before_any_launch(lib):
    """Every refusal happens before a kernel is enqueued, so none needs a GPU: the pointers are host addresses that are never read."""
    one = ctypes.c_void_p(16)
    Q, M = lib.sconf_noise_tile(), lib.sconf_noise_max_levels()
    err = lib.sconf_last_error

    def power(**kw):
        a = dict(dict(src=one, rs=1000, rows=2, lens=None, sl=None, off=None, L=1000, B=2, power=one, ws=one, wsb=16), **kw)
        return lib.sconf_noise_power(a['src'], a['rs'], a['rows'], a['lens'], a['sl'], a['off'], a['L'], a['B'], a['power'], a['ws'], a['wsb'], None)
    assert power(L=-1) != 0 and b'negative' in err()
    assert power(B=-2) != 0 and b'negative' in err()
    assert power(src=None) != 0 and b'null' in err()
    assert power(power=None) != 0 and b'null' in err()
    assert power(rows=3) != 0 and b'src_rows' in err()
    assert power(rs=999) != 0 and b'stride' in err()
    assert power(wsb=15) != 0 and b'workspace' in err()
    assert power(L=Q + 1, rs=Q + 1, wsb=31) != 0 and b'workspace' in err()
    assert power(ws=None) != 0 and b'workspace' in err()
    assert power(B=2 ** 30, rows=1, L=Q + 1, wsb=2 ** 40) != 0 and b'too many' in err()

    def gauss(**kw):
        a = dict(dict(wave=one, rs=1000, lens=None, L=1000, B=2, power=one, snr=one, K=3, seed=1, row=0, first=0, out=one, os=1000), **kw)
        return lib.sconf_noise_add_gaussian(a['wave'], a['rs'], a['lens'], a['L'], a['B'], a['power'], a['snr'], a['K'], a['seed'], a['row'],
                                            a['first'], a['out'], a['os'], None)

    def back(**kw):
        a = dict(dict(wave=one, rs=1000, lens=None, L=1000, B=2, noise=one, ns=500, nrows=1, nl=None, off=None, power=one, npower=one, snr=one,
                      K=3, out=one, os=1000), **kw)
        return lib.sconf_noise_add_background(a['wave'], a['rs'], a['lens'], a['L'], a['B'], a['noise'], a['ns'], a['nrows'], a['nl'], a['off'],
                                              a['power'], a['npower'], a['snr'], a['K'], a['out'], a['os'], None)
    for call in (gauss, back):
        assert call(K=0) != 0 and b'levels' in err()
        assert call(K=M + 1) != 0 and b'sconf_noise_max_levels' in err()
        assert call(L=-1) != 0 and b'negative' in err()
        assert call(B=-1) != 0 and b'negative' in err()
        assert call(os=999) != 0 and b'stride' in err()
        assert call(rs=999) != 0 and b'stride' in err()
        for name in ('wave', 'power', 'snr', 'out'):
            assert call(**{name: None}) != 0 and b'null' in err()
        assert call(B=2 ** 30, L=Q + 1, rs=Q + 1, os=Q + 1) != 0 and b'too many' in err()
    assert gauss(row=-1) != 0 and b'first_row' in err()
    assert gauss(first=-4) != 0 and b'first_sample' in err()
    assert gauss(first=2 ** 63 - 1000) != 0 and b'first_sample' in err()
    assert gauss(B=2 ** 30, L=Q - 2, rs=Q, os=Q, first=3) != 0 and b'too many' in err()              # the quads of 3 + L samples take a second tile
    assert back(nrows=3) != 0 and b'noise_rows' in err()
    assert back(nrows=0) != 0 and b'noise_rows' in err()
    assert back(ns=-1) != 0 and b'noise stride' in err()
    assert back(noise=None) != 0 and b'null' in err()
    assert back(npower=None) != 0 and b'null' in err()


# ---- host logic -----------------------------------------------------------------------------------------------------------------
def test_snr_forms_and_shapes(emulated):
    A = emulated
    L, lens = 3000, [3000, 5, 1577]
    w = torch.full((3, L + 40), float('nan'))
    for b, n in enumerate(lens): w[b, :n] = NR.test_signal(n, seed=b)
    view = w[:, :L]                                                        # a row stride larger than L
    p = A.wave_power(view, lengths=lens)
    assert p.dtype == torch.float64 and torch.equal(p, NR.power(view, lens)) and A.wave_power(view[0]).shape == (1,)
    one = A.add_gaussian_snr(view, 10.0, lengths=lens)
    y, bd, _ = NR.gaussian(view, 10.0, lens)
    assert one.shape == (3, L) and one.dtype == torch.float32 and bool(((one.double() - y[:, 0]).abs() <= bd[:, 0]).all())
    assert not bool(one[1, 5:].any()) and bool(torch.isfinite(one).all())
    many = A.add_gaussian_snr(view, [10.0, 0.0], lengths=torch.tensor(lens, dtype=torch.int32))
    assert many.shape == (3, 2, L) and torch.equal(many[:, 0], one)
    per_row = A.add_gaussian_snr(view, torch.tensor([[10.0], [0.0], [10.0]]), lengths=lens)
    assert per_row.shape == (3, 1, L) and torch.equal(per_row[0, 0], one[0]) and torch.equal(per_row[1, 0], many[1, 1])
    flat = A.add_gaussian_snr(view[2, :lens[2]], [10.0, 0.0], first_row=2)                  # a row alone: the bits of the row in the batch
    assert flat.shape == (2, lens[2]) and torch.equal(flat, many[2, :, :lens[2]])
    assert A.add_gaussian_snr(view[0], 3).shape == (L,) and A.add_gaussian_snr(view[0], np.float32(3)).shape == (L,)
    assert torch.equal(A.add_gaussian_snr(view[0], math.inf), view[0]) and not torch.equal(A.add_gaussian_snr(view[0], 3, seed=2), A.add_gaussian_snr(view[0], 3))
    # pieces of a recording: the power of the whole is not known to a piece, the normals are
    whole, cut = A.add_gaussian_snr(view[0], 0.0), 1001
    piece = A.add_gaussian_snr(view[0, cut:], 0.0, first_sample=cut)
    z_whole = (whole.double() - view[0].double())[cut:] / float(NR.power(view[0:1]).sqrt())
    z_piece = (piece.double() - view[0, cut:].double()) / float(NR.power(view[0:1, cut:]).sqrt())
    assert float((z_whole - z_piece).abs().max()) < 1e-5

    clip = NR.test_signal(777, seed=9)
    bg = A.add_background_noise(view, clip, [10.0, 20.0], lengths=lens, offsets=[0, 776, 3])
    y, bd, _ = NR.background(view, clip[None], [10.0, 20.0], lens, None, [0, 776, 3])
    assert bg.shape == (3, 2, L) and bool(((bg.double() - y).abs() <= bd).all())
    assert A.add_background_noise(view[0], clip, 10.0).shape == (L,)
    clips = torch.stack([NR.test_signal(4000, seed=10 + b) for b in range(3)])
    bg = A.add_background_noise(view, clips, 5.0, lengths=lens, noise_lengths=[4000, 100, 3577], offsets=[1000, 99, 2000])
    y, bd, _ = NR.background(view, clips, 5.0, lens, [4000, 100, 3577], [1000, 99, 2000])
    assert bg.shape == (3, L) and bool(((bg.double() - y[:, 0]).abs() <= bd[:, 0]).all())
    assert torch.equal(A.add_background_noise(view[0], torch.full((50,), 1e-10), 10.0), view[0])       # a silent clip: the input


def test_refusals(emulated):
    A = emulated
    w = torch.zeros(2, 100)
    for f in (lambda x, **k: A.add_gaussian_snr(x, 10.0, **k), lambda x, **k: A.add_background_noise(x, torch.ones(10), 10.0, **k), A.wave_power):
        with pytest.raises(TypeError, match='float32'):
            f(w.double())
        with pytest.raises(ValueError, match='1D or 2D'):
            f(torch.zeros(1, 2, 100))
        with pytest.raises(ValueError, match='empty'):
            f(torch.zeros(2, 0))
        with pytest.raises(ValueError, match='lengths'):
            f(w, lengths=[100])
        with pytest.raises(ValueError, match='lengths'):
            f(w, lengths=[100, 101])
    for bad in (float('nan'), [10.0, float('nan')], torch.tensor([[1.0], [float('nan')]])):
        with pytest.raises(ValueError, match='NaN'):
            A.add_gaussian_snr(w, bad)
    with pytest.raises(ValueError, match='sconf_noise_max_levels'):
        A.add_gaussian_snr(w, list(range(17)))
    with pytest.raises(ValueError, match='sconf_noise_max_levels'):
        A.add_gaussian_snr(w, [])
    with pytest.raises(ValueError, match='rows'):
        A.add_gaussian_snr(w, torch.zeros(3, 2))
    with pytest.raises(ValueError, match='snr_db'):
        A.add_gaussian_snr(w, torch.zeros(2, 2, 2))
    with pytest.raises(ValueError, match='clips'):
        A.add_background_noise(w, torch.ones(3, 10), 10.0)
    with pytest.raises(TypeError, match='noise'):
        A.add_background_noise(w, torch.ones(10).double(), 10.0)
    with pytest.raises(ValueError, match='offsets'):
        A.add_background_noise(w, torch.ones(10), 10.0, offsets=[0, 10])
    with pytest.raises(ValueError, match='noise_lengths'):
        A.add_background_noise(w, torch.ones(10), 10.0, noise_lengths=[0])


def test_a_cpu_tensor_is_refused_by_the_product_path(lib):
    from lcasr_amd.hip import noise
    from lcasr_amd.utils import audio_tools as A
    w = NR.test_signal(1000)
    for call in (lambda: A.wave_power(w), lambda: A.add_gaussian_snr(w, 10.0), lambda: A.add_background_noise(w, w[:100], 10.0),
                 lambda: noise.power(w[None]), lambda: noise.add_gaussian(w[None], None, torch.ones(1).double(), torch.ones(1, 1), 1)):
        with pytest.raises(RuntimeError, match='GPU'):
            call()


def test_transforms_draw_on_the_host(emulated):
    from lcasr_amd.utils.augmentation import AddBackgroundNoise, AddGaussianSNR
    x = NR.test_signal(2000, seed=3)[None]
    assert AddGaussianSNR(p=0.0)(x, sample_rate=16000) is x and AddBackgroundNoise([x[0]], p=0.0)(x, 16000) is x
    t = AddGaussianSNR(min_snr_db=10, max_snr_db=10, p=1, seed=1)
    first, second = t(x, sample_rate=16000), t(x, sample_rate=16000)
    assert first.shape == x.shape and torch.equal(first, emulated.add_gaussian_snr(x, 10.0, seed=1)) and not torch.equal(first, second)
    assert torch.equal(second, emulated.add_gaussian_snr(x, 10.0, seed=1, first_row=1))    # the next file: the next row of normals
    again = AddGaussianSNR(min_snr_db=10, max_snr_db=10, p=1, seed=1)
    assert torch.equal(again(x), first) and torch.equal(again(x), second)
    a, b = AddGaussianSNR(5, 40, p=0.5, seed=7), AddGaussianSNR(5, 40, p=0.5, seed=7)
    draws = [a.draw_snr() for _ in range(200)]
    assert draws == [b.draw_snr() for _ in range(200)] and draws != [AddGaussianSNR(5, 40, p=0.5, seed=8).draw_snr() for _ in range(200)]
    hit = [d for d in draws if d is not None]
    assert 60 < len(hit) < 140 and all(5 <= d <= 40 for d in hit) and len(set(hit)) == len(hit)
    with pytest.raises(ValueError, match='min_snr_db'):
        AddGaussianSNR(min_snr_db=11, max_snr_db=10)
    with pytest.raises(ValueError, match='p ='):
        AddGaussianSNR(p=1.5)

    sounds = [NR.test_signal(n, seed=20 + i) for i, n in enumerate((500, 2000, 2600, 5000))]
    with pytest.raises(ValueError, match='sounds'):
        AddBackgroundNoise([])
    a, b = AddBackgroundNoise(sounds, 3, 30, p=1, seed=5), AddBackgroundNoise(sounds, 3, 30, p=1, seed=5)
    draws = [a.draw(2000) for _ in range(300)]
    assert draws == [b.draw(2000) for _ in range(300)]
    assert {w for _, w, _ in draws} == {0, 1, 2, 3} and all(3 <= s <= 30 for s, _, _ in draws)
    for _, which, off in draws:                                            # the offset rule: cropped only where the clip is longer
        assert off == 0 if sounds[which].shape[0] <= 2000 else 0 <= off <= sounds[which].shape[0] - 2000
    assert {off for _, w, off in draws if w == 2} >= {0, 600} or len({off for _, w, off in draws if w == 2}) > 20
    t = AddBackgroundNoise(sounds, 10, 10, p=1, seed=5)
    snr, which, off = AddBackgroundNoise(sounds, 10, 10, p=1, seed=5).draw(2000)
    assert snr == 10.0 and torch.equal(t(x, sample_rate=16000), emulated.add_background_noise(x, sounds[which], 10.0, offsets=[off]))


def test_processing_chain_corrupts_before_the_spectrogram(emulated):
    from lcasr_amd.utils.augmentation import AddGaussianSNR
    A = emulated
    w = torch.stack([NR.test_signal(3200, seed=3), NR.test_signal(3200, seed=4)])
    clean = A.processing_chain(w, 16000)
    assert torch.equal(A.processing_chain(w, 16000, corrupt=None), clean)
    got = A.processing_chain(w, 16000, corrupt=AddGaussianSNR(10, 10, p=1, seed=1))
    assert got.shape == clean.shape and not torch.equal(got, clean)
    assert torch.equal(got, A.to_spectogram(A.add_gaussian_snr(w[0:1], 10.0, seed=1)))
    seen = []
    A.processing_chain(w, 16000, corrupt=lambda x, sample_rate: seen.append((tuple(x.shape), sample_rate)) or x)
    assert seen == [((1, 3200), 16000)]
