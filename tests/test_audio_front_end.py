"""CPU tests of the audio front end: the restatement (tests/audio_refs.py) against an independent direct DFT, the filterbank's
sparsity, the host logic of lcasr_amd.utils.audio_tools and of eval.run.transcribe / spectrograms_of with the binding replaced by
the restatement, and the host-side queries and refusals of the audio unit (test_cabi.py holds its binding to include/sconf_audio.h).
The HIP kernels themselves are tested in test_audio_front_end_gpu.py."""
import ctypes

import pytest
import torch

import audio_refs as AR
import eval_refs as E
from common_model import build_from_fixture
from conftest import load_golden


@pytest.fixture
def emulated_audio(monkeypatch):
    """The binding layer (lcasr_amd.hip.audio.melspec) replaced by the f32 restatement: host logic without a GPU."""
    from lcasr_amd.utils import audio_tools
    monkeypatch.setattr(audio_tools.audio, 'melspec', AR.melspec)
    return audio_tools


# ---- the yardstick ------------------------------------------------------------------------------------------------------------
def test_f64_restatement_against_a_direct_dft():
    w = AR.test_signal(1000)
    got, want = AR.mel_row(w, 80, torch.float64), AR.direct_dft_mel(w, 80)
    assert got.shape == want.shape == (80, 7)
    err = float((got - want).abs().max() / want.abs().max())
    print(f'[audio] stft restatement vs direct DFT, L = 1000: rel max err {err:.2e}')
    assert err <= 1e-12


def test_the_test_signal_has_no_flat_mel_row():
    for L in (400, 1000, 48077):
        s = AR.mel_row(AR.test_signal(L), 80, torch.float64)
        assert bool((s.std(-1) > 0).all()) and bool(torch.isfinite(AR.normalise_row(s)).all()), L


def test_filterbank_is_sparse_and_the_product_builds_the_same_table():
    from lcasr_amd.hip import audio
    from lcasr_amd.utils import audio_tools
    fb = AR.mel_filterbank(80)
    assert fb.shape == (257, 80) and fb.dtype == torch.float32
    nz = fb != 0
    assert int(nz.sum(0).min()) >= 1                                       # no all-zero filter
    assert int(nz.sum(1).max()) <= 2                                       # an FFT bin feeds at most two filters
    assert int(nz.sum(0).max()) <= 16
    for n_mels in (1, 40, 64, 80, 128):
        ref = AR.mel_filterbank(n_mels)
        assert torch.equal(audio_tools.mel_filterbank(n_mels), ref), n_mels
        rng = audio.filter_ranges(ref)
        assert rng.dtype == torch.int32 and torch.equal(rng, AR.filter_ranges(ref)), n_mels
        assert int((ref != 0).sum(1).max()) <= 2 and int((rng[:, 1] - rng[:, 0]).sum()) <= 2 * 257
        inside = torch.zeros_like(ref, dtype=torch.bool)
        for m, (lo, hi) in enumerate(rng.tolist()): inside[lo:hi, m] = True
        assert not bool(((ref != 0) & ~inside).any())                      # nothing outside the ranges the kernel visits


# ---- host logic ---------------------------------------------------------------------------------------------------------------
def test_frame_count_and_refusals(emulated_audio):
    A = emulated_audio
    for L in (257, 400, 799, 800, 801):
        s = A.to_spectogram(AR.test_signal(L)[None], global_normalisation=False)
        assert s.shape == (1, 80, 1 + L // 160) and s.dtype == torch.float32, L
        assert A.to_spectogram(AR.test_signal(L), global_normalisation=False).shape == (80, 1 + L // 160)
        assert int(A.spectogram_lengths(L)) == 1 + L // 160
    with pytest.raises(ValueError, match='256'):
        A.to_spectogram(AR.test_signal(256)[None])
    with pytest.raises(NotImplementedError, match='44100'):
        A.processing_chain(AR.test_signal(1000)[None], 44100)
    with pytest.raises(ValueError):
        A.to_spectogram(torch.zeros(2, 2, 1000))
    with pytest.raises(TypeError):
        A.to_spectogram(torch.zeros(1000, dtype=torch.float64))
    with pytest.raises(ValueError, match='length'):
        A.to_spectogram(torch.zeros(2, 1000), lengths=[1000, 256])
    with pytest.raises(ValueError, match='length'):
        A.to_spectogram(torch.zeros(2, 1000), lengths=[1000, 1001])
    with pytest.raises(ValueError, match='length'):
        A.to_spectogram(torch.zeros(2, 1000), lengths=[1000])
    with pytest.raises(ValueError, match='n_mels'):
        A.to_spectogram(torch.zeros(1000), n_mels=129)


def test_a_cpu_tensor_is_refused_by_the_product_path():
    from lcasr_amd.utils import audio_tools as A
    with pytest.raises(RuntimeError, match='GPU'):
        A.to_spectogram(AR.test_signal(1000))
    with pytest.raises(RuntimeError, match='GPU'):
        A.processing_chain(AR.test_signal(1000)[None], 16000)


def test_helpers_follow_the_reference_arithmetic():
    from lcasr_amd.utils import audio_tools as A
    assert (A.WIN_LENGTH, A.HOP_LENGTH, A.SR) == (400, 160, 16000)
    for n in (0, 1, 100, 360000):
        assert A.total_seconds(n) == (n * 160) / 16000
    for s in (0.0, 0.004, 1.0, 3.14159, 3600.0):
        assert A.total_frames(s) == int((s * 16000) / 160)
    stereo = torch.arange(12.).reshape(2, 6)
    assert torch.equal(A.grab_left_channel(stereo), stereo[0, None]) and A.grab_left_channel(stereo[0]).shape == (1, 6)
    assert torch.equal(A.take_mean_channel(stereo), stereo.mean(0, keepdim=True)) and A.take_mean_channel(stereo[1]).shape == (1, 6)
    for fn in (A.grab_left_channel, A.take_mean_channel):
        with pytest.raises(ValueError, match='1D or 2D'):
            fn(torch.zeros(1, 2, 3))
    n = torch.tensor([257, 799, 800, 57600000])
    assert A.spectogram_lengths(n).tolist() == [2, 5, 6, 360001]


def test_to_spectogram_host_logic_equals_the_restatement(emulated_audio):
    A = emulated_audio
    L = 2000
    lens = [2000, 257, 1077]
    w = torch.full((3, L + 40), float('nan'))
    for b, n in enumerate(lens): w[b, :n] = AR.test_signal(n, seed=b)
    view = w[:, :L]                                                        # a row stride larger than L
    for norm in (True, False):
        got = A.to_spectogram(view, global_normalisation=norm, lengths=lens)
        assert got.shape == (3, 80, 13) and got.dtype == torch.float32
        for b, n in enumerate(lens):
            alone = A.to_spectogram(w[b, :n].clone(), global_normalisation=norm)
            tb = int(A.spectogram_lengths(n))
            assert alone.shape == (80, tb) and torch.equal(got[b, :, :tb], alone), (norm, b)
            assert bool((got[b, :, tb:] == 0).all()) and bool(torch.isfinite(got[b]).all())
        assert torch.equal(got, A.to_spectogram(view, global_normalisation=norm, lengths=torch.tensor(lens, dtype=torch.int32)))
        assert torch.equal(got, AR.to_spectogram(view, norm, lens, dtype=torch.float32))
    bf = A.to_spectogram(view, lengths=lens, out_dtype=torch.bfloat16)
    assert bf.dtype == torch.bfloat16 and torch.equal(bf, A.to_spectogram(view, lengths=lens).bfloat16())
    m64 = A.to_spectogram(view[0], n_mels=64)
    assert m64.shape == (64, 13) and torch.equal(m64, AR.to_spectogram(view[0], n_mels=64, dtype=torch.float32))
    strided = torch.stack([w[0, :L], w[0, :L]], 1)                         # (L, 2): channel-last storage, transposed view
    assert torch.equal(A.to_spectogram(strided.T)[1], A.to_spectogram(w[0, :L].clone()))
    chain = A.processing_chain(torch.stack([w[0, :L], w[2, :L]]), 16000, normalise=False)
    assert chain.shape == (1, 80, 13) and torch.equal(chain[0], A.to_spectogram(w[0, :L].clone(), global_normalisation=False))


class WordTok:
    """Toy tokenizer: id i decodes to the word 'w<i % 7>'."""
    def __init__(self, V): self.V = V
    def vocab_size(self): return self.V
    def decode(self, ids): return ' '.join(f'w{int(i) % 7}' for i in ids)


@pytest.mark.parametrize('mode', ['averaged_moving_window', 'buffered', 'windowed_attention'])
def test_transcribe_and_spectrograms_of_on_the_tiny_model(emulated_ops, emulated_audio, monkeypatch, mode):
    from lcasr_amd.decoding.greedy import GreedyCTCDecoder
    from lcasr_amd.eval import run as R
    E.attach(monkeypatch, emulated_ops)
    fx = load_golden('infer_tiny')
    m = build_from_fixture(fx).eval()
    tok = WordTok(int(fx['cfg.vocab_size']))
    wave = AR.test_signal(3 * 16000, seed=3)
    spec = emulated_audio.to_spectogram(wave[None])
    assert spec.shape == (1, 80, 301)
    att = R._windowed_modules(m)
    text = R.transcribe(m, wave, tok, 128, 32, evaluation_mode=mode)
    assert all(a.left_window == -1 and a.right_window == -1 for a in att)
    # the same by hand: the logits of the mode on the spectrogram, greedy decoding
    if mode == 'windowed_attention':
        for a in att: a.left_window = a.right_window = 128 // m.subsampling.subsampling_factor // 2
        fn, sl = R.moving_average_eval, 3600000
    else:
        fn, sl = (R.buffered_eval if mode == 'buffered' else R.moving_average_eval), 128
    logits = fn(R._Args(), m, spec, sl, 32, tok, use_tqdm=False, return_numpy=False)
    for a in att: a.left_window = a.right_window = -1
    want = GreedyCTCDecoder(tokenizer=tok, blank_id=m.decoder.num_classes - 1)(logits)
    assert isinstance(text, str) and text == want and len(text) > 0
    assert R.transcribe(m, torch.stack([wave, -wave]), tok, 128, 32, evaluation_mode=mode) == text        # left channel
    raw = R.transcribe(m, wave, tok, 128, 32, evaluation_mode=mode, normalise=False)
    assert isinstance(raw, str)
    recs = [('r0', wave, 'w1 w2 w3'), ('r1', wave[:20000], 'w5 w6')]
    specs = list(R.spectrograms_of(recs))
    assert [(i, g) for i, _, g in specs] == [('r0', 'w1 w2 w3'), ('r1', 'w5 w6')]
    assert torch.equal(specs[0][1], spec) and specs[1][1].shape == (1, 80, 126)
    assert R.evaluate(m, R.spectrograms_of(recs), tok, 128, 32, evaluation_mode=mode) == R.evaluate(m, specs, tok, 128, 32, evaluation_mode=mode)
    with pytest.raises(ValueError, match='evaluation_mode'):
        R.transcribe(m, wave, tok, 128, 32, evaluation_mode='beam')


# ---- host side of the audio unit (its header is held to the binding in test_cabi.py) ----------------------------------------
def test_audio_host_side_validation_and_queries():
    from lcasr_amd.hip import audio
    lib = audio.load()
    F = lib.sconf_audio_tile_frames()
    assert F >= 8 and audio.tile_frames() == F
    assert audio.melspec_workspace(2, F + 1, 80) == lib.sconf_audio_melspec_workspace(2, F + 1, 80) > 0
    with pytest.raises(ValueError):
        audio.melspec_workspace(1, 10, 0)
    one = ctypes.c_void_p(16)                                              # never dereferenced: every call below is refused on the host
    call = lambda L, T, n_mels, dtype=0, ws=1 << 30, stride=None, raw=None, norm=0: lib.sconf_audio_melspec(
        one, L if stride is None else stride, None, L, one, one, one, dtype, raw, norm, one, ws, 1, T, n_mels, None)
    assert call(256, 2, 80) != 0 and b'reflect' in lib.sconf_last_error()
    assert call(1000, 6, 80) != 0 and b'1 + L / 160' in lib.sconf_last_error()
    assert call(1000, 7, 129) != 0 and b'n_mels' in lib.sconf_last_error()
    assert call(1000, 7, 80, dtype=2) != 0 and b'spec_dtype' in lib.sconf_last_error()
    assert call(1000, 7, 80, ws=lib.sconf_audio_melspec_workspace(1, 7, 80) - 1) != 0 and b'workspace' in lib.sconf_last_error()
    assert call(1000, 7, 80, stride=999) != 0 and b'stride' in lib.sconf_last_error()
    assert call(1000, 7, 80, dtype=1, norm=1) != 0 and b'raw' in lib.sconf_last_error()


def test_torchaudio_agrees_with_the_f32_restatement():
    torchaudio = pytest.importorskip('torchaudio')
    w = AR.test_signal(48077)
    ref = torchaudio.transforms.MelSpectrogram(win_length=400, hop_length=160, n_fft=512, n_mels=80)(w[None])
    got = AR.to_spectogram(w[None], global_normalisation=False, dtype=torch.float32)
    assert ref.shape == got.shape
    assert bool(((ref - got).abs().amax(-1) <= 1e-5 * ref.abs().amax(-1)).all())
