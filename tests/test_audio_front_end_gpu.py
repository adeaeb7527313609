"""GPU tests of the audio front end (csrc/audio.hip through lcasr_amd.utils.audio_tools.to_spectogram) against tests/audio_refs.py.

Error measure: for an output x and the float64 restatement r, E(x) = max over rows (b, mel) of max_t |x - r| / max_t |r|.
Bound of every parity test: E(kernel) <= 4 E(f32 restatement) + 1e-6, the f32 restatement (what the reference computes: torch.stft
and a matmul in f32) evaluated in the same test on the same input; the factor 4 allows for another butterfly order and fused
multiply-adds.  bf16 output adds E of the bf16 rounding of r itself.  Every test prints its figures before it asserts.

Shapes are the smallest at which the indexing can go wrong: one frame reflecting at both ends, hop multiples and their neighbours,
the frames around one and two tiles of the kernel (sconf_audio_tile_frames), a ragged batch at a row stride, row offsets past
2^31 elements, and one 60 s row for the fixed-order merge of the tile statistics."""
import pytest
import torch

import audio_refs as AR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def A():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from lcasr_amd.hip import audio
    from lcasr_amd.utils import audio_tools
    audio.load()
    return audio_tools


@pytest.fixture(scope='module')
def F(A):
    return A.audio.tile_frames()


def check(name, got, wave, norm, lengths=None, n_mels=80, bf16=False):
    """Print and assert the bound for got against the restatement of `wave` (CPU); returns E(kernel)."""
    r = AR.to_spectogram(wave, norm, lengths, n_mels=n_mels, dtype=torch.float64)
    f = AR.to_spectogram(wave, norm, lengths, n_mels=n_mels, dtype=torch.float32)
    assert got.shape == r.shape, (name, tuple(got.shape), tuple(r.shape))
    e_k, e_f = AR.row_error(got, r), AR.row_error(f, r)
    bound = 4 * e_f + 1e-6 + (AR.row_error(r.bfloat16(), r) if bf16 else 0.0)
    print(f'[audio gpu] {name}: E(kernel) {e_k:.2e}  E(f32 restatement) {e_f:.2e}  bound {bound:.2e}')
    assert bool(torch.isfinite(got).all()), name
    assert e_k <= bound, (name, e_k, e_f, bound)
    return e_k


@pytest.mark.parametrize('norm', [False, True], ids=['raw', 'normalised'])
@pytest.mark.parametrize('L', [257, 400, 512, 640, 799, 800, 801])
def test_single_row(A, L, norm):
    w = AR.test_signal(L, seed=L)
    got = A.to_spectogram(w.cuda(), global_normalisation=norm)
    assert got.shape == (80, 1 + L // 160) and got.dtype == torch.float32 and got.is_cuda
    check(f'single row L={L} norm={norm}', got, w, norm)
    assert torch.equal(A.to_spectogram(w.cuda()[None], global_normalisation=norm)[0], got)


@pytest.mark.parametrize('r', [0, 159])
@pytest.mark.parametrize('tiles', ['F-1', 'F', 'F+1', '2F+1'])
def test_tile_edges(A, F, tiles, r):
    T = {'F-1': F - 1, 'F': F, 'F+1': F + 1, '2F+1': 2 * F + 1}[tiles]
    L = 160 * (T - 1) + r
    w = AR.test_signal(L, seed=T + r)
    for norm in (False, True):
        got = A.to_spectogram(w.cuda(), global_normalisation=norm)
        assert got.shape == (80, T)
        check(f'tile edge T={tiles}={T} r={r} norm={norm}', got, w, norm)


@pytest.fixture(scope='module')
def ragged(A, F):
    Lmax = 160 * (F + 1) + 5
    lens = [Lmax, 257, Lmax // 2 + 77]
    buf = torch.full((3, Lmax + 72), float('nan'))
    for b, n in enumerate(lens): buf[b, :n] = AR.test_signal(n, seed=40 + b)
    dev = buf.cuda()
    return dict(Lmax=Lmax, lens=lens, cpu=buf[:, :Lmax], dev=dev[:, :Lmax])


@pytest.mark.parametrize('norm', [False, True], ids=['raw', 'normalised'])
def test_ragged_batch(A, ragged, norm):
    lens, view = ragged['lens'], ragged['dev']
    assert view.stride(0) > ragged['Lmax']
    got = A.to_spectogram(view, global_normalisation=norm, lengths=lens)
    assert got.shape == (3, 80, 1 + ragged['Lmax'] // 160)
    check(f'ragged batch norm={norm}', got, ragged['cpu'], norm, lengths=lens)
    for b, n in enumerate(lens):
        tb = 1 + n // 160
        alone = A.to_spectogram(view[b, :n].clone(), global_normalisation=norm)
        check(f'ragged row {b} alone norm={norm}', alone, ragged['cpu'][b, :n], norm)
        e = AR.row_error(got[b, :, :tb], alone)
        print(f'[audio gpu] ragged row {b} in the batch vs alone: {e:.2e}')
        assert torch.equal(got[b, :, :tb], alone)                          # the same tiles, the same order: the same bits
        assert bool(torch.isfinite(got[b, :, :tb]).all()) and bool((got[b, :, tb:] == 0).all())
    on_device = A.to_spectogram(view, global_normalisation=norm, lengths=torch.tensor(lens).cuda())
    assert torch.equal(on_device, got)


def test_determinism(A, ragged):
    for norm in (True, False):
        a = A.to_spectogram(ragged['dev'], global_normalisation=norm, lengths=ragged['lens'])
        b = A.to_spectogram(ragged['dev'], global_normalisation=norm, lengths=ragged['lens'])
        assert torch.equal(a, b)


def test_row_offsets_beyond_2_to_the_31(A):
    stride, L = 2 ** 31 + 4096, 801
    try:
        buf = torch.empty(stride + L, dtype=torch.float32, device='cuda')
    except RuntimeError as e:                                              # torch.cuda.OutOfMemoryError is one
        pytest.skip(f'cannot allocate {4 * (stride + L) >> 20} MiB: {e}')
    view = buf.as_strided((2, L), (stride, 1))
    w = torch.stack([AR.test_signal(L, seed=70), AR.test_signal(L, seed=71)])
    view.copy_(w.cuda())
    for norm in (False, True):
        got = A.to_spectogram(view, global_normalisation=norm)
        check(f'row stride 2^31 + 4096 norm={norm}', got, w, norm)
        assert torch.equal(got[1], A.to_spectogram(w[1].cuda(), global_normalisation=norm))
    del buf, view


def test_many_tiles_one_minute(A, F):
    L = 960000
    w = AR.test_signal(L, seed=5)
    got = A.to_spectogram(w.cuda())
    assert got.shape == (80, 6001) and 6001 > 100 * F
    check('60 s, normalised', got, w, True)
    assert torch.equal(got, A.to_spectogram(w.cuda()))


def test_options(A, F):
    L = 160 * F + 77
    w = torch.stack([AR.test_signal(L, seed=80), AR.test_signal(L, seed=81)])
    for norm in (True, False):
        got = A.to_spectogram(w.cuda(), global_normalisation=norm, out_dtype=torch.bfloat16)
        assert got.dtype == torch.bfloat16
        check(f'bf16 output norm={norm}', got, w, norm, bf16=True)
    for norm in (True, False):
        got = A.to_spectogram(w.cuda(), global_normalisation=norm, n_mels=64)
        assert got.shape == (2, 64, F + 1)
        check(f'64 mels norm={norm}', got, w, norm, n_mels=64)
    for n_mels in (1, 128):
        check(f'{n_mels} mels raw', A.to_spectogram(w.cuda(), global_normalisation=False, n_mels=n_mels), w, False, n_mels=n_mels)


def test_zero_variance_rows_are_non_finite_as_in_the_reference(A):
    w = torch.zeros(801)
    got = A.to_spectogram(w.cuda()).cpu()
    want = AR.to_spectogram(w, dtype=torch.float32)
    assert bool(want.isnan().all()) and torch.equal(got.isnan(), want.isnan())
    raw = A.to_spectogram(w.cuda(), global_normalisation=False)
    assert bool((raw == 0).all())


def test_refusals_on_the_device_path(A):
    with pytest.raises(ValueError):
        A.to_spectogram(torch.zeros(256, device='cuda'))
    with pytest.raises(RuntimeError, match='GPU'):
        A.to_spectogram(torch.zeros(1000))
    with pytest.raises(TypeError):
        A.to_spectogram(torch.zeros(1000, device='cuda'), out_dtype=torch.float16)


# ---- end to end, tiny model -------------------------------------------------------------------------------------------------
class WordTok:
    def __init__(self, V): self.V = V
    def vocab_size(self): return self.V
    def decode(self, ids): return ' '.join(f'w{int(i) % 7}' for i in ids)


CFG = dict(vocab_size=127, n_layers=2, d_model=64, n_heads=2, head_dim=32, subsampling_conv_channels=32, use_rotary=True,
           rotary_base_freq=1500000, decoder_norm=True, self_conditioning=True, bias_in_ff=False, default_norm='layer_norm')


@pytest.fixture(scope='module')
def tiny(A):
    from lcasr_amd.models.sconformer_xl import SCConformerXL
    torch.manual_seed(12345)
    model = SCConformerXL(**CFG)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    return model.cuda().eval(), sd, AR.test_signal(3 * 16000, seed=9)


def test_transcribe_is_front_end_plus_eval_loop(A, tiny):
    from lcasr_amd.decoding.greedy import GreedyCTCDecoder
    from lcasr_amd.eval import run as R
    model, _, wave = tiny
    tok = WordTok(127)
    text = R.transcribe(model, wave.cuda(), tok, 128, 32)
    spec = A.to_spectogram(wave.cuda()[None])
    assert spec.shape == (1, 80, 301)
    logits = R.moving_average_eval(R._Args(), model, spec, 128, 32, tok, use_tqdm=False, return_numpy=False)
    want = GreedyCTCDecoder(tokenizer=tok, blank_id=model.decoder.num_classes - 1)(logits)
    assert isinstance(text, str) and len(text) > 0 and text == want
    for mode in ('buffered', 'windowed_attention'):
        assert isinstance(R.transcribe(model, wave.cuda(), tok, 128, 32, evaluation_mode=mode), str)
    recs = [('r0', wave.cuda(), 'w1 w2 w3'), ('r1', wave[:20000].cuda(), 'w5 w6')]
    specs = [(i, A.to_spectogram(w[None]), g) for i, w, g in recs]
    assert R.evaluate(model, R.spectrograms_of(recs), tok, 128, 32, include_per_recording_evaluations=True) == \
        R.evaluate(model, specs, tok, 128, 32, include_per_recording_evaluations=True)


def test_model_on_the_front_end_against_the_oracle_on_the_restatement(A, tiny):
    from oracle import sconformer_ref as O
    model, sd, wave = tiny
    with torch.no_grad():
        lp = model(A.to_spectogram(wave.cuda()[None]))['final_posteriors'].float().cpu()
        ref = O.forward(sd, O.make_config(**CFG), AR.to_spectogram(wave[None], dtype=torch.float64).float(), training=False)
    d = (lp - ref['final_posteriors']).abs()
    print(f'[audio gpu] tiny model on the device front end vs oracle on the f64 restatement: log-prob max|d| {float(d.max()):.3f} '
          f'mean|d| {float(d.mean()):.4f}')
    assert lp.shape == ref['final_posteriors'].shape and float(d.mean()) < 0.05
