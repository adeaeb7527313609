"""GPU tests of the noise corruption (csrc/noise.hip through lcasr_amd.utils.audio_tools and lcasr_amd.hip.noise) against
tests/noise_refs.py.

Every value is compared with the float64 restatement within the bounds derived there, per sample, and every test prints
max err / bound before it asserts.  Shapes are the smallest at which the indexing can go wrong: rows of 1, 2, 3, 5 and 6 samples (the
quad boundary), around one and two tiles of the kernels (sconf_noise_tile), a ragged batch at a row stride with NaN behind every
length, bases and strides that are and are not multiples of 16 bytes, a first_sample past 2^34 that is no multiple of four, clips
that wrap and clips that are cropped, a row stride and a row past 2^31 samples, and the tiny model behind the corruption."""
import math

import pytest
import torch

import noise_refs as NR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def A():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from lcasr_amd.hip import noise
    from lcasr_amd.utils import audio_tools
    noise.load()
    return audio_tools


@pytest.fixture(scope='module')
def Q(A):
    return A.noiser.tile()


def check(name, got, y, bd):
    """Print and assert |got - y| <= bd per element (bd == 0: equal)."""
    assert tuple(got.shape) == tuple(y.shape), (name, tuple(got.shape), tuple(y.shape))
    g = got.detach().double().cpu()
    assert bool(torch.isfinite(g).all()), name
    err = (g - y).abs()
    ratio = float((err / bd.clamp(min=1e-300)).max()) if err.numel() else 0.0
    print(f'[noise gpu] {name}: max err / bound = {ratio:.3f}  (max bound {float(bd.max()) if bd.numel() else 0.0:.2e})')
    assert bool((err <= bd).all()), (name, ratio)
    return ratio


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32 if a.dtype == torch.float32 else torch.int64),
                                                                     b.contiguous().view(torch.int32 if b.dtype == torch.float32 else torch.int64))


def edge_lengths(Q):
    return {'1': 1, '5': 5, 'Q-1': Q - 1, 'Q': Q, 'Q+1': Q + 1, '2Q+1': 2 * Q + 1}


@pytest.fixture(scope='module')
def ragged(A, Q):
    L = 2 * Q + 1
    lens = [L, 5, L // 2 + 77]
    w = torch.full((3, L + 40), float('nan'))
    for b, n in enumerate(lens): w[b, :n] = NR.test_signal(n, seed=20 + b)
    return {'lens': lens, 'L': L, 'cpu': w[:, :L], 'dev': w.cuda()[:, :L]}


# ---- power ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('edge', ['1', '5', 'Q-1', 'Q', 'Q+1', '2Q+1'])
def test_power_of_one_row(A, Q, edge):
    L = edge_lengths(Q)[edge]
    w = NR.test_signal(L, seed=L)
    got = A.wave_power(w.cuda())
    exact = NR.power(w[None])
    assert got.is_cuda and got.dtype == torch.float64
    check(f'power L={edge}', got, exact, NR.power_bound(exact, None, L))
    assert same_bits(got, A.wave_power(w.cuda()[None]))
    pad = torch.zeros(L + 1, device='cuda')
    pad[1:] = w.cuda()
    assert same_bits(got, A.wave_power(pad[1:]))                             # a base that is no multiple of 16 bytes: the same bits


def test_power_of_a_ragged_batch(A, ragged):
    lens, view = ragged['lens'], ragged['dev']
    assert view.stride(0) > ragged['L']
    got = A.wave_power(view, lengths=lens)
    exact = NR.power(ragged['cpu'], lens)
    check('power, ragged batch', got, exact, NR.power_bound(exact, lens, ragged['L']))
    for b, n in enumerate(lens):
        assert same_bits(got[b:b + 1], A.wave_power(view[b, :n].clone())), b
    assert same_bits(got, A.wave_power(view, lengths=torch.tensor(lens, device='cuda')))
    assert float(A.wave_power(view, lengths=[0, 5, 0])[0]) == 0.0


@pytest.mark.parametrize('sl', ['1', '7', 'Q+3'])
def test_power_of_a_wrapped_clip(A, Q, sl):
    n = {'1': 1, '7': 7, 'Q+3': Q + 3}[sl]
    L = 2 * Q + 1
    clip = torch.full((1, n + 9), float('nan'))
    clip[0, :n] = NR.test_signal(n, seed=60 + n) + 0.01
    lens, offs = [L, 5, n - min(n - 1, 3)], [n - 1, n // 2, min(n - 1, 3)]   # the last row: off + len == sl exactly
    dev = lambda v: torch.tensor(v, dtype=torch.int64, device='cuda')
    got = A.noiser.power(clip.cuda(), dev(lens), dev([n]), dev(offs), L=L, B=3)
    exact = NR.power(clip, lens, [n], offs, L=L, B=3)
    check(f'wrapped power sl={sl}', got, exact, NR.power_bound(exact, lens, L))
    rows = clip.expand(3, -1).contiguous().cuda()
    assert same_bits(got, A.noiser.power(rows, dev(lens), dev([n] * 3), dev(offs), L=L, B=3))         # a clip per row: the same bits


# ---- gaussian ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('edge', ['1', '2', '3', '5', '6', 'Q-1', 'Q', 'Q+1', '2Q+1'])
def test_gaussian_of_one_row(A, Q, edge):
    L = dict(edge_lengths(Q), **{'2': 2, '3': 3, '6': 6})[edge]
    w = NR.test_signal(L, seed=100 + L) + (0.1 if L < 4 else 0.0)
    snrs = [10.0, 0.0, 25.0]
    y, bd, _ = NR.gaussian(w[None], snrs)
    three = A.add_gaussian_snr(w.cuda(), snrs)
    assert three.is_cuda and three.dtype == torch.float32
    check(f'gaussian L={edge} K=3', three, y[0], bd[0])
    one = A.add_gaussian_snr(w.cuda(), 10.0)
    check(f'gaussian L={edge} K=1', one, y[0, 0], bd[0, 0])
    assert same_bits(one, three[0]) and same_bits(three, A.add_gaussian_snr(w.cuda()[None], snrs)[0])
    pad = torch.zeros(L + 1, device='cuda')
    pad[1:] = w.cuda()
    assert same_bits(three, A.add_gaussian_snr(pad[1:], snrs))              # element path against 16-byte path
    assert same_bits(A.add_gaussian_snr(w.cuda(), math.inf), w.cuda())      # no noise: the input, bit for bit
    assert not torch.equal(A.add_gaussian_snr(w.cuda(), 10.0, seed=17926), one)


def test_gaussian_of_a_ragged_batch(A, ragged):
    lens, view, cpu, L = ragged['lens'], ragged['dev'], ragged['cpu'], ragged['L']
    snrs = torch.tensor([[20.0, 3.0, -5.0], [10.0, 0.0, 30.0], [0.0, 40.0, 6.0]])
    got = A.add_gaussian_snr(view, snrs, lengths=lens, seed=99)
    y, bd, sigma = NR.gaussian(cpu, snrs, lens, seed=99)
    assert got.shape == (3, 3, L)
    check('gaussian, ragged batch', got, y, bd)
    assert same_bits(got, A.add_gaussian_snr(view, snrs.cuda(), lengths=lens, seed=99))
    for b, n in enumerate(lens):
        alone = A.add_gaussian_snr(view[b, :n].clone(), snrs[b], seed=99, first_row=b)
        assert same_bits(alone, got[b, :, :n]), b
        assert not bool(got[b, :, n:].any())                                # tails behind the lengths are 0
        # the K levels are one z: (y_k - x) / sigma_k of every level, each within its share of the bound of the others
        z = (got[b, :, :n].double().cpu() - cpu[b, :n].double()[None]) / sigma[b, :, None]
        slack = bd[b, :, :n] / sigma[b, :, None]
        for k in (1, 2):
            assert bool(((z[k] - z[0]).abs() <= slack[k] + slack[0]).all()), (b, k)
    silent = A.add_gaussian_snr(torch.zeros(2, 50, device='cuda'), [10.0, 0.0])
    assert not bool(silent.any())


def test_gaussian_first_sample_in_the_high_counter_word(A, Q):
    first, L = 2 ** 34 + 3, Q + 6
    w = torch.stack([NR.test_signal(L, seed=70), NR.test_signal(L, seed=71)])
    got = A.add_gaussian_snr(w.cuda(), [5.0, 15.0], seed=2 ** 40 + 17, first_row=2 ** 32 + 1, first_sample=first)
    y, bd, _ = NR.gaussian(w, [5.0, 15.0], seed=2 ** 40 + 17, first_row=2 ** 32 + 1, first_sample=first)
    check('gaussian, first_sample 2^34 + 3', got, y, bd)
    cut = 4097                                                              # the row in two pieces: the normals of one pass
    p = A.wave_power(w.cuda())
    snr = torch.tensor([[5.0], [5.0]], device='cuda')
    whole = A.noiser.add_gaussian(w.cuda(), None, p, snr, 3, 0, first)
    a = A.noiser.add_gaussian(w.cuda()[:, :cut], None, p, snr, 3, 0, first)
    b = A.noiser.add_gaussian(w.cuda()[:, cut:], None, p, snr, 3, 0, first + cut)
    assert same_bits(torch.cat([a, b], 2), whole)


# ---- background -------------------------------------------------------------------------------------------------------------------
def test_background_clips_wrap_and_crop(A, Q, ragged):
    lens, view, cpu, L = ragged['lens'], ragged['dev'], ragged['cpu'], ragged['L']
    snrs = [10.0, 0.0, 20.0]
    short = NR.test_signal(Q // 3 + 1, seed=80)                             # shorter than the row: it wraps, shared by the rows
    got = A.add_background_noise(view, short.cuda(), snrs, lengths=lens, offsets=[0, Q // 3, 100])
    y, bd, _ = NR.background(cpu, short[None], snrs, lens, None, [0, Q // 3, 100])
    check('background, shared clip that wraps', got, y, bd)
    for b, n in enumerate(lens):
        assert not bool(got[b, :, n:].any())
        alone = A.add_background_noise(view[b, :n].clone(), short.cuda(), snrs, offsets=[[0, Q // 3, 100][b]])
        assert same_bits(alone, got[b, :, :n]), b
    clips = torch.full((3, L + 60), float('nan'))                           # a clip per row: longer and cropped to end with the row, wrapping, one sample
    nl, offs = [L + 33, 700, 1], [33, 699, 0]
    for b, n in enumerate(nl): clips[b, :n] = NR.test_signal(n, seed=84 + b) + 0.01
    got = A.add_background_noise(view, clips.cuda(), 6.0, lengths=lens, noise_lengths=nl, offsets=offs)
    y, bd, _ = NR.background(cpu, clips, 6.0, lens, nl, offs)
    assert got.shape == (3, L)
    check('background, a clip per row', got, y[:, 0], bd[:, 0])
    pad = torch.zeros(L + 1, device='cuda')
    pad[1:] = view[0]
    assert same_bits(A.add_background_noise(pad[1:], short.cuda(), snrs), A.add_background_noise(view[0].clone(), short.cuda(), snrs))


def test_background_silence(A, Q):
    L = Q + 1
    x = NR.test_signal(L, seed=90).cuda()
    x[7] = -0.0
    for clip in (torch.zeros(100), torch.full((100,), 9e-10), torch.zeros(2 * L)):
        assert same_bits(A.add_background_noise(x, clip.cuda(), -10.0), x)                  # a silent clip: the input, bit for bit
    assert not same_bits(A.add_background_noise(x, torch.full((100,), 2e-9).cuda(), -10.0), x)
    quiet = A.add_background_noise(torch.zeros(2, L, device='cuda'), NR.test_signal(100, seed=91).cuda(), [10.0, 0.0])
    assert quiet.shape == (2, 2, L) and not bool(quiet.any())                               # a silent row: all zeros


def test_background_realises_the_requested_snr(A, Q):
    L = 2 * Q + 1
    x, clip = NR.test_signal(L, seed=92), NR.test_signal(5000, seed=93)
    snrs = [0.0, 10.0, 20.0]
    y = A.add_background_noise(x.cuda(), clip.cuda(), snrs, offsets=[1234]).double().cpu()
    px = float(NR.power(x[None]))
    for k, snr in enumerate(snrs):
        got = 10 * math.log10(px / float(((y[k] - x.double()) ** 2).mean()))
        print(f'[noise gpu] background at {snr} dB: realised {got:.6f} dB')
        assert abs(got - snr) < 1e-3


# ---- addressing -------------------------------------------------------------------------------------------------------------------
def test_row_offsets_beyond_2_to_the_31(A, Q):
    stride, L = 2 ** 31 + 4096, Q + 1
    try:
        buf = torch.empty(stride + L, dtype=torch.float32, device='cuda')
    except RuntimeError as e:                                              # torch.cuda.OutOfMemoryError is one
        pytest.skip(f'cannot allocate {4 * (stride + L) >> 20} MiB: {e}')
    view = buf.as_strided((2, L), (stride, 1))
    w = torch.stack([NR.test_signal(L, seed=70), NR.test_signal(L, seed=71)])
    view.copy_(w.cuda())
    exact = NR.power(w)
    check('row stride 2^31 + 4096: power', A.wave_power(view), exact, NR.power_bound(exact, None, L))
    y, bd, _ = NR.gaussian(w, [10.0, 0.0])
    check('row stride 2^31 + 4096: gaussian', A.add_gaussian_snr(view, [10.0, 0.0]), y, bd)
    clip = NR.test_signal(777, seed=72)
    y, bd, _ = NR.background(w, clip[None], [10.0], None, None, [0, 5])
    check('row stride 2^31 + 4096: background', A.add_background_noise(view, clip.cuda(), [10.0], offsets=[0, 5]), y, bd)
    del buf, view


def test_sample_positions_beyond_2_to_the_31(A):
    """One row of 2^31 + 7 samples, zero except for its last 20000: its power, and the Gaussian and background mixes over the tail
    against the restatement at first_sample = the tail's start (the factors from the whole row's power)."""
    L, N, nl = 2 ** 31 + 7, 20000, 777
    tail, clip = NR.test_signal(N, seed=90), NR.test_signal(nl, seed=91)
    try:
        x = torch.zeros(L, dtype=torch.float32, device='cuda')
        x[L - N:] = tail.cuda()
        p = A.wave_power(x)
        mixed = A.add_gaussian_snr(x, -30.0, seed=4)
    except torch.cuda.OutOfMemoryError as e:
        pytest.skip(f'cannot allocate two rows of {4 * L >> 20} MiB: {e}')
    exact = NR.power(tail[None]) * N / L
    check('positions past 2^31: power', p, exact, NR.power_bound(exact, None, L))
    sigma = float(exact.sqrt()) * 10.0 ** 1.5
    z, r = NR.normals(4, 0, L - N, N)
    y = tail.double() + sigma * z
    check('positions past 2^31: gaussian tail', mixed[L - N:], y, NR.U24 * (y.abs() + 10 * sigma * r))
    head = mixed[:1 << 20].double().cpu()                                   # and the head: noise alone, the row's first normals
    z, r = NR.normals(4, 0, 0, 1 << 20)
    check('positions past 2^31: gaussian head', head, sigma * z, NR.U24 * (sigma * z.abs() + 10 * sigma * r))
    del mixed
    try:
        pv = A.noiser.power(clip.cuda()[None], None, None, torch.zeros(1, dtype=torch.int64, device='cuda'), L=L, B=1)
        mixed = A.add_background_noise(x, clip.cuda(), 0.0)
    except torch.cuda.OutOfMemoryError as e:
        pytest.skip(f'cannot allocate two rows of {4 * L >> 20} MiB: {e}')
    count = torch.full((nl,), L // nl, dtype=torch.float64) + (torch.arange(nl) < L % nl)          # how often the row takes each sample
    pv_exact = (clip.double() ** 2 * count).sum() / L
    check('positions past 2^31: power of the wrapped clip', pv, pv_exact.reshape(1), NR.power_bound(pv_exact.reshape(1), None, L))
    g = math.sqrt(float(exact) / float(pv_exact))
    gv = g * clip.double()[(L - N + torch.arange(N)) % nl]
    y = tail.double() + gv
    check('positions past 2^31: background tail', mixed[L - N:], y, NR.U24 * y.abs() + 2 * NR.U24 * gv.abs())
    del x, mixed


# ---- end to end, tiny model -------------------------------------------------------------------------------------------------
class WordTok:
    def __init__(self, V): self.V = V
    def vocab_size(self): return self.V
    def decode(self, ids): return ' '.join(f'w{int(i) % 7}' for i in ids)


CFG = dict(vocab_size=127, n_layers=2, d_model=64, n_heads=2, head_dim=32, subsampling_conv_channels=32, use_rotary=True,
           rotary_base_freq=1500000, decoder_norm=True, self_conditioning=True, bias_in_ff=False, default_norm='layer_norm')


def test_transcribe_and_snr_sweep(A):
    from lcasr_amd.eval import run as R
    from lcasr_amd.models.sconformer_xl import SCConformerXL
    from lcasr_amd.utils.augmentation import AddGaussianSNR
    torch.manual_seed(12345)
    model = SCConformerXL(**CFG).cuda().eval()
    tok = WordTok(127)
    x = NR.test_signal(3 * 16000, seed=9).cuda()
    clean = R.transcribe(model, x, tok, 128, 32)
    before = A.add_gaussian_snr(x, 10.0, seed=1)
    text = R.transcribe(model, x, tok, 128, 32, corrupt=AddGaussianSNR(10, 10, p=1, seed=1))
    assert isinstance(text, str) and len(text) > 0 and text == R.transcribe(model, before, tok, 128, 32)
    specs = list(R.spectrograms_of([('r0', x, 'w1 w2')], corrupt=AddGaussianSNR(10, 10, p=1, seed=1)))
    assert torch.equal(specs[0][1], A.to_spectogram(before[None]))
    snrs = [100, 0, -20]
    sweep = R.sweep_spectrograms(x, snrs)
    assert sweep.shape == (3, 80, 301)
    for k, snr in enumerate(snrs):
        assert same_bits(sweep[k], A.to_spectogram(A.add_gaussian_snr(x, snr))), snr
    records = R.snr_sweep(model, [('r0', x, clean.lower())], tok, 128, 32, snrs)
    assert [r['snr_db'] for r in records] == [100.0, 0.0, -20.0] and all(set(r) == {'snr_db', 'wer', 'words', 'ins_rate', 'del_rate', 'sub_rate'} for r in records)
    print('[noise gpu] snr_sweep of the tiny model: ' + '  '.join(f'{r["snr_db"]:.0f} dB: WER {r["wer"]:.3f}' for r in records))
    assert records[0]['wer'] == 0.0 and records[0]['words'] == len(clean.split())           # at 100 dB the transcript is the clean one
    assert R.transcribe(model, A.add_gaussian_snr(x, 100.0), tok, 128, 32) == clean
    clip = NR.test_signal(5000, seed=10).cuda()
    records = R.snr_sweep(model, [('r0', x, clean.lower())], tok, 128, 32, [100.0], noise=clip)
    assert len(records) == 1 and records[0]['wer'] == 0.0
