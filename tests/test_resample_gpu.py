"""GPU tests of the resampler (csrc/resample.hip through lcasr_amd.utils.audio_tools.resample) against tests/resample_refs.py.

Every case compares with the float64 restatement (f64 taps, f64 sums) per sample within resample_refs.bound,
(K + C + 2) 2^-24 sum_k |h[p][k]| |x[..]|, and prints max err / bound of the kernel and of the f32 restatement (what the reference
computes) before it asserts.

Shapes are the smallest at which the indexing can go wrong: rows shorter than the filter and around one and two input periods,
outputs around one and two tiles of the kernel (sconf_resample_tile) for input spans of 2.76, 3, 0.5 and 0.69 times the tile (the
last with the largest table), a down- and an up-sampling to other rates, a ragged batch at a row stride, channels mixed while
staging, row offsets and sample positions past 2^31, and the tiny model behind the resampler."""
import pytest
import torch

import audio_refs as AR
import resample_refs as RR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def A():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from lcasr_amd.hip import resample
    from lcasr_amd.utils import audio_tools
    resample.load()
    return audio_tools


@pytest.fixture(scope='module')
def Q(A):
    return A.resampler.tile()


def check(name, got, wave, orig, new, lengths=None, channels=0, mag=None):
    """Print and assert the bound for got against the float64 restatement of `wave` (CPU); `mag` where the bound's |x| is not |wave|."""
    r = RR.resample(wave.double(), orig, new, lengths)
    f = RR.resample(wave.float(), orig, new, lengths, dtype=torch.float32)
    bd = RR.bound(wave if mag is None else mag, orig, new, lengths, channels=channels)
    assert got.shape == r.shape and got.dtype == torch.float32, (name, tuple(got.shape), tuple(r.shape))
    g = got.detach().double().cpu()
    assert bool(torch.isfinite(g).all()), name
    tiny = 1e-300
    e_k, e_f = float(((g - r).abs() / bd.clamp(min=tiny)).max()), float(((f.double() - r).abs() / bd.clamp(min=tiny)).max())
    print(f'[resample gpu] {name}: L_out {r.shape[-1]}  max err / bound: kernel {e_k:.3f}  f32 restatement {e_f:.3f}  (max bound {float(bd.max()):.2e})')
    assert bool(((g - r).abs() <= bd).all()), (name, e_k)
    return e_k


def length_for(target, orig, new):
    """The shortest row whose output has at least `target` samples (exactly `target` where the ratio can reach it)."""
    O, P = RR.ratio(orig, new)
    L = max(1, target * O // P)
    while RR.out_length(L, orig, new) < target: L += 1
    return L


@pytest.mark.parametrize('L', [1, 5, 440, 441, 442, 882, 883])
def test_short_rows_44100(A, L):
    w = RR.test_signal(L, 44100, seed=L)
    got = A.resample(w.cuda(), 44100, 16000)
    assert got.is_cuda and got.shape == (RR.out_length(L, 44100, 16000),)
    check(f'44100 -> 16000 L={L}', got, w, 44100, 16000)
    assert torch.equal(A.resample(w.cuda()[None], 44100, 16000)[0], got)


@pytest.mark.parametrize('edge', ['Q-1', 'Q', 'Q+1', '2Q+1'])
@pytest.mark.parametrize('orig', [44100, 48000, 8000, 11025])
def test_tile_edges(A, Q, orig, edge):
    target = {'Q-1': Q - 1, 'Q': Q, 'Q+1': Q + 1, '2Q+1': 2 * Q + 1}[edge]
    L = length_for(target, orig, 16000)
    w = RR.test_signal(L, orig, seed=target)
    got = A.resample(w.cuda(), orig, 16000)
    assert target <= got.shape[0] <= target + 1
    check(f'{orig} -> 16000 L_out {edge} (L={L})', got, w, orig, 16000)


@pytest.mark.parametrize('orig, new', [(16000, 8000), (44100, 48000)])
def test_other_target_rates(A, Q, orig, new):
    L = length_for(2 * Q + 1, orig, new)
    w = RR.test_signal(L, orig, seed=7)
    check(f'{orig} -> {new} L_out 2Q+1 (L={L})', A.resample(w.cuda(), orig, new), w, orig, new)


@pytest.fixture(scope='module')
def ragged(A, Q):
    Lmax = length_for(Q + 1, 44100, 16000) + 5
    lens = [Lmax, 5, Lmax // 2 + 77]
    w = torch.full((3, Lmax + 40), float('nan'))
    for b, n in enumerate(lens): w[b, :n] = RR.test_signal(n, 44100, seed=20 + b)
    return {'lens': lens, 'Lmax': Lmax, 'cpu': w[:, :Lmax], 'dev': w.cuda()[:, :Lmax]}


def test_ragged_batch_rows_equal_the_rows_alone(A, ragged):
    lens, view = ragged['lens'], ragged['dev']
    assert view.stride(0) > ragged['Lmax']
    got = A.resample(view, 44100, 16000, lengths=lens)
    check('ragged batch 44100 -> 16000', got, ragged['cpu'], 44100, 16000, lengths=lens)
    nl = A.resampled_lengths(torch.tensor(lens), 44100, 16000).tolist()
    for b, n in enumerate(lens):
        alone = A.resample(view[b, :n].clone(), 44100, 16000)
        assert alone.shape == (nl[b],) and torch.equal(got[b, :nl[b]], alone), b
        assert not bool(got[b, nl[b]:].any())
    assert torch.equal(got, A.resample(view, 44100, 16000, lengths=torch.tensor(lens, device='cuda')))
    assert torch.equal(got.view(torch.int32), A.resample(view, 44100, 16000, lengths=lens).view(torch.int32))        # two calls, the same bits


@pytest.mark.parametrize('channels', [2, 3])
def test_mix_in_one_pass_against_the_two_step_forms(A, Q, channels):
    L = length_for(Q + 1, 44100, 16000)
    w = torch.stack([RR.test_signal(L, 44100, seed=30 + c) for c in range(channels)])
    d = w.cuda()
    left, mean = A.resample(d, 44100, 16000, mix='left'), A.resample(d, 44100, 16000, mix='mean')
    assert left.shape == mean.shape == (1, RR.out_length(L, 44100, 16000))
    check(f"mix='left' of {channels}", left, w[0:1], 44100, 16000)
    mag = w.double().abs().mean(0, keepdim=True)
    check(f"mix='mean' of {channels}", mean, w.double().mean(0, keepdim=True), 44100, 16000, channels=channels, mag=mag)
    assert torch.equal(left, A.resample(A.grab_left_channel(d), 44100, 16000))
    two_step = A.resample(A.take_mean_channel(d), 44100, 16000)
    check(f"take_mean_channel of {channels}, then resample", two_step, w.double().mean(0, keepdim=True), 44100, 16000, channels=channels, mag=mag)
    nan_right = d.clone()
    nan_right[1:] = float('nan')
    assert torch.equal(A.resample(nan_right, 44100, 16000, mix='left'), left)               # nothing of the other channels is read
    assert torch.equal(A.resample(d[0], 16000, 16000, mix='mean'), d[0:1]) and A.resample(d, 16000, 16000) is d


def test_row_offsets_beyond_2_to_the_31(A):
    stride, L = 2 ** 31 + 4096, 883
    try:
        buf = torch.empty(stride + L, dtype=torch.float32, device='cuda')
    except RuntimeError as e:                                              # torch.cuda.OutOfMemoryError is one
        pytest.skip(f'cannot allocate {4 * (stride + L) >> 20} MiB: {e}')
    view = buf.as_strided((2, L), (stride, 1))
    w = torch.stack([RR.test_signal(L, 44100, seed=70), RR.test_signal(L, 44100, seed=71)])
    view.copy_(w.cuda())
    got = A.resample(view, 44100, 16000)
    check('row stride 2^31 + 4096', got, w, 44100, 16000)
    assert torch.equal(got[1], A.resample(w[1].cuda(), 44100, 16000))
    del buf, view


def test_sample_positions_beyond_2_to_the_31(A):
    """One row of 2^31 + 3 * 441 + 7 samples, zero except for its last 20000: the outputs over the tail against the restatement of
    the tail cut at a multiple of 441 (so that the phases line up), the outputs before it zero."""
    L, N = 2 ** 31 + 3 * 441 + 7, 20000
    try:
        x = torch.zeros(L, dtype=torch.float32, device='cuda')
        tail = RR.test_signal(N, 44100, seed=90)
        x[L - N:] = tail.cuda()
        got = A.resample(x, 44100, 16000)
    except torch.cuda.OutOfMemoryError as e:
        pytest.skip(f'cannot allocate {4 * L >> 20} MiB in and {4 * RR.out_length(L, 44100, 16000) >> 20} MiB out: {e}')
    assert got.shape == (RR.out_length(L, 44100, 16000),) and got.shape[0] > 779_000_000
    cut = (L - N - 441) // 441 * 441                                       # at least 441 zeros before the tail: no tap reaches back over them
    j_cut = cut // 441 * 160
    w = torch.zeros(L - cut)
    w[L - N - cut:] = tail
    check('positions past 2^31: the tail', got[j_cut:], w, 44100, 16000)
    assert not bool(got[:j_cut].any())
    del x, got


# ---- end to end, tiny model -------------------------------------------------------------------------------------------------
class WordTok:
    def __init__(self, V): self.V = V
    def vocab_size(self): return self.V
    def decode(self, ids): return ' '.join(f'w{int(i) % 7}' for i in ids)


CFG = dict(vocab_size=127, n_layers=2, d_model=64, n_heads=2, head_dim=32, subsampling_conv_channels=32, use_rotary=True,
           rotary_base_freq=1500000, decoder_norm=True, self_conditioning=True, bias_in_ff=False, default_norm='layer_norm')


def test_transcribe_and_processing_chain_at_44100(A):
    from lcasr_amd.eval import run as R
    from lcasr_amd.models.sconformer_xl import SCConformerXL
    torch.manual_seed(12345)
    model = SCConformerXL(**CFG).cuda().eval()
    tok = WordTok(127)
    wave = torch.stack([RR.test_signal(3 * 44100, 44100, seed=9), RR.test_signal(3 * 44100, 44100, seed=10)])
    d = wave.cuda()
    at16 = A.resample(d[0:1], 44100, 16000)
    assert at16.shape == (1, 48000)
    check('3 s at 44100', at16, wave[0:1], 44100, 16000)
    text = R.transcribe(model, d, tok, 128, 32, sample_rate=44100)
    assert isinstance(text, str) and len(text) > 0 and text == R.transcribe(model, at16, tok, 128, 32)
    chain = A.processing_chain(d, 44100, resample_input=True)
    assert chain.shape == (1, 80, 301) and torch.equal(chain, A.processing_chain(at16, 16000)) and torch.equal(chain, A.to_spectogram(at16))
    host = RR.resample(wave[0:1], 44100, 16000, dtype=torch.float32)       # the host detour the keyword replaces
    e = AR.row_error(chain, A.to_spectogram(host.cuda()))
    print(f'[resample gpu] processing_chain(44100, resample_input=True) against the 16 kHz path on the host-resampled waveform: E = {e:.2e}')
    specs = list(R.spectrograms_of([('r0', d, 'w1 w2')], sample_rate=44100))
    assert specs[0][0] == 'r0' and specs[0][2] == 'w1 w2' and torch.equal(specs[0][1], chain)
    with pytest.raises(NotImplementedError, match='44100'):
        A.processing_chain(d, 44100)
