"""Write-footprint cases of the audio ABI unit (include/sconf_audio.h), laid out with tests/footprint.py: the table that
tests/test_audio_footprint.py checks on the CPU and tests/test_audio_footprint_gpu.py runs on the device.  TEST INFRASTRUCTURE.

CASES maps a case id to (entry point, builder); builder(lib) needs the library only for the two host-side queries.  Shapes: three
rows at a row stride larger than L, lengths [L, 257, about half] with T one frame past a tile, so that a row ends inside the first
tile, one ends inside the second and one has a second tile with a single frame; samples at and beyond a row's length are NaN."""
import torch

import audio_refs as AR
import footprint as FP
from footprint import IN, OUT, SCRATCH

NO_LAUNCH = {'sconf_audio_tile_frames', 'sconf_audio_melspec_workspace'}          # return a value, launch nothing
CASES = {}


def melspec_case(lib, id, n_mels, normalise, out_dtype, ragged):
    F = lib.sconf_audio_tile_frames()
    B, L = 3, 160 * F + 5                                                  # T = F + 1
    T = 1 + L // 160
    stride = L + 24
    lens = [L, 257, L // 2 + 77] if ragged else [L] * B
    wave = torch.stack([AR.test_signal(L, seed=10 + b) for b in range(B)])
    for b, n in enumerate(lens): wave[b, n:] = float('nan')
    fb = AR.mel_filterbank(n_mels)
    a = FP.Arena()
    r_wave = a.take('wave', (B, L), torch.float32, IN, ld=stride, init=wave)
    r_len = a.take('lengths', B, torch.int64, IN, init=torch.tensor(lens, dtype=torch.int64)) if ragged else None
    r_fb = a.take('fb', (AR.N_BINS, n_mels), torch.float32, IN, init=fb)
    r_rng = a.take('ranges', (n_mels, 2), torch.int32, IN, init=AR.filter_ranges(fb))
    r_spec = a.take('spec', (B, n_mels, T), out_dtype, OUT)
    two_pass = normalise and out_dtype == torch.bfloat16
    r_raw = a.take('raw', (B, n_mels, T), torch.float32, SCRATCH) if two_pass else None
    nbytes = int(lib.sconf_audio_melspec_workspace(B, T, n_mels))
    assert nbytes > 0
    r_ws = a.take('workspace', nbytes, torch.uint8, SCRATCH)

    def restate(v):
        return {'spec': AR.to_spectogram(v['wave'], bool(normalise), v.get('lengths'), n_mels=n_mels, dtype=torch.float64)}

    args = [r_wave, stride, r_len, L, r_fb, r_rng, r_spec, 0 if out_dtype == torch.float32 else 1, r_raw, int(normalise), r_ws, nbytes,
            B, T, n_mels]
    return FP.Case(id, 'sconf_audio_melspec', a, args, 'audio_refs.to_spectogram', restate, variant=f'tile{F}')


for _id, _a in {'melspec-f32-raw-ragged': (80, 0, torch.float32, True), 'melspec-f32-norm-ragged': (80, 1, torch.float32, True),
                'melspec-bf16-norm-ragged-40mels': (40, 1, torch.bfloat16, True), 'melspec-bf16-raw-128mels': (128, 0, torch.bfloat16, False),
                'melspec-f32-norm-1mel': (1, 1, torch.float32, False)}.items():
    CASES[_id] = ('sconf_audio_melspec', lambda lib, _id=_id, _a=_a: melspec_case(lib, _id, *_a))


def build(id, lib):
    return CASES[id][1](lib)
