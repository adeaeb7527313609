"""Write-footprint cases of the resampler's ABI unit (include/sconf_resample.h), laid out with tests/footprint.py: the table that
tests/test_resample_footprint.py checks on the CPU and tests/test_resample_footprint_gpu.py runs on the device.  TEST INFRASTRUCTURE.

CASES maps a case id to (entry point, builder); builder(lib) needs the library only for the host-side queries.  Shapes: three rows
at a row stride larger than L, lengths [L, 5, about half], L the shortest row whose output goes past one tile, so that a row ends
inside the first tile's first outputs, one inside the first tile and one has a second tile; samples at and beyond a row's length
are NaN, and so is the whole right channel where only the left one may be read.  The value check is the bound of
tests/resample_refs.py against the float64 restatement, per sample: the case hands the harness the count of samples outside it,
which must be 0."""
import torch

import footprint as FP
import resample_refs as RR
from footprint import IN, OUT

NO_LAUNCH = {'sconf_resample_tile', 'sconf_resample_max_table', 'sconf_resample_out_length'}          # return a value, launch nothing
CASES = {}


def rows_case(lib, id, orig, new, channels, mix):
    from lcasr_amd.utils import audio_tools as A
    Q = lib.sconf_resample_tile()
    taps, first, O, P = A.resample_table(orig, new)
    K = taps.shape[1]
    B, L = 3, Q * O // P + 1
    L_out = int(lib.sconf_resample_out_length(L, O, P))
    assert Q < L_out <= Q + 2
    stride, out_stride = L + 24, L_out + 8
    lens = [L, 5, L // 2 + 77]
    wave = torch.stack([torch.stack([RR.test_signal(L, orig, seed=10 + 4 * b + c) for c in range(channels)]) for b in range(B)])
    for b, n in enumerate(lens): wave[b, :, n:] = float('nan')
    if channels > 1 and not mix: wave[:, 1:] = float('nan')
    a = FP.Arena()
    if channels == 1:
        r_wave = a.take('wave', (B, L), torch.float32, IN, ld=stride, init=wave[:, 0])
    else:
        r_wave = a.take('wave', (B, channels, L), torch.float32, IN, strides=(channels * stride, stride, 1), init=wave)
    r_len = a.take('lengths', B, torch.int64, IN, init=torch.tensor(lens, dtype=torch.int64))
    r_taps = a.take('taps', (P, K), torch.float32, IN, init=taps)
    r_first = a.take('first', P, torch.int32, IN, init=first)
    r_out = a.take('out', (B, L_out), torch.float32, OUT, ld=out_stride, tol=0.0)

    def restate(v):
        w = v['wave'] if channels == 1 else v['wave'].double().mean(1) if mix else v['wave'][:, 0]
        mag = v['wave'].double().abs().mean(1) if channels > 1 and mix else w
        y = RR.resample(w, orig, new, v['lengths'])
        bd = RR.bound(mag, orig, new, v['lengths'], channels=channels if mix else 0)
        outside = lambda out: ((out.double().cpu() - y).abs() > bd).sum().double().reshape(1)
        return {'out': (torch.zeros(1, dtype=torch.float64), outside)}

    args = [r_wave, stride, channels * stride, channels, int(mix), r_len, L, r_taps, r_first, O, P, K, r_out, out_stride, L_out, B]
    return FP.Case(id, 'sconf_resample_rows', a, args, 'resample_refs.resample', restate, variant=f'tile{Q} O{O} P{P} K{K}')


for _id, _a in {'rows-44100-mono-ragged': (44100, 16000, 1, False), 'rows-44100-stereo-left-ragged': (44100, 16000, 2, False),
                'rows-44100-stereo-mean-ragged': (44100, 16000, 2, True), 'rows-8000-mono-ragged': (8000, 16000, 1, False),
                'rows-48000-mono-ragged': (48000, 16000, 1, False)}.items():
    CASES[_id] = ('sconf_resample_rows', lambda lib, _id=_id, _a=_a: rows_case(lib, _id, *_a))


def build(id, lib):
    return CASES[id][1](lib)
