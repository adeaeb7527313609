"""Write-footprint cases of the noise unit (include/sconf_noise.h), laid out with tests/footprint.py: the table that
tests/test_noise_footprint.py checks on the CPU and tests/test_noise_footprint_gpu.py runs on the device.  TEST INFRASTRUCTURE.

CASES maps a case id to (entry point, builder); builder(lib) needs the library only for the host-side queries.  Shapes: three rows
of L = tile + 1 samples at a row stride larger than L, lengths [L, 5, about half]: one row with a second tile, one that ends inside
the first quad and one inside the first tile.  Samples at and beyond a row's length are NaN, and so is everything behind a clip's
noise_lengths.  One case of each mixing launcher has strides that are multiples of four elements (16-byte path), one has not; the
Gaussian one without starts at first_sample = 2^34 + 3.  Values: the bounds of tests/noise_refs.py against its float64 restatement,
per sample; a case hands the harness the count of samples outside them, which must be 0."""
import torch

import footprint as FP
import noise_refs as NR
from footprint import IN, OUT, SCRATCH

NO_LAUNCH = {'sconf_noise_tile', 'sconf_noise_max_levels', 'sconf_noise_workspace'}          # return a value, launch nothing
CASES = {}
B = 3
SNR = [[20.0, 3.0, -5.0], [10.0, 0.0, 30.0], [0.0, 40.0, 6.0]]


def _outside(y, bd):
    """(expected, fn) of footprint.Case: the count of elements of the region outside |got - y| <= bd, against 0."""
    return torch.zeros(1, dtype=torch.float64), lambda out: ((out.double().cpu().reshape(y.shape) - y).abs() > bd).sum().double().reshape(1)


def _rows(a, L, stride, seed):
    lens = [L, 5, L // 2 + 77]
    wave = torch.stack([NR.test_signal(L, seed=seed + b) for b in range(B)])
    for b, n in enumerate(lens): wave[b, n:] = float('nan')
    return (a.take('wave', (B, L), torch.float32, IN, ld=stride, init=wave),
            a.take('lengths', B, torch.int64, IN, init=torch.tensor(lens, dtype=torch.int64)), wave, lens)


def _clips(a, rows, NL, lens, offs, seed):
    noise = torch.stack([0.5 * NR.test_signal(NL, seed=seed + r) for r in range(rows)])
    for r, n in enumerate(lens): noise[r, n:] = float('nan')
    return (a.take('noise', (rows, NL), torch.float32, IN, ld=NL + 12, init=noise),
            a.take('noise_lengths', rows, torch.int64, IN, init=torch.tensor(lens, dtype=torch.int64)),
            a.take('offsets', B, torch.int64, IN, init=torch.tensor(offs, dtype=torch.int64)), noise)


def power_case(lib, id, wrapped):
    Q = lib.sconf_noise_tile()
    L = Q + 1
    a = FP.Arena()
    if wrapped:                                                           # per-row clips: shorter than the row twice over, longer, of one sample
        lens = [L, 5, L // 2 + 77]
        a.take('lengths', B, torch.int64, IN, init=torch.tensor(lens, dtype=torch.int64))
        r_src, r_sl, r_off, _ = _clips(a, B, L + 40, [Q // 2 - 3, L + 33, 1], [Q // 2 - 4, 7, 0], 40)
        r_len, stride, rows = a.regions['lengths'], L + 40 + 12, B
    else:
        stride, rows = L + 24, B
        r_src, r_len, _, lens = _rows(a, L, stride, 10)
        r_sl = r_off = None
    r_pow = a.take('power', B, torch.float64, OUT, tol=0.0)
    nbytes = int(lib.sconf_noise_workspace(B, L))
    r_ws = a.take('ws', nbytes, torch.uint8, SCRATCH)

    def restate(v):
        exact = NR.power(v['noise' if wrapped else 'wave'], v['lengths'], v.get('noise_lengths'), v.get('offsets'), L=L, B=B)
        return {'power': _outside(exact, NR.power_bound(exact, v['lengths'], L))}

    args = [r_src, stride, rows, r_len, r_sl, r_off, L, B, r_pow, r_ws, nbytes]
    return FP.Case(id, 'sconf_noise_power', a, args, 'noise_refs.power', restate, variant=f'tile{Q} {"wrapped" if wrapped else "plain"}')


def gaussian_case(lib, id, vec):
    Q = lib.sconf_noise_tile()
    L, K = Q + 1, 3
    stride, out_stride, first_sample = (L + 27, L + 11, 8) if vec else (L + 24, L + 8, 2 ** 34 + 3)
    assert (stride % 4 == 0) == (out_stride % 4 == 0) == vec
    a = FP.Arena()
    r_wave, r_len, wave, lens = _rows(a, L, stride, 20)
    r_pow = a.take('power', B, torch.float64, IN, init=NR.power(wave, lens))
    r_snr = a.take('snr_db', (B, K), torch.float32, IN, init=torch.tensor(SNR))
    r_out = a.take('out', (B * K, L), torch.float32, OUT, ld=out_stride, tol=0.0)
    seed, first_row = 0x1234567887654321, 2 ** 32 + 5

    def restate(v):
        y, bd, _ = NR.gaussian(v['wave'], v['snr_db'], v['lengths'], seed, first_row, first_sample)
        return {'out': _outside(y.reshape(B * K, L), bd.reshape(B * K, L))}

    args = [r_wave, stride, r_len, L, B, r_pow, r_snr, K, seed, first_row, first_sample, r_out, out_stride]
    return FP.Case(id, 'sconf_noise_add_gaussian', a, args, 'noise_refs.gaussian', restate, variant=f'tile{Q} K{K} {"vec" if vec else "scalar"}')


def background_case(lib, id, vec, shared):
    Q = lib.sconf_noise_tile()
    L, K = Q + 1, 3
    stride, out_stride = (L + 27, L + 11) if vec else (L + 24, L + 8)
    a = FP.Arena()
    r_wave, r_len, wave, lens = _rows(a, L, stride, 30)
    if shared:                                                            # one clip shorter than the row: it wraps, at three offsets
        nlens, offs, NL = [Q // 3 + 1], [0, Q // 3, 100], Q // 3 + 20
    else:                                                                 # a longer clip cropped so that it ends with the row, a wrapping one, one sample
        nlens, offs, NL = [L + 33, 700, 1], [33, 699, 0], L + 40
    r_noise, r_nl, r_off, noise = _clips(a, len(nlens), NL, nlens, offs, 50)
    r_pow = a.take('power', B, torch.float64, IN, init=NR.power(wave, lens))
    r_npow = a.take('noise_power', B, torch.float64, IN, init=NR.power(noise, lens, nlens, offs, L=L, B=B))
    r_snr = a.take('snr_db', (B, K), torch.float32, IN, init=torch.tensor(SNR))
    r_out = a.take('out', (B * K, L), torch.float32, OUT, ld=out_stride, tol=0.0)

    def restate(v):
        y, bd, _ = NR.background(v['wave'], v['noise'], v['snr_db'], v['lengths'], v['noise_lengths'], v['offsets'])
        return {'out': _outside(y.reshape(B * K, L), bd.reshape(B * K, L))}

    args = [r_wave, stride, r_len, L, B, r_noise, NL + 12, len(nlens), r_nl, r_off, r_pow, r_npow, r_snr, K, r_out, out_stride]
    return FP.Case(id, 'sconf_noise_add_background', a, args, 'noise_refs.background', restate,
                   variant=f'tile{Q} K{K} {"vec" if vec else "scalar"} {"shared" if shared else "per-row"}')


for _id, _w in {'power-ragged': False, 'power-wrapped-clips': True}.items():
    CASES[_id] = ('sconf_noise_power', lambda lib, _id=_id, _w=_w: power_case(lib, _id, _w))
for _id, _v in {'gaussian-ragged-vec': True, 'gaussian-ragged-first-sample-2^34+3': False}.items():
    CASES[_id] = ('sconf_noise_add_gaussian', lambda lib, _id=_id, _v=_v: gaussian_case(lib, _id, _v))
for _id, _a in {'background-shared-clip-vec': (True, True), 'background-per-row-clips': (False, False)}.items():
    CASES[_id] = ('sconf_noise_add_background', lambda lib, _id=_id, _a=_a: background_case(lib, _id, *_a))


def build(id, lib):
    return CASES[id][1](lib)
