"""Write-footprint cases of the calibration unit (include/sconf_calib.h), laid out with tests/footprint.py: the table that
tests/test_calib_footprint.py checks on the CPU and tests/test_calib_footprint_gpu.py runs on the device.  TEST INFRASTRUCTURE.

CASES maps a case id to (entry point, builder); builder(lib) needs the library only for the host-side queries.  Every output is an OUT
region at tol = 0: the maps, the counts and the sweep's idx are integers, equal to the restatement to the bit; for the sweep's conf a
case hands the harness the count of elements outside the confidence unit's own rule on the scaled input (calib_refs.sweep_tolerance
of the float64 restatement), which must be 0, as tests/confid_footprint_cases.py does.  No case produces a NaN (the harness reads a
NaN in an output as an element left unwritten): invalid rows and temperatures are in tests/test_calib_gpu.py.
The alignment's workspace is SCRATCH at exactly ws_off[P] bytes, its offsets and the ids are IN.  The columns behind `classes`
hold NaN: a kernel that reads them poisons every row."""
import numpy as np
import torch

import calib_refs as AR
import confid_refs as CR
import footprint as FP
from footprint import IN, OUT, SCRATCH

NO_LAUNCH = {'sconf_edit_align_strip_cols', 'sconf_edit_align_pass_cols', 'sconf_edit_align_block_rows', 'sconf_edit_align_cells_per_word',
             'sconf_edit_align_tile_bytes', 'sconf_edit_align_max_len', 'sconf_edit_align_pair_bytes', 'sconf_calib_max_temps'}      # return a value, launch nothing
CASES = {}


def align_case(lib, id, kind, sizes, short=(), seed=3):
    pairs = [AR.pair_case(kind, H, R, seed + n) for n, (H, R) in enumerate(sizes)]
    hyp = np.concatenate([p[0] for p in pairs] + [np.zeros(0, np.int32)]).astype(np.int32)
    ref = np.concatenate([p[1] for p in pairs] + [np.zeros(0, np.int32)]).astype(np.int32)
    ho = np.cumsum([0] + [s[0] for s in sizes]).astype(np.int64)
    ro = np.cumsum([0] + [s[1] for s in sizes]).astype(np.int64)
    need = [int(lib.sconf_edit_align_pair_bytes(H, R)) for H, R in sizes]
    assert need == [AR.pair_bytes(H, R) for H, R in sizes]
    wo = np.cumsum([0] + [n - (16 if p in short else 0) for p, n in enumerate(need)]).astype(np.int64)
    P = len(sizes)
    a = FP.Arena()
    r_h = a.take('hyp', len(hyp), torch.int32, IN, init=torch.from_numpy(hyp))
    r_ho = a.take('hyp_off', P + 1, torch.int64, IN, init=torch.from_numpy(ho))
    r_r = a.take('ref', len(ref), torch.int32, IN, init=torch.from_numpy(ref))
    r_ro = a.take('ref_off', P + 1, torch.int64, IN, init=torch.from_numpy(ro))
    r_wo = a.take('ws_off', P + 1, torch.int64, IN, init=torch.from_numpy(wo))
    r_h2r = a.take('hyp_to_ref', len(hyp), torch.int32, OUT, tol=0.0)
    r_r2h = a.take('ref_to_hyp', len(ref), torch.int32, OUT, tol=0.0)
    r_c = a.take('counts', (P, 4), torch.int64, OUT, tol=0.0)
    r_ws = a.take('workspace', int(wo[-1]), torch.uint8, SCRATCH)

    def restate(v):
        h2r, r2h, counts = AR.align_batch(v['hyp'].numpy(), v['hyp_off'].tolist(), v['ref'].numpy(), v['ref_off'].tolist(), v['ws_off'].tolist())
        return {'hyp_to_ref': torch.from_numpy(h2r), 'ref_to_hyp': torch.from_numpy(r2h), 'counts': torch.from_numpy(counts)}

    return FP.Case(id, 'sconf_edit_align', a, [r_h, r_ho, r_r, r_ro, P, r_h2r, r_r2h, r_c, r_ws, r_wo], 'calib_refs.align_batch', restate,
                   variant=f'{kind} P{P} ws{int(wo[-1])}')


def _outside(y, bd):
    """(expected, fn) of footprint.Case: the count of elements of the region outside |got - y| <= bd, against 0."""
    return torch.zeros(1, dtype=torch.float64), lambda out: ((out.double().cpu().reshape(y.shape) - y).abs() > bd).sum().double().reshape(1)


def sweep_case(lib, id, M, classes, pad, method, norm, alpha, inv_temps, seed=5):
    C = classes + pad
    x = np.full((M, C), np.nan, dtype=np.float32)
    x[:, :classes] = np.random.default_rng(seed).normal(size=(M, classes)).astype(np.float32) * 3
    x[1, 2:classes:3] = -np.inf
    K = len(inv_temps)
    a = FP.Arena()
    r_x = a.take('x', (M, C), torch.float32, IN, init=torch.from_numpy(x))
    r_it = a.take('inv_temps', K, torch.float32, IN, init=torch.tensor(inv_temps, dtype=torch.float32))
    r_i = a.take('idx', M, torch.int32, OUT, tol=0.0)
    r_c = a.take('conf', (K, M), torch.float32, OUT, tol=0.0)

    def restate(v):
        xs, its = v['x'].numpy(), v['inv_temps'].tolist()
        idx, conf = AR.sweep(xs, its, classes, method, norm, alpha)
        bd = torch.tensor([AR.sweep_tolerance(xs, it, classes, method, norm, alpha)[0] for it in its], dtype=torch.float64)[:, None]
        return {'idx': torch.from_numpy(idx), 'conf': _outside(torch.from_numpy(conf), bd)}

    args = [r_x, M, classes, C, CR.METHODS.index(method), CR.NORMS.index(norm), float(alpha), r_it, K, r_i, r_c]
    return FP.Case(id, 'sconf_calib_frames_sweep', a, args, 'calib_refs.sweep', restate, variant=f'{method}/{norm} classes{classes}/{C} K{K}')


for _id, _a in {
        'align-ragged-batch-with-empty-sides': ('edits', [(40, 50), (0, 7), (9, 0), (0, 0), (33, 20)]),
        'align-two-symbols-past-a-tile': ('two', [(AR.ROWS + 1, AR.STRIP + 1), (7, 9)]),
        'align-past-a-pass': ('edits', [(17, AR.PASS + 1), (AR.CPL + 1, 2 * AR.CPL - 1)]),
        'align-one-slice-too-small': ('edits', [(12, 30), (AR.ROWS + 5, 40), (25, 25)], (1,))}.items():
    CASES[_id] = ('sconf_edit_align', lambda lib, _id=_id, _a=_a: align_case(lib, _id, *_a))

for _id, _a in {
        'sweep-8-classes-one-temperature': (9, 8, 0, 'tsallis', 'exp', 1 / 3, [1.0]),
        'sweep-129-of-144-three-temperatures': (11, 129, 15, 'shannon', 'lin', 1 / 3, [0.5, 1.0, 1.7]),
        'sweep-257-classes-a-wave-per-row': (6, 257, 3, 'renyi', 'exp', 0.5, [2.0, 1.0]),
        'sweep-1025-classes-a-workgroup-per-row': (5, 1025, 0, 'max_prob', 'lin', 1 / 3, [1.0] + [0.4 + 0.17 * k for k in range(15)]),
        'sweep-4097-classes-out-of-the-cache': (3, 4097, 15, 'tsallis', 'lin', 2.0, [0.8, 1.0, 1.25])}.items():
    CASES[_id] = ('sconf_calib_frames_sweep', lambda lib, _id=_id, _a=_a: sweep_case(lib, _id, *_a))


def build(id, lib):
    return CASES[id][1](lib)
