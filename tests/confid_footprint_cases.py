"""Write-footprint cases of the confidence unit (include/sconf_confid.h), laid out with tests/footprint.py: the table that
tests/test_confid_footprint.py checks on the CPU and tests/test_confid_footprint_gpu.py runs on the device.  TEST INFRASTRUCTURE.

CASES maps a case id to (entry point, builder); builder(lib) needs the library only for the host-side queries.  One case per
kernel geometry: sconf_confid_frames with 16 lanes per row and one to four quads per lane, a wave per row and two or four quads, a
workgroup per row in registers and a row above its capacity (two passes), at row strides above `classes` with NaN in the columns behind `classes` - a multiple of four elements (16-byte loads) and
not; sconf_confid_runs over more than one scan chunk with a sequence that has one label more than S_cap; sconf_confid_aggregate with
and without idx.  No case produces a NaN (the harness reads a NaN in an output as an element left unwritten); invalid rows and
refused spans are in tests/test_confid_gpu.py.  Confidences: a case hands the harness the count of elements outside
confid_refs.tolerance of the float64 restatement, which must be 0; integers are exact."""
import numpy as np
import torch

import confid_refs as CR
import footprint as FP
from footprint import IN, OUT

NO_LAUNCH = {'sconf_confid_row_capacity', 'sconf_confid_block_capacity', 'sconf_confid_scan_chunk'}          # return a value, launch nothing
CASES = {}
METHOD = {'max_prob': 0, 'shannon': 1, 'tsallis': 2, 'renyi': 3}
NORM = {'lin': 0, 'exp': 1}
AGG = {'mean': 0, 'min': 1, 'max': 2, 'prod': 3}


def _outside(y, bd):
    """(expected, fn) of footprint.Case: the count of elements of the region outside |got - y| <= bd, against 0."""
    return torch.zeros(1, dtype=torch.float64), lambda out: ((out.double().cpu().reshape(y.shape) - y).abs() > bd).sum().double().reshape(1)


def frames_case(lib, id, geometry, method, norm, alpha, pad):
    cap = lib.sconf_confid_row_capacity()
    classes = {'group16x1': 40, 'group16x2': 100, 'group16x3': 129, 'group16x4': 250, 'wave2': 257, 'wave4': cap, 'block': cap + 1,
               'stream': lib.sconf_confid_block_capacity() + 1}[geometry]
    M, stride = 6, classes + pad
    x = torch.full((M, stride), float('nan'))
    x[:, :classes] = torch.from_numpy(np.random.default_rng(classes).normal(size=(M, classes)).astype(np.float32) * 3)
    x[1, 2:classes:3] = float('-inf')
    a = FP.Arena()
    r_x = a.take('x', (M, stride), torch.float32, IN, init=x)
    r_idx = a.take('idx', M, torch.int32, OUT, tol=0.0)
    r_conf = a.take('conf', M, torch.float32, OUT, tol=0.0)

    def restate(v):
        xs = v['x'].numpy()
        idx, conf = CR.frames(xs, classes, method, norm, alpha)
        tol, _ = CR.tolerance(xs, classes, method, norm, alpha)
        return {'idx': torch.from_numpy(idx), 'conf': _outside(torch.from_numpy(conf), tol)}

    args = [r_x, M, classes, stride, METHOD[method], NORM[norm], float(alpha), r_idx, r_conf]
    return FP.Case(id, 'sconf_confid_frames', a, args, 'confid_refs.frames', restate,
                   variant=f'{geometry} classes{classes} stride{stride} {"vec" if stride % 4 == 0 else "scalar"} {method}/{norm}')


def runs_case(lib, id):
    chunk = lib.sconf_confid_scan_chunk()
    B, N, blank = 3, chunk + 37, 0
    rng = np.random.default_rng(7)
    idx = rng.integers(0, 3, size=(B, N)).astype(np.int32)
    idx[0, chunk - 3:chunk + 2] = 5                                        # a run across the chunk boundary
    idx[0, 20] = -1
    idx[1, :] = np.tile([1, 2], N)[:N]                                     # a label per frame: more than S_cap
    lens = [N, N - 5, 9]
    counts = CR.runs(idx, lens, blank)[2].tolist()
    s_cap = counts[0] + 3
    assert counts[1] == N - 5 > s_cap > counts[0] > counts[2] > 0
    a = FP.Arena()
    r_idx = a.take('idx', (B, N), torch.int32, IN, init=torch.from_numpy(idx))
    r_len = a.take('lengths', B, torch.int32, IN, init=torch.tensor(lens, dtype=torch.int32))
    r_tg = a.take('targets', (B, s_cap), torch.int32, OUT, tol=0.0)
    r_sp = a.take('spans', (B, s_cap, 3), torch.int32, OUT, tol=0.0)
    r_tl = a.take('target_lengths', B, torch.int32, OUT, tol=0.0)

    def restate(v):
        tg, sp, tl = CR.runs(v['idx'].numpy(), v['lengths'].tolist(), blank, s_cap)
        return {'targets': torch.from_numpy(tg), 'spans': torch.from_numpy(sp), 'target_lengths': torch.from_numpy(tl)}

    args = [r_idx, r_len, B, N, blank, r_tg, r_sp, r_tl, s_cap]
    return FP.Case(id, 'sconf_confid_runs', a, args, 'confid_refs.runs', restate, variant=f'chunk{chunk} N{N} S_cap{s_cap} overflow')


def aggregate_case(lib, id, agg, with_idx):
    M, blank = 1500, 1
    rng = np.random.default_rng(11)
    values = torch.from_numpy(rng.uniform(0.05, 1.0, size=M).astype(np.float32))
    idx = torch.from_numpy(rng.integers(0, 3, size=M).astype(np.int32))
    idx[400:420] = blank; idx[3] = -1
    spans = torch.tensor([[0, 1], [3, 4], [10, 73], [10, 74], [10, 75], [100, 1100], [50, 90], [400, 420], [1499, 1500], [0, 1500]], dtype=torch.int32)
    a = FP.Arena()
    r_v = a.take('values', M, torch.float32, IN, init=values)
    r_i = a.take('idx', M, torch.int32, IN, init=idx) if with_idx else None
    r_s = a.take('spans', tuple(spans.shape), torch.int32, IN, init=spans)
    r_o = a.take('out', spans.shape[0], torch.float32, OUT, tol=0.0)

    def restate(v):
        want = CR.aggregate(v['values'].numpy(), v['spans'].tolist(), agg, v['idx'].numpy() if with_idx else None, blank)
        n = (v['spans'][:, 1] - v['spans'][:, 0]).double()
        bound = (n + 2) * 2.0 ** -24 * 1.01 * (torch.from_numpy(want).abs() if agg == 'prod' else 1.0) + 1e-37 if agg in ('mean', 'prod') else 0.0
        return {'out': _outside(torch.from_numpy(want), bound)}

    args = [r_v, r_i, blank, M, r_s, spans.shape[0], AGG[agg], r_o]
    return FP.Case(id, 'sconf_confid_aggregate', a, args, 'confid_refs.aggregate', restate, variant=f'{agg} {"idx" if with_idx else "no idx"}')


for _id, _a in {'frames-group16x1-scalar-shannon-exp': ('group16x1', 'shannon', 'exp', 1.0, 1), 'frames-group16x2-vec-renyi-exp': ('group16x2', 'renyi', 'exp', 0.5, 4),
                'frames-group16x3-vec-tsallis-exp': ('group16x3', 'tsallis', 'exp', 1 / 3, 15), 'frames-group16x4-scalar-tsallis-lin': ('group16x4', 'tsallis', 'lin', 2.0, 3),
                'frames-wave2-scalar-shannon-lin': ('wave2', 'shannon', 'lin', 1.0, 6), 'frames-wave4-scalar-max-prob': ('wave4', 'max_prob', 'lin', 1.0, 1),
                'frames-block-vec-renyi-lin': ('block', 'renyi', 'lin', 2.0, 3), 'frames-stream-vec-tsallis-exp': ('stream', 'tsallis', 'exp', 1 / 3, 3)}.items():
    CASES[_id] = ('sconf_confid_frames', lambda lib, _id=_id, _a=_a: frames_case(lib, _id, *_a))
CASES['runs-two-chunks-overflow'] = ('sconf_confid_runs', lambda lib: runs_case(lib, 'runs-two-chunks-overflow'))
for _id, _a in {'aggregate-mean-idx': ('mean', True), 'aggregate-min': ('min', False), 'aggregate-prod-idx': ('prod', True)}.items():
    CASES[_id] = ('sconf_confid_aggregate', lambda lib, _id=_id, _a=_a: aggregate_case(lib, _id, *_a))


def build(id, lib):
    return CASES[id][1](lib)
