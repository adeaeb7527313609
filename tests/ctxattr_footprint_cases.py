"""Write-footprint cases of context attribution (include/sconf_ctxattr.h), laid out with tests/footprint.py: the table that
tests/test_ctxattr_footprint.py checks on the CPU and tests/test_ctxattr_gpu.py runs on the device.  TEST INFRASTRUCTURE.

CASES maps a case id to (entry point, builder); builder(lib) needs the library only for the host-side queries.  Every output is an
OUT region (every element written, from the inputs alone); the workspace of sconf_ctxattr_score is SCRATCH at exactly the queried
size: the harness fills it with 0xFF bytes in one run and random bytes in the other, so a boundary row or a padded reference id that
a workgroup reads before it was written changes an error count between the runs.  frame_windows is the unit's one HOST array: a
ctypes array in the argument list.  The restatement is tests/ctxattr_refs.py."""
import ctypes

import numpy as np
import torch

import ctxattr_refs as CR
import footprint as FP
from footprint import IN, OUT, SCRATCH

NO_LAUNCH = {'sconf_ctxattr_max_ref', 'sconf_ctxattr_max_window_frames', 'sconf_ctxattr_threads', 'sconf_ctxattr_cells_per_thread',
             'sconf_ctxattr_score_workspace'}                                    # return a value, launch nothing
CASES = {}


def _spec_case(seed, F, T, windows):
    g = torch.Generator().manual_seed(seed)
    spec = torch.randn(F, T, generator=g) * 3 + 1
    a = FP.Arena()
    return a, a.take('spec', (F, T), torch.float32, IN, init=spec), a.take('windows', (len(windows), 2), torch.int32, IN,
                                                                            init=torch.tensor(windows, dtype=torch.int32))


def means_case(lib, id, F, T, windows):
    a, r_spec, r_win = _spec_case(3, F, T, windows)
    J = len(windows)
    r_means = a.take('means', J, torch.float32, OUT)
    return FP.Case(id, 'sconf_ctxattr_window_means', a, [r_spec, r_win, r_means, F, T, J], 'ctxattr_refs.window_means',
                   lambda v: {'means': CR.window_means(v['spec'], v['windows'])}, variant=f'{J} workgroups')


def fill_case(lib, id, F, T, windows, j0, b):
    a, r_spec, r_win = _spec_case(5, F, T, windows)
    J = len(windows)
    r_means = a.take('means', J, torch.float32, IN, init=torch.arange(J, dtype=torch.float32) - 100)
    r_dst = a.take('dst', (b, F, T), torch.float32, OUT)
    return FP.Case(id, 'sconf_ctxattr_mask_fill', a, [r_spec, r_win, r_means, r_dst, F, T, J, j0, b], 'ctxattr_refs.mask_fill',
                   lambda v: {'dst': CR.mask_fill(v['spec'], v['windows'], v['means'], j0, b)}, variant='x4' if T % 4 == 0 else 'x1')


def score_case(lib, id, N, J, R, frame_windows, alphabet, with_tokens):
    rng = np.random.default_rng(R + N)
    blank = alphabet
    clean, masked = CR.random_labels(rng, J, N, alphabet, blank)
    ref = rng.integers(0, alphabet, R).astype(np.int32)
    I = len(frame_windows)
    cap = max(1, max(min(g + 1, N) - f for f, g in frame_windows))
    a = FP.Arena()
    r_clean = a.take('clean', N, torch.int32, IN, init=torch.from_numpy(clean))
    r_masked = a.take('masked', (J, N), torch.int32, IN, init=torch.from_numpy(masked))
    r_ref = a.take('ref', R, torch.int32, IN, init=torch.from_numpy(ref)) if R else None
    r_err = a.take('errors', (I, J), torch.int32, OUT)
    r_ce = a.take('clean_errors', 1, torch.int32, OUT)
    r_cl = a.take('clean_len', 1, torch.int32, OUT)
    r_ml = a.take('mid_len', (I, J), torch.int32, OUT)
    r_mt = a.take('mid_tokens', (I, J, cap), torch.int32, OUT) if with_tokens else None
    nbytes = int(lib.sconf_ctxattr_score_workspace(N, I, J, R))
    assert nbytes > 0
    r_ws = a.take('workspace', nbytes, torch.uint8, SCRATCH)
    fw = (ctypes.c_int32 * (2 * I))(*[v for pair in frame_windows for v in pair])

    def restate(v):
        out = CR.score(v['clean'], v['masked'], v.get('ref', torch.zeros(0, dtype=torch.int32)), frame_windows, blank, with_tokens)
        return {k: t for k, t in out._asdict().items() if t is not None}

    args = [r_clean, r_masked, r_ref, fw, r_err, r_ce, r_cl, r_ml, r_mt, r_ws, nbytes, N, I, J, R, cap, blank]
    return FP.Case(id, 'sconf_ctxattr_score', a, args, 'ctxattr_refs.score', restate,
                   variant=f'{lib.sconf_ctxattr_threads(R)}x{lib.sconf_ctxattr_cells_per_thread(R)}')


# (F, T, windows): one frame, the whole spectrogram, empty, T not a multiple of the window
CASES['means-ragged-windows'] = ('sconf_ctxattr_window_means',
                                 lambda lib: means_case(lib, 'means-ragged-windows', 5, 203, [(0, 96), (96, 192), (192, 203), (7, 8), (0, 203), (50, 50)]))
# (F, T, windows, j0, b)
for _id, _a in {'fill-x4-batch-3': (6, 200, [(0, 96), (96, 192), (192, 200), (3, 5)], 1, 3),
                'fill-x1-odd-T': (3, 203, [(0, 96), (96, 192), (192, 203)], 2, 1)}.items():
    CASES[_id] = ('sconf_ctxattr_mask_fill', lambda lib, _id=_id, _a=_a: fill_case(lib, _id, *_a))
# (N, J, R, frame windows, alphabet, mid_tokens given): every workgroup size of the pair kernel, 2 cells per thread, an empty window
for _id, _a in {'score-64-threads': (60, 3, 40, [(0, 20), (20, 41), (41, 60)], 3, True),
                'score-128-empty-window': (90, 2, 100, [(0, 30), (30, 30), (30, 90), (90, 90)], 2, False),
                'score-256-unordered-overlapping': (120, 3, 200, [(60, 120), (0, 70), (10, 20)], 3, True),
                'score-512': (80, 2, 400, [(0, 40), (40, 80)], 2, False),
                'score-1024': (150, 2, 1000, [(0, 50), (50, 100), (100, 150)], 3, True),
                'score-1024x2': (100, 2, 1500, [(0, 50), (50, 100)], 2, False),
                'score-no-reference': (40, 2, 0, [(0, 20), (20, 40)], 2, True)}.items():
    CASES[_id] = ('sconf_ctxattr_score', lambda lib, _id=_id, _a=_a: score_case(lib, _id, *_a))


def build(id, lib):
    return CASES[id][1](lib)
