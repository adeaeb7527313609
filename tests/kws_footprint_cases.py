"""Write-footprint cases of the keyword-search unit (include/sconf_kws.h), laid out with tests/footprint.py: the table that
tests/test_kws_footprint.py checks on the CPU and tests/test_kws_footprint_gpu.py runs on the device.  TEST INFRASTRUCTURE.

CASES maps a case id to (entry point, builder); builder(lib) needs the library only for the host-side queries.  The three outputs
are OUT regions at tol = 0 (every element written from the inputs alone, and equal to the restatement: the contract is bit-exact),
the workspace is SCRATCH at exactly the queried size, the log-scores, the lengths and the image are IN.  The columns behind
`classes` hold NaN: a kernel that reads them poisons every row.  The cases cross the gather's three row geometries (16 lanes, a
wave, a workgroup per row), rows of C = classes and C = classes + 15 (no 16-byte loads), U = 1, 4 and 5 columns, one wave and
several, a length 0, and a keyword that reaches its cap."""
import numpy as np
import torch

import footprint as FP
import kws_refs as KR
from footprint import IN, OUT, SCRATCH

NO_LAUNCH = {'sconf_kws_max_labels', 'sconf_kws_prefetch', 'sconf_kws_max_hits', 'sconf_kws_workspace'}      # return a value, launch nothing
CASES = {}


def search_case(lib, id, B, N, classes, pad, phrases, per_label, lengths, cap, seed=5):
    from lcasr_amd.decoding.kws import KeywordSet
    C, blank = classes + pad, classes - 1
    ks = KeywordSet(phrases, per_label)
    x = np.full((B, N, C), np.nan, dtype=np.float32)
    x[..., :classes] = KR.random_case(seed, B, N, classes)
    a = FP.Arena()
    r_x = a.take('x', (B, N, C), torch.float32, IN, init=torch.from_numpy(x))
    r_il = a.take('input_lengths', B, torch.int32, IN, init=torch.tensor(lengths, dtype=torch.int32)) if lengths is not None else None
    r_im = a.take('image', ks.image.size, torch.int32, IN, init=torch.from_numpy(ks.image.copy()))
    r_f = a.take('hit_frames', (B, ks.K, cap, 2), torch.int32, OUT, tol=0.0)
    r_s = a.take('hit_score', (B, ks.K, cap), torch.float32, OUT, tol=0.0)
    r_c = a.take('hit_count', (B, ks.K), torch.int32, OUT, tol=0.0)
    nbytes = int(lib.sconf_kws_workspace(B, N, ks.U))
    assert nbytes > 0
    r_ws = a.take('workspace', nbytes, torch.uint8, SCRATCH)

    def restate(v):
        il = v['input_lengths'].numpy() if 'input_lengths' in v else None
        f, s, c = KR.search32(v['x'].numpy(), ks.phrases, ks.thresholds, blank, il, cap, classes)
        return {'hit_frames': torch.from_numpy(f), 'hit_score': torch.from_numpy(s), 'hit_count': torch.from_numpy(c)}

    args = [r_x, r_il, r_im, ks.n_waves, ks.U, ks.K, r_f, r_s, r_c, cap, r_ws, nbytes, B, N, C, classes, blank]
    return FP.Case(id, 'sconf_kws_search', a, args, 'kws_refs.search32', restate, variant=f'classes{classes}/{C} U{ks.U} waves{ks.n_waves} cap{cap}')


def _phrases(seed, K, labels, hi):
    return KR.random_phrases(seed, K, labels, 1, hi)


for _id, _a in {
        'search-8-classes-ragged-length-0': (3, 21, 8, 0, [(0, 1), (2,), (3, 3), (1, 0, 2)], -4.0, [21, 0, 13], 3),
        'search-129-of-144-null-lengths': (2, 19, 129, 15, _phrases(1, 40, list(range(0, 128, 3)), 5), -6.0, None, 4),
        'search-one-column': (1, 30, 8, 15, [(2,), (2,)], -3.0, [29], 2),
        'search-four-columns-cap-reached': (1, 40, 8, 0, [(0, 1), (2,), (1, 2, 0)], -6.0, None, 2),
        'search-257-classes-a-wave-per-row': (1, 12, 257, 3, _phrases(2, 12, list(range(0, 256, 5)), 4), -8.0, None, 4),
        'search-1025-classes-a-workgroup-per-row': (2, 9, 1025, 0, _phrases(3, 12, list(range(0, 1024, 9)), 4), -9.0, [9, 4], 4)}.items():
    CASES[_id] = ('sconf_kws_search', lambda lib, _id=_id, _a=_a: search_case(lib, _id, *_a))


def build(id, lib):
    return CASES[id][1](lib)
