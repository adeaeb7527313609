"""Write-footprint cases of the long form of forced alignment (include/sconf_align_long.h), laid out with tests/footprint.py: the
table that tests/test_align_long.py checks on the CPU and tests/test_align_long_gpu.py runs on the device.  TEST INFRASTRUCTURE.

CASES maps a case id to (entry point, builder); builder(lib) needs the library only for the host-side queries.  All five outputs are
OUT regions (every element written, from the inputs alone), the workspace is SCRATCH at exactly the queried size: the harness fills
it with 0xFF bytes in one run and random bytes in the other, so an edge cell that a slab reads before the slab below wrote it
changes the path between the runs.  The restatement is tests/align_refs.py in f64 whatever the size."""
import numpy as np
import torch

import align_refs as AR
import footprint as FP
from footprint import IN, OUT, SCRATCH

NO_LAUNCH = {'sconf_lalign_max_labels', 'sconf_lalign_default_slab_states', 'sconf_lalign_threads', 'sconf_lalign_states_per_thread',
             'sconf_lalign_slabs', 'sconf_lalign_workspace'}                     # return a value, launch nothing
CASES = {}


def lalign_case(lib, id, B, N, C, Smax, in_len, tg_len, slab_states):
    blank = C - 1
    lp, tg = AR.random_case(7, B, N, C, Smax, in_len, tg_len)
    a = FP.Arena()
    r_lp = a.take('log_probs', (B, N, C), torch.float32, IN, init=lp)
    r_tg = a.take('targets', (B, Smax), torch.int32, IN, init=tg)
    r_il = a.take('input_lengths', B, torch.int32, IN, init=torch.tensor(in_len, dtype=torch.int32)) if in_len is not None else None
    r_tl = a.take('target_lengths', B, torch.int32, IN, init=torch.tensor(tg_len, dtype=torch.int32)) if tg_len is not None else None
    r_path = a.take('path', (B, N), torch.int32, OUT)
    r_lab = a.take('labels', (B, N), torch.int32, OUT)
    r_sp = a.take('spans', (B, Smax, 2), torch.int32, OUT)
    r_logp = a.take('token_logp', (B, Smax), torch.float32, OUT)
    r_score = a.take('score', B, torch.float64, OUT)
    nbytes = int(lib.sconf_lalign_workspace(B, N, Smax, slab_states))
    assert nbytes > 0
    r_ws = a.take('workspace', nbytes, torch.uint8, SCRATCH)

    def restate(v):
        out = AR.ctc_align(v['log_probs'], v['targets'], v.get('input_lengths'), v.get('target_lengths'), blank, dtype=np.float64)
        return {k: t for k, t in out._asdict().items() if t.numel()}       # (Smax = 0: spans and token_logp have no element)

    args = [r_lp, r_tg, r_il, r_tl, r_path, r_lab, r_sp, r_logp, r_score, r_ws, nbytes, B, N, C, Smax, blank, slab_states]
    return FP.Case(id, 'sconf_lalign_ctc', a, args, 'align_refs.ctc_align', restate,
                   variant=f'{lib.sconf_lalign_slabs(Smax, slab_states)} slabs of {lib.sconf_lalign_threads(slab_states)}x'
                           f'{lib.sconf_lalign_states_per_thread(slab_states)}')


# (B, N, C, Smax, input lengths, target lengths, slab_states)
for _id, _a in {'lalign-3-slabs-ragged-infeasible': (3, 330, 32, 300, [330, 305, 9], [300, 140, 300], 256),   # 3, 2 and 3 slabs; T = 9: no path
                'lalign-one-state-last-slab': (2, 140, 8, 128, [140, 128], None, 256),                        # L - 1 = 256; T = S: ends on L - 2
                'lalign-512-null-lengths': (1, 300, 16, 260, None, None, 512),
                'lalign-2-states-per-thread': (1, 1100, 8, 1030, [1096], [1030], 2048),
                'lalign-default-slab': (2, 40, 32, 12, [40, 25], [12, 7], 0),
                'lalign-no-labels': (2, 19, 4, 0, [19, 5], None, 256)}.items():
    CASES[_id] = ('sconf_lalign_ctc', lambda lib, _id=_id, _a=_a: lalign_case(lib, _id, *_a))


def build(id, lib):
    return CASES[id][1](lib)
