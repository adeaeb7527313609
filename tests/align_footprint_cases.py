"""Write-footprint cases of the alignment ABI unit (include/sconf_align.h), laid out with tests/footprint.py: the table that
tests/test_align_footprint.py checks on the CPU and tests/test_align_gpu.py runs on the device.  TEST INFRASTRUCTURE.

CASES maps a case id to (entry point, builder); builder(lib) needs the library only for the host-side queries.  All five outputs are
OUT regions (every element written, from the inputs alone), the workspace is SCRATCH at exactly the queried size.  The ragged case
holds a sample that ends before N, one with fewer labels than Smax and an infeasible one (score -inf, everything else -1 / 0)."""
import torch

import align_refs as AR
import footprint as FP
from footprint import IN, OUT, SCRATCH

NO_LAUNCH = {'sconf_align_max_labels', 'sconf_align_state_bytes', 'sconf_align_threads', 'sconf_align_states_per_thread',
             'sconf_align_walk_window', 'sconf_align_workspace'}                  # return a value, launch nothing
CASES = {}


def align_case(lib, id, B, N, C, Smax, in_len, tg_len):
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
    nbytes = int(lib.sconf_align_workspace(B, N, Smax))
    assert nbytes > 0
    r_ws = a.take('workspace', nbytes, torch.uint8, SCRATCH)
    dtype = AR.state_dtype(lib.sconf_align_state_bytes(Smax))

    def restate(v):
        out = AR.ctc_align(v['log_probs'], v['targets'], v.get('input_lengths'), v.get('target_lengths'), blank, dtype=dtype)
        return {k: t for k, t in out._asdict().items() if t.numel()}       # (Smax = 0: spans and token_logp have no element)

    args = [r_lp, r_tg, r_il, r_tl, r_path, r_lab, r_sp, r_logp, r_score, r_ws, nbytes, B, N, C, Smax, blank]
    return FP.Case(id, 'sconf_align_ctc', a, args, 'align_refs.ctc_align', restate,
                   variant=f'{lib.sconf_align_threads(Smax)}x{lib.sconf_align_states_per_thread(Smax)}')


for _id, _a in {'align-ragged-infeasible': (3, 50, 32, 12, [50, 37, 9], [12, 7, 12]),
                'align-null-lengths': (2, 45, 32, 9, None, None),
                'align-512-threads': (2, 230, 32, 200, [230, 221], [200, 150]),
                'align-2-states-per-thread': (1, 560, 8, 530, [556], [530]),
                'align-no-labels': (2, 19, 4, 0, [19, 5], None)}.items():
    CASES[_id] = ('sconf_align_ctc', lambda lib, _id=_id, _a=_a: align_case(lib, _id, *_a))


def build(id, lib):
    return CASES[id][1](lib)
