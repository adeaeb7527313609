"""Write-footprint cases of the beam-search ABI unit (include/sconf_beam.h), laid out with tests/footprint.py: the table that
tests/test_beam_footprint.py checks on the CPU and tests/test_beam_gpu.py runs on the device.  TEST INFRASTRUCTURE.

CASES maps a case id to (entry point, builder); builder(lib) needs the library only for the host-side queries.  All five outputs are
OUT regions (every element written, from the inputs alone), the workspace is SCRATCH at exactly the queried size.  One case per
workgroup size of the search kernel (sconf_beam_threads: 64, 128, 256, 512, 1024); the ragged case holds a sample that ends before
N, an empty one (T = 0: one empty hypothesis) and hypotheses longer than Lmax."""
import torch

import beam_refs as BR
import footprint as FP
from footprint import IN, OUT, SCRATCH

NO_LAUNCH = {'sconf_beam_max_width', 'sconf_beam_max_tokens', 'sconf_beam_threads', 'sconf_beam_rank_limit', 'sconf_beam_sort_size', 'sconf_beam_prefetch_frames',
             'sconf_beam_workspace'}                                          # return a value, launch nothing
CASES = {}
TOKEN_MIN_LOGP, BEAM_PRUNE_LOGP = -5.0, -10.0


def beam_case(lib, id, B, N, C, W, nbest, Kmax, Lmax, in_len):
    blank = C - 1
    lp, _ = BR.spiky_case(11, B, N, C, blank, every=3, in_len=in_len)
    a = FP.Arena()
    r_lp = a.take('log_probs', (B, N, C), torch.float32, IN, init=lp)
    r_il = a.take('input_lengths', B, torch.int32, IN, init=torch.tensor(in_len, dtype=torch.int32)) if in_len is not None else None
    r_count = a.take('count', B, torch.int32, OUT)
    r_tok = a.take('tokens', (B, nbest, Lmax), torch.int32, OUT)
    r_len = a.take('lengths', (B, nbest), torch.int32, OUT)
    r_fr = a.take('token_frames', (B, nbest, Lmax), torch.int32, OUT)
    r_sc = a.take('scores', (B, nbest), torch.float64, OUT, tol=1e-12)
    nbytes = int(lib.sconf_beam_workspace(B, N, W, Kmax))
    assert nbytes > 0
    r_ws = a.take('workspace', nbytes, torch.uint8, SCRATCH)

    def restate(v):
        return BR.ctc_beam(v['log_probs'], v.get('input_lengths'), blank, W, nbest, TOKEN_MIN_LOGP, BEAM_PRUNE_LOGP, Kmax, Lmax)._asdict()

    args = [r_lp, r_il, r_count, r_tok, r_len, r_fr, r_sc, r_ws, nbytes, B, N, C, blank, W, nbest, TOKEN_MIN_LOGP, BEAM_PRUNE_LOGP, Kmax, Lmax]
    return FP.Case(id, 'sconf_beam_ctc', a, args, 'beam_refs.ctc_beam', restate, variant=f'{lib.sconf_beam_threads(W, Kmax)} threads')


#                                       B   N   C   W  nbest Kmax Lmax in_len
for _id, _a in {'beam-ragged-64-threads': (3, 40, 32, 8, 3, 3, 6, [40, 23, 0]),
                'beam-null-lengths-128-threads': (2, 35, 32, 8, 8, 16, 35, None),
                'beam-256-threads': (1, 48, 32, 16, 2, 16, 48, [47]),
                'beam-512-threads': (1, 48, 8, 32, 1, 16, 20, [48]),
                'beam-1024-threads': (2, 50, 32, 128, 4, 16, 50, [50, 31])}.items():
    CASES[_id] = ('sconf_beam_ctc', lambda lib, _id=_id, _a=_a: beam_case(lib, _id, *_a))


def build(id, lib):
    return CASES[id][1](lib)
