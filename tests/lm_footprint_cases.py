"""Write-footprint cases of the LM-fused beam search's ABI unit (include/sconf_lm.h), laid out with tests/footprint.py: the table that
tests/test_lm_footprint.py checks on the CPU and tests/test_lm_gpu.py runs on the device.  TEST INFRASTRUCTURE.

CASES maps a case id to (entry point, builder); builder(lib) needs the library only for the host-side queries.  All six outputs are
OUT regions (every element written, from the inputs alone), the workspace is SCRATCH at exactly the queried size, the image and the
log-probs are IN.  One case per workgroup size of the search kernel (sconf_lm_beam_threads: 64, 128, 256, 512, 1024); the ragged
case holds a sample that ends before N, an empty one (T = 0: one empty hypothesis) and hypotheses longer than Lmax."""
import numpy as np
import torch

import beam_refs as BR
import footprint as FP
import lm_refs as LR
from footprint import IN, OUT, SCRATCH

NO_LAUNCH = {'sconf_lm_max_order', 'sconf_lm_beam_threads', 'sconf_lm_beam_workspace'}           # return a value, launch nothing
CASES = {}
TOKEN_MIN_LOGP, BEAM_PRUNE_LOGP, ALPHA, BETA = -5.0, -10.0, 0.5, 1.5
_lms = {}


def lm_of(V, order=3):
    """(image, restatement) of a trigram trained on a seeded random stream over V tokens."""
    if (V, order) not in _lms:
        stream = np.random.default_rng(V).integers(0, V, 40 * V).tolist()
        _lms[(V, order)] = LR.lm_pair(LR.train([stream], order, V, bos=True), order, V)
    return _lms[(V, order)]


def lm_case(lib, id, B, N, C, W, nbest, Kmax, Lmax, in_len):
    blank = C - 1
    lp, _ = BR.spiky_case(11, B, N, C, blank, every=3, in_len=in_len)
    img, ref = lm_of(C - 1)
    a = FP.Arena()
    r_lp = a.take('log_probs', (B, N, C), torch.float32, IN, init=lp)
    r_il = a.take('input_lengths', B, torch.int32, IN, init=torch.tensor(in_len, dtype=torch.int32)) if in_len is not None else None
    r_im = a.take('image', img.image.size, torch.int32, IN, init=torch.from_numpy(img.image.copy()))
    r_count = a.take('count', B, torch.int32, OUT)
    r_tok = a.take('tokens', (B, nbest, Lmax), torch.int32, OUT)
    r_len = a.take('lengths', (B, nbest), torch.int32, OUT)
    r_fr = a.take('token_frames', (B, nbest, Lmax), torch.int32, OUT)
    r_sc = a.take('scores', (B, nbest), torch.float64, OUT, tol=1e-12)
    r_lg = a.take('logit_scores', (B, nbest), torch.float64, OUT, tol=1e-12)
    nbytes = int(lib.sconf_lm_beam_workspace(B, N, W, Kmax))
    assert nbytes > 0
    r_ws = a.take('workspace', nbytes, torch.uint8, SCRATCH)

    def restate(v):
        return LR.ctc_beam_lm(v['log_probs'], v.get('input_lengths'), ref, blank, W, nbest, TOKEN_MIN_LOGP, BEAM_PRUNE_LOGP, Kmax, Lmax,
                              ALPHA, BETA)._asdict()

    args = [r_lp, r_il, r_im, img.n_states, img.n_entries, img.num_tokens, img.order, img.start_state, r_count, r_tok, r_len, r_fr, r_sc,
            r_lg, r_ws, nbytes, B, N, C, blank, W, nbest, TOKEN_MIN_LOGP, BEAM_PRUNE_LOGP, Kmax, Lmax, ALPHA, BETA]
    return FP.Case(id, 'sconf_lm_beam_ctc', a, args, 'lm_refs.ctc_beam_lm', restate, variant=f'{lib.sconf_lm_beam_threads(W, Kmax)} threads')


#                                     B   N   C   W  nbest Kmax Lmax in_len
for _id, _a in {'lm-ragged-64-threads': (3, 40, 32, 8, 3, 3, 6, [40, 23, 0]),
                'lm-null-lengths-128-threads': (2, 35, 32, 8, 8, 16, 35, None),
                'lm-256-threads': (1, 48, 32, 16, 2, 16, 48, [47]),
                'lm-512-threads': (1, 48, 8, 32, 1, 16, 20, [48]),
                'lm-1024-threads': (2, 50, 32, 128, 4, 16, 50, [50, 31])}.items():
    CASES[_id] = ('sconf_lm_beam_ctc', lambda lib, _id=_id, _a=_a: lm_case(lib, _id, *_a))


def build(id, lib):
    return CASES[id][1](lib)
