"""Write-footprint cases of the hotword beam search's ABI unit (include/sconf_hot.h), laid out with tests/footprint.py: the table that
tests/test_hot_footprint.py checks on the CPU and tests/test_hot_footprint_gpu.py runs on the device.  TEST INFRASTRUCTURE.

CASES maps a case id to (entry point, builder); builder(lib) needs the library only for the host-side queries.  All seven outputs are
OUT regions (every element written, from the inputs alone), the workspace is SCRATCH at exactly the queried size, the two images and
the log-probs are IN (read-only regions: a write into an image trips its guards or its content check).  One case per workgroup size
of the search kernel (sconf_hot_beam_threads: 64, 128, 256, 512, 1024), with and without an LM (a NULL LM image); the ragged case
holds a sample that ends before N, an empty one (T = 0: one empty hypothesis) and hypotheses longer than Lmax."""
import numpy as np
import torch

import beam_refs as BR
import footprint as FP
import hot_refs as HR
import lm_footprint_cases as LC
from footprint import IN, OUT, SCRATCH

NO_LAUNCH = {'sconf_hot_max_len', 'sconf_hot_max_width', 'sconf_hot_max_tokens', 'sconf_hot_beam_threads', 'sconf_hot_beam_workspace'}
CASES = {}
TOKEN_MIN_LOGP, BEAM_PRUNE_LOGP, ALPHA, BETA, WEIGHT = -5.0, -10.0, 0.5, 1.5, 3.0
_hots = {}


def hot_of(V, labels):
    """(HotwordSet, BruteHot) over V tokens: the structured set of hot_refs.phrase_set (phrases of up to 9 tokens) plus two- and
    three-token stretches of the planted labels, so that phrases do end and do break off in the search."""
    key = (V, tuple(map(tuple, labels)))
    if key not in _hots:
        phrases, weights = HR.phrase_set(np.random.default_rng(V), V, 9)
        for lab in labels:
            for k in range(0, max(len(lab) - 3, 0), 5):
                phrases.append(tuple(lab[k:k + 2 + k % 2]))
                weights.append(0.5 + 0.25 * (k % 3))
        _hots[key] = HR.hot_pair(phrases, weights)
    return _hots[key]


def hot_case(lib, id, B, N, C, W, nbest, Kmax, Lmax, in_len, with_lm):
    blank = C - 1
    lp, labels = BR.spiky_case(11, B, N, C, blank, every=3, in_len=in_len)
    img, ref = LC.lm_of(C - 1) if with_lm else (None, None)
    hot, brute = hot_of(C - 1, labels)
    a = FP.Arena()
    r_lp = a.take('log_probs', (B, N, C), torch.float32, IN, init=lp)
    r_il = a.take('input_lengths', B, torch.int32, IN, init=torch.tensor(in_len, dtype=torch.int32)) if in_len is not None else None
    r_im = a.take('lm_image', img.image.size, torch.int32, IN, init=torch.from_numpy(img.image.copy())) if with_lm else None
    r_hi = a.take('hot_image', hot.image.size, torch.int32, IN, init=torch.from_numpy(hot.image.copy()))
    r_count = a.take('count', B, torch.int32, OUT)
    r_tok = a.take('tokens', (B, nbest, Lmax), torch.int32, OUT)
    r_len = a.take('lengths', (B, nbest), torch.int32, OUT)
    r_fr = a.take('token_frames', (B, nbest, Lmax), torch.int32, OUT)
    r_sc = a.take('scores', (B, nbest), torch.float64, OUT, tol=1e-12)
    r_lg = a.take('logit_scores', (B, nbest), torch.float64, OUT, tol=1e-12)
    r_ht = a.take('hot_scores', (B, nbest), torch.float64, OUT, tol=1e-12)
    nbytes = int(lib.sconf_hot_beam_workspace(B, N, W, Kmax))
    assert nbytes > 0
    r_ws = a.take('workspace', nbytes, torch.uint8, SCRATCH)

    def restate(v):
        return HR.ctc_beam_hot(v['log_probs'], v.get('input_lengths'), ref, brute, WEIGHT, blank, W, nbest, TOKEN_MIN_LOGP, BEAM_PRUNE_LOGP,
                               Kmax, Lmax, ALPHA, BETA)._asdict()

    lm_sizes = [img.n_states, img.n_entries, img.num_tokens, img.order, img.start_state] if with_lm else [0, 0, 0, 0, 0]
    args = [r_lp, r_il, r_im, *lm_sizes, r_hi, hot.n_states, hot.n_entries, hot.max_len, WEIGHT, r_count, r_tok, r_len, r_fr, r_sc, r_lg, r_ht,
            r_ws, nbytes, B, N, C, blank, W, nbest, TOKEN_MIN_LOGP, BEAM_PRUNE_LOGP, Kmax, Lmax, ALPHA, BETA]
    return FP.Case(id, 'sconf_hot_beam_ctc', a, args, 'hot_refs.ctc_beam_hot', restate, variant=f'{lib.sconf_hot_beam_threads(W, Kmax)} threads')


#                                      B   N   C   W  nbest Kmax Lmax in_len    LM
for _id, _a in {'hot-ragged-64-threads': (3, 40, 32, 8, 3, 3, 6, [40, 23, 0], True),
                'hot-null-lengths-no-lm-128-threads': (2, 35, 32, 8, 8, 16, 35, None, False),
                'hot-256-threads': (1, 48, 32, 16, 2, 16, 48, [47], True),
                'hot-no-lm-512-threads': (1, 48, 8, 32, 1, 16, 20, [48], False),
                'hot-1024-threads': (2, 50, 32, 128, 4, 16, 50, [50, 31], True)}.items():
    CASES[_id] = ('sconf_hot_beam_ctc', lambda lib, _id=_id, _a=_a: hot_case(lib, _id, *_a))


def build(id, lib):
    return CASES[id][1](lib)
