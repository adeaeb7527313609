"""Write-footprint cases of the segmentation unit (include/sconf_seg.h), laid out with tests/footprint.py: the table that
tests/test_seg_footprint.py checks on the CPU and tests/test_seg_footprint_gpu.py runs on the device.  TEST INFRASTRUCTURE.

CASES maps a case id to (entry point, builder); builder(lib) needs the library only for the host-side queries.  sconf_seg_align: all
six outputs are OUT regions (every element written, from the inputs alone), the workspace is SCRATCH at exactly the queried size;
the ragged case holds a sample that ends before N, one with fewer labels than Smax and an infeasible one, and every row holds stars.
The long form (more than 8191 labels) has no case here: its workspace alone is 400 MB at the smallest such size; the routing test of
tests/test_seg_gpu.py runs it.  sconf_seg_score: the three outputs are OUT regions and there is no workspace.  No score case
produces a NaN (the harness reads a NaN in an output as an element left unwritten); invalid utterances are in tests/test_seg_gpu.py.
A score case hands the harness the count of elements outside seg_refs.score_bound of the float64 restatement, which must be 0."""
import numpy as np
import torch

import align_refs as AR
import footprint as FP
import seg_refs as SR
from footprint import IN, OUT, SCRATCH

NO_LAUNCH = {'sconf_seg_star_label', 'sconf_seg_max_window', 'sconf_seg_score_tile', 'sconf_seg_workspace'}      # return a value, launch nothing
CASES = {}


def star_targets(tg, tg_len, C, every=4):
    """`tg` with the star C at the first and last label of every row (within its length) and at every `every`-th in between
    (where the two meet, two adjacent stars: a repeat)."""
    tg = tg.clone()
    for b in range(tg.shape[0]):
        S = tg.shape[1] if tg_len is None else max(min(int(tg_len[b]), tg.shape[1]), 0)
        if S:
            tg[b, 0:S:every] = C
            tg[b, S - 1] = C
    return tg


def align_case(lib, id, B, N, C, Smax, in_len, tg_len, star_logp):
    blank = C - 1
    lp, tg = AR.random_case(7, B, N, C, Smax, in_len, tg_len)
    tg = star_targets(tg, tg_len, C)
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
    r_g = a.take('frame_logp', (B, N), torch.float32, OUT)
    nbytes = int(lib.sconf_seg_workspace(B, N, Smax, 0))
    assert nbytes > 0
    r_ws = a.take('workspace', nbytes, torch.uint8, SCRATCH)
    dtype = AR.state_dtype(lib.sconf_align_state_bytes(Smax))

    def restate(v):
        out = SR.align(v['log_probs'], v['targets'], v.get('input_lengths'), v.get('target_lengths'), blank, star_logp, dtype=dtype)
        return {k: t for k, t in out._asdict().items() if t.numel()}       # (Smax = 0: spans and token_logp have no element)

    args = [r_lp, r_tg, r_il, r_tl, r_path, r_lab, r_sp, r_logp, r_score, r_g, r_ws, nbytes, B, N, C, Smax, blank, float(star_logp)]
    return FP.Case(id, 'sconf_seg_align', a, args, 'seg_refs.align', restate,
                   variant=f'{lib.sconf_align_threads(Smax)}x{lib.sconf_align_states_per_thread(Smax)} star_logp {star_logp}')


def _outside(y):
    """(expected, fn) of footprint.Case: the count of elements of the region outside seg_refs.score_bound of y, against 0."""
    return torch.zeros(1, dtype=torch.float64), lambda out: ((out.double().cpu().reshape(y.shape) - y.double()).abs() > SR.score_bound(y)).sum().double().reshape(1)


def score_case(lib, id, window, with_lengths):
    tile = lib.sconf_seg_score_tile()
    B, N, Smax, Umax = 2, max(2 * tile, window) + 45, 12, 5               # (the utterance of every frame holds a whole window)
    rng = np.random.default_rng(13)
    g = torch.from_numpy(-rng.exponential(2.0, size=(B, N)).astype(np.float32))
    lens, tls = [N, N - 9], [Smax, Smax - 2]
    spans = torch.full((B, Smax, 2), -1, dtype=torch.int32)
    for b in range(B):                                                      # token j holds [cut[j], cut[j + 1]): no blanks, every frame a token's
        cut = np.concatenate([[0, 1, tile - 3, tile, tile + 1], np.sort(rng.choice(np.arange(tile + 2, lens[b]), size=tls[b] - 5, replace=False)), [lens[b]]])
        spans[b, :tls[b]] = torch.from_numpy(np.stack([cut[:-1], cut[1:]], -1).astype(np.int32))
    # the rounds of an utterance start at its own first frame.  Sample 0: one frame; exactly one tile; one frame more; every frame of
    # the sample; the last tokens.  Sample 1: one frame; one frame less than a tile; a few frames across the cut; every frame.
    utt = torch.tensor([[[0, 1], [0, 3], [0, 4], [0, tls[0]], [7, tls[0]]], [[0, 1], [1, 3], [2, 5], [0, tls[1]], [0, 0]]], dtype=torch.int32)
    counts = [5, 4]
    score = torch.tensor([-12.5, -3.0], dtype=torch.float64)
    a = FP.Arena()
    r_sp = a.take('spans', (B, Smax, 2), torch.int32, IN, init=spans)
    r_g = a.take('frame_logp', (B, N), torch.float32, IN, init=g)
    r_sc = a.take('score', B, torch.float64, IN, init=score)
    r_il = a.take('input_lengths', B, torch.int32, IN, init=torch.tensor(lens, dtype=torch.int32)) if with_lengths else None
    r_tl = a.take('target_lengths', B, torch.int32, IN, init=torch.tensor(tls, dtype=torch.int32))
    r_utt = a.take('utt', (B, Umax, 2), torch.int32, IN, init=utt)
    r_uc = a.take('utt_counts', B, torch.int32, IN, init=torch.tensor(counts, dtype=torch.int32))
    r_uf = a.take('utt_frames', (B, Umax, 2), torch.int32, OUT, tol=0.0)
    r_ul = a.take('utt_logp', (B, Umax), torch.float32, OUT, tol=0.0)
    r_cf = a.take('utt_conf', (B, Umax), torch.float32, OUT, tol=0.0)

    def restate(v):
        out = SR.score(v['spans'], v['frame_logp'], v['score'], v.get('input_lengths'), v['target_lengths'], v['utt'], v['utt_counts'], window)
        assert not bool(torch.isnan(out.utt_logp).any())
        return {'utt_frames': out.utt_frames, 'utt_logp': _outside(out.utt_logp), 'utt_conf': _outside(out.utt_conf)}

    args = [r_sp, r_g, r_sc, r_il, r_tl, r_utt, r_uc, int(window), r_uf, r_ul, r_cf, B, N, Smax, Umax]
    return FP.Case(id, 'sconf_seg_score', a, args, 'seg_refs.score', restate, variant=f'tile{tile} N{N} window{window}')


for _id, _a in {'align-star-ragged-infeasible': (3, 50, 32, 12, [50, 37, 9], [12, 7, 12], 0.0),
                'align-star-null-lengths': (2, 45, 32, 9, None, None, -1.0),
                'align-star-512-threads': (2, 230, 32, 200, [230, 221], [200, 150], -1.0),
                'align-star-2-states-per-thread': (1, 560, 8, 530, [556], [530], 0.0),
                'align-star-no-labels': (2, 19, 4, 0, [19, 5], None, 0.0)}.items():
    CASES[_id] = ('sconf_seg_align', lambda lib, _id=_id, _a=_a: align_case(lib, _id, *_a))
for _id, _a in {'score-window-30': (30, True), 'score-window-1-null-input-lengths': (1, False), 'score-largest-window': (None, True)}.items():
    CASES[_id] = ('sconf_seg_score', lambda lib, _id=_id, _a=_a: score_case(lib, _id, _a[0] or lib.sconf_seg_max_window(), _a[1]))


def build(id, lib):
    return CASES[id][1](lib)
