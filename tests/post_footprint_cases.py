"""Write-footprint cases of the posterior unit (include/sconf_post.h), laid out with tests/footprint.py: the table that
tests/test_post_footprint.py checks on the CPU and tests/test_post_footprint_gpu.py runs on the device.  TEST INFRASTRUCTURE.

CASES maps a case id to (entry point, builder); builder(lib) needs the library only for the host-side queries.  The batches are
ragged, with a sample without labels and one without an alignment, so the outputs hold NaN by contract: in the slots at and past
target_lengths[b], the gaps past it, and throughout the sample whose log-likelihood is -inf.  The harness reads a NaN in an output as
an element left unwritten, so those elements are declared `unspecified` for its own two checks and every float output hands it
instead the count of elements that are NaN where the restatement is not (or the reverse), differ in being -inf, or lie outside the
header's tolerance (computed from sconf_post_step_error()), which must be 0: after the random-filled run a padded slot the kernel did
not write is not a NaN.  The integer alternatives are compared to the bit (the inputs leave no row tied).
The rows of log_probs lie row_stride apart: the columns behind C are stride gaps of the region, 0xFF (NaN) in one run and random in
the other, and so are the frames behind input_lengths[b] NaN by content: a kernel that reads either poisons its sample.  The
workspace is SCRATCH for the lattice and an input the lattice produced for the neighbours, at exactly sconf_post_workspace bytes."""
import ctypes

import numpy as np
import torch

import footprint as FP
import post_refs as PR
from footprint import IN, OUT, SCRATCH

NO_LAUNCH = {'sconf_post_max_labels', 'sconf_post_workspace', 'sconf_post_step_error'}       # return a value, launch nothing
CASES = {}


def step_error(lib):
    v = ctypes.c_double()
    assert lib.sconf_post_step_error(ctypes.byref(v)) == 0
    return float(v.value)


def _outside(want, tol):
    """(expected, fn) of footprint.Case: the count of elements of the region that differ from `want` in being NaN or -inf, or lie
    outside |got - want| <= tol where both are finite, against 0."""
    want = torch.as_tensor(want, dtype=torch.float64)
    tol = torch.as_tensor(tol, dtype=torch.float64).expand(want.shape)

    def count(out):
        got = out.double().cpu().reshape(want.shape)
        bad = (torch.isnan(got) != torch.isnan(want)) | ((got == -np.inf) != (want == -np.inf)) | (got == np.inf)
        f = torch.isfinite(want) & torch.isfinite(got)
        bad |= f & ((got - want).abs() > tol)
        return bad.sum().double().reshape(1)
    return torch.zeros(1, dtype=torch.float64), count


def _batch(samples, C, pad, seed, pad_labels=1):
    lp, tg, il, tl, blank = PR.parity_case(samples, C, seed, pad_labels=pad_labels)
    lp = lp.copy()
    for b, (T, _) in enumerate(samples):
        lp[b, T:] = np.nan                                                   # frames behind the sample: never read
    return lp, tg, il, tl, blank


def _inputs(a, lp, tg, il, tl, pad):
    B, N, C = lp.shape
    stride = C + pad
    r_lp = a.take('log_probs', (B, N, C), torch.float32, IN, strides=(N * stride, stride, 1), init=torch.from_numpy(lp))
    r_tg = a.take('targets', tuple(tg.shape), torch.int32, IN, init=torch.from_numpy(tg))
    r_il = a.take('input_lengths', B, torch.int32, IN, init=torch.from_numpy(il))
    r_tl = a.take('target_lengths', B, torch.int32, IN, init=torch.from_numpy(tl))
    return r_lp, r_tg, r_il, r_tl, stride


def _restated(v, blank):
    return PR.neighbours_batch(v['log_probs'].numpy(), v['targets'].numpy(), v['input_lengths'].tolist(), v['target_lengths'].tolist(), blank)


def lattice_case(lib, id, samples, C, pad, seed, pad_labels=1):
    lp, tg, il, tl, blank = _batch(samples, C, pad, seed, pad_labels)
    B, N, _ = lp.shape
    Smax = tg.shape[1]
    need = int(lib.sconf_post_workspace(B, N, Smax))
    assert need == 16 * B * N * (2 * Smax + 1)
    step = step_error(lib)
    a = FP.Arena()
    r_lp, r_tg, r_il, r_tl, stride = _inputs(a, lp, tg, il, tl, pad)
    r_ws = a.take('workspace', need, torch.uint8, SCRATCH)
    ll0 = PR.neighbours_batch(lp, tg, il, tl, blank)[0]
    r_ll = a.take('loglik', B, torch.float64, OUT, tol=0.0, unspecified=torch.from_numpy(np.isnan(ll0)))

    def restate(v):
        ll = _restated(v, blank)[0]
        return {'loglik': _outside(ll, PR.loglik_tol(np.asarray(v['input_lengths'].tolist(), dtype=np.float64), step))}

    args = [r_lp, r_tg, r_il, r_tl, B, N, C, stride, Smax, blank, r_ws, need, r_ll]
    return FP.Case(id, 'sconf_post_lattice', a, args, 'post_refs.neighbours_batch', restate, variant=f'{samples} C{C}/{stride} Smax{Smax} ws{need}')


def neighbours_case(lib, id, samples, C, pad, seed, pad_labels=1):
    lp, tg, il, tl, blank = _batch(samples, C, pad, seed, pad_labels)
    B, N, _ = lp.shape
    Smax = tg.shape[1]
    need = int(lib.sconf_post_workspace(B, N, Smax))
    step = step_error(lib)
    a = FP.Arena()
    r_lp, r_tg, r_il, r_tl, stride = _inputs(a, lp, tg, il, tl, pad)
    r_ws = a.take('workspace', need, torch.uint8, IN, produced=True)
    r_ll = a.take('loglik', B, torch.float64, IN, produced=True)
    _, sub0, ins0 = PR.neighbours_batch(lp, tg, il, tl, blank)
    r_sub = a.take('sub_llr', (B, Smax, C), torch.float32, OUT, tol=0.0, unspecified=torch.from_numpy(np.isnan(sub0)))
    r_ins = a.take('ins_llr', (B, Smax + 1, C), torch.float32, OUT, tol=0.0, unspecified=torch.from_numpy(np.isnan(ins0)))

    def restate(v):
        _, sub, ins = _restated(v, blank)
        T = np.asarray(v['input_lengths'].tolist(), dtype=np.float64)[:, None, None]
        return {'sub_llr': _outside(sub, PR.llr_tol(T, sub, step)), 'ins_llr': _outside(ins, PR.llr_tol(T, ins, step))}

    common = [r_lp, r_tg, r_il, r_tl, B, N, C, stride, Smax, blank, r_ws, need, r_ll]
    return FP.Case(id, 'sconf_post_neighbours', a, common + [r_sub, r_ins], 'post_refs.neighbours_batch', restate,
                   before=[('sconf_post_lattice', common)], variant=f'{samples} C{C}/{stride} Smax{Smax} ws{need}')


def slots_case(lib, id, samples, C, seed, pad_labels=1):
    lp, tg, il, tl, blank = _batch(samples, C, 0, seed, pad_labels)
    _, sub, ins = PR.neighbours_batch(lp, tg, il, tl, blank)
    sub, ins = sub.astype(np.float32), ins.astype(np.float32)               # the kernel's input: the ratios as f32, NaN where padded
    B, Smax = tg.shape
    a = FP.Arena()
    r_sub = a.take('sub_llr', (B, Smax, C), torch.float32, IN, init=torch.from_numpy(sub))
    r_ins = a.take('ins_llr', (B, Smax + 1, C), torch.float32, IN, init=torch.from_numpy(ins))
    r_tg = a.take('targets', (B, Smax), torch.int32, IN, init=torch.from_numpy(tg))
    dead_s, dead_g = torch.from_numpy(np.isnan(sub).any(-1)), torch.from_numpy(np.isnan(ins).any(-1))
    outs = [a.take(n, (B, Smax + g), torch.int32 if 'alt' == n[-3:] else torch.float32, OUT, tol=0.0,
                   unspecified=None if 'alt' == n[-3:] else (dead_g if g else dead_s))
            for n, g in (('post', 0), ('alt', 0), ('alt_post', 0), ('gap_post', 1), ('gap_alt', 1), ('gap_alt_post', 1))]

    def restate(v):
        out = PR.slots(v['sub_llr'].numpy(), v['ins_llr'].numpy(), v['targets'].numpy(), blank)
        names = ('post', 'alt', 'alt_post', 'gap_post', 'gap_alt', 'gap_alt_post')
        return {n: torch.from_numpy(o.astype(np.int32)) if n.endswith('alt') else _outside(o, 2.0 ** -22) for n, o in zip(names, out)}

    return FP.Case(id, 'sconf_post_slots', a, [r_sub, r_ins, r_tg, B, C, Smax, blank] + outs, 'post_refs.slots', restate,
                   variant=f'{samples} C{C} Smax{Smax}')


# (samples, C, columns of padding behind C, seed[, labels of padding]): ragged, a sample without labels, one without an alignment
_BATCHES = {
    'three-classes-tight-rows': ([(9, 3), (7, 0), (4, 5)], 3, 0, 301),
    '129-classes-in-rows-of-144': ([(20, 4), (19, 0), (3, 4)], 129, 15, 302),
    '257-classes-five-waves-a-slot': ([(12, 2), (5, 0), (2, 3)], 257, 15, 303),
    'a-wide-label-buffer': ([(6, 3), (4, 0), (2, 3)], 5, 15, 304, 2090),
}
for _id, _a in _BATCHES.items():
    CASES['lattice-' + _id] = ('sconf_post_lattice', lambda lib, _id=_id, _a=_a: lattice_case(lib, 'lattice-' + _id, *_a))
    CASES['neighbours-' + _id] = ('sconf_post_neighbours', lambda lib, _id=_id, _a=_a: neighbours_case(lib, 'neighbours-' + _id, *_a))
for _id, _a in {'three-classes': ([(9, 3), (7, 0), (4, 5)], 3, 311), '130-classes-not-a-multiple-of-four': ([(20, 4), (19, 0), (3, 4)], 130, 312),
                '257-classes': ([(12, 2), (5, 0), (2, 3)], 257, 313)}.items():
    CASES['slots-' + _id] = ('sconf_post_slots', lambda lib, _id=_id, _a=_a: slots_case(lib, 'slots-' + _id, *_a))


def build(id, lib):
    return CASES[id][1](lib)
