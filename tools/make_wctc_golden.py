"""Writes tests/golden/wctc_cases.npz: the reference's own wild-card CTC loss (lcasr/losses/wctc.py, imported at run time from REF and
run in float64 on the CPU) and its autograd gradient, in all three modes, on small cases.  Only numbers are written.  Inert where REF
does not exist (development container only).

Per case <c> (batch-major, as the kernels take them):
  <c>.lp (B, N, C) f32            log_softmax of seeded noise; the reference is fed its float64 widening, time-major
  <c>.targets (B, Smax) int64     negative past target_lengths where the case says so
  <c>.input_lengths, <c>.target_lengths (B) int64, <c>.blank
  <c>.<mode>.loss (B) f64, <c>.<mode>.grad (B, N, C) f64      d loss[b] / d lp, zero rows from input_lengths[b] on
The reference ignores input_lengths, so a ragged sample is the reference run on log_probs[:len_b, b:b+1] alone.
For max_prob the two largest e_t of every sample must differ by more than 1e-3 (else the case's seed moves on): a tie cannot
decide a test."""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle.make_golden import GOLD, REF   # noqa: E402
import wctc_refs as WR                     # noqa: E402

# name -> (B, N, C, blank, targets per sample (None = padding), input_lengths or None, scale of the noise)
P = None
CASES = {
    'one_label': (1, 9, 5, 0, [[3]], None, 1.0),
    'one_frame_one_label': (1, 1, 4, 2, [[1]], None, 1.0),
    'doubled_label': (2, 12, 6, 5, [[2, 2, 4, 1], [0, 3, 3, 3]], None, 1.0),
    'exactly_labels_plus_repeats': (1, 4, 5, 0, [[1, 1, 2]], None, 1.0),
    'negative_padding_middle_blank': (3, 20, 8, 3, [[1, 5, 5, 0, 7], [6, 2, 4, P, P], [7, P, P, P, P]], None, 2.0),
    'ragged_batch': (3, 24, 12, 11, [[4, 1, 1, 9, 0, 3], [2, 8, 8, P, P, P], [5, 10, 3, 7, P, P]], [24, 17, 9], 1.5),
    'unreachable_early_frames': (2, 64, 12, 0, [list(range(1, 12)) + [11, 11, 4, 4, 2, 9, 9, 1, 3], [7, 7, 7, 7, 7, 7, 2] + [P] * 13], None, 3.0),
}


def load_wctc():
    spec = importlib.util.spec_from_file_location('reference_wctc', os.path.join(REF, 'lcasr', 'losses', 'wctc.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_reference(ref, lp, targets, tl, blank, mode):
    """lp (N, B, C) float64 -> loss (B), grad (N, B, C) through autograd (the samples are independent: one backward of the sum)."""
    x = lp.clone().requires_grad_(True)
    N, B, _ = x.shape
    loss = ref.wctc_loss(x, targets, torch.full((B,), N), tl, blank=blank, mode=mode)
    loss.sum().backward()
    return loss.detach(), x.grad


def make_case(ref, name, seed):
    B, N, C, blank, tg, il, scale = CASES[name]
    g = torch.Generator().manual_seed(seed)
    lp = torch.log_softmax(torch.randn(B, N, C, generator=g) * scale, -1)                     # f32, batch-major
    targets = torch.tensor([[-1 if v is None else v for v in row] for row in tg], dtype=torch.int64)
    tl = torch.tensor([sum(v is not None for v in row) for row in tg], dtype=torch.int64)
    il = torch.tensor(il if il is not None else [N] * B, dtype=torch.int64)
    out = {'lp': lp.numpy(), 'targets': targets.numpy(), 'input_lengths': il.numpy(), 'target_lengths': tl.numpy(), 'blank': np.int64(blank)}
    x = lp.double().transpose(0, 1).contiguous()                                               # (N, B, C), as the reference takes it
    for mode in WR.MODES:
        loss, grad = torch.zeros(B, dtype=torch.float64), torch.zeros(N, B, C, dtype=torch.float64)
        if il is not None and bool((il != N).any()):
            for b in range(B):
                T = int(il[b])
                l, gr = run_reference(ref, x[:T, b:b + 1], targets[b:b + 1], tl[b:b + 1], blank, mode)
                loss[b], grad[:T, b:b + 1] = l[0], gr
        else:
            loss, grad = run_reference(ref, x, targets, tl, blank, mode)
        out[f'{mode}.loss'], out[f'{mode}.grad'] = loss.numpy(), grad.transpose(0, 1).contiguous().numpy()
    _, _, info = WR.wctc(lp.numpy(), targets.numpy(), il.numpy(), tl.numpy(), blank, 'max_prob')
    for e, _ in info:
        top = np.sort(e[np.isfinite(e)])[::-1]
        if len(top) > 1 and top[0] - top[1] <= 1e-3:
            return None                                                                       # a near-tie of the maximum: another seed
    return out


def main():
    assert os.path.isdir(REF), 'reference not present: this script only runs in the development container'
    ref = load_wctc()
    arrays = {'cases': np.array(list(CASES))}
    for i, name in enumerate(CASES):
        seed = 100 * (i + 1)
        while (case := make_case(ref, name, seed)) is None:
            seed += 1
        arrays[f'{name}.seed'] = np.int64(seed)
        for k, v in case.items():
            arrays[f'{name}.{k}'] = v
        print(f'{name}: seed {seed}, ' + ', '.join(f'{m} loss {np.array2string(case[m + ".loss"], precision=4)}' for m in WR.MODES))
    path = os.path.join(GOLD, 'wctc_cases.npz')
    np.savez_compressed(path, **arrays)
    print(f'wrote {path}: {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
