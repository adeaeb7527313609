"""Plain references of the evaluation-loop ops (same signatures as lcasr_amd.hip.ops) and what the CPU and GPU tests of the
evaluation loop share: the brute-force definition of the edit counts, pair generators, the fixture's stub model.

Contract of the counts (set by the issue): `errors` is the unit-cost Levenshtein distance; the split is that of the optimal
alignment with the fewest substitutions, which is unique because ins - del = len(hyp) - len(ref) and sub + del + ins = errors.
All comparisons against these references are exact integer equality."""
import itertools

import numpy as np
import torch

STEP = 1 << 32          # one deletion or insertion in the packed key  cost * 2^32 + substitutions
SUB = STEP + 1          # one substitution


def _split(key, m, n):
    cost, sub = int(key) >> 32, int(key) & 0xffffffff
    dele = (cost - sub - (m - n)) // 2
    return [cost, sub, dele, dele + m - n]


def edit_key_loop(h, r):
    """min-plus DP over the packed key, cell by cell."""
    m, n = len(h), len(r)
    prev = [j * STEP for j in range(n + 1)]
    for i in range(1, m + 1):
        row = [i * STEP] + [0] * n
        for j in range(1, n + 1):
            row[j] = min(prev[j - 1] + (0 if h[i - 1] == r[j - 1] else SUB), prev[j] + STEP, row[j - 1] + STEP)
        prev = row
    return prev[n]


def edit_key_rows(h, r):
    """The same DP with each row vectorised: cand[j] = min(prev[j-1] + sub_cost, prev[j] + 2^32), then the horizontal steps as a
    running minimum of cand - j * 2^32.  int64 throughout, exact."""
    h, r = np.asarray(h, dtype=np.int64), np.asarray(r, dtype=np.int64)
    n = len(r)
    ramp = np.arange(n + 1, dtype=np.int64) * STEP
    prev = ramp.copy()
    cand = np.empty(n + 1, dtype=np.int64)
    for hi in h:
        cand[0] = prev[0] + STEP
        np.minimum(prev[:-1] + np.where(r == hi, 0, SUB), prev[1:] + STEP, out=cand[1:])
        prev = np.minimum.accumulate(cand - ramp) + ramp
    return int(prev[n])


def _counts(key_fn, hyp, hyp_off, ref, ref_off):
    hyp, ref = hyp.cpu().numpy(), ref.cpu().numpy()
    ho, ro = hyp_off.cpu().tolist(), ref_off.cpu().tolist()
    out = []
    for p in range(len(ho) - 1):
        h, r = hyp[ho[p]:ho[p + 1]], ref[ro[p]:ro[p + 1]]
        out.append(_split(key_fn(h, r), len(h), len(r)))
    return torch.tensor(out, dtype=torch.int64, device=hyp_off.device).reshape(-1, 4)


def edit_counts_loop(hyp, hyp_off, ref, ref_off):
    return _counts(lambda h, r: edit_key_loop(h.tolist(), r.tolist()), hyp, hyp_off, ref, ref_off)


def edit_counts(hyp, hyp_off, ref, ref_off):
    return _counts(edit_key_rows, hyp, hyp_off, ref, ref_off)


def brute_force_counts(h, r):
    """Every alignment of h against r enumerated: the (S, D, I) triples of the alignments with the lexicographically smallest
    (cost, substitutions).  The definition says this set has exactly one element."""
    m, n = len(h), len(r)
    found = set()

    def walk(i, j, s, d, ins):
        if i == m and j == n:
            found.add((s + d + ins, s, d, ins))
            return
        if i < m and j < n:
            walk(i + 1, j + 1, s + (h[i] != r[j]), d, ins)
        if j < n:
            walk(i, j + 1, s, d + 1, ins)          # a reference token with no partner: deletion
        if i < m:
            walk(i + 1, j, s, d, ins + 1)          # a hypothesis token with no partner: insertion

    walk(0, 0, 0, 0, 0)
    best = min((c, s) for c, s, _, _ in found)
    return sorted({(c, s, d, i) for c, s, d, i in found if (c, s) == best})


def copy_row_spans_(src, spans, dst):
    W, n, _ = src.shape
    for w, (s0, rows, d0) in enumerate(spans.cpu().tolist()):
        if s0 < 0 or rows <= 0 or d0 < 0 or s0 + rows > n or d0 + rows > dst.shape[0]:
            continue
        dst[d0:d0 + rows] = src[w, s0:s0 + rows]


def attach(monkeypatch, kernel_refs):
    """kernel_refs.py has no entry for the new ops: hang these (and ctc_collapse of dyneval_refs) on it for the duration of a test."""
    import dyneval_refs
    for name, fn in (('edit_counts', edit_counts), ('copy_row_spans_', copy_row_spans_), ('ctc_collapse', dyneval_refs.ctc_collapse)):
        monkeypatch.setattr(kernel_refs, name, fn, raising=False)


# ---- pairs ----------------------------------------------------------------------------------------------------------------
def ragged(seqs, device='cpu'):
    flat = np.concatenate([np.asarray(s, dtype=np.int32) for s in seqs] + [np.zeros(0, dtype=np.int32)])
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    return torch.from_numpy(flat).to(device), torch.from_numpy(off).to(device)


def random_pair(rng, m, n, alphabet):
    return rng.integers(0, alphabet, m).astype(np.int32), rng.integers(0, alphabet, n).astype(np.int32)


def planted_pair(rng, n, alphabet, edits):
    """A hypothesis made from a random reference by `edits` random substitutions, deletions and insertions."""
    r = rng.integers(0, alphabet, n).astype(np.int32)
    h = r.tolist()
    for _ in range(edits):
        kind, at = int(rng.integers(0, 3)), int(rng.integers(0, max(len(h), 1)))
        if kind == 0 and h: h[at] = int(rng.integers(0, alphabet))
        elif kind == 1 and h: del h[at]
        else: h.insert(at, int(rng.integers(0, alphabet)))
    return np.asarray(h, dtype=np.int32), r


# ---- the buffered fixture's stub model ---------------------------------------------------------------------------------
class _Sub:
    subsampling_factor = 8


class StubModel(torch.nn.Module):
    """The placement cases of buffered_tiny.npz: frame t of the stub recording has value t in every feature, and a window's
    posteriors (rows as the x8 subsampler counts them, 4 classes) are  first_frame * 4096 + row  in every class: exact integers
    that name the window and the row a value came from."""
    def __init__(self):
        super().__init__()
        self.subsampling = _Sub()
        self.anchor = torch.nn.Parameter(torch.zeros(1))

    @staticmethod
    def rows(frames):
        for _ in range(3):
            frames = (frames - 1) // 2 + 1
        return frames

    def forward(self, x):
        n = self.rows(x.shape[-1])
        v = x[:, 0, 0].round()[:, None, None] * 4096 + torch.arange(n, device=x.device, dtype=torch.float32)[None, :, None]
        return {'final_posteriors': v.expand(x.shape[0], n, 4).contiguous()}


def stub_spec(spec_n):
    return torch.arange(spec_n, dtype=torch.float32)[None, None, :].expand(1, 2, spec_n).contiguous()


class StubTok:
    def vocab_size(self): return 3


class Args:
    config = {'audio_chunking': {'size': 512, 'overlap': 128}}
