"""The calibration unit (include/sconf_calib.h) restated in numpy, sharing nothing with the kernels.  TEST INFRASTRUCTURE, plain
importable module.

The alignment in three forms: `align_plain`, the recurrence and the backtrace of the header cell by cell; `align_fast`, row by row
with (errors, substitutions) as one integer key and the left move as a running minimum; `align_brute`, every alignment of a pair
enumerated.  The sweep as `sweep` (float64) and `sweep32` (float32, used ONLY to set tolerances), both tests/confid_refs.py on the
scaled input.  `op_*` wrap the restatements with the signatures of lcasr_amd.hip.calib, on CPU tensors, for the host-logic tests."""
import numpy as np
import torch

import confid_refs as CR

KEY = 1 << 32                 # key = errors * KEY + substitutions
DIAG, UP, LEFT = 0, 1, 2
# the geometry the header states (the tests hold the library's queries against it)
STRIP, PASS, ROWS, CPL = 512, 2048, 256, 8
TILE_BYTES = (ROWS + 63) * 128
MAX_LEN = 65535


def pair_bytes(H, R):
    """The header's formula."""
    if H < 0 or R < 0 or H > MAX_LEN or R > MAX_LEN:
        return -1
    if H == 0 or R == 0:
        return 0
    parked = -(-8 * (H + 1) // 16) * 16 if R > PASS else 0
    return parked + -(-H // ROWS) * -(-R // STRIP) * TILE_BYTES


def _counts(errors, subs, H, R):
    dels = (errors - subs - (H - R)) // 2
    return np.array([errors, subs, dels, dels + H - R], dtype=np.int64)


def _backtrace(move, H, R):
    """From (H, R): the stored first move of each cell; at j == 0 up, at i == 0 left."""
    h2r, r2h = np.full(H, -1, dtype=np.int32), np.full(R, -1, dtype=np.int32)
    i, j = H, R
    while i > 0 and j > 0:
        d = move(i, j)
        if d == DIAG:
            h2r[i - 1], r2h[j - 1] = j - 1, i - 1
            i, j = i - 1, j - 1
        elif d == UP:
            i -= 1
        else:
            j -= 1
    return h2r, r2h


def align_plain(hyp, ref):
    """(hyp_to_ref, ref_to_hyp, counts): E(i, j) as tuples, three moves per cell, the first that reproduces the minimum."""
    H, R = len(hyp), len(ref)
    E = [[None] * (R + 1) for _ in range(H + 1)]
    D = [[LEFT] * (R + 1) for _ in range(H + 1)]
    for i in range(H + 1):
        for j in range(R + 1):
            if i == 0 or j == 0:
                E[i][j] = (i + j, 0)
                continue
            step = (0, 0) if hyp[i - 1] == ref[j - 1] else (1, 1)
            cands = []
            for (a, b), (da, db) in (((i - 1, j - 1), step), ((i - 1, j), (1, 0)), ((i, j - 1), (1, 0))):
                cands.append((E[a][b][0] + da, E[a][b][1] + db))
            E[i][j] = min(cands)
            D[i][j] = cands.index(E[i][j])
    h2r, r2h = _backtrace(lambda i, j: D[i][j], H, R)
    return h2r, r2h, _counts(E[H][R][0], E[H][R][1], H, R)


def align_fast(hyp, ref):
    """The same, a row at a time: t[j] = min(diagonal, up) elementwise; the left move adds KEY per column, so
    cur[j] - j KEY = min over k <= j of (t[k] - k KEY), a running minimum."""
    hyp, ref = np.asarray(hyp, dtype=np.int64), np.asarray(ref, dtype=np.int64)
    H, R = len(hyp), len(ref)
    if H == 0 or R == 0:
        return np.full(H, -1, dtype=np.int32), np.full(R, -1, dtype=np.int32), _counts(max(H, R), 0, H, R)
    cols = np.arange(R + 1, dtype=np.int64) * KEY
    prev = cols.copy()
    dirs = np.empty((H, R), dtype=np.uint8)
    for i in range(1, H + 1):
        cd = prev[:-1] + np.where(ref == hyp[i - 1], 0, KEY + 1)
        cu = prev[1:] + KEY
        t = np.concatenate([[i * KEY], np.minimum(cd, cu)])
        cur = np.minimum.accumulate(t - cols) + cols
        dirs[i - 1] = np.where(cd == cur[1:], DIAG, np.where(cu == cur[1:], UP, LEFT))
        prev = cur
    h2r, r2h = _backtrace(lambda i, j: dirs[i - 1, j - 1], H, R)
    return h2r, r2h, _counts(int(prev[R] // KEY), int(prev[R] % KEY), H, R)


def align_brute(hyp, ref):
    """Every alignment enumerated as its moves from the END backwards.  -> (the smallest (errors, substitutions), and among the
    alignments that reach it the one whose backward move sequence is the smallest with diagonal < up < left, as maps)."""
    H, R = len(hyp), len(ref)
    best = None

    def walk(i, j, moves, e, s):
        nonlocal best
        if i == 0 and j == 0:
            cand = ((e, s), tuple(moves))
            if best is None or cand < best:
                best = cand
            return
        if i > 0 and j > 0:
            mis = int(hyp[i - 1] != ref[j - 1])
            walk(i - 1, j - 1, moves + [DIAG], e + mis, s + mis)
        if i > 0:
            walk(i - 1, j, moves + [UP], e + 1, s)
        if j > 0:
            walk(i, j - 1, moves + [LEFT], e + 1, s)

    walk(H, R, [], 0, 0)
    (e, s), moves = best
    h2r, r2h = np.full(H, -1, dtype=np.int32), np.full(R, -1, dtype=np.int32)
    i, j = H, R
    for d in moves:
        if d == DIAG:
            h2r[i - 1], r2h[j - 1] = j - 1, i - 1
            i, j = i - 1, j - 1
        elif d == UP:
            i -= 1
        else:
            j -= 1
    return h2r, r2h, _counts(e, s, H, R)


def align_batch(hyp, hyp_off, ref, ref_off, ws_off=None, form=align_fast):
    """The entry point on flat arrays: (hyp_to_ref like hyp, ref_to_hyp like ref, counts (P, 4)); a pair whose slice of the workspace
    is below pair_bytes, or that is longer than MAX_LEN, is -1 throughout."""
    hyp, ref = np.asarray(hyp), np.asarray(ref)
    P = len(hyp_off) - 1
    h2r, r2h = np.full(len(hyp), -1, dtype=np.int32), np.full(len(ref), -1, dtype=np.int32)
    counts = np.full((P, 4), -1, dtype=np.int64)
    for p in range(P):
        h0, h1, r0, r1 = int(hyp_off[p]), int(hyp_off[p + 1]), int(ref_off[p]), int(ref_off[p + 1])
        need = pair_bytes(h1 - h0, r1 - r0)
        if need < 0 or (ws_off is not None and int(ws_off[p + 1]) - int(ws_off[p]) < need):
            continue
        h2r[h0:h1], r2h[r0:r1], counts[p] = form(hyp[h0:h1], ref[r0:r1])
    return h2r, r2h, counts


def edits(rng, ref, rate, vocab):
    """`ref` with about rate * len(ref) random substitutions, deletions and insertions."""
    out = []
    for t in ref:
        u = rng.random()
        if u < rate / 3:
            out.append(int(rng.integers(0, vocab)))
        elif u < 2 * rate / 3:
            continue
        elif u < rate:
            out.extend([int(t), int(rng.integers(0, vocab))])
        else:
            out.append(int(t))
    return out


def pair_case(kind, H, R, seed=0):
    """(hyp, ref) int32 arrays of exactly H and R ids: 'identical' (the shorter a prefix of the longer), 'edits' (10 % random edits),
    'disjoint' (no id in common), 'two' (a 2-symbol alphabet: maximal ties)."""
    rng = np.random.default_rng(seed)
    if kind == 'two':
        return rng.integers(0, 2, H).astype(np.int32), rng.integers(0, 2, R).astype(np.int32)
    if kind == 'disjoint':
        return rng.integers(0, 50, H).astype(np.int32), rng.integers(50, 100, R).astype(np.int32)
    ref = rng.integers(0, 1000, R).astype(np.int32)
    hyp = ref.tolist() if kind == 'identical' else edits(rng, ref, 0.1, 1000)
    hyp = (hyp + rng.integers(0, 1000, max(H - len(hyp), 0)).tolist())[:H]
    assert kind in ('identical', 'edits')
    return np.array(hyp, dtype=np.int32).reshape(H), ref


# ---- the sweep ------------------------------------------------------------------------------------------------------------------
def inv32(inv_temps):
    """The factors the ABI carries: C floats, as float64 values."""
    return [float(np.float32(v)) for v in inv_temps]


def scaled(x, classes, inv_temp):
    """inv_temp * x over the first `classes` columns, in float64 (exact: a product of two float32 values)."""
    x = np.asarray(x)
    classes = x.shape[1] if classes is None else classes
    with np.errstate(invalid='ignore'):
        return x[:, :classes].astype(np.float64) * float(np.float32(inv_temp))


def sweep(x, inv_temps, classes=None, method='tsallis', norm='exp', alpha=1.0 / 3.0):
    """idx (M) int32, conf (K, M) float64: column k is confid_refs.frames of inv_temps[k] * x; a factor that is not finite and
    positive gives NaN."""
    x = np.asarray(x)
    idx, _ = CR.frames(x, classes, method, norm, alpha)
    conf = np.full((len(inv_temps), x.shape[0]), np.nan)
    for k, it in enumerate(inv32(inv_temps)):
        if np.isfinite(it) and it > 0:
            conf[k] = CR.frames(scaled(x, classes, it), None, method, norm, alpha)[1]
    return idx, conf


def sweep32(x, inv_temps, classes=None, method='tsallis', norm='exp', alpha=1.0 / 3.0):
    """conf (K, M) float32 in float32 arithmetic: confid_refs.frames32 of the scaled input."""
    x = np.asarray(x)
    conf = np.full((len(inv_temps), x.shape[0]), np.nan, dtype=np.float32)
    for k, it in enumerate(inv32(inv_temps)):
        if np.isfinite(it) and it > 0:
            conf[k] = CR.frames32(scaled(x, classes, it), None, method, norm, CR.alpha32(alpha))
    return conf


def sweep_tolerance(x, inv_temp, classes, method, norm, alpha):
    """confid_refs.tolerance on the scaled input: (4 d32 + 1e-6, d32)."""
    return CR.tolerance(scaled(x, classes, inv_temp), None, method, norm, alpha)


# ---- the ops of lcasr_amd.hip.calib on CPU tensors -----------------------------------------------------------------------------------
def op_edit_align(hyp, hyp_off, ref, ref_off, ws_off, ws=None):
    h2r, r2h, counts = align_batch(hyp.numpy(), hyp_off.tolist(), ref.numpy(), ref_off.tolist(), ws_off.tolist())
    return torch.from_numpy(h2r), torch.from_numpy(r2h), torch.from_numpy(counts)


def op_frames_sweep(x, inv_temps, classes=None, method='tsallis', norm='exp', alpha=1.0 / 3.0):
    idx, conf = sweep(x.detach().float().numpy(), inv_temps.tolist(), classes, method, norm, alpha)
    return torch.from_numpy(idx), torch.from_numpy(conf.astype(np.float32))
