"""Plain-PyTorch references of the two attention-map ops (hip/ops.py::attn_scores, attn_offset_profile), with the same signatures,
and the stand-in op layer of the CPU tests: these two plus tests/kernel_refs.py for everything else."""
import torch

import kernel_refs


def mask(B, N, lengths, window, device):
    """[b, i, j] True where the position is visible: key j < length, j inside [i - left, i + right], and query row i < length."""
    ok = kernel_refs._attn_mask(B, N, lengths, window, device)
    if lengths is not None:
        ok = ok & (torch.arange(N, device=device)[None, :, None] < lengths[:, None, None])
    return ok


def scores_f64(q, k, lengths, window=(-1, -1), scale=None):
    """(B,H,N,N) f64 = scale * q_i . k_j from the operands as given (bf16 values, exact in f64), -inf at masked positions."""
    B, N, H, D = q.shape
    sc = scale if scale is not None else D ** -0.5
    s = torch.einsum('bihd,bjhd->bhij', q.double(), k.double()) * sc
    return s.masked_fill(~mask(B, N, lengths, window, q.device)[:, None], float('-inf'))


def attn_scores(q, k, lengths, window=(-1, -1), scale=None, out_dtype=torch.float32):
    return scores_f64(q, k, lengths, window, scale).to(out_dtype)


def diagonal_sums(p):
    """(..., N, N) -> (..., 2N-1): entry delta + N - 1 = sum_i p[i, i + delta]."""
    n = p.shape[-1]
    return torch.stack([p.diagonal(d, -2, -1).sum(-1) for d in range(-(n - 1), n)], -1)


def profile_f64(q, k, lse, lengths, window=(-1, -1), scale=None):
    s = scores_f64(q, k, lengths, window, scale)
    p = torch.exp(s - lse.double()[..., None])                      # lse = +inf (padded row, row without a key): exp(-inf) = 0
    p = torch.nan_to_num(p, nan=0.0)                                # -inf - (-inf) cannot occur with an lse of the forward; be safe
    return diagonal_sums(p)


def attn_offset_profile(q, k, lse, lengths, window=(-1, -1), scale=None):
    return profile_f64(q, k, lse, lengths, window, scale).float()


def exact_profile_f64(q, k, lengths, window=(-1, -1), scale=None):
    """The profile of the exact f64 softmax of the scores (its own log-sum-exp; rows without a visible key contribute nothing)."""
    s = scores_f64(q, k, lengths, window, scale)
    lse = torch.logsumexp(s, -1)
    lse = lse.masked_fill(torch.isinf(lse), float('inf'))
    return diagonal_sums(torch.exp(s - lse[..., None]))


def banded_profile_f64(q, k, window, lse=None, scale=None):
    """The profile for B = 1, no lengths and a two-sided window, without the N x N matrix: one f64 dot product per (row, offset)
    pair of the band.  lse (1,H,N): the log-sum-exp to use; None: the exact one of the band.  -> (H, 2N-1)."""
    B, N, H, D = q.shape
    assert B == 1 and window[0] >= 0 and window[1] >= 0
    sc = scale if scale is not None else D ** -0.5
    qd, kd = q[0].double().transpose(0, 1), k[0].double().transpose(0, 1)      # (H, N, D)
    offs = list(range(-min(window[0], N - 1), min(window[1], N - 1) + 1))
    band = torch.full((H, N, len(offs)), float('-inf'), dtype=torch.float64, device=q.device)
    for c, d in enumerate(offs):
        i0, i1 = max(0, -d), min(N, N - d)
        band[:, i0:i1, c] = (qd[:, i0:i1] * kd[:, i0 + d:i1 + d]).sum(-1) * sc
    row_lse = torch.logsumexp(band, -1) if lse is None else lse[0].double()
    out = torch.zeros(H, 2 * N - 1, dtype=torch.float64, device=q.device)
    out[:, offs[0] + N - 1:offs[-1] + N] = torch.exp(band - row_lse[..., None]).sum(1)
    return out


class Ops:
    """The op layer the CPU tests install in lcasr_amd.functional: the two references above, kernel_refs for everything else."""
    attn_scores = staticmethod(attn_scores)
    attn_offset_profile = staticmethod(attn_offset_profile)

    def __getattr__(self, name):
        return getattr(kernel_refs, name)
