"""Plain PyTorch restatements of the fused autograd blocks of ``lcasr_amd.functional``, one function per block.

TEST INFRASTRUCTURE.  Nothing here imports the product package and nothing casts to bf16: every function is dtype-generic and
runs unchanged in float64 (the truth of tests/block_parity.py) and under ``torch.autocast('cpu', torch.bfloat16)`` (its
yardstick).  The math is restated from the module sources that functional.py's section headers name (sconformer_xl.py,
fused_dense.py, attention.py, convolution.py, batchrenorm.py, decoder.py, subsampling.py); tests/test_blocks.py anchors every
function to the reference's own captures in the ``tiny_*`` fixtures (f32, relative L2 <= 1e-4).

Argument order follows the fused block of the same name; tokens are flattened to (M, d) = (B * N, d) as there.  A weight may
come in its state_dict shape (a 1x1 conv's (out, in, 1)); it is viewed 2-D.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F


def _rmax_dmax(nbt: float):
    """batchrenorm.py:40-50."""
    return min(max(2 / 35000 * nbt + 25 / 35, 1.0), 3.0), min(max(5 / 20000 * nbt - 25 / 20, 0.0), 5.0)


def _pad_mask(lengths, B, N, device):
    """(B, N) True where the position is padding; None without lengths."""
    if lengths is None:
        return None
    return torch.arange(N, device=device)[None, :] >= lengths.to(device)[:, None]


def norm(x, weight, bias=None, mode='layer_norm', eps=1e-5):
    d = x.shape[-1]
    if mode == 'layer_norm':
        return F.layer_norm(x, (d,), weight, bias, eps)
    if mode == 'rms_norm':                                       # normalisation.py: x / (||x|| d^-1/2 + eps) * scale
        return weight * (x / (x.norm(2, dim=-1, keepdim=True) * d ** -0.5 + eps))
    if mode == 'rms_norm_apex':
        return weight * x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)
    if mode == 'none':
        return x
    raise ValueError(mode)


def norm2(x, w1, b1, w2, b2, eps1=1e-5, eps2=1e-5, twice=False):
    """(y1, h2): norm_out of a layer, then the decoder norm of y1 (applied two times with `twice`)."""
    y1 = norm(x, w1, b1, 'layer_norm', eps1)
    h2 = norm(y1, w2, b2, 'layer_norm', eps2)
    if twice:
        h2 = norm(h2, w2, b2, 'layer_norm', eps2)
    return y1, h2


def ff(x, nw, nb, w1, w2, b1, b2, scale=0.5, mode='layer_norm', eps=1e-5, residual=True):
    h = norm(x, nw, nb, mode, eps)
    h = F.gelu(F.linear(h, w1, b1), approximate='tanh')
    h = F.linear(h, w2, b2) * scale
    return x + h if residual else h


def _rotary(t, cos, sin):
    """NeoX rotary on (B, N, H, D) with (N, D/2) tables: the halves of the head dimension are the rotated pairs."""
    h = t.shape[-1] // 2
    c, s = cos[None, :, None, :], sin[None, :, None, :]
    t1, t2 = t[..., :h], t[..., h:]
    return torch.cat([t1 * c - t2 * s, t2 * c + t1 * s], dim=-1)


def attn(x, nw, nb, wqkv, wout, bqkv, bout, cos, sin, lengths, B, N, H, D, window=(-1, -1), mode='layer_norm', eps=1e-5,
         residual=True):
    dev = x.device
    h = norm(x, nw, nb, mode, eps)
    pad = _pad_mask(lengths, B, N, dev)
    if pad is not None:
        h = h.masked_fill(pad.reshape(B * N, 1), 0.0)            # attention.py:511
    qkv = F.linear(h, wqkv, bqkv).reshape(B, N, H, D, 3)         # rows "(h d qkv)"
    q, k, v = qkv[..., 0], qkv[..., 1], qkv[..., 2]
    if cos is not None:
        q, k = _rotary(q, cos, sin), _rotary(k, cos, sin)
    s = torch.einsum('bihd,bjhd->bhij', q, k) / math.sqrt(D)
    ok = torch.ones(B, N, N, dtype=torch.bool, device=dev)       # [b, query, key]
    if pad is not None:
        ok = ok & ~pad[:, None, :]
    i, j = torch.arange(N, device=dev)[:, None], torch.arange(N, device=dev)[None, :]
    if window[0] >= 0: ok = ok & (j >= i - window[0])[None]
    if window[1] >= 0: ok = ok & (j <= i + window[1])[None]
    ok = ok | ~ok.any(-1, keepdim=True)                          # a padded query may see no key at all: its row is zeroed below
    a = s.masked_fill(~ok[:, None], float('-inf')).softmax(dim=-1)
    o = torch.einsum('bhij,bjhd->bihd', a, v).reshape(B, N, H * D)
    if pad is not None:
        o = o.masked_fill(pad[..., None], 0.0)                   # attention.py:546-547
    y = F.linear(o.reshape(B * N, H * D), wout, bout)
    return x + y if residual else y


def conv(x, nw, nb, wpw1, bpw1, wdw, bdw, brn_w, brn_b, running_mean, running_std, nbt, wpw2, bpw2, lengths, B, N, training,
         mode='layer_norm', eps=1e-5, residual=True, brn_eps=1e-3, momentum=0.01):
    """-> (y, (running_mean, running_std, num_batches_tracked) after the step); the buffers passed in are left alone."""
    d = x.shape[-1]
    h = norm(x, nw, nb, mode, eps)
    h = F.linear(h, wpw1.reshape(2 * d, d), bpw1)
    h = h[..., :d] * torch.sigmoid(h[..., d:])                   # GLU over channels
    pad = _pad_mask(lengths, B, N, x.device)
    if pad is not None:
        h = h.masked_fill(pad.reshape(B * N, 1), 0.0)            # convolution.py:109-110
    ks = wdw.numel() // d
    h = F.conv1d(h.reshape(B, N, d).transpose(1, 2), wdw.reshape(d, 1, ks), bdw, padding=(ks - 1) // 2, groups=d)
    h = h.transpose(1, 2).reshape(B * N, d)
    rm, rs = running_mean.to(x.dtype), running_std.to(x.dtype)
    if training:                                                 # batchrenorm.py:52-92: statistics over all B*N positions
        mean = h.mean(0)
        std = h.std(0, unbiased=False) + brn_eps
        rmax, dmax = _rmax_dmax(float(nbt))
        r = (std.detach() / rs).clamp(1 / rmax, rmax)
        dd = ((mean.detach() - rm) / rs).clamp(-dmax, dmax)
        h = (h - mean) / std * r + dd
        new = (rm + momentum * (mean.detach() - rm), rs + momentum * (std.detach() - rs), int(nbt) + 1)
    else:
        h = (h - rm) / rs
        new = (rm, rs, int(nbt))
    h = F.silu(brn_w * h + brn_b)
    y = F.linear(h, wpw2.reshape(d, d), bpw2)
    return (x + y if residual else y), new


def selfcond(x, nw, nb, wff, bff, wre, bre, has_norm=True, mode='layer_norm', eps=1e-5, prenormed=None):
    """sconformer_xl.py:241-243.  prenormed: norm(x) as made by the producer of x (norm2)."""
    h = prenormed if prenormed is not None else (norm(x, nw, nb, mode, eps) if has_norm else x)
    p = F.linear(h, wff, bff).softmax(dim=-1)
    return x + F.linear(p, wre, bre)


def head(x, nw, nb, wff, bff, n_norms=1, mode='layer_norm', eps=1e-5, return_logits=False, prenormed=None):
    """decoder.py:22-26 behind the legacy double norm (sconformer_xl.py:246): n_norms applications of ONE norm."""
    if prenormed is not None:
        h = prenormed
    else:
        h = x
        for _ in range(n_norms):
            h = norm(h, nw, nb, mode, eps)
    logits = F.linear(h, wff, bff)
    return logits if return_logits else F.log_softmax(logits, dim=-1)


def head_ctc(x, nw, nb, wff, bff, B, targets, input_lengths, target_lengths, blank, n_norms=1, mode='layer_norm', eps=1e-5,
             prenormed=None):
    """Per-sample CTC negative log-likelihoods (B,) of the head's log-probabilities."""
    logits = head(x, nw, nb, wff, bff, n_norms, mode, eps, True, prenormed)
    if logits.dtype not in (torch.float32, torch.float64):       # ctc_loss takes f32 / f64 (as the training loop hands it)
        logits = logits.float()
    lp = F.log_softmax(logits, dim=-1)
    lp = lp.reshape(B, -1, lp.shape[-1]).transpose(0, 1)
    return F.ctc_loss(lp, targets.long(), input_lengths.long(), target_lengths.long(), blank=blank, reduction='none',
                      zero_infinity=False)


def _sub_stages(audio, stages):
    """conv0 + SiLU, then (depthwise stride 2, 1x1 conv, SiLU) per stage -> (B, C, T', F')."""
    (w0, b0), rest = stages[0], stages[1:]
    C = w0.shape[0]
    x = F.silu(F.conv2d(audio.transpose(1, 2).unsqueeze(1), w0.reshape(C, 1, 3, 3), b0, stride=2, padding=1))
    for wd, bd, wp, bp in rest:
        x = F.conv2d(x, wd.reshape(C, 1, 3, 3), bd, stride=2, padding=1, groups=C)
        x = F.silu(F.conv2d(x, wp.reshape(C, C, 1, 1), bp))
    return x


def _sub_out(x, wout, bout):
    b, c, t, f = x.shape
    return F.linear(x.transpose(1, 2).reshape(b, t, c * f), wout, bout)   # subsampling.py:422-423


def subsample(audio, w0, b0, wd1, bd1, wp1, bp1, wd2, bd2, wp2, bp2, wout, bout):
    """'dw_striding' x8: audio (B, F, T) -> (B, N, d_model)."""
    return _sub_out(_sub_stages(audio, [(w0, b0), (wd1, bd1, wp1, bp1), (wd2, bd2, wp2, bp2)]), wout, bout)


def subsample4(audio, w0, b0, wd1, bd1, wp1, bp1, wout, bout):
    """'dw_striding' x4: the x8 chain without its last stage."""
    return _sub_out(_sub_stages(audio, [(w0, b0), (wd1, bd1, wp1, bp1)]), wout, bout)


def out_lengths(lengths, stages=3):
    """subsampling.py:557-567 (padding 1, kernel 3, stride 2, floor)."""
    for _ in range(stages):
        lengths = torch.div(lengths - 1, 2, rounding_mode='floor') + 1
    return lengths


def rotary_tables(N, D, base=10000.0, dtype=torch.float32):
    """(cos, sin), each (N, D/2) - rotary_emb.py:23,44-57, one column per rotated pair."""
    inv = 1.0 / (base ** (torch.arange(0, D, 2, dtype=torch.float64) / D))
    fr = torch.arange(N, dtype=torch.float64)[:, None] * inv[None, :]
    return fr.cos().to(dtype), fr.sin().to(dtype)
