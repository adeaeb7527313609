"""ctypes binding and tensor-level op of CTC prefix beam search with an n-gram LM fused in (include/sconf_lm.h), the fifth ABI unit of
libsconf_hip.so.

Same discipline as hip/beam.py: GPU tensors in and out, outputs and workspace allocated here, kernels enqueued on torch's current
stream, no fallback - a CPU tensor, a missing library or a failing call raises.  `tests/lm_refs.py` restates the op in numpy.  The
image is what decoding.lm.NGramLM builds; this module is imported by decoding/lm.py and, for a search with an LM, by decoding/beam.py -
not by the package's other units."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import torch

from . import _lib
from ._lib import vp, i64, i32, f32, f64
from .ops import _chk_log_probs, _chk_lengths, _p, _stream, _workspace

MAX_ORDER = 5           # sconf_lm_max_order(), for code that builds an image without the library (tests hold the two together)

# name -> argtypes (status-returning launchers).  Must match include/sconf_lm.h.
PROTOTYPES = {
    'sconf_lm_beam_ctc': [vp, vp, vp, i64, i64, i64, i32, i32, vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, i64, i32, i32, i32, f32, f64, i32,
                          i64, f64, f64, vp],
}
# name -> (argtypes, restype): the queries
PLAIN = {
    'sconf_lm_max_order': ([], C.c_int),
    'sconf_lm_beam_threads': ([i64, i64], C.c_int),
    'sconf_lm_beam_workspace': ([i64, i64, i64, i64], C.c_int64),
}

_lib.register(PROTOTYPES, PLAIN)
load = _lib.load


class BeamsLM(NamedTuple):
    """What sconf_lm_beam_ctc writes: the five outputs of sconf_beam_ctc (scores: acoustic total + LM bonus) and logit_scores (B, nbest)
    f64, the acoustic totals."""
    count: torch.Tensor
    tokens: torch.Tensor
    lengths: torch.Tensor
    token_frames: torch.Tensor
    scores: torch.Tensor
    logit_scores: torch.Tensor


def max_order() -> int:
    return int(load().sconf_lm_max_order())


def beam_workspace(B: int, N: int, W: int, Kmax: int) -> int:
    n = int(load().sconf_lm_beam_workspace(B, N, W, Kmax))
    if n < 0:
        raise ValueError(f'ctc_beam_lm: invalid sizes B={B} N={N} beam_width={W} max_tokens_per_frame={Kmax}')
    return n


def ctc_beam_lm(log_probs: torch.Tensor, input_lengths: Optional[torch.Tensor], image: torch.Tensor, n_states: int, n_entries: int,
                num_tokens: int, order: int, start_state: int, blank: int, beam_width: int, nbest: int, token_min_logp: float,
                beam_prune_logp: float, max_tokens_per_frame: int, max_len: int, alpha: float, beta: float) -> BeamsLM:
    """log_probs (B, N, C) f32, input_lengths (B,) int32 or None (= N), image: the LM's flat int32 buffer on the same device ->
    BeamsLM of device tensors.  See include/sconf_lm.h for the image and the semantics."""
    B, N, Cn = _chk_log_probs(log_probs, 'ctc_beam_lm')
    if B < 1 or N < 1:
        raise ValueError(f'ctc_beam_lm: empty input B={B} N={N}')
    _chk_lengths(input_lengths, B, 'ctc_beam_lm', 'input_lengths')
    if not torch.is_tensor(image) or not image.is_cuda or image.device != log_probs.device:
        raise RuntimeError('ctc_beam_lm: the LM image must be a GPU tensor on the device of log_probs (NGramLM.to(device))')
    if image.dtype != torch.int32 or image.dim() != 1 or not image.is_contiguous():
        raise TypeError(f'ctc_beam_lm: the LM image must be a contiguous 1-D int32 tensor, got {image.dtype} {tuple(image.shape)}')
    S, E, V = int(n_states), int(n_entries), int(num_tokens)
    if S < 1 or E < 0 or V < 1 or image.numel() != 4 * S + 4 * E + 2 * V:
        raise ValueError(f'ctc_beam_lm: an image of {image.numel()} words does not hold {S} states, {E} entries and {V} tokens')
    W, nb, K, L = int(beam_width), int(nbest), int(max_tokens_per_frame), int(max_len)
    if not 1 <= nb <= W or L < 1:
        raise ValueError(f'ctc_beam_lm: nbest={nb} must be in 1..beam_width={W} and max_len={L} at least 1')
    nbytes = beam_workspace(B, N, W, K)
    dev = log_probs.device
    out = BeamsLM(torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, nb, L, dtype=torch.int32, device=dev),
                  torch.empty(B, nb, dtype=torch.int32, device=dev), torch.empty(B, nb, L, dtype=torch.int32, device=dev),
                  torch.empty(B, nb, dtype=torch.float64, device=dev), torch.empty(B, nb, dtype=torch.float64, device=dev))
    ws = _workspace(nbytes, dev)
    _lib.call('sconf_lm_beam_ctc', _p(log_probs), _p(input_lengths), _p(image), S, E, V, int(order), int(start_state), _p(out.count),
              _p(out.tokens), _p(out.lengths), _p(out.token_frames), _p(out.scores), _p(out.logit_scores), _p(ws), nbytes, B, N, Cn,
              int(blank), W, nb, float(token_min_logp), float(beam_prune_logp), K, L, float(alpha), float(beta), _stream())
    return out
