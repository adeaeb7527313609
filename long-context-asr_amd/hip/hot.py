"""ctypes binding and tensor-level op of CTC prefix beam search with hotword boosting (include/sconf_hot.h), the eleventh ABI unit of
libsconf_hip.so.

Same discipline as hip/lm.py: GPU tensors in and out, outputs and workspace allocated here, kernels enqueued on torch's current
stream, no fallback - a CPU tensor, a missing library or a failing call raises.  `tests/hot_refs.py` restates the op in numpy.  The
hotword image is what decoding.hotwords.HotwordSet builds, the LM image (optional) what decoding.lm.NGramLM builds; this module is
imported by decoding/hotwords.py and, for a search with hotwords, by decoding/beam.py - not by the package's other units."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import torch

from . import _lib
from ._lib import vp, i64, i32, f32, f64
from .ops import _chk_log_probs, _chk_lengths, _p, _stream, _workspace

MAX_LEN = 32            # sconf_hot_max_len(), for code that builds an image without the library (tests hold the two together)

# name -> argtypes (status-returning launchers).  Must match include/sconf_hot.h.
PROTOTYPES = {
    'sconf_hot_beam_ctc': [vp, vp, vp, i64, i64, i64, i32, i32, vp, i64, i64, i32, f64, vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, i64,
                           i32, i32, i32, f32, f64, i32, i64, f64, f64, vp],
}
# name -> (argtypes, restype): the queries
PLAIN = {
    'sconf_hot_max_len': ([], C.c_int),
    'sconf_hot_max_width': ([], C.c_int),
    'sconf_hot_max_tokens': ([], C.c_int),
    'sconf_hot_beam_threads': ([i64, i64], C.c_int),
    'sconf_hot_beam_workspace': ([i64, i64, i64, i64], C.c_int64),
}

_lib.register(PROTOTYPES, PLAIN)
load = _lib.load


class BeamsHot(NamedTuple):
    """What sconf_hot_beam_ctc writes: the six outputs of sconf_lm_beam_ctc (scores: acoustic total + LM bonus + hotword credit) and
    hot_scores (B, nbest) f64, the hotword credit alone."""
    count: torch.Tensor
    tokens: torch.Tensor
    lengths: torch.Tensor
    token_frames: torch.Tensor
    scores: torch.Tensor
    logit_scores: torch.Tensor
    hot_scores: torch.Tensor


def max_len() -> int:
    return int(load().sconf_hot_max_len())


def beam_workspace(B: int, N: int, W: int, Kmax: int) -> int:
    n = int(load().sconf_hot_beam_workspace(B, N, W, Kmax))
    if n < 0:
        raise ValueError(f'ctc_beam_hot: invalid sizes B={B} N={N} beam_width={W} max_tokens_per_frame={Kmax}')
    return n


def _chk_image(image, dev, words, what, how):
    if not torch.is_tensor(image) or not image.is_cuda or image.device != dev:
        raise RuntimeError(f'ctc_beam_hot: the {what} image must be a GPU tensor on the device of log_probs ({how})')
    if image.dtype != torch.int32 or image.dim() != 1 or not image.is_contiguous():
        raise TypeError(f'ctc_beam_hot: the {what} image must be a contiguous 1-D int32 tensor, got {image.dtype} {tuple(image.shape)}')
    if image.numel() != words:
        raise ValueError(f'ctc_beam_hot: a {what} image of {image.numel()} words does not hold the sizes given ({words} words)')


def ctc_beam_hot(log_probs: torch.Tensor, input_lengths: Optional[torch.Tensor], lm_image: Optional[torch.Tensor], n_states: int,
                 n_entries: int, num_tokens: int, order: int, start_state: int, hot_image: torch.Tensor, hot_states: int, hot_entries: int,
                 hot_max_len: int, weight: float, blank: int, beam_width: int, nbest: int, token_min_logp: float, beam_prune_logp: float,
                 max_tokens_per_frame: int, max_len: int, alpha: float, beta: float) -> BeamsHot:
    """log_probs (B, N, C) f32, input_lengths (B,) int32 or None (= N), lm_image: the LM's flat int32 buffer on the same device or None
    (then the five integers behind it are 0), hot_image: the hotword set's -> BeamsHot of device tensors.  See include/sconf_hot.h for
    the images and the semantics."""
    B, N, Cn = _chk_log_probs(log_probs, 'ctc_beam_hot')
    if B < 1 or N < 1:
        raise ValueError(f'ctc_beam_hot: empty input B={B} N={N}')
    _chk_lengths(input_lengths, B, 'ctc_beam_hot', 'input_lengths')
    S, E, V = int(n_states), int(n_entries), int(num_tokens)
    if lm_image is None:
        if S or E or V:
            raise ValueError(f'ctc_beam_hot: no LM image, but sizes of {S} states, {E} entries and {V} tokens')
        order = start_state = 0
    else:
        if S < 1 or E < 0 or V < 1:
            raise ValueError(f'ctc_beam_hot: an LM image of {S} states, {E} entries and {V} tokens')
        _chk_image(lm_image, log_probs.device, 4 * S + 4 * E + 2 * V, 'LM', 'NGramLM.to(device)')
    HS, HE = int(hot_states), int(hot_entries)
    if HS < 1 or HE < 0:
        raise ValueError(f'ctc_beam_hot: a hotword image of {HS} states and {HE} entries')
    _chk_image(hot_image, log_probs.device, 6 * HS + 2 * HE, 'hotword', 'HotwordSet.to(device)')
    W, nb, K, L = int(beam_width), int(nbest), int(max_tokens_per_frame), int(max_len)
    if not 1 <= nb <= W or L < 1:
        raise ValueError(f'ctc_beam_hot: nbest={nb} must be in 1..beam_width={W} and max_len={L} at least 1')
    nbytes = beam_workspace(B, N, W, K)
    dev = log_probs.device
    out = BeamsHot(torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, nb, L, dtype=torch.int32, device=dev),
                   torch.empty(B, nb, dtype=torch.int32, device=dev), torch.empty(B, nb, L, dtype=torch.int32, device=dev),
                   torch.empty(B, nb, dtype=torch.float64, device=dev), torch.empty(B, nb, dtype=torch.float64, device=dev),
                   torch.empty(B, nb, dtype=torch.float64, device=dev))
    ws = _workspace(nbytes, dev)
    _lib.call('sconf_hot_beam_ctc', _p(log_probs), _p(input_lengths), _p(lm_image), S, E, V, int(order), int(start_state), _p(hot_image),
              HS, HE, int(hot_max_len), float(weight), _p(out.count), _p(out.tokens), _p(out.lengths), _p(out.token_frames), _p(out.scores),
              _p(out.logit_scores), _p(out.hot_scores), _p(ws), nbytes, B, N, Cn, int(blank), W, nb, float(token_min_logp),
              float(beam_prune_logp), K, L, float(alpha), float(beta), _stream())
    return out
