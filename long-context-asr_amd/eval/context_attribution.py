"""Context attribution — the per-recording analysis of eval/bin/run_context_attribution.py:76-127 of the reference, without its square.

The reference cuts the spectrogram into windows of `window_size` frames and, for every pair (i, j), masks window j with its own mean,
runs the whole recording through the model, splices the frames of window i into the clean log-probs, decodes greedily and scores the
transcript against the gold text: W^2 full forwards and W^2 full-length edit distances for a W x (W + 1) matrix of WER * 100 (the last
column is the clean WER).  Here:

  forwards   the masked forward does not depend on i (eval mode, BatchRenorm on its running statistics), so there is one clean forward
             and ceil(W / batch_size) batches of masked copies, each built by ONE launch (hip.ctxattr.mask_fill), reduced to its
             per-frame argmax (ops.argmax_rows) and dropped: (W + 1) x N int32 labels are all that is kept.
  scoring    splicing log-probs and taking the argmax is splicing argmaxes, and hypothesis (i, j) differs from the clean one inside
             window i only: hip.ctxattr.score (include/sconf_ctxattr.h) scores all W^2 pairs against tokenizer.encode(gold_text) at
             the cost of W middles plus two full DPs.

level='token' is that, entirely on the device: units are reference token ids.  level='word' gives the reference's own numbers: the
middles are downloaded, every hypothesis is composed on the host as pre_i + mid_ij + suf_i, decoded, normalised, lower-cased, and
scored against the gold words, one row of W pairs per edit_counts_of_ids launch.  Its cost is W^2 tokenizer decodes on the host.
The reference normalises with Whisper's EnglishTextNormalizer, which is not a dependency of this package: `normalize` defaults to the
identity, as in eval/run.py."""
from __future__ import annotations

import contextlib
from typing import Callable, List, NamedTuple, Optional, Tuple

import torch

from .. import functional as Fn          # Fn.ops: the HIP op layer (tests swap it for the CPU kernel references)
from ..hip import ctxattr as kernels
from .run import _Args, _evaluation_mode
from .wer import edit_counts_of_ids

EVALUATION_MODES = ('windowed_attention', 'full')


class ContextAttribution(NamedTuple):
    """wer_matrix (W, W + 1) float32: errors / units * 100, entry (i, j) for window i scored with window j masked, the clean figure in
    the last column (the reference's wer_matrix).  errors (W, W + 1) int64 and units: what it was computed from.  windows: the
    (start, end) spectrogram frames; frame_windows: the (f, g) model frames; frame_labels (W + 1, N) int32: the per-frame argmax of the
    W masked forwards and, last, of the clean one; unharmed: the clean transcript; transcripts: the W x W texts, on request."""
    wer_matrix: torch.Tensor
    errors: torch.Tensor
    units: int
    windows: List[Tuple[int, int]]
    frame_windows: List[Tuple[int, int]]
    frame_labels: torch.Tensor
    unharmed: str
    transcripts: Optional[List[List[str]]]


def attribution_windows(spec_n: int, logits_n: int, window_size: int) -> Tuple[List[Tuple[int, int]], List[Tuple[int, int]]]:
    """(windows, frame_windows) exactly as the reference computes them (lines 80-87), Python floats included."""
    windows = [(i, min(i + window_size, spec_n)) for i in range(0, spec_n, window_size)]
    downsampled_by = spec_n / logits_n
    return windows, [(int(start / downsampled_by), int(end / downsampled_by)) for start, end in windows]


def _collapse(labels: List[int], blank: int, prev: Optional[int] = None) -> List[int]:
    out = []
    for a in labels:
        if a != blank and a != prev: out.append(a)
        prev = a
    return out


def _frame_labels(model, x: torch.Tensor) -> torch.Tensor:
    """(b, F, T) -> (b, N) int32: the per-frame argmax of one forward; the posteriors are dropped here."""
    lp = model(x)['final_posteriors'].float().contiguous()
    return Fn.ops.argmax_rows(lp).reshape(lp.shape[0], lp.shape[1])


@torch.no_grad()
def context_attribution(model, spec: torch.Tensor, gold_text: str, tokenizer, seq_len: int, window_size: int = 2048, level: str = 'token',
                        normalize: Optional[Callable[[str], str]] = None, batch_size: int = 4,
                        evaluation_mode: str = 'windowed_attention', args=None, return_transcripts: bool = False) -> ContextAttribution:
    """The context-attribution matrix of one recording spec (1, F, T).  evaluation_mode 'windowed_attention': every attention module
    limited to seq_len // subsampling_factor // 2 tokens to either side and the whole recording in one forward, as the reference;
    'full': the modules' windows left alone.  level 'token' or 'word' (see the module text; 'word' costs W^2 tokenizer decodes on the
    host).  Raises ValueError for an empty reference, more than 65535 reference ids, or a window of more model frames than
    hip.ctxattr.max_window_frames() - 1."""
    if spec.dim() != 3 or spec.shape[0] != 1:
        raise ValueError(f'spec must be (1, features, time), got {tuple(spec.shape)}')
    if level not in ('token', 'word'):
        raise ValueError(f"level must be 'token' or 'word', got {level!r}")
    if evaluation_mode not in EVALUATION_MODES:
        raise ValueError(f'evaluation_mode must be one of {EVALUATION_MODES}, got {evaluation_mode!r}')
    if window_size < 1 or batch_size < 1:
        raise ValueError(f'window_size and batch_size must be at least 1, got {window_size} and {batch_size}')
    args = _Args() if args is None else args
    normalize = (lambda s: s) if normalize is None else normalize
    blank = model.decoder.num_classes - 1
    ref_ids = [int(i) for i in tokenizer.encode(gold_text)]
    gold_words = gold_text.split()
    if not ref_ids or (level == 'word' and not gold_words):
        raise ValueError('context_attribution: the reference is empty')
    if len(ref_ids) > kernels.MAX_REF:
        raise ValueError(f'context_attribution: {len(ref_ids)} reference ids: at most {kernels.MAX_REF} are supported')

    dev = next(model.parameters()).device
    spec2 = spec[0].to(dev).float().contiguous()
    T = spec2.shape[1]
    windows = [(i, min(i + window_size, T)) for i in range(0, T, window_size)]
    W = len(windows)
    win_dev = torch.tensor(windows, dtype=torch.int32).to(dev)
    # 'full' is not a mode of eval.run: nothing to set, nothing to restore
    with (_evaluation_mode(model, evaluation_mode, seq_len, args) if evaluation_mode == 'windowed_attention' else contextlib.nullcontext()):
        clean = _frame_labels(model, spec2[None])[0]
        N = clean.shape[0]
        windows, frame_windows = attribution_windows(T, N, window_size)
        widest = max(g - f for f, g in frame_windows) + 1
        if widest > kernels.MAX_WINDOW_FRAMES:
            raise ValueError(f'context_attribution: a window of {widest - 1} model frames: at most {kernels.MAX_WINDOW_FRAMES - 1} are supported '
                             f'(window_size {window_size})')
        means = kernels.window_means(spec2, win_dev)
        rows = []
        for j0 in range(0, W, batch_size):
            rows.append(_frame_labels(model, kernels.mask_fill(spec2, win_dev, means, j0, min(batch_size, W - j0))))
    masked = torch.cat(rows, 0).contiguous()
    frame_labels = torch.cat([masked, clean[None]], 0)

    ref = torch.tensor(ref_ids, dtype=torch.int32).to(dev)
    need_text = level == 'word' or return_transcripts
    sc = kernels.score(clean, masked, ref, frame_windows, blank, with_tokens=need_text)
    clean_list = clean.cpu().tolist()
    unharmed = normalize(tokenizer.decode(_collapse(clean_list, blank))).lower()
    transcripts = None
    if need_text:
        mid_len, mid_tokens = sc.mid_len.cpu().tolist(), sc.mid_tokens.cpu()
        transcripts, hyps = [], []
        for i, (f, g) in enumerate(frame_windows):
            ge = min(g + 1, N)
            pre = _collapse(clean_list[:f], blank)
            suf = _collapse(clean_list[ge:], blank, clean_list[ge - 1] if ge > 0 else None)
            hyps.append([pre + mid_tokens[i, j, :mid_len[i][j]].tolist() + suf for j in range(W)])
            transcripts.append([normalize(tokenizer.decode(h)).lower() for h in hyps[-1]])
    if level == 'token':
        units = len(ref_ids)
        errors = torch.cat([sc.errors, sc.clean_errors.expand(W)[:, None]], 1).cpu().to(torch.int64)
    else:
        units = len(gold_words)
        ids: dict = {}
        gold = [ids.setdefault(w, len(ids)) for w in gold_words]
        as_ids = lambda text: [ids.setdefault(w, len(ids)) for w in text.split()]
        errors = torch.zeros(W, W + 1, dtype=torch.int64)
        for i in range(W):                                     # one row of W pairs per launch
            errors[i, :W] = edit_counts_of_ids([as_ids(t) for t in transcripts[i]], [gold] * W)[:, 0]
        errors[:, W] = edit_counts_of_ids([as_ids(unharmed)], [gold])[0, 0]
    wer_matrix = (errors.double() / units * 100).float()
    return ContextAttribution(wer_matrix, errors, units, windows, frame_windows, frame_labels, unharmed,
                              transcripts if return_transcripts else None)
