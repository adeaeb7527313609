"""CTC forced alignment: when was each token, and each word, of a known transcript said.

`ctc_forced_align` is what torchaudio.functional.forced_align computes - the most probable frame path that collapses to the
transcript - for batches with ragged lengths, run on the GPU (csrc/align.hip through hip/align.py; include/sconf_align.h holds the
exact contract).  A transcript of more than 8191 labels - a whole recording - goes through the long form of the same contract
(csrc/align_long.hip through hip/align_long.py, include/sconf_align_long.h), up to 65535 labels.  `word_timestamps` turns token spans into the word-level {'word', 'startTime', 'endTime'} records from which the
reference's loader cuts per-chunk targets (lcasr/utils/dataloading.py:28-57)."""
from __future__ import annotations

from typing import Callable, List, NamedTuple, Optional

import torch

from ..hip import align as align_kernels          # the HIP op layer (tests swap align_kernels.ctc_align for the numpy restatement)

SHORT_FORM_LABELS = 8191                           # sconf_align_max_labels(): routing below it needs no library (the tests hold it to the query)


class CTCAlignment(NamedTuple):
    """path, labels (B, N) int32: lattice state and label per frame, -1 past the sample's frames; spans (B, Smax, 2) int32:
    [first frame, one past the last) of each token; token_logp (B, Smax) f32: the token's log-probs summed over its span; score (B)
    f64: the path's log-probability (-inf: the transcript does not fit the frames).  Without the batch dimension for (N, C) input."""
    path: torch.Tensor
    labels: torch.Tensor
    spans: torch.Tensor
    token_logp: torch.Tensor
    score: torch.Tensor


def ctc_forced_align(log_probs: torch.Tensor, targets, input_lengths=None, target_lengths=None, blank: int = 0) -> CTCAlignment:
    """log_probs (N, C) or (B, N, C) log-probabilities; targets (S,) or (B, Smax) token ids (tensor or list); lengths (B,) or None.
    A batch of up to 8191 labels per row runs on the short unit, a wider one of up to 65535 on the long unit; more raises ValueError."""
    single = log_probs.dim() == 2
    if log_probs.dim() not in (2, 3):
        raise ValueError(f'log_probs must be (N, C) or (B, N, C), got {tuple(log_probs.shape)}')
    lp = (log_probs[None] if single else log_probs).float().contiguous()
    dev = lp.device
    tg = torch.as_tensor(targets).to(device=dev, dtype=torch.int32)
    if tg.dim() == 1 and (single or lp.shape[0] == 1):
        tg = tg[None]
    if tg.dim() != 2 or tg.shape[0] != lp.shape[0]:
        raise ValueError(f'targets must be (S,) or (B, Smax) with B = {lp.shape[0]}, got {tuple(tg.shape)}')
    as_len = lambda v: None if v is None else torch.as_tensor(v).reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
    op = align_kernels.ctc_align
    if tg.shape[1] > SHORT_FORM_LABELS:
        from ..hip import align_long as long_kernels  # the sixth ABI unit: bound only when a transcript needs it
        if tg.shape[1] > long_kernels.MAX_LABELS:
            raise ValueError(f'ctc_forced_align: {tg.shape[1]} labels: at most {long_kernels.MAX_LABELS} '
                             f'(a lattice of {2 * long_kernels.MAX_LABELS + 1} states) are supported')
        op = long_kernels.ctc_align
    out = op(lp, tg.contiguous(), as_len(input_lengths), as_len(target_lengths), int(blank))
    return CTCAlignment(*(t[0] for t in out)) if single else CTCAlignment(*out)


def _seconds(x: float) -> str:
    return f'{x:.2f}s'


def word_timestamps(token_ids, spans, tokenizer, seconds_per_frame: float, token_logp=None,
                    word_start: Optional[Callable[[int], bool]] = None) -> List[dict]:
    """Token spans -> [{'word', 'startTime': '12.34s', 'endTime': '12.81s'}], the string forms chunk_text_json parses with
    float(x[:-1]).  token_ids (S,), spans (S, 2) frames [first, one past the last); token_logp (S,) adds 'logp', the mean log-prob
    per frame over the word's tokens.  A token opens a word where word_start(id) says so; else where
    tokenizer.id_to_piece(id) starts with the sentencepiece marker; a tokenizer without id_to_piece makes every token a word,
    spelt tokenizer.decode([id]).  The first token always opens a word."""
    ids = [int(i) for i in (token_ids.tolist() if torch.is_tensor(token_ids) else token_ids)]
    sp = spans.tolist() if torch.is_tensor(spans) else [list(s) for s in spans]
    lps = None if token_logp is None else (token_logp.tolist() if torch.is_tensor(token_logp) else list(token_logp))
    if len(sp) < len(ids) or (lps is not None and len(lps) < len(ids)):
        raise ValueError(f'{len(ids)} tokens but {len(sp)} spans')
    pieces = hasattr(tokenizer, 'id_to_piece')
    if word_start is None:
        word_start = (lambda i: tokenizer.id_to_piece(i).startswith('▁')) if pieces else (lambda i: True)
    groups: List[List[int]] = []
    for k, i in enumerate(ids):
        if k == 0 or word_start(i):
            groups.append([])
        groups[-1].append(k)
    words = []
    for g in groups:
        w = {'word': tokenizer.decode([ids[k] for k in g]).strip(), 'startTime': _seconds(sp[g[0]][0] * seconds_per_frame),
             'endTime': _seconds(sp[g[-1]][1] * seconds_per_frame)}
        if lps is not None:
            frames = sum(sp[k][1] - sp[k][0] for k in g)
            w['logp'] = sum(lps[k] for k in g) / max(frames, 1)
        words.append(w)
    return words
