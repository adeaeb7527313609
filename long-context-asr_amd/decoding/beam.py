"""CTC prefix beam search without a language model: the n best transcripts of a recording, with the frame of every token.

What the reference's evaluation drivers run through pyctcdecode (`build_ctcdecoder(vocab, kenlm_model_path=None, alpha=None,
beta=None)` and `decode_beams`, lcasr/eval/utils.py:14-43), as the textbook two-score prefix search on the GPU (csrc/beam.hip through
hip/beam.py; include/sconf_beam.h holds the exact contract).  Without a language model `lm_score` equals `logit_score`.

With `lm=` (a decoding.lm.NGramLM, token-level) the search is the fused one of include/sconf_lm.h (csrc/beam_lm.hip through
hip/lm.py): every created token adds alpha ln P(token | LM context) + beta to its prefix's ranking key, as pyctcdecode's
`build_ctcdecoder(vocab, kenlm_model_path, alpha, beta)` does per unit.  pyctcdecode's word-level merging, word-level and neural LMs,
hotwords and </s> scoring are not part of it."""
from __future__ import annotations

from typing import Callable, List, NamedTuple, Optional, Tuple

import torch

from ..hip import beam as beam_kernels            # the HIP op layer (tests swap beam_kernels.ctc_beam for the numpy restatement)


class CTCBeams(NamedTuple):
    """count (B) int32: hypotheses returned per sample; tokens, token_frames (B, nbest, max_len) int32: token ids and the frame at
    which each was emitted, -1 behind the hypothesis; lengths (B, nbest) int32: true lengths (also above max_len); scores (B, nbest)
    f64: log-probabilities, best first, -inf behind `count`.  Without the batch dimension for (N, C) input."""
    count: torch.Tensor
    tokens: torch.Tensor
    lengths: torch.Tensor
    token_frames: torch.Tensor
    scores: torch.Tensor


def ctc_beam_search(log_probs: torch.Tensor, input_lengths=None, blank: int = 0, beam_width: int = 100, nbest: int = 1,
                    token_min_logp: float = -5.0, beam_prune_logp: float = -10.0, max_tokens_per_frame: int = 16,
                    max_len: Optional[int] = None) -> CTCBeams:
    """log_probs (N, C) or (B, N, C) log-probabilities on the GPU; input_lengths (B,) or None.  max_len defaults to N.  A class count
    that is not a multiple of 4 is padded with -inf columns (classes that are never kept)."""
    single = log_probs.dim() == 2
    if log_probs.dim() not in (2, 3):
        raise ValueError(f'log_probs must be (N, C) or (B, N, C), got {tuple(log_probs.shape)}')
    lp = (log_probs[None] if single else log_probs).float()
    pad = -lp.shape[-1] % 4
    if pad:
        lp = torch.nn.functional.pad(lp, (0, pad), value=float('-inf'))
    lp = lp.contiguous()
    il = None if input_lengths is None else torch.as_tensor(input_lengths).reshape(-1).to(device=lp.device, dtype=torch.int32).contiguous()
    out = beam_kernels.ctc_beam(lp, il, int(blank), int(beam_width), int(nbest), float(token_min_logp), float(beam_prune_logp),
                                int(max_tokens_per_frame), int(lp.shape[1] if max_len is None else max_len))
    return CTCBeams(*(t[0] for t in out)) if single else CTCBeams(*out)


class CTCBeamsLM(NamedTuple):
    """CTCBeams of a search with a language model: scores are the ranking keys (acoustic log-probability + the LM's bonus), best
    first; logit_scores (B, nbest) f64 the acoustic log-probabilities of the same hypotheses."""
    count: torch.Tensor
    tokens: torch.Tensor
    lengths: torch.Tensor
    token_frames: torch.Tensor
    scores: torch.Tensor
    logit_scores: torch.Tensor


def ctc_beam_search_lm(log_probs: torch.Tensor, lm, alpha: float = 0.5, beta: float = 1.5, input_lengths=None, blank: int = 0,
                       beam_width: int = 100, nbest: int = 1, token_min_logp: float = -5.0, beam_prune_logp: float = -10.0,
                       max_tokens_per_frame: int = 16, max_len: Optional[int] = None) -> CTCBeamsLM:
    """ctc_beam_search with the n-gram LM `lm` (decoding.lm.NGramLM) fused in: a created token adds alpha ln P(token | context) + beta
    to its prefix's key.  The other options, the class padding and the shapes are those of ctc_beam_search."""
    if lm is None:
        raise ValueError('ctc_beam_search_lm needs a language model; ctc_beam_search is the search without one')
    from ..hip import lm as lm_kernels               # the fifth ABI unit: bound only when an LM is used
    single = log_probs.dim() == 2
    if log_probs.dim() not in (2, 3):
        raise ValueError(f'log_probs must be (N, C) or (B, N, C), got {tuple(log_probs.shape)}')
    lp = (log_probs[None] if single else log_probs).float()
    if lm.num_tokens > lp.shape[-1]:
        raise ValueError(f'the LM has {lm.num_tokens} tokens, log_probs have {lp.shape[-1]} classes')
    pad = -lp.shape[-1] % 4
    if pad:
        lp = torch.nn.functional.pad(lp, (0, pad), value=float('-inf'))
    lp = lp.contiguous()
    il = None if input_lengths is None else torch.as_tensor(input_lengths).reshape(-1).to(device=lp.device, dtype=torch.int32).contiguous()
    out = lm_kernels.ctc_beam_lm(lp, il, lm.device_image(lp.device), lm.n_states, lm.n_entries, lm.num_tokens, lm.order, lm.start_state,
                                 int(blank), int(beam_width), int(nbest), float(token_min_logp), float(beam_prune_logp),
                                 int(max_tokens_per_frame), int(lp.shape[1] if max_len is None else max_len), float(alpha), float(beta))
    return CTCBeamsLM(*(t[0] for t in out)) if single else CTCBeamsLM(*out)


class OutputBeam(NamedTuple):
    """One hypothesis, with the field names of pyctcdecode's OutputBeam that the reference's drivers read."""
    text: str
    tokens: List[int]
    logit_score: float
    lm_score: float
    text_frames: List[Tuple[str, Tuple[int, int]]]


def _word_groups(ids: List[int], tokenizer, word_start: Optional[Callable[[int], bool]]) -> List[List[int]]:
    """Positions of the tokens of each word: decoding.align.word_timestamps' grouping rule."""
    if word_start is None:
        pieces = hasattr(tokenizer, 'id_to_piece')
        word_start = (lambda i: tokenizer.id_to_piece(i).startswith('▁')) if pieces else (lambda i: True)
    groups: List[List[int]] = []
    for k, i in enumerate(ids):
        if k == 0 or word_start(i):
            groups.append([])
        groups[-1].append(k)
    return groups


class BeamSearchCTCDecoder(torch.nn.Module):
    """GreedyCTCDecoder's interface over the beam search; `decode_beams` is pyctcdecode's.  Search options (beam_width, nbest,
    token_min_logp, beam_prune_logp, max_tokens_per_frame, max_len) are those of ctc_beam_search; word_start as in word_timestamps.
    lm (a decoding.lm.NGramLM) with alpha, beta: the fused search of ctc_beam_search_lm; lm=None: the search without an LM."""

    def __init__(self, tokenizer=None, blank_id=0, word_start: Optional[Callable[[int], bool]] = None, lm=None, alpha: float = 0.5,
                 beta: float = 1.5, **search_options):
        super().__init__()
        self.tokenizer = tokenizer
        self.blank = blank_id
        self.word_start = word_start
        self.options = dict(search_options)
        self.lm, self.alpha, self.beta = lm, float(alpha), float(beta)

    def _search(self, emission, **override):
        if not torch.is_tensor(emission):
            emission = torch.as_tensor(emission)
        if emission.dim() != 2:
            raise ValueError(f'emission must be (num_seq, num_label), got {tuple(emission.shape)}')
        if not emission.is_cuda and torch.cuda.is_available():
            emission = emission.cuda()                                      # (no GPU: the op layer refuses CPU tensors loudly)
        opts = {**self.options, **{k: v for k, v in override.items() if v is not None}}
        if 'nbest' in opts and 'beam_width' in opts:
            opts['nbest'] = min(opts['nbest'], opts['beam_width'])
        if self.lm is not None:
            return ctc_beam_search_lm(emission, self.lm, self.alpha, self.beta, blank=self.blank, **opts)
        return ctc_beam_search(emission, blank=self.blank, **opts)

    def forward(self, emission: torch.Tensor, decode=True):
        """emission: (num_seq, num_label) log-probs.  Returns the best transcript (tokenizer given and decode=True) or its token ids."""
        decode = decode and self.tokenizer is not None
        out = self._search(emission, nbest=1)
        if int(out.count) == 0:
            ids: List[int] = []
        else:
            n = int(out.lengths[0])
            if n > out.tokens.shape[-1]:
                raise ValueError(f'the best hypothesis has {n} tokens, max_len is {out.tokens.shape[-1]}')
            ids = out.tokens[0, :n].tolist()
        return self.tokenizer.decode(ids) if decode else ids

    def decode_beams(self, logits, beam_width: Optional[int] = None) -> List[OutputBeam]:
        """The hypotheses of `logits` (num_seq, num_label), best first: .text, .tokens, .logit_score (the acoustic log-probability),
        .lm_score (the ranking key: logit_score plus the LM's alpha ln P + beta per token; = logit_score without an LM) and
        .text_frames = [(word, (first frame, last token's frame + 1))]."""
        out = self._search(logits, beam_width=beam_width)
        count, lengths, scores = int(out.count), out.lengths.tolist(), out.scores.tolist()
        logit = out.logit_scores.tolist() if self.lm is not None else scores
        tokens, frames = out.tokens.cpu(), out.token_frames.cpu()
        beams = []
        for r in range(count):
            n = min(lengths[r], tokens.shape[-1])
            ids, fr = tokens[r, :n].tolist(), frames[r, :n].tolist()
            groups = _word_groups(ids, self.tokenizer, self.word_start) if self.tokenizer is not None else [[k] for k in range(n)]
            spell = (lambda g: self.tokenizer.decode([ids[k] for k in g]).strip()) if self.tokenizer is not None else (lambda g: str(ids[g[0]]))
            text_frames = [(spell(g), (fr[g[0]], fr[g[-1]] + 1)) for g in groups]
            text = self.tokenizer.decode(ids) if self.tokenizer is not None else ' '.join(str(i) for i in ids)
            beams.append(OutputBeam(text, ids, logit[r], scores[r], text_frames))
        return beams
