"""CTC prefix beam search without a language model: the n best transcripts of a recording, with the frame of every token.

What the reference's evaluation drivers run through pyctcdecode (`build_ctcdecoder(vocab, kenlm_model_path=None, alpha=None,
beta=None)` and `decode_beams`, lcasr/eval/utils.py:14-43), as the textbook two-score prefix search on the GPU (csrc/beam.hip through
hip/beam.py; include/sconf_beam.h holds the exact contract).  Without a language model `lm_score` equals `logit_score`.

With `lm=` (a decoding.lm.NGramLM, token-level) the search is the fused one of include/sconf_lm.h (csrc/beam_lm.hip through
hip/lm.py): every created token adds alpha ln P(token | LM context) + beta to its prefix's ranking key, as pyctcdecode's
`build_ctcdecoder(vocab, kenlm_model_path, alpha, beta)` does per unit.

With `hotwords=` (a decoding.hotwords.HotwordSet, phrases as token sequences) the search is the boosted one of include/sconf_hot.h
(csrc/beam_hot.hip through hip/hot.py), with or without an LM: every finished hotword adds hotword_weight times its relative weight
to its prefix's key, and a hotword in progress holds its partial credit while it keeps matching - pyctcdecode's
`decode_beams(..., hotwords=[...], hotword_weight=10.0)`, acting INSIDE the search.  `token_min_logp` still decides which tokens a
frame proposes: a hotword whose pieces fall below it is never proposed, so lower `token_min_logp` when boosting rare words.

pyctcdecode's word-level merging, word-level and neural LMs, hotword matching on decoded text and </s> scoring are not part of it."""
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


class CTCBeamsHot(NamedTuple):
    """CTCBeamsLM of a search with hotwords: scores are the ranking keys (acoustic log-probability + the LM's bonus + the hotword
    credit), best first; hot_scores (B, nbest) f64 the hotword credit of the same hypotheses (hotword_weight times the relative
    weights of every hotword occurrence in the transcript)."""
    count: torch.Tensor
    tokens: torch.Tensor
    lengths: torch.Tensor
    token_frames: torch.Tensor
    scores: torch.Tensor
    logit_scores: torch.Tensor
    hot_scores: torch.Tensor


def ctc_beam_search_hot(log_probs: torch.Tensor, hotwords, hotword_weight: float = 10.0, lm=None, alpha: float = 0.5, beta: float = 1.5,
                        input_lengths=None, blank: int = 0, beam_width: int = 100, nbest: int = 1, token_min_logp: float = -5.0,
                        beam_prune_logp: float = -10.0, max_tokens_per_frame: int = 16, max_len: Optional[int] = None) -> CTCBeamsHot:
    """ctc_beam_search with the hotwords `hotwords` (decoding.hotwords.HotwordSet) boosted inside the search, and the n-gram LM `lm`
    fused in if one is given (without one alpha and beta are not used).  A created token that finishes a hotword adds hotword_weight
    times the phrase's relative weight to its prefix's key for good; a prefix in the middle of a hotword holds hotword_weight times
    (tokens matched / tokens of the shortest matching phrase) until it stops matching, and nothing of it at the end.
    token_min_logp is unchanged: a hotword whose pieces fall below it in a frame is never proposed there - lower it when boosting
    rare words.  The other options, the class padding and the shapes are those of ctc_beam_search."""
    if hotwords is None:
        raise ValueError('ctc_beam_search_hot needs a HotwordSet; ctc_beam_search / ctc_beam_search_lm are the searches without one')
    from ..hip import hot as hot_kernels             # the eleventh ABI unit: bound only when hotwords are used
    single = log_probs.dim() == 2
    if log_probs.dim() not in (2, 3):
        raise ValueError(f'log_probs must be (N, C) or (B, N, C), got {tuple(log_probs.shape)}')
    weight = float(hotword_weight)
    if not (weight >= 0.0 and weight < float('inf')):
        raise ValueError(f'hotword_weight must be finite and >= 0, got {hotword_weight}')
    lp = (log_probs[None] if single else log_probs).float()
    if lm is not None and lm.num_tokens > lp.shape[-1]:
        raise ValueError(f'the LM has {lm.num_tokens} tokens, log_probs have {lp.shape[-1]} classes')
    hotwords.validate(blank=int(blank), num_classes=lp.shape[-1])
    pad = -lp.shape[-1] % 4
    if pad:
        lp = torch.nn.functional.pad(lp, (0, pad), value=float('-inf'))
    lp = lp.contiguous()
    il = None if input_lengths is None else torch.as_tensor(input_lengths).reshape(-1).to(device=lp.device, dtype=torch.int32).contiguous()
    lm_args = (None, 0, 0, 0, 0, 0) if lm is None else (lm.device_image(lp.device), lm.n_states, lm.n_entries, lm.num_tokens, lm.order,
                                                        lm.start_state)
    out = hot_kernels.ctc_beam_hot(lp, il, *lm_args, hotwords.device_image(lp.device), hotwords.n_states, hotwords.n_entries,
                                   hotwords.max_len, weight, int(blank), int(beam_width), int(nbest), float(token_min_logp),
                                   float(beam_prune_logp), int(max_tokens_per_frame), int(lp.shape[1] if max_len is None else max_len),
                                   float(alpha), float(beta))
    return CTCBeamsHot(*(t[0] for t in out)) if single else CTCBeamsHot(*out)


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
    lm (a decoding.lm.NGramLM) with alpha, beta: the fused search of ctc_beam_search_lm; lm=None: the search without an LM.
    hotwords (a list of strings, encoded with the tokenizer, or a decoding.hotwords.HotwordSet) with hotword_weight: the defaults of
    every call, boosted inside the search (ctc_beam_search_hot); hotwords=None: the search of today.  Sets compiled from strings are
    cached per tuple of strings, the HOTWORD_SETS_KEPT most recently used ones (with their device images)."""

    HOTWORD_SETS_KEPT = 16

    def __init__(self, tokenizer=None, blank_id=0, word_start: Optional[Callable[[int], bool]] = None, lm=None, alpha: float = 0.5,
                 beta: float = 1.5, hotwords=None, hotword_weight: float = 10.0, **search_options):
        super().__init__()
        self.tokenizer = tokenizer
        self.blank = blank_id
        self.word_start = word_start
        self.options = dict(search_options)
        self.lm, self.alpha, self.beta = lm, float(alpha), float(beta)
        self.hotwords, self.hotword_weight = hotwords, float(hotword_weight)
        self._hotword_sets = {}                         # tuple of strings -> its compiled HotwordSet, least recently used first

    def _hotword_set(self, hotwords):
        """A HotwordSet as it is; a sequence of strings compiled with the tokenizer, once per tuple of strings."""
        if hotwords is None or hasattr(hotwords, 'device_image'):
            return hotwords
        if isinstance(hotwords, str):
            raise TypeError('hotwords must be a list of strings or a HotwordSet, not one string')
        key = tuple(hotwords)
        if not key:
            return None
        if not all(isinstance(w, str) for w in key):
            raise TypeError('hotwords must be a list of strings or a HotwordSet (token-id phrases go through HotwordSet(phrases))')
        if self.tokenizer is None:
            raise ValueError('hotwords given as strings need the tokenizer; without one pass a HotwordSet of token-id phrases')
        hot = self._hotword_sets.pop(key, None)          # (taken out and put back last: the dict's order is the order of use)
        if hot is None:
            from .hotwords import HotwordSet
            hot = HotwordSet.from_text(key, self.tokenizer)
        self._hotword_sets[key] = hot
        while len(self._hotword_sets) > self.HOTWORD_SETS_KEPT:            # per-utterance lists must not grow the decoder for good
            del self._hotword_sets[next(iter(self._hotword_sets))]
        return hot

    def _search(self, emission, hotwords=None, hotword_weight=None, **override):
        if not torch.is_tensor(emission):
            emission = torch.as_tensor(emission)
        if emission.dim() != 2:
            raise ValueError(f'emission must be (num_seq, num_label), got {tuple(emission.shape)}')
        if not emission.is_cuda and torch.cuda.is_available():
            emission = emission.cuda()                                      # (no GPU: the op layer refuses CPU tensors loudly)
        opts = {**self.options, **{k: v for k, v in override.items() if v is not None}}
        if 'nbest' in opts and 'beam_width' in opts:
            opts['nbest'] = min(opts['nbest'], opts['beam_width'])
        hot = self._hotword_set(self.hotwords if hotwords is None else hotwords)
        if hot is not None:
            weight = self.hotword_weight if hotword_weight is None else float(hotword_weight)
            return ctc_beam_search_hot(emission, hot, weight, self.lm, self.alpha, self.beta, blank=self.blank, **opts)
        if self.lm is not None:
            return ctc_beam_search_lm(emission, self.lm, self.alpha, self.beta, blank=self.blank, **opts)
        return ctc_beam_search(emission, blank=self.blank, **opts)

    def forward(self, emission: torch.Tensor, decode=True, hotwords=None, hotword_weight: Optional[float] = None):
        """emission: (num_seq, num_label) log-probs.  Returns the best transcript (tokenizer given and decode=True) or its token ids.
        hotwords / hotword_weight: as decode_beams; None: the constructor's."""
        decode = decode and self.tokenizer is not None
        out = self._search(emission, hotwords=hotwords, hotword_weight=hotword_weight, nbest=1)
        if int(out.count) == 0:
            ids: List[int] = []
        else:
            n = int(out.lengths[0])
            if n > out.tokens.shape[-1]:
                raise ValueError(f'the best hypothesis has {n} tokens, max_len is {out.tokens.shape[-1]}')
            ids = out.tokens[0, :n].tolist()
        return self.tokenizer.decode(ids) if decode else ids

    def decode_beams(self, logits, beam_width: Optional[int] = None, hotwords=None, hotword_weight: Optional[float] = None) -> List[OutputBeam]:
        """The hypotheses of `logits` (num_seq, num_label), best first: .text, .tokens, .logit_score (the acoustic log-probability),
        .lm_score (the ranking key: logit_score plus the LM's alpha ln P + beta per token and the hotword credit; = logit_score
        without an LM and hotwords) and .text_frames = [(word, (first frame, last token's frame + 1))].
        hotwords: pyctcdecode's keyword - a list of strings (encoded with the tokenizer; compiled sets are cached per tuple of strings)
        or a decoding.hotwords.HotwordSet - with hotword_weight (pyctcdecode's default 10.0); None: the constructor's."""
        out = self._search(logits, hotwords=hotwords, hotword_weight=hotword_weight, beam_width=beam_width)
        count, lengths, scores = int(out.count), out.lengths.tolist(), out.scores.tolist()
        logit = out.logit_scores.tolist() if hasattr(out, 'logit_scores') else scores
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
