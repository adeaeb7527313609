"""Posterior token confidences: how sure is the model of a decoded token, measured against the strings it competes with?

The confidences of decoding/confidence.py read the shape of single frames' posteriors.  These read the CTC likelihood itself: for a
hypothesis y of L labels over C classes, the exact likelihood of every string at edit distance 1 - each substitution, each deletion,
each insertion - as a log-likelihood ratio against y.  All of it runs on the GPU (csrc/post.hip through hip/post.py;
include/sconf_post.h holds the definitions, the algorithm and the error contract): the forward and backward rows of y once, then
one serial chain per neighbour, (2 L + 1)(C - 1) of them side by side.

    scores = neighbour_scores(log_probs, tokens, blank)             # loglik, sub_llr (L, C), ins_llr (L + 1, C)
    conf = posterior_confidence(log_probs, tokens, blank)           # per token: posterior, best alternative and its posterior;
                                                                    # per gap: the posterior of "nothing is missing here"
    top = alternatives(scores, 3)                                   # a token-level confusion network around y
    conf = posterior_confidence_long(log_probs, tokens, spans, blank)   # recordings of any length, in pieces

Row i of sub_llr is the unnormalised log-distribution of slot i over C distinct strings: column c is y with y_i replaced by c, column
`blank` is y with y_i deleted, column y_i is y itself (0).  A ratio does not change when a constant is added to a frame's scores, so
logits, log-probabilities and the log of averaged posteriors are all valid input.

Not part of it: neighbours at edit distance 2, n-best or lattice word posteriors, a gradient through these quantities."""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

from ..hip import post as post_kernels            # the HIP op layer (tests swap its three ops for the numpy restatement)
from .confidence import _on_device


class NeighbourScores(NamedTuple):
    """loglik: (B,) f64, log p(y | x) in nats (-inf: no alignment produces y; NaN: invalid input, see include/sconf_post.h).
    sub_llr (B, Smax, C) and ins_llr (B, Smax + 1, C) f32: log p(neighbour) - log p(y); NaN in the slots at and past the sample's
    length, the gaps past it, and throughout a sample whose loglik is not finite.  Without the batch dimension for (N, C) input."""
    loglik: torch.Tensor
    sub_llr: torch.Tensor
    ins_llr: torch.Tensor


class PosteriorConfidence(NamedTuple):
    """token_posterior: softmax(sub_llr row)[y_i]; alternative: the best other column of the row (int32; `blank` means "delete this
    token") and alternative_posterior its softmax.  gap_posterior: softmax(ins_llr row)[blank], the posterior that nothing is missing
    in the gap; gap_alternative: the best insertion, gap_alternative_posterior its softmax.  All on the device, (B, Smax) and
    (B, Smax + 1), without the batch dimension for (N, C) input; NaN / -1 where sub_llr and ins_llr are NaN."""
    token_posterior: torch.Tensor
    alternative: torch.Tensor
    alternative_posterior: torch.Tensor
    gap_posterior: torch.Tensor
    gap_alternative: torch.Tensor
    gap_alternative_posterior: torch.Tensor


def _batch(log_probs, targets, input_lengths, target_lengths, temperature):
    """The five tensors the kernels take, on the device, and whether the input was a single (N, C) sequence."""
    lp = _on_device(log_probs)
    if lp.dim() not in (2, 3):
        raise ValueError(f'log_probs must be (N, C) or (B, N, C), got {tuple(lp.shape)}')
    single = lp.dim() == 2
    lp = (lp[None] if single else lp).float()
    if lp.shape[2] > 1 and lp.stride(2) != 1 or lp.shape[1] > 1 and lp.stride(1) < lp.shape[2] or lp.shape[0] > 1 and lp.stride(0) != lp.shape[1] * lp.stride(1):
        lp = lp.contiguous()
    if temperature is not None:
        t = float(temperature)
        if not (t > 0.0 and t < float('inf')):
            raise ValueError(f'temperature {temperature!r} must be finite and positive')
        lp = lp * (1.0 / t)
    B, N, _ = lp.shape
    if not torch.is_tensor(targets):
        rows = [list(targets)] if single else [list(r) for r in targets]
        if len(rows) != B:
            raise ValueError(f'{len(rows)} transcripts for {B} sequences')
        if target_lengths is None:
            target_lengths = [len(r) for r in rows]
        width = max([len(r) for r in rows] + [0])
        targets = torch.tensor([[int(v) for v in r] + [0] * (width - len(r)) for r in rows], dtype=torch.int32).reshape(B, width)
    tg = _on_device(targets)
    tg = (tg.reshape(1, -1) if single and tg.dim() == 1 else tg).to(torch.int32).contiguous()
    if tg.dim() != 2 or tg.shape[0] != B:
        raise ValueError(f'targets must be (B, Smax) for (B, N, C) scores and (L,) for (N, C) scores, got {tuple(tg.shape)}')
    lengths = []
    for v, dflt in ((input_lengths, N), (target_lengths, tg.shape[1])):
        v = torch.full((B,), dflt, dtype=torch.int32) if v is None else torch.as_tensor(v).reshape(-1)
        if v.shape[0] != B:
            raise ValueError(f'{v.shape[0]} lengths for {B} sequences')
        lengths.append(_on_device(v).to(torch.int32).contiguous())
    return lp, tg, lengths[0], lengths[1], single


def _scores(lp, tg, il, tl, blank) -> NeighbourScores:
    lat = post_kernels.lattice(lp, tg, il, tl, int(blank))
    sub, ins = post_kernels.neighbours(lp, tg, il, tl, int(blank), lat)
    return NeighbourScores(lat.loglik, sub, ins)


def neighbour_scores(log_probs: torch.Tensor, targets, blank: int, input_lengths=None, target_lengths=None,
                     temperature: Optional[float] = None) -> NeighbourScores:
    """log_probs (B, N, C) or (N, C); targets (B, Smax) / (L,) ids (a tensor, a list, or a list of lists of ragged lengths) -> the
    log-likelihood of the transcripts and the ratios of all their neighbours at edit distance 1.  input_lengths / target_lengths:
    per sample, default the whole buffers.  temperature: the scores are divided by it first (in torch).  Two launches."""
    lp, tg, il, tl, single = _batch(log_probs, targets, input_lengths, target_lengths, temperature)
    s = _scores(lp, tg, il, tl, blank)
    return NeighbourScores(s.loglik[0], s.sub_llr[0], s.ins_llr[0]) if single else s


def posterior_confidence(log_probs: torch.Tensor, targets, blank: int, input_lengths=None, target_lengths=None,
                         temperature: Optional[float] = None) -> PosteriorConfidence:
    """The arguments of neighbour_scores -> the posterior of every token among its alternatives and of every gap against the
    insertions into it, with the best alternative of each.  Three launches, nothing copied to the host."""
    lp, tg, il, tl, single = _batch(log_probs, targets, input_lengths, target_lengths, temperature)
    s = _scores(lp, tg, il, tl, blank)
    out = post_kernels.slots(s.sub_llr, s.ins_llr, tg, int(blank))
    return PosteriorConfidence(*(v[0] for v in out)) if single else PosteriorConfidence(*out)


def alternatives(scores: NeighbourScores, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The k most probable strings of every slot: (posterior (..., S, k) f32, column (..., S, k) int64) by torch.topk over the
    softmax of sub_llr's rows, best first.  The columns read as in sub_llr: y_i is the decoded token itself, `blank` its deletion."""
    C = scores.sub_llr.shape[-1]
    if not 1 <= int(k) <= C:
        raise ValueError(f'k = {k} of {C} classes')
    return torch.topk(torch.softmax(scores.sub_llr.float(), dim=-1), int(k), dim=-1)


def cut_pieces(spans: Sequence[Sequence[int]], N: int, max_frames: int, max_labels: int) -> List[Tuple[int, int, int, int]]:
    """The pieces of the long form: [(first token, one past the last token, first frame, one past the last frame)].  Greedy: the
    piece that begins with token k0 at frame f0 takes token k while it would then hold at most max_labels labels and end at most
    max_frames frames behind f0; it ends where the next piece begins, at the midpoint (run_end[k - 1] + start[k]) // 2 of the pause
    in front of the first token k it does not take, and behind the last token of all at N.  A piece takes its first token whatever
    its length.  No tokens: the one piece (0, 0, 0, N)."""
    n = len(spans)
    if n == 0:
        return [(0, 0, 0, int(N))]
    end = [(int(spans[k][1]) + int(spans[k + 1][0])) // 2 for k in range(n - 1)] + [int(N)]
    pieces, k0, f0 = [], 0, 0
    while k0 < n:
        k = k0 + 1
        while k < n and k - k0 + 1 <= max_labels and end[k] - f0 <= max_frames:
            k += 1
        pieces.append((k0, k, f0, end[k - 1]))
        k0, f0 = k, end[k - 1]
    return pieces


def posterior_confidence_long(log_probs: torch.Tensor, tokens: Sequence[int], spans: Sequence[Sequence[int]], blank: int,
                              max_frames: int = 2048, max_labels: Optional[int] = None) -> PosteriorConfidence:
    """posterior_confidence for a recording of any length: log_probs (N, C), tokens its n decoded ids and spans their (start, run_end)
    frames (the first two entries of greedy_confidence's spans or of the forced aligner's).  The recording is cut between tokens
    into pieces of at most max_frames frames and max_labels labels (default and upper limit: the kernels' cap) by `cut_pieces`,
    the pieces are gathered into one padded batch and go through ONE launch of each of the three kernels, and the results are
    concatenated: (n,) token entries and (n + 1,) gap entries.  The gap at a cut is reported from the piece on its left.

    AN APPROXIMATION: every figure is conditioned on the cuts - inside a piece the competing strings are aligned to that piece's
    frames alone, as if the recording were known to pass from one piece's tokens to the next exactly at the cut frame.  A neighbour
    whose best alignment would move a token across a cut is scored without that alignment.  Where the scores left of a cut admit
    only labels that those right of it exclude, the pieces' figures are those of the whole recording."""
    lp = _on_device(log_probs)
    if lp.dim() != 2:
        raise ValueError(f'log_probs must be (N, C), got {tuple(lp.shape)}')
    N = lp.shape[0]
    ids = [int(i) for i in (tokens.tolist() if torch.is_tensor(tokens) else tokens)]
    sp = [[int(v) for v in s[:2]] for s in (spans.tolist() if torch.is_tensor(spans) else spans)]
    if len(sp) != len(ids):
        raise ValueError(f'{len(ids)} tokens but {len(sp)} spans')
    cap = post_kernels.max_labels()
    max_labels = cap if max_labels is None else int(max_labels)
    if not 1 <= max_labels <= cap or max_frames < 1:
        raise ValueError(f'max_labels = {max_labels} must be in 1 .. {cap} and max_frames = {max_frames} at least 1')
    for k, (s, e) in enumerate(sp):
        if not (0 <= s < e <= N and (k == 0 or sp[k - 1][1] <= s)):
            raise ValueError(f'span {k} = ({s}, {e}) is not inside 0 .. {N} behind the span in front of it')
    pieces = cut_pieces(sp, N, int(max_frames), max_labels)
    P = len(pieces)
    frames = max(f1 - f0 for _, _, f0, f1 in pieces)
    width = max(k1 - k0 for k0, k1, _, _ in pieces)
    first = torch.tensor([f0 for _, _, f0, _ in pieces], dtype=torch.int64)
    il = torch.tensor([f1 - f0 for _, _, f0, f1 in pieces], dtype=torch.int32)
    tl = torch.tensor([k1 - k0 for k0, k1, _, _ in pieces], dtype=torch.int32)
    tg = torch.tensor([ids[k0:k1] + [0] * (width - (k1 - k0)) for k0, k1, _, _ in pieces], dtype=torch.int32).reshape(P, width)
    rows = (_on_device(first)[:, None] + torch.arange(frames, device=lp.device)[None]).clamp(max=max(N - 1, 0))
    batch = lp.float()[rows.reshape(-1)].reshape(P, frames, lp.shape[1]) if N else lp.float().new_zeros(P, 0, lp.shape[1])
    il, tl, tg = _on_device(il), _on_device(tl), _on_device(tg)
    s = _scores(batch, tg, il, tl, blank)
    out = post_kernels.slots(s.sub_llr, s.ins_llr, tg, int(blank))
    tok_rows = _on_device(torch.tensor([p * width + k for p, (k0, k1, _, _) in enumerate(pieces) for k in range(k1 - k0)], dtype=torch.int64))
    gap_rows = _on_device(torch.tensor([p * (width + 1) + k for p, (k0, k1, _, _) in enumerate(pieces)
                                        for k in range(0 if p == 0 else 1, k1 - k0 + 1)], dtype=torch.int64))
    return PosteriorConfidence(*(v.reshape(-1)[tok_rows] for v in out[:3]), *(v.reshape(-1)[gap_rows] for v in out[3:]))
