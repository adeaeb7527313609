"""CTC segmentation: a loose transcript - a list of utterances with unknown times, which may skip intros, music, adverts and
cross-talk, and may hold utterances that were never said - becomes utterances with times and a confidence each.

The tool of Kürzinger et al. 2020 (the `ctc-segmentation` package, ESPnet's and NeMo's aligners built on it) and of
torchaudio.functional.forced_align with a <star> token, run on the GPU (csrc/seg.hip through hip/seg.py; include/sconf_seg.h holds
the exact contract).  Two parts:

  * `ctc_forced_align_star`: forced alignment in which the STAR label, id `star_id(num_classes)` = the first id past the classes,
    absorbs any audio.  Its emission is `star_logp` at every frame.
  * `ctc_segment`: the star row `[*] u0 [*] u1 ... [*]` of a list of utterances (`build_targets`), its alignment, and per utterance
    the frames it covers, its mean log-probability per frame and its confidence: the lowest mean over any `window` consecutive frames
    of it (Kürzinger's rule: an utterance is as good as its worst stretch, so one wrong word sinks it while the mean hardly moves).
    window = 30 frames is their `score_min_mean_over_L`; it is adopted here, not tuned.

What a star does, and does not:
  * A star always takes at least one frame: it is a label.  Two adjacent stars are a repeat and need a blank frame between them.
  * star_logp = 0 (the default, torchaudio's choice) makes the star free, so it also takes the frames of its neighbours that cost
    anything at all: a token next to a star shrinks towards one frame.  That is torchaudio's behaviour too.
  * A negative star_logp makes a star win only over frames that match nothing in the transcript: on the planted case of
    tests/test_seg.py, -1.0 recovers exactly the planted spans and 0.0 does not.
  * No value has been tuned on real recordings here; the default stays 0.0.

Nothing here loops over frames or tokens on the host: the only host loop is over the utterances of the list, to lay out the row."""
from __future__ import annotations

from typing import List, NamedTuple, Sequence, Tuple

import torch

from ..hip import seg as seg_kernels              # the HIP op layer (tests swap seg_kernels.align / .score for the numpy restatement)
from .align import CTCAlignment

MAX_LABELS = seg_kernels.MAX_LABELS


class CTCSegmentation(NamedTuple):
    """alignment: the CTCAlignment of the star row; frame_logp (B, N) f32: the emission of the path's state per frame; utt_frames
    (B, Umax, 2) int32: [first frame, one past the last) of each utterance; utt_logp, utt_conf (B, Umax) f32: its mean log-prob per
    frame and its lowest windowed mean.  Rows past a sample's utterances hold (-1, -1), 0, 0; an utterance of a sample whose
    transcript does not fit holds (-1, -1), NaN, NaN.  Without the batch dimension for (N, C) input."""
    alignment: CTCAlignment
    frame_logp: torch.Tensor
    utt_frames: torch.Tensor
    utt_logp: torch.Tensor
    utt_conf: torch.Tensor


def star_id(num_classes: int) -> int:
    """The star's label: the first id past the classes (sconf_seg_star_label)."""
    if num_classes < 1:
        raise ValueError(f'star_id: {num_classes} classes')
    return int(num_classes)


def build_targets(utterances: Sequence[Sequence[int]], star: int, star_between: bool = True,
                  star_ends: bool = True) -> Tuple[List[int], List[Tuple[int, int]]]:
    """The target row `[*] u0 [*] u1 ... [*]` of a list of utterances (each a list of token ids) and each utterance's token range
    [j0, j1) in it.  star_ends: a star before the first and after the last utterance; star_between: one between two utterances.  An
    empty utterance raises ValueError (it has no frames to score)."""
    row: List[int] = []
    ranges: List[Tuple[int, int]] = []
    for k, u in enumerate(utterances):
        ids = [int(i) for i in u]
        if not ids:
            raise ValueError(f'build_targets: utterance {k} is empty')
        if (k == 0 and star_ends) or (k > 0 and star_between):
            row.append(int(star))
        ranges.append((len(row), len(row) + len(ids)))
        row.extend(ids)
    if star_ends and ranges:
        row.append(int(star))
    return row, ranges


def _as_len(v, dev):
    return None if v is None else torch.as_tensor(v).reshape(-1).to(device=dev, dtype=torch.int32).contiguous()


def _star_align(lp: torch.Tensor, tg: torch.Tensor, input_lengths, target_lengths, blank: int, star_logp: float):
    if tg.shape[1] > MAX_LABELS:
        raise ValueError(f'ctc_forced_align_star: {tg.shape[1]} labels: at most {MAX_LABELS} (a lattice of {2 * MAX_LABELS + 1} states) '
                         f'are supported')
    return seg_kernels.align(lp, tg.contiguous(), input_lengths, target_lengths, int(blank), float(star_logp))


def ctc_forced_align_star(log_probs: torch.Tensor, targets, input_lengths=None, target_lengths=None, blank: int = 0,
                          star_logp: float = 0.0) -> CTCAlignment:
    """`ctc_forced_align` for targets that may hold the star label `star_id(C)`: log_probs (N, C) or (B, N, C); targets (S,) or
    (B, Smax) token ids (tensor or list); lengths (B,) or None.  Up to 65535 labels per row, stars included; more raises ValueError.
    Targets without a star give the bits of `ctc_forced_align`.  See the module docstring for what star_logp does."""
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
    out = _star_align(lp, tg, _as_len(input_lengths, dev), _as_len(target_lengths, dev), blank, star_logp)[:5]
    return CTCAlignment(*(t[0] for t in out)) if single else CTCAlignment(*out)


def ctc_segment(log_probs: torch.Tensor, utterances, blank: int, star_between: bool = True, star_ends: bool = True,
                star_logp: float = 0.0, window: int = 30) -> CTCSegmentation:
    """log_probs (N, C) with `utterances` a list of token-id lists, or (B, N, C) with one such list per sample -> CTCSegmentation.
    Every sample is aligned over all N frames.  See the module docstring for the stars, star_logp and window."""
    single = log_probs.dim() == 2
    if log_probs.dim() not in (2, 3):
        raise ValueError(f'log_probs must be (N, C) or (B, N, C), got {tuple(log_probs.shape)}')
    lp = (log_probs[None] if single else log_probs).float().contiguous()
    per_sample = [utterances] if single else list(utterances)
    if len(per_sample) != lp.shape[0]:
        raise ValueError(f'{lp.shape[0]} samples but {len(per_sample)} lists of utterances')
    dev, star = lp.device, star_id(lp.shape[2])
    built = [build_targets(u, star, star_between, star_ends) for u in per_sample]
    Smax, Umax = max(len(r) for r, _ in built), max(len(g) for _, g in built)
    tg = torch.tensor([r + [0] * (Smax - len(r)) for r, _ in built], dtype=torch.int32).reshape(len(built), Smax).to(dev)
    utt = torch.tensor([[list(x) for x in g] + [[0, 0]] * (Umax - len(g)) for _, g in built], dtype=torch.int32).reshape(len(built), Umax, 2).to(dev)
    tg_len = torch.tensor([len(r) for r, _ in built], dtype=torch.int32).to(dev)
    counts = torch.tensor([len(g) for _, g in built], dtype=torch.int32).to(dev)
    al = _star_align(lp, tg, None, tg_len, blank, star_logp)
    sc = seg_kernels.score(al[2], al[5], al[4], None, tg_len, utt, counts, int(window))
    out = CTCSegmentation(CTCAlignment(*al[:5]), al[5], *sc)
    if single:
        return CTCSegmentation(CTCAlignment(*(t[0] for t in out.alignment)), *(t[0] for t in out[1:]))
    return out
