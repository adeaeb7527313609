"""Word / character error rate — mirror of lcasr/eval/wer.py:5-73 (`word_error_rate_detail`) without jiwer.

The reference hands every pair to jiwer.  Here all pairs of a call are scored by ONE launch of the edit-count kernel
(csrc/editdist.hip, ops.edit_counts): one upload of the id arrays, one launch, one download of (P, 4) integers.

Contract of the counts (jiwer is not a dependency of this package and could not be run against it): `errors` is the unit-cost
Levenshtein distance, on which every correct implementation agrees, so the WER itself is the reference's.  The split into
substitutions / deletions / insertions is that of the optimal alignment with the FEWEST substitutions; it is unique, because
every alignment has ins - del = len(hyp) - len(ref) and sub + del + ins = errors.  jiwer takes its split from one backtrace
(RapidFuzz `editops`), which may walk another, equally optimal alignment: its three rates can differ from these, their sum cannot.

`use_cer=True` follows jiwer's DOCUMENTED default character transform (strip both ends, then every remaining character is a
token, inner spaces included); `words` counts len(list(reference)) exactly as the reference function does."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

from .. import functional as Fn          # Fn.ops: the HIP op layer (tests swap it for the CPU kernel references)
from ..hip import calib as calib_kernels  # the alignment kernel (tests swap its ops for the numpy restatement)


def _device():
    return torch.device('cuda' if torch.cuda.is_available() else 'cpu')     # (no GPU: the op layer refuses CPU tensors loudly)


def _ragged(seqs: Sequence[Sequence[int]], device) -> Tuple[torch.Tensor, torch.Tensor]:
    flat = [i for s in seqs for i in s]
    off = [0]
    for s in seqs:
        off.append(off[-1] + len(s))
    return torch.tensor(flat, dtype=torch.int32).to(device), torch.tensor(off, dtype=torch.int64).to(device)


def edit_counts_of_ids(hyps: Sequence[Sequence[int]], refs: Sequence[Sequence[int]]) -> torch.Tensor:
    """(P,4) int64 [errors, substitutions, deletions, insertions] on the host for P pairs of id lists: one launch."""
    if len(hyps) != len(refs):
        raise ValueError(f'need as many hypotheses as references, got {len(hyps)} and {len(refs)}')
    if len(hyps) == 0:
        return torch.zeros(0, 4, dtype=torch.int64)
    dev = _device()
    h, ho = _ragged(hyps, dev)
    r, ro = _ragged(refs, dev)
    return Fn.ops.edit_counts(h, ho, r, ro).cpu()


def word_error_rate_detail(hypotheses: List[str], references: List[str], use_cer=False) -> Tuple[float, int, float, float, float]:
    """(wer, words, ins_rate, del_rate, sub_rate) over all pairs, as lcasr.eval.wer.word_error_rate_detail.

    Words are str.split() tokens (characters with use_cer), mapped to int32 ids through one dictionary over both lists.  An empty
    reference counts its hypothesis tokens as insertions; with no reference tokens at all the four rates are inf."""
    if len(hypotheses) != len(references):
        raise ValueError(
            "In word error rate calculation, hypotheses and reference"
            " lists must have the same number of elements. But I got:"
            "{0} and {1} correspondingly".format(len(hypotheses), len(references))
        )
    ids: dict = {}
    hyps, refs, words = [], [], 0
    for h, r in zip(hypotheses, references):
        if use_cer:
            words += len(list(r))
            h_list, r_list = (list(h.strip()), list(r.strip())) if len(list(r)) != 0 else (list(h), [])
        else:
            h_list, r_list = h.split(), r.split()
            words += len(r_list)
        hyps.append([ids.setdefault(t, len(ids)) for t in h_list])
        refs.append([ids.setdefault(t, len(ids)) for t in r_list])
    if words == 0:
        return float('inf'), words, float('inf'), float('inf'), float('inf')
    errors, subs, dels, ins = (int(v) for v in edit_counts_of_ids(hyps, refs).sum(0))
    assert errors == subs + dels + ins
    return 1.0 * errors / words, words, 1.0 * ins / words, 1.0 * dels / words, 1.0 * subs / words


def _tokens(h: str, r: str, use_cer: bool) -> Tuple[list, list]:
    """The tokens of one pair, exactly as word_error_rate_detail cuts them."""
    if use_cer:
        return (list(h.strip()), list(r.strip())) if len(list(r)) != 0 else (list(h), [])
    return h.split(), r.split()


def edit_alignment_on_device(hyps: Sequence[Sequence[int]], refs: Sequence[Sequence[int]]):
    """P pairs of id lists -> (hyp, hyp_off, ref, ref_off, hyp_to_ref, ref_to_hyp, counts), flat tensors on the device as
    include/sconf_calib.h lays them out: one upload, one launch of the alignment kernel (csrc/calib.hip), nothing read back.  Every
    pair's slice of the workspace is sized from the host lengths, so no pair comes back refused."""
    if len(hyps) != len(refs):
        raise ValueError(f'need as many hypotheses as references, got {len(hyps)} and {len(refs)}')
    dev = _device()
    h, ho = _ragged(hyps, dev)
    r, ro = _ragged(refs, dev)
    off = calib_kernels.workspace_offsets([len(s) for s in hyps], [len(s) for s in refs])
    ws = torch.empty(off[-1], dtype=torch.uint8, device=dev) if off[-1] else None
    h2r, r2h, counts = calib_kernels.edit_align(h, ho, r, ro, torch.tensor(off, dtype=torch.int64).to(dev), ws)
    return h, ho, r, ro, h2r, r2h, counts


def edit_alignment_of_ids(hyps: Sequence[Sequence[int]], refs: Sequence[Sequence[int]]) -> List[Tuple[List[int], List[int], List[int]]]:
    """Per pair (hyp_to_ref, ref_to_hyp, counts) on the host: for every hypothesis id the index of the reference id it is aligned to
    (-1: an insertion), for every reference id the index of its hypothesis id (-1: a deletion), and [errors, substitutions,
    deletions, insertions] as edit_counts_of_ids gives them.  The alignment is the unique one of include/sconf_calib.h: fewest
    errors, among those fewest substitutions, among those the backtrace's order diagonal, up, left."""
    if len(hyps) == 0 and len(refs) == 0:
        return []
    _, _, _, _, h2r, r2h, counts = edit_alignment_on_device(hyps, refs)
    h2r, r2h, counts = h2r.cpu().tolist(), r2h.cpu().tolist(), counts.cpu().tolist()
    out, a, b = [], 0, 0
    for p, (hs, rs) in enumerate(zip(hyps, refs)):
        out.append((h2r[a:a + len(hs)], r2h[b:b + len(rs)], counts[p]))
        a, b = a + len(hs), b + len(rs)
    return out


def word_error_alignment(hypotheses: List[str], references: List[str], use_cer=False) -> List[List[dict]]:
    """The error listing behind word_error_rate_detail: per pair a list of {'op': 'hit' | 'sub' | 'ins' | 'del', 'hyp', 'ref',
    'hyp_index', 'ref_index'} (the word and its position on each side, None on the side an insertion or a deletion lacks), in
    reference order with every insertion placed before the next aligned reference word.  Tokens are cut exactly as
    word_error_rate_detail cuts them; all pairs are aligned by one launch (edit_alignment_of_ids)."""
    if len(hypotheses) != len(references):
        raise ValueError(f'need as many hypotheses as references, got {len(hypotheses)} and {len(references)}')
    ids: dict = {}
    words, hyps, refs = [], [], []
    for h, r in zip(hypotheses, references):
        h_list, r_list = _tokens(h, r, use_cer)
        words.append((h_list, r_list))
        hyps.append([ids.setdefault(t, len(ids)) for t in h_list])
        refs.append([ids.setdefault(t, len(ids)) for t in r_list])
    out = []
    for (h_list, r_list), (h2r, r2h, _) in zip(words, edit_alignment_of_ids(hyps, refs)):
        ops, i = [], 0

        def insertions(upto):
            nonlocal i
            while i < upto:
                if h2r[i] < 0:
                    ops.append({'op': 'ins', 'hyp': h_list[i], 'ref': None, 'hyp_index': i, 'ref_index': None})
                i += 1

        for j, a in enumerate(r2h):
            if a < 0:
                ops.append({'op': 'del', 'hyp': None, 'ref': r_list[j], 'hyp_index': None, 'ref_index': j})
                continue
            insertions(a)
            ops.append({'op': 'hit' if h_list[a] == r_list[j] else 'sub', 'hyp': h_list[a], 'ref': r_list[j], 'hyp_index': a, 'ref_index': j})
            i = a + 1
        insertions(len(h_list))
        out.append(ops)
    return out


def confusion_pairs(alignments, references: Optional[List[str]] = None, use_cer=False) -> List[Tuple[str, str, int]]:
    """(reference word, hypothesis word, count) of every substitution, sorted by falling count and then by the two words.
    alignments: what word_error_alignment returns - or, with `references`, the hypotheses it takes."""
    if references is not None:
        alignments = word_error_alignment(alignments, references, use_cer)
    tally: dict = {}
    for ops in alignments:
        for o in ops:
            if o['op'] == 'sub':
                tally[(o['ref'], o['hyp'])] = tally.get((o['ref'], o['hyp']), 0) + 1
    return sorted(((r, h, n) for (r, h), n in tally.items()), key=lambda t: (-t[2], t[0], t[1]))


def _compact(padded: torch.Tensor, lengths: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(B,S) zero-padded ids + (B,) lengths -> flat ids and (B+1,) int64 offsets, on the device and without a sync (index
    arithmetic only; rows past a length go to one spare slot at the end)."""
    B, S = padded.shape
    lengths = lengths.to(torch.int64).clamp(min=0, max=S)
    off = torch.zeros(B + 1, dtype=torch.int64, device=padded.device)
    off[1:] = torch.cumsum(lengths, 0)
    j = torch.arange(S, device=padded.device)[None, :]
    idx = torch.where(j < lengths[:, None], off[:-1, None] + j, torch.full_like(j, B * S))
    flat = torch.zeros(B * S + 1, dtype=torch.int32, device=padded.device)
    flat.scatter_(0, idx.reshape(-1), padded.to(torch.int32).reshape(-1))
    return flat[:B * S].contiguous(), off


def token_error_counts(log_probs: torch.Tensor, lengths, targets: torch.Tensor, target_lengths: torch.Tensor, blank: int) -> torch.Tensor:
    """(B,4) int64 [errors, substitutions, deletions, insertions] of the greedy CTC labels of log_probs (B,N,C) (frames past
    lengths[b] ignored; lengths may be None) against targets (B,S) with target_lengths (B,): ops.ctc_collapse followed by
    ops.edit_counts, all on the device and without a sync — a token error rate for validation inside a training loop."""
    x = log_probs.float().contiguous()
    if lengths is not None:
        lengths = lengths.to(torch.int32).contiguous()
    labels, tl = Fn.ops.ctc_collapse(x, lengths, int(blank))
    h, ho = _compact(labels, tl)
    r, ro = _compact(targets, target_lengths)
    return Fn.ops.edit_counts(h, ho, r, ro)
