"""Buffered (streaming-style) inference — mirror of lcasr/eval/buffered_transcription.py:10-97 (`fetch_logits`).

Each chunk of `seq_len - overlap` frames is transcribed inside a buffer of seq_len frames that gives it overlap // 2 frames of
context on either side; only the chunk's own rows of the buffer's posteriors are kept.  Signature and window arithmetic are
the reference's, quirks included: the buffer is clamped at both ends of the recording, rows are cut with
int(rel / (buffer_size / logit_size)), seq_len > spec_n gives one window, overlap must be a multiple of the subsampling factor.

What changes is the execution.  Every buffer is seq_len frames long, except that the last one is shorter when the recording ends
inside its right context, so the windows go through the model in batches of `max_batch` (a shorter last one on its own); the kept rows are placed by one HIP launch per batch (ops.copy_row_spans_, csrc/infer.hip) from a span table that
is uploaded once for the whole recording.  Log-probs are copied, never averaged, so there is no exp / log round trip."""
from __future__ import annotations

from typing import List, Tuple

import torch

from .. import functional as Fn          # Fn.ops: the HIP op layer (tests swap it for the CPU kernel references)
from .utils import resolve_windowing


def buffer_plan(spec_n: int, seq_len: int, overlap: int) -> List[Tuple[int, int, int, int]]:
    """(buffer_start, buffer_end, chunk_start, chunk_end) in frames of every window of the reference loop
    (buffered_transcription.py:42-71), for seq_len / overlap already resolved (seq_len <= spec_n)."""
    chunk_size = seq_len - overlap
    if chunk_size <= 0:
        raise ValueError(f'buffer_plan(spec_n={spec_n}, seq_len={seq_len}, overlap={overlap}): the chunk seq_len - overlap must be positive')
    plan, chunk_start, chunk_end = [], 0, chunk_size
    while True:
        spec_start, spec_end = chunk_start - overlap // 2, chunk_end + overlap // 2
        if spec_start < 0:
            spec_start, spec_end = 0, seq_len
        elif spec_end > spec_n:
            spec_end = spec_n
            spec_start = spec_end - seq_len
        plan.append((spec_start, spec_end, chunk_start, chunk_end))
        chunk_start += chunk_size
        chunk_end += chunk_size
        if chunk_end >= spec_n:
            chunk_end = spec_n
        if chunk_start >= spec_n:
            return plan


def buffer_spans(plan, logit_sizes, buffer_rows: int, what: str = 'plan') -> Tuple[List[Tuple[int, int, int]], int]:
    """(src_row0, rows, dst_row0) per window and the number of output rows, for windows of logit_sizes posterior rows (one int
    for all windows, or one per window).

    The reference adds rows [s, e) of window i to rows [pos + s, pos + e) of a zeroed buffer of buffer_rows rows, advances pos by
    e - s, and finally keeps the rows that were written (buffered_transcription.py:81-95).  The kept rows are those spans in buffer
    order, so dst_row0 here is the row in that final, compacted output.  Where the reference's slice assignment or its
    `logit_count.max() == 1` check fails, this raises ValueError."""
    if isinstance(logit_sizes, int):
        logit_sizes = [logit_sizes] * len(plan)
    raw, pos = [], 0
    for i, (b0, b1, c0, c1) in enumerate(plan):
        logit_size = logit_sizes[i]
        per_row = (b1 - b0) / logit_size
        s, e = int((c0 - b0) / per_row), int((c1 - b0) / per_row)
        rows = max(e - s, 0)
        if s < 0 or s + rows > logit_size or pos + s + rows > buffer_rows:
            raise ValueError(f'{what}: window {i} keeps rows [{s}, {e}) of {logit_size} at output row {pos + s} of {buffer_rows}: does not fit')
        raw.append((pos + s, i, s, rows))
        pos += e - s
    spans, total, end = [None] * len(plan), 0, 0
    for d0, i, s, rows in sorted(raw):
        if rows and d0 < end:
            raise ValueError(f'{what}: window {i} overlaps the rows kept before it (output row {d0} < {end})')
        spans[i] = (s, rows, total)
        total += rows
        end = max(end, d0 + rows)
    if total == 0:
        raise ValueError(f'{what}: no rows are kept')
    return spans, total


@torch.no_grad()
def fetch_logits(args, model, spec: torch.Tensor, seq_len: int, overlap: int, tokenizer, use_tqdm=True, max_batch: int = 16,
                 return_numpy: bool = True):
    """Log-probs (N, vocab+1) of a whole recording spec (1, F, T): each chunk of seq_len - overlap frames transcribed inside a
    buffer of seq_len frames, only the chunk's rows kept.

    args / tokenizer are used exactly as in the reference (config defaults for -1, vocab size).  Returns a numpy array like the
    reference unless return_numpy=False (then the GPU tensor)."""
    if spec.dim() != 3 or spec.shape[0] != 1:
        raise ValueError(f'spec must be (1, features, time), got {tuple(spec.shape)}')
    spec_n = spec.shape[-1]
    seq_len, overlap = resolve_windowing(args, spec_n, seq_len, overlap, model.subsampling.subsampling_factor)

    what = f'buffer_plan(spec_n={spec_n}, seq_len={seq_len}, overlap={overlap})'
    plan = buffer_plan(spec_n, seq_len, overlap)
    full = [i for i, (b0, b1, _, _) in enumerate(plan) if b1 - b0 == seq_len]
    short = [i for i, (b0, b1, _, _) in enumerate(plan) if b1 - b0 != seq_len]   # at most the last: its buffer ends with the recording
    dev = next(model.parameters()).device
    C = tokenizer.vocab_size() + 1
    spec = spec.to(dev)

    def posteriors(idx):
        chunk = torch.stack([spec[0, :, plan[i][0]:plan[i][1]] for i in idx])
        lp = model(chunk)['final_posteriors'].float().contiguous()          # (W, logit_size, C)
        if lp.shape[2] != C:
            raise ValueError(f'model returns {lp.shape[2]} classes, tokenizer.vocab_size() + 1 is {C}')
        return lp

    # a shorter window has its own number of rows, which the span table needs: it goes first and is placed with the others
    held = [(i, posteriors([i])) for i in short]
    order = full + short                                                    # rows of the span table
    out, table = None, None
    for k in range(0, len(full), max_batch):
        grp = full[k:k + max_batch]
        lp = posteriors(grp)
        if table is None:                                                   # the span table of the whole recording: one upload
            sizes = {i: h.shape[1] for i, h in held}
            spans, total = buffer_spans(plan, [sizes.get(i, lp.shape[1]) for i in range(len(plan))], spec_n // 4 + seq_len, what)
            table = torch.tensor([spans[i] for i in order], dtype=torch.int32).to(dev)
            out = torch.empty(total, C, dtype=torch.float32, device=dev)
        Fn.ops.copy_row_spans_(lp, table[k:k + len(grp)], out)
    for j, (i, lp) in enumerate(held):
        Fn.ops.copy_row_spans_(lp, table[len(full) + j:len(full) + j + 1], out)
    return out.cpu().numpy() if return_numpy else out
