"""CTC keyword search: "where in this recording does anyone say X?" for a list of hundreds or thousands of X, answered from the
posteriors on the GPU (csrc/kws.hip through hip/kws.py; include/sconf_kws.h holds the exact contract).

Searching the 1-best text misses every term the greedy path got slightly wrong; hotword boosting changes the transcript instead of
reporting occurrences; forced alignment needs the term's place in a transcript of everything.  Here every keyword is its own small
CTC lattice `l_1 blank l_2 .. l_L` with a free start at every frame.  A hit's score is the log-likelihood ratio of the keyword's
best path over its span against the greedy path over the same frames: 0 means the keyword IS the greedy decode there, -0.2 that one
label lost 0.45 to 0.55, and a missing label costs what the model gave it, typically several nats.  Overlapping candidates of one
keyword are thinned on the device (the best of a run of overlapping ones stays), so hits of a keyword never overlap.

`KeywordSet` compiles the list into the lane-packed image of the header once and uploads it once; `ctc_keyword_search` returns
device tensors; `KeywordHits.records` is the one copy to the host.  Nothing here loops over frames."""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ..hip import kws as kws_kernels              # the HIP op layer (tests swap kws_kernels.search for the numpy restatement)

MAX_LABELS = kws_kernels.MAX_LABELS
FIRST, SKIP, LAST = kws_kernels.FIRST, kws_kernels.SKIP, kws_kernels.LAST
WAVE = 64


def _f32_bits(x) -> int:
    return int(np.array([x], dtype=np.float32).view(np.int32)[0])


class KeywordSet:
    """phrases: non-empty token-id sequences of at most MAX_LABELS (32) labels, none of them the blank of the search.  Keyword k is
    reported when its score reaches `min_score_per_label * len(phrase k)`, which must be finite.  The default, -0.5 per label, lets
    every label lose about 0.38 to 0.62 against its strongest competitor; it is NOT tuned on real recordings.  A phrase given twice
    is two keywords.  `words` (optional) are the names the records carry; `one_per_wave=True` gives every keyword a wave of its own
    instead of packing them end to end (tools/kws_bench.py measures what packing buys with it).

    The image (include/sconf_kws.h): `lanes` (n_waves * 64, 4) int32 of (column, flags, keyword, threshold bits), then `columns` (U):
    the distinct labels in order of first appearance, then -1, the blank of the call, if a phrase of two labels or more needs it."""

    def __init__(self, phrases: Sequence[Sequence[int]], min_score_per_label: float = -0.5, words: Optional[Sequence[str]] = None,
                 one_per_wave: bool = False):
        phrases = [tuple(int(c) for c in p) for p in phrases]
        if not phrases:
            raise ValueError('keywords: an empty list')
        if not math.isfinite(float(min_score_per_label)):
            raise ValueError(f'keywords: min_score_per_label = {min_score_per_label} must be finite')
        for p in phrases:
            if not p:
                raise ValueError('keywords: an empty phrase')
            if len(p) > MAX_LABELS:
                raise ValueError(f'keywords: the phrase {p} has {len(p)} labels, at most {MAX_LABELS}')
            if min(p) < 0:
                raise ValueError(f'keywords: the phrase {p} holds a negative label')
        if words is not None and len(words) != len(phrases):
            raise ValueError(f'keywords: {len(phrases)} phrases but {len(words)} words')
        self.phrases: Optional[List[Tuple[int, ...]]] = phrases
        self.words: Optional[List[str]] = None if words is None else [str(w) for w in words]
        self.min_score_per_label = float(min_score_per_label)
        with np.errstate(over='ignore'):
            thresholds = [float(np.float32(self.min_score_per_label) * np.float32(len(p))) for p in phrases]
        if not all(math.isfinite(t) for t in thresholds):
            raise ValueError('keywords: a threshold that is not finite in float32')
        self._set_image(*self._compile(phrases, thresholds, one_per_wave))

    # ---- construction ----------------------------------------------------------------------------------------------------------
    @staticmethod
    def _compile(phrases, thresholds, one_per_wave: bool):
        col: Dict[int, int] = {}
        for p in phrases:
            for c in p:
                col.setdefault(c, len(col))
        columns = list(col)
        blank_col = -1
        if any(len(p) > 1 for p in phrases):
            blank_col = len(columns)
            columns.append(-1)
        lanes: List[Tuple[int, int, int, int]] = []
        for k, p in enumerate(phrases):
            W = 2 * len(p) - 1
            used = len(lanes) % WAVE
            if used and (one_per_wave or used + W > WAVE):                  # no keyword straddles two waves
                lanes.extend([(-1, 0, 0, 0)] * (WAVE - used))
            bits = _f32_bits(thresholds[k])
            for s in range(W):
                flags = (FIRST if s == 0 else 0) | (LAST if s == W - 1 else 0)
                if s % 2 == 0 and s >= 2 and p[s // 2] != p[s // 2 - 1]:
                    flags |= SKIP
                lanes.append((col[p[s // 2]] if s % 2 == 0 else blank_col, flags, k, bits))
        lanes.extend([(-1, 0, 0, 0)] * (-len(lanes) % WAVE))
        image = np.concatenate([np.asarray(lanes, dtype=np.int32).reshape(-1), np.asarray(columns, dtype=np.int32)])
        return image, len(lanes) // WAVE, len(columns), len(phrases)

    def _set_image(self, image, n_waves, U, K):
        self.image = np.ascontiguousarray(image, dtype=np.int32)
        self.n_waves, self.U, self.K = int(n_waves), int(U), int(K)
        self._device_images: Dict[str, torch.Tensor] = {}
        self.validate()

    @classmethod
    def from_text(cls, words: Sequence[str], tokenizer, min_score_per_label: float = -0.5, one_per_wave: bool = False) -> 'KeywordSet':
        """Each string through tokenizer.encode (what spells it in the transcripts the model was trained on)."""
        if isinstance(words, str):
            raise TypeError('keywords: a list of strings, not one string')
        phrases = []
        for w in words:
            ids = [int(i) for i in tokenizer.encode(w)]
            if not ids:
                raise ValueError(f'keywords: {w!r} encodes to no token')
            phrases.append(ids)
        return cls(phrases, min_score_per_label, words=list(words), one_per_wave=one_per_wave)

    @classmethod
    def from_image(cls, image: np.ndarray, n_waves: int, U: int, K: int) -> 'KeywordSet':
        """A set from its image alone (validated); `phrases` and `words` are None."""
        self = cls.__new__(cls)
        self.phrases = self.words = None
        self.min_score_per_label = float('nan')
        self._set_image(image, n_waves, U, K)
        return self

    # ---- the two arrays as views of the image ----------------------------------------------------------------------------------
    @property
    def lanes(self) -> np.ndarray:
        return self.image[:self.n_waves * WAVE * 4].reshape(-1, 4)

    @property
    def columns(self) -> np.ndarray:
        return self.image[self.n_waves * WAVE * 4:]

    @property
    def thresholds(self) -> np.ndarray:
        """(K,) f32: the threshold of every keyword, from its LAST lane."""
        ln = self.lanes
        out = np.zeros(self.K, dtype=np.float32)
        last = ln[(ln[:, 0] >= 0) & ((ln[:, 1] & LAST) != 0)]
        out[last[:, 2]] = np.ascontiguousarray(last[:, 3]).view(np.float32)
        return out

    def name(self, k: int):
        return self.words[k] if self.words is not None else int(k)

    # ---- checks ----------------------------------------------------------------------------------------------------------------
    def validate(self, blank: Optional[int] = None, num_classes: Optional[int] = None) -> None:
        """The image is what the kernel may assume: sizes, every column and keyword index in range, every keyword one run of
        2L - 1 neighbouring lanes inside one wave that opens with FIRST and closes with LAST, labels on its even and the blank on
        its odd states, SKIP exactly where two neighbouring labels differ, one finite threshold per keyword, every keyword present
        once; with `blank` / `num_classes` (the search passes its own): no phrase holds the blank or a label outside the classes."""
        nw, U, K = self.n_waves, self.U, self.K
        if nw < 1 or U < 1 or K < 1 or self.image.ndim != 1 or self.image.size != nw * WAVE * 4 + U:
            raise ValueError(f'keyword image: {self.image.size} words do not hold {nw} waves and {U} columns')
        ln, cols = self.lanes, self.columns
        if (cols < -1).any() or len(set(cols.tolist())) != U:
            raise ValueError('keyword image: the columns are not distinct class ids (or -1 for the blank)')
        live = ln[:, 0] >= 0
        if (ln[:, 0] < -1).any() or (ln[:, 0] >= U).any():
            raise ValueError('keyword image: a column index out of range')
        if ((ln[:, 1] < 0) | (ln[:, 1] > (FIRST | SKIP | LAST))).any() or (ln[~live, 1] != 0).any():
            raise ValueError('keyword image: unknown flags, or flags on an idle lane')
        if ((ln[live, 2] < 0) | (ln[live, 2] >= K)).any():
            raise ValueError('keyword image: a keyword index out of range')
        seen = np.zeros(K, dtype=np.int64)
        i, n = 0, nw * WAVE
        while i < n:
            if not live[i]:
                i += 1
                continue
            k = int(ln[i, 2])
            if not ln[i, 1] & FIRST:
                raise ValueError(f'keyword image: lane {i} is inside a keyword that no FIRST lane opens')
            j = i
            while not ln[j, 1] & LAST:
                j += 1
                if j >= n or j // WAVE != i // WAVE or not live[j] or int(ln[j, 2]) != k or ln[j, 1] & FIRST:
                    raise ValueError(f'keyword image: keyword {k} from lane {i} is not closed by a LAST lane inside its wave (straddles)')
            W = j - i + 1
            if W % 2 == 0 or W > 2 * MAX_LABELS - 1:
                raise ValueError(f'keyword image: keyword {k} has {W} states: an odd number up to {2 * MAX_LABELS - 1}')
            if len({int(t) for t in ln[i:j + 1, 3]}) != 1 or not math.isfinite(float(np.int32(ln[j, 3]).view(np.float32))):
                raise ValueError(f'keyword image: keyword {k} has no single finite threshold')
            for s in range(W):
                c = int(cols[ln[i + s, 0]])
                if (c == -1) != (s % 2 == 1):
                    raise ValueError(f'keyword image: keyword {k} state {s}: labels on even states, the blank on odd ones')
                want = s % 2 == 0 and s >= 2 and int(ln[i + s, 0]) != int(ln[i + s - 2, 0])
                if bool(ln[i + s, 1] & SKIP) != want:
                    raise ValueError(f'keyword image: keyword {k} state {s}: SKIP exactly where the label differs from the one before')
            seen[k] += 1
            i = j + 1
        if (seen != 1).any():
            raise ValueError(f'keyword image: keyword {int(np.nonzero(seen != 1)[0][0])} is present {int(seen[seen != 1][0])} times, not once')
        labels = cols[cols >= 0]
        if blank is not None and (labels == int(blank)).any():
            raise ValueError(f'keywords: a phrase holds the blank ({int(blank)}), which is never a token of a transcript')
        if num_classes is not None and labels.size and int(labels.max()) >= int(num_classes):
            raise ValueError(f'keywords: a phrase holds the label {int(labels.max())}, the model has {int(num_classes)} classes')

    # ---- upload ----------------------------------------------------------------------------------------------------------------
    def to(self, device) -> 'KeywordSet':
        """Upload the image to `device` once; the search takes it from there."""
        self.device_image(device)
        return self

    def device_image(self, device) -> torch.Tensor:
        d = torch.device(device)
        if d.type == 'cuda' and d.index is None:
            d = torch.device('cuda', torch.cuda.current_device())
        key = str(d)
        if key not in self._device_images:
            self._device_images[key] = torch.from_numpy(self.image.copy()).to(d)        # (a copy: on the CPU `to` would alias the image)
        return self._device_images[key]


class KeywordHits:
    """frames (B, K, cap, 2) int32: [start, end) of the first `cap` hits of every keyword in time order, (-1, -1) in unused slots;
    score (B, K, cap) f32: their log-likelihood ratio, -inf in unused slots; count (B, K) int32: the TRUE number of hits, which may
    exceed cap.  Without the batch dimension for (N, C) input.  Device tensors; `records` is the one copy to the host."""

    def __init__(self, frames: torch.Tensor, score: torch.Tensor, count: torch.Tensor, keywords: KeywordSet):
        self.frames, self.score, self.count, self.keywords = frames, score, count, keywords

    def records(self, spf: Optional[float] = None):
        """The hits sorted by start: {'keyword', 'start', 'end', 'score'} with frames, or with `spf` (seconds per frame)
        {'keyword', 'startTime', 'endTime', 'score'} with times in the '12.34s' form.  'keyword' is the word (`from_text`) or the
        keyword's index.  A keyword with more hits than slots carries 'truncated': True on its records.  One list for (N, C) input,
        one list per sample otherwise."""
        single = self.count.dim() == 1
        fr, sc, cn = (t[None] if single else t for t in (self.frames, self.score, self.count))
        B, K, cap = sc.shape
        packed = torch.cat([fr.reshape(B, K, cap * 2), sc.contiguous().view(torch.int32), cn[..., None]], -1).cpu().numpy()
        frames = packed[..., :cap * 2].reshape(B, K, cap, 2)
        score = np.ascontiguousarray(packed[..., cap * 2:cap * 3]).view(np.float32)
        count = packed[..., -1]
        out = []
        for b in range(B):
            rows = []
            for k in np.nonzero(count[b])[0].tolist():
                for i in range(min(int(count[b, k]), cap)):
                    rows.append((int(frames[b, k, i, 0]), int(frames[b, k, i, 1]), k, float(score[b, k, i]), int(count[b, k]) > cap))
            rows.sort()
            recs = []
            for s, e, k, E, cut in rows:
                r = {'keyword': self.keywords.name(k)}
                if spf is None:
                    r['start'], r['end'] = s, e
                else:
                    r['startTime'], r['endTime'] = f'{s * spf:.2f}s', f'{e * spf:.2f}s'
                r['score'] = E
                if cut:
                    r['truncated'] = True
                recs.append(r)
            out.append(recs)
        return out[0] if single else out


def ctc_keyword_search(log_probs: torch.Tensor, keywords, blank: int, input_lengths=None, max_hits: int = 64,
                       classes: Optional[int] = None) -> KeywordHits:
    """log_probs (N, C) or (B, N, C) f32 log-scores (they need not be normalised); keywords: a KeywordSet, or a list of token-id
    phrases with the default threshold; blank: the blank's class; input_lengths (B,) or None; max_hits: slots per keyword and sample;
    classes: read only the first `classes` columns of every row -> KeywordHits of device tensors."""
    if not isinstance(keywords, KeywordSet):
        keywords = KeywordSet(keywords)
    single = log_probs.dim() == 2
    if log_probs.dim() not in (2, 3):
        raise ValueError(f'log_probs must be (N, C) or (B, N, C), got {tuple(log_probs.shape)}')
    lp = (log_probs[None] if single else log_probs).float().contiguous()
    C = lp.shape[2]
    classes = C if classes is None else int(classes)
    if not 1 <= classes <= C or not 0 <= int(blank) < classes:
        raise ValueError(f'ctc_keyword_search: classes = {classes} of {C} and blank = {blank}: 1 <= classes <= C, 0 <= blank < classes')
    keywords.validate(blank=int(blank), num_classes=classes)
    dev = lp.device
    il = None if input_lengths is None else torch.as_tensor(input_lengths).reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
    out = kws_kernels.search(lp, keywords.device_image(dev), keywords.n_waves, keywords.U, keywords.K, int(blank), il, int(max_hits), classes)
    if single:
        return KeywordHits(out[0][0], out[1][0], out[2][0], keywords)
    return KeywordHits(out[0], out[1], out[2], keywords)
