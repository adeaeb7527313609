"""Hotwords for the boosted beam search (decoding.beam.ctc_beam_search_hot): phrases as TOKEN sequences, compiled into the
Aho-Corasick automaton image of include/sconf_hot.h.

What pyctcdecode's `decode_beams(..., hotwords=[...], hotword_weight=w)` takes, for phrases spelt in the model's tokens
(`from_text` encodes strings with the tokenizer; with sentencepiece a word then starts with its `▁` piece, so it matches at a word
start).  The image is one flat int32 buffer (floats stored by their bits) plus three integers:

  states   (first_child, n_children, fail_state, 0)   the nodes of the phrases' trie; state 0 = the root
  credit   (emit f32, phi f32)                        per state: the weights of every phrase that ends here (as a suffix of the path),
                                                      and the partial credit of the phrase in progress
  entries  (token, next_state)                        the children of every state, sorted by token

`step` and `score` walk the host copy in Python exactly as the kernel walks the device copy; `to(device)` uploads it once."""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ..hip import hot as hot_kernels                # the HIP op layer of the unit (its limits; the search itself runs from decoding.beam)


def _f32_bits(x) -> int:
    return int(np.array([x], dtype=np.float32).view(np.int32)[0])


def _f32(bits) -> float:
    return float(np.int32(bits).view(np.float32))


class HotwordSet:
    """phrases: non-empty token-id sequences of at most hip.hot.MAX_LEN tokens; weights: relative, finite and > 0 (default 1.0 each;
    the search multiplies them by its hotword_weight); a phrase given twice counts with the sum of its weights.  `phrases` / `weights`
    hold the merged set (None after `load`); `paths[s]` is the token tuple of state s (None after `load`)."""

    def __init__(self, phrases: Sequence[Sequence[int]], weights: Optional[Sequence[float]] = None):
        phrases = [tuple(int(c) for c in p) for p in phrases]
        if weights is None:
            weights = [1.0] * len(phrases)
        weights = [float(w) for w in weights]
        if len(weights) != len(phrases):
            raise ValueError(f'hotwords: {len(phrases)} phrases but {len(weights)} weights')
        merged: Dict[Tuple[int, ...], float] = {}
        for p, w in zip(phrases, weights):
            if not p:
                raise ValueError('hotwords: an empty phrase')
            if len(p) > hot_kernels.MAX_LEN:
                raise ValueError(f'hotwords: the phrase {p} has {len(p)} tokens, at most {hot_kernels.MAX_LEN}')
            if min(p) < 0:
                raise ValueError(f'hotwords: the phrase {p} holds a negative token')
            if not (math.isfinite(w) and w > 0):
                raise ValueError(f'hotwords: the weight {w} of the phrase {p} must be finite and > 0')
            merged[p] = merged.get(p, 0.0) + w
        self.phrases: Optional[List[Tuple[int, ...]]] = list(merged)
        self.weights: Optional[List[float]] = list(merged.values())
        self._set_image(*self._compile(merged))

    # ---- construction ----------------------------------------------------------------------------------------------------------
    @staticmethod
    def _compile(merged: Dict[Tuple[int, ...], float]):
        nodes = {()}
        for p in merged:
            nodes.update(p[:k] for k in range(1, len(p) + 1))
        paths = sorted(nodes, key=lambda g: (len(g), g))                  # by depth: a failure state comes before the states that use it
        sid = {g: s for s, g in enumerate(paths)}
        S = len(paths)
        fail, emit, own, phi = [0] * S, [0.0] * S, [0.0] * S, [0.0] * S
        for p, w in merged.items():
            for k in range(1, len(p)):
                own[sid[p[:k]]] = max(own[sid[p[:k]]], w * k / len(p))
        for s, g in enumerate(paths):
            if s == 0: continue
            fail[s] = next(sid[g[k:]] for k in range(1, len(g) + 1) if g[k:] in sid)
            emit[s] = merged.get(g, 0.0) + emit[fail[s]]
            phi[s] = max(own[s], phi[fail[s]])
        kids: Dict[Tuple[int, ...], List[int]] = {}
        for g in paths[1:]:
            kids.setdefault(g[:-1], []).append(g[-1])
        E = S - 1
        image = np.zeros(6 * S + 2 * E, dtype=np.int32)
        st, cr, en = image[:4 * S].reshape(-1, 4), image[4 * S:6 * S].reshape(-1, 2), image[6 * S:].reshape(-1, 2)
        at = 0
        for s, g in enumerate(paths):
            ws = sorted(kids.get(g, ()))
            st[s] = (at, len(ws), fail[s], 0)
            cr[s] = (_f32_bits(emit[s]), _f32_bits(phi[s]))
            for w in ws:
                en[at] = (w, sid[g + (w,)])
                at += 1
        return image, S, E, max((len(g) for g in paths), default=0), paths

    def _set_image(self, image, n_states, n_entries, max_len, paths=None):
        self.image = np.ascontiguousarray(image, dtype=np.int32)
        self.n_states, self.n_entries, self.max_len = int(n_states), int(n_entries), int(max_len)
        self.paths = paths
        self._device_images: Dict[str, torch.Tensor] = {}
        self.validate()

    @classmethod
    def from_text(cls, words: Sequence[str], tokenizer, weights: Optional[Sequence[float]] = None) -> 'HotwordSet':
        """Each string through tokenizer.encode (what spells it in the transcripts the model was trained on)."""
        if isinstance(words, str):
            raise TypeError('hotwords: a list of strings, not one string')
        phrases = []
        for w in words:
            ids = [int(i) for i in tokenizer.encode(w)]
            if not ids:
                raise ValueError(f'hotwords: {w!r} encodes to no token')
            phrases.append(ids)
        return cls(phrases, weights)

    # ---- the three arrays as views of the image --------------------------------------------------------------------------------
    @property
    def states(self) -> np.ndarray:
        return self.image[:4 * self.n_states].reshape(-1, 4)

    @property
    def credit(self) -> np.ndarray:
        return self.image[4 * self.n_states:6 * self.n_states].reshape(-1, 2)

    @property
    def entries(self) -> np.ndarray:
        return self.image[6 * self.n_states:].reshape(-1, 2)

    # ---- the walk --------------------------------------------------------------------------------------------------------------
    def step(self, state: int, token: int) -> Tuple[int, float, float]:
        """(next_state, emit, phi) of include/sconf_hot.h: the state after `token` and its two credits (f32 values)."""
        c, s = int(token), int(state)
        st, en = self.states, self.entries
        nxt = 0
        for _ in range(self.max_len + 1):
            first, cnt, fail, _0 = (int(v) for v in st[s])
            toks = en[first:first + cnt, 0]
            k = int(np.searchsorted(toks, c))
            if k < cnt and int(toks[k]) == c:
                nxt = int(en[first + k, 1])
                break
            if s == 0:
                break
            s = fail
        e, p = self.credit[nxt]
        return nxt, _f32(e), _f32(p)

    def score(self, tokens: Sequence[int], state: int = 0) -> Tuple[float, float]:
        """(permanent, phi of the last state) of a token sequence from `state`: the summed relative weights of every phrase
        occurrence, and the partial credit of the phrase the sequence ends inside.  The search adds hotword_weight times the
        first for good and holds hotword_weight times the second while the prefix is live."""
        s, total, phi = int(state), 0.0, _f32(self.credit[int(state), 1])
        for c in tokens:
            s, e, phi = self.step(s, c)
            total += e
        return total, phi

    # ---- checks ----------------------------------------------------------------------------------------------------------------
    def validate(self, blank: Optional[int] = None, num_classes: Optional[int] = None) -> None:
        """Every index in range, children sorted by token, every failure chain ending in the root within max_len arcs, finite
        non-negative credits; with `blank` / `num_classes` (the search passes its own): no phrase holds the blank or a token outside
        the classes."""
        S, E = self.n_states, self.n_entries
        if not 0 <= self.max_len <= hot_kernels.MAX_LEN:
            raise ValueError(f'hotword image: phrases of up to {self.max_len} tokens: at most {hot_kernels.MAX_LEN}')
        if S < 1 or E < 0 or self.image.ndim != 1 or self.image.size != 6 * S + 2 * E:
            raise ValueError(f'hotword image: {self.image.size} words do not hold {S} states and {E} entries')
        st, cr, en = self.states, self.credit, self.entries
        first, cnt, fail = st[:, 0].astype(np.int64), st[:, 1].astype(np.int64), st[:, 2]
        if (first < 0).any() or (cnt < 0).any() or (first + cnt > E).any():
            raise ValueError('hotword image: a state\'s children lie outside the entries (index out of range)')
        if ((fail < 0) | (fail >= S)).any() or (E and ((en[:, 1] < 0) | (en[:, 1] >= S)).any()):
            raise ValueError('hotword image: a state index out of range')
        if E and (en[:, 0] < 0).any():
            raise ValueError('hotword image: a negative token')
        if fail[0] != 0:
            raise ValueError('hotword image: the root must fail to itself')
        if E > 1:
            inside = np.ones(E, dtype=bool)             # entry e and e - 1 belong to the same state
            inside[first[cnt > 0]] = False
            if (inside[1:] & (en[1:, 0] <= en[:-1, 0])).any():
                raise ValueError('hotword image: the children of a state are not sorted by token (unsorted or repeated)')
        hops, s = 0, np.arange(S)
        while (s != 0).any():
            if hops >= self.max_len:
                raise ValueError('hotword image: a failure chain does not reach the root (cycle or too long)')
            s = np.where(s != 0, fail[s], 0)
            hops += 1
        vals = np.ascontiguousarray(cr).view(np.float32)
        if not np.isfinite(vals).all() or (vals < 0).any() or tuple(vals[0]) != (0.0, 0.0):
            raise ValueError('hotword image: a credit that is not finite and >= 0, or a root with credit')
        if E and blank is not None and (en[:, 0] == int(blank)).any():
            raise ValueError(f'hotwords: a phrase holds the blank ({int(blank)}), which is never a token of a transcript')
        if E and num_classes is not None and (en[:, 0] >= int(num_classes)).any():
            raise ValueError(f'hotwords: a phrase holds the token {int(en[:, 0].max())}, the model has {int(num_classes)} classes')

    # ---- storage and upload ----------------------------------------------------------------------------------------------------
    def save(self, path: str) -> None:
        """The image as .npz."""
        with open(path, 'wb') as f:
            np.savez(f, image=self.image, sizes=np.asarray([self.n_states, self.n_entries, self.max_len], dtype=np.int64))

    @classmethod
    def load(cls, path: str) -> 'HotwordSet':
        with np.load(path) as z:
            return cls.from_image(z['image'], *(int(v) for v in z['sizes']))

    @classmethod
    def from_image(cls, image: np.ndarray, n_states: int, n_entries: int, max_len: int) -> 'HotwordSet':
        """A set from its image alone (validated); `phrases`, `weights` and `paths` are None."""
        self = cls.__new__(cls)
        self.phrases = self.weights = None
        self._set_image(image, n_states, n_entries, max_len)
        return self

    def to(self, device) -> 'HotwordSet':
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
