"""A token-level back-off n-gram language model for the fused beam search (decoding.beam.ctc_beam_search_lm): an ARPA file read into
the automaton image of include/sconf_lm.h.

What pyctcdecode gets from kenlm, for a model whose words ARE the CTC tokens (an LM trained on `spm_encode --output_format=id`
text): one ARPA word is one token.  The image is one flat int32 buffer (floats stored by their bits) plus a few integers:

  states   (first_child, n_children, backoff f32, backoff_state)   one per gram shorter than the order; state 0 = the empty context
  entries  (token, logp f32, next_state, 0)                        the children of every state but state 0, sorted by token
  dense    (logp f32, next_state)                                  the unigram level, one record per token, `unk_logp, 0` where absent

`step` and `score` walk the host copy in Python exactly as the kernel walks the device copy; `to(device)` uploads it once."""
from __future__ import annotations

import math
from typing import Callable, Dict, Iterable, List, Optional, Tuple, Union

import numpy as np
import torch

from ..hip import lm as lm_kernels                  # the HIP op layer of the unit (its limits; the search itself runs from decoding.beam)

LN10 = math.log(10.0)


def _f32_bits(x) -> int:
    return int(np.array([x], dtype=np.float32).view(np.int32)[0])


class NGramLM:
    """The image on the host (`image`: int32 numpy array) with n_states, n_entries, num_tokens, order and start_state; `contexts[s]`
    is the token tuple of state s when the model was built from a table (None after `load`; "<s>" is the id num_tokens)."""

    def __init__(self, image: np.ndarray, n_states: int, n_entries: int, num_tokens: int, order: int, start_state: int,
                 contexts: Optional[List[Tuple[int, ...]]] = None):
        self.image = np.ascontiguousarray(image, dtype=np.int32)
        self.n_states, self.n_entries, self.num_tokens = int(n_states), int(n_entries), int(num_tokens)
        self.order, self.start_state = int(order), int(start_state)
        self.contexts = contexts
        self._device_images: Dict[str, torch.Tensor] = {}
        self.validate()

    # ---- the three arrays as views of the image --------------------------------------------------------------------------------
    @property
    def states(self) -> np.ndarray:
        return self.image[:4 * self.n_states].reshape(-1, 4)

    @property
    def entries(self) -> np.ndarray:
        return self.image[4 * self.n_states:4 * (self.n_states + self.n_entries)].reshape(-1, 4)

    @property
    def dense(self) -> np.ndarray:
        return self.image[4 * (self.n_states + self.n_entries):].reshape(-1, 2)

    # ---- construction ----------------------------------------------------------------------------------------------------------
    @classmethod
    def from_table(cls, grams: Dict[Tuple[int, ...], Tuple[float, float]], order: int, num_tokens: int, unk_logp: Optional[float] = None,
                   use_bos: bool = True) -> 'NGramLM':
        """grams: token tuple -> (natural-log probability, natural-log back-off), values already rounded to f32; "<s>" is the id
        num_tokens and stands only first.  The table must be prefix-closed."""
        V = int(num_tokens)
        if not 1 <= order <= lm_kernels.MAX_ORDER:
            raise ValueError(f'n-gram order {order}: from 1 to {lm_kernels.MAX_ORDER}')
        for g in grams:
            if not 1 <= len(g) <= order:
                raise ValueError(f'gram {g} has {len(g)} words, the order is {order}')
            if any(not 0 <= w < V for w in g[1:]) or not 0 <= g[0] <= V:
                raise ValueError(f'gram {g}: a token outside [0, {V}) ("<s>" = {V} may only stand first)')
            if len(g) > 1 and g[:-1] not in grams:
                raise ValueError(f'the table is not prefix-closed: {g} is a gram, its context {g[:-1]} is not')
        if unk_logp is None and any((w,) not in grams for w in range(V)):
            raise ValueError('tokens without a unigram and no unk_logp: the ARPA file has no <unk> and none was given')
        unk = 0.0 if unk_logp is None else float(np.float32(unk_logp))
        ctx = [()] + sorted((g for g in grams if len(g) < order), key=lambda g: (len(g), g))
        sid = {g: s for s, g in enumerate(ctx)}

        def suffix_state(g, proper):
            """The longest (proper) suffix of g that is a state."""
            for k in range(1 if proper else 0, len(g) + 1):
                if g[k:] in sid: return sid[g[k:]]
            return 0

        kids: Dict[Tuple[int, ...], List[int]] = {}
        for g in grams:
            if len(g) > 1: kids.setdefault(g[:-1], []).append(g[-1])
        S = len(ctx)
        E = sum(len(v) for v in kids.values())
        image = np.zeros(4 * S + 4 * E + 2 * V, dtype=np.int32)
        st, en, de = image[:4 * S].reshape(-1, 4), image[4 * S:4 * (S + E)].reshape(-1, 4), image[4 * (S + E):].reshape(-1, 2)
        at = 0
        for s, g in enumerate(ctx):
            if s == 0: continue                        # (0, 0, 0.0f, 0): its children are the dense table
            ws = sorted(kids.get(g, ()))
            st[s] = (at, len(ws), _f32_bits(grams[g][1]), suffix_state(g, True))
            for w in ws:
                en[at] = (w, _f32_bits(grams[g + (w,)][0]), suffix_state(g + (w,), False), 0)
                at += 1
        for w in range(V):
            de[w] = (_f32_bits(grams[(w,)][0]), suffix_state((w,), False)) if (w,) in grams else (_f32_bits(unk), 0)
        start = sid.get((V,), 0) if use_bos else 0
        return cls(image, S, E, V, order, start, contexts=ctx)

    @classmethod
    def from_arpa(cls, path_or_lines: Union[str, Iterable[str]], num_tokens: int, token_of: Optional[Callable[[str], int]] = None,
                  tokenizer=None, unk_logp: Optional[float] = None, use_bos: bool = True) -> 'NGramLM':
        r"""Read an ARPA file (a path, or its lines): \data\, `ngram n=count`, \n-grams: sections of
        `log10 p <TAB> w1 .. wn [<TAB> log10 backoff]`, \end\.  A word is a token: token_of(word), tokenizer.piece_to_id(word), or
        int(word).  Grams with </s> are dropped (a decoded unit is a window of a recording, not a sentence); <s> is kept as the first
        word of a gram (with use_bos its state is the start state); the unigram of <unk> is the default unk_logp and every other gram
        with <unk> is dropped.  Values become natural logs, rounded to f32 here, once."""
        V = int(num_tokens)
        if token_of is None:
            token_of = tokenizer.piece_to_id if tokenizer is not None else int
        if isinstance(path_or_lines, str):
            with open(path_or_lines) as f:
                lines = f.read().split('\n')
        else:
            lines = list(path_or_lines)
        grams: Dict[Tuple[int, ...], Tuple[float, float]] = {}
        declared, section, unk = set(), 0, None
        nat = lambda v: float(np.float32(float(v) * LN10))
        for raw in lines:
            line = raw.strip()
            if not line or line == '\\data\\':
                continue
            if line == '\\end\\':
                break
            if line.startswith('ngram '):
                n, cnt = line[6:].split('=')
                if int(cnt) > 0: declared.add(int(n))
                continue
            if line.startswith('\\') and line.endswith('-grams:'):
                section = int(line[1:-7])
                if section > lm_kernels.MAX_ORDER:
                    raise ValueError(f'ARPA file of order {section}: at most {lm_kernels.MAX_ORDER}')
                continue
            if section == 0:
                raise ValueError(f'ARPA: {line!r} before the first \\n-grams: section')
            f = line.split()
            if len(f) not in (section + 1, section + 2):
                raise ValueError(f'ARPA: {line!r} is not a {section}-gram line')
            words = f[1:1 + section]
            if '</s>' in words or '<s>' in words[1:]:
                continue
            if '<unk>' in words:
                if section == 1: unk = nat(f[0])
                continue
            ids = []
            for k, w in enumerate(words):
                i = V if w == '<s>' else int(token_of(w))
                if w != '<s>' and not 0 <= i < V:
                    raise ValueError(f'ARPA: the word {w!r} maps to token {i}, outside [0, {V})')
                ids.append(i)
            grams[tuple(ids)] = (nat(f[0]), nat(f[section + 1]) if len(f) == section + 2 else 0.0)
        if max(declared, default=0) > lm_kernels.MAX_ORDER:
            raise ValueError(f'ARPA file of order {max(declared)}: at most {lm_kernels.MAX_ORDER}')
        order = max([len(g) for g in grams] + [1])
        return cls.from_table(grams, order, V, unk if unk_logp is None else unk_logp, use_bos)

    # ---- the walk --------------------------------------------------------------------------------------------------------------
    def step(self, state: int, token: int) -> Tuple[float, int]:
        """(q, next_state) of include/sconf_lm.h: q is the f64 sum of the f32 values in the order met."""
        c, s = int(token), int(state)
        if not 0 <= c < self.num_tokens:
            return 0.0, 0
        st, en, q = self.states, self.entries, 0.0
        f32 = lambda bits: float(np.int32(bits).view(np.float32))
        lvl = 1
        while lvl < self.order and s != 0:
            first, cnt, bo, nxt = (int(v) for v in st[s])
            toks = en[first:first + cnt, 0]
            k = int(np.searchsorted(toks, c))
            if k < cnt and int(toks[k]) == c:
                return q + f32(en[first + k, 1]), int(en[first + k, 2])
            q += f32(bo)
            s = nxt
            lvl += 1
        d = self.dense[c]
        return q + f32(d[0]), int(d[1])

    def score(self, tokens: Iterable[int], state: Optional[int] = None) -> float:
        """Natural-log probability of the token sequence from `state` (default: the start state): the sum of the steps' q."""
        s = self.start_state if state is None else int(state)
        total = 0.0
        for c in tokens:
            q, s = self.step(s, c)
            total += q
        return total

    # ---- checks ----------------------------------------------------------------------------------------------------------------
    def validate(self) -> None:
        """Every index in range, children sorted by token, every back-off chain ending in state 0 within `order` arcs, finite values."""
        S, E, V = self.n_states, self.n_entries, self.num_tokens
        if not 1 <= self.order <= lm_kernels.MAX_ORDER:
            raise ValueError(f'LM image: order {self.order}: from 1 to {lm_kernels.MAX_ORDER}')
        if S < 1 or E < 0 or V < 1 or self.image.ndim != 1 or self.image.size != 4 * S + 4 * E + 2 * V:
            raise ValueError(f'LM image: {self.image.size} words do not hold {S} states, {E} entries and {V} tokens')
        if not 0 <= self.start_state < S:
            raise ValueError(f'LM image: start state {self.start_state} out of range')
        st, en, de = self.states, self.entries, self.dense
        first, cnt, nxt = st[:, 0].astype(np.int64), st[:, 1].astype(np.int64), st[:, 3]
        if (first < 0).any() or (cnt < 0).any() or (first + cnt > E).any():
            raise ValueError('LM image: a state\'s children lie outside the entries (index out of range)')
        if ((nxt < 0) | (nxt >= S)).any() or ((en[:, 2] < 0) | (en[:, 2] >= S)).any() or ((de[:, 1] < 0) | (de[:, 1] >= S)).any():
            raise ValueError('LM image: a state index out of range')
        if E and ((en[:, 0] < 0) | (en[:, 0] >= V)).any():
            raise ValueError('LM image: an entry\'s token out of range')
        if tuple(st[0]) != (0, 0, 0, 0):
            raise ValueError('LM image: state 0 must be (0, 0, 0.0, 0)')
        if E > 1:
            inside = np.ones(E, dtype=bool)             # entry e and e - 1 belong to the same state
            inside[first[cnt > 0]] = False
            bad = inside[1:] & (en[1:, 0] <= en[:-1, 0])
            if bad.any():
                raise ValueError('LM image: the children of a state are not sorted by token (unsorted or repeated)')
        hops, s = 0, np.arange(S)
        while (s != 0).any():
            if hops >= self.order - 1:
                raise ValueError('LM image: a back-off chain does not reach state 0 (cycle or too long)')
            s = np.where(s != 0, nxt[s], 0)
            hops += 1
        for what, bits in (('back-off', st[:, 2]), ('entry', en[:, 1]), ('unigram', de[:, 0])):
            if not np.isfinite(np.ascontiguousarray(bits).view(np.float32)).all():
                raise ValueError(f'LM image: a non-finite {what} value')

    # ---- storage and upload ----------------------------------------------------------------------------------------------------
    def save(self, path: str) -> None:
        """The image as .npz (a large ARPA file is parsed once)."""
        with open(path, 'wb') as f:
            np.savez(f, image=self.image, sizes=np.asarray([self.n_states, self.n_entries, self.num_tokens, self.order, self.start_state],
                                                          dtype=np.int64))

    @classmethod
    def load(cls, path: str) -> 'NGramLM':
        with np.load(path) as z:
            return cls(z['image'], *(int(v) for v in z['sizes']))

    def to(self, device) -> 'NGramLM':
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
