"""Evaluation driver — the per-recording loop of eval/run.py:71-125 of the reference without its dataset loading; `transcribe` and
`spectrograms_of` put the audio front end (utils/audio_tools.py) before it, so that a waveform is enough: at 16 kHz, or at the rate it
was decoded at (`sample_rate`), resampled on the device.

Four steps per recording, as there: log-probs in one of three modes, CTC decoding (greedy, or beam search for beam_width > 1), text normalisation, and
word_error_rate_detail.  The modes are the reference's `--evaluation_mode` choices (run.py:37-44):
  'averaged_moving_window'   eval.utils.fetch_logits: overlapping windows, posteriors averaged where they overlap;
  'buffered'                 eval.buffered_transcription.fetch_logits: chunks transcribed inside a context buffer;
  'windowed_attention'       one window over the whole recording (up to max_sequence_length frames) with every attention module
                             limited to seq_len // subsampling_factor // 2 tokens to either side.  The reference sets this in the
                             config before it builds the model; here the modules' windows are set for the duration of the call and
                             restored afterwards, also when the model raises.
The reference normalises with Whisper's EnglishTextNormalizer, which is not a dependency of this package: `normalize` defaults
to the identity (`.lower()` is applied as in the reference)."""
from __future__ import annotations

import contextlib
import dataclasses
import math
from typing import Callable, Iterable, List, Optional, Sequence, Tuple

import torch

from ..decoding.align import ctc_forced_align, word_timestamps
from ..decoding import confidence as confidence_module
from ..decoding.beam import BeamSearchCTCDecoder, _word_groups
from ..decoding.calibration import calibration_metrics, fit_temperature, frame_confidence_sweep
from ..decoding.confidence import (ConfidenceConfig, frame_confidence, greedy_confidence, spans_from_token_frames, token_confidence,
                                   word_confidence)
from ..decoding.greedy import GreedyCTCDecoder
from ..decoding.posterior import posterior_confidence_long
from ..decoding.segment import build_targets, ctc_segment, star_id
from ..hip import noise as noiser
from ..utils.audio_tools import HOP_LENGTH, SR, add_background_noise, add_gaussian_snr, grab_left_channel, resample, to_spectogram
from .buffered_transcription import fetch_logits as buffered_eval
from .utils import fetch_logits as moving_average_eval
from .wer import confusion_pairs, word_error_alignment, word_error_rate_detail

MODES = ('averaged_moving_window', 'buffered', 'windowed_attention')


def _decoder(model, tokenizer, beam_width: int, lm=None, alpha: float = 0.5, beta: float = 1.5, hotwords=None, hotword_weight: float = 10.0):
    """beam_width 1: the greedy decoder (per-frame argmax); above: prefix beam search, with the n-gram LM `lm` (decoding.lm.NGramLM)
    fused in if one is given, and `hotwords` (a list of strings or a decoding.hotwords.HotwordSet) boosted by hotword_weight inside
    the search if any are given."""
    if beam_width < 1:
        raise ValueError(f'beam_width must be at least 1, got {beam_width}')
    blank = model.decoder.num_classes - 1
    if beam_width == 1:
        if lm is not None:
            raise ValueError('a language model needs a beam search: beam_width must be above 1 (the greedy decoder takes no LM)')
        if hotwords is not None:
            raise ValueError('hotwords need a beam search: beam_width must be above 1 (greedy decoding cannot boost: it keeps one path)')
        return GreedyCTCDecoder(tokenizer=tokenizer, blank_id=blank)
    hot = {} if hotwords is None else dict(hotwords=hotwords, hotword_weight=hotword_weight)
    if lm is None:
        return BeamSearchCTCDecoder(tokenizer=tokenizer, blank_id=blank, beam_width=beam_width, **hot)
    return BeamSearchCTCDecoder(tokenizer=tokenizer, blank_id=blank, beam_width=beam_width, lm=lm, alpha=alpha, beta=beta, **hot)


class _Args:
    """Stand-in for the reference's argparse namespace when the caller has none (seq_len / overlap of -1 then have no default)."""
    def __init__(self):
        self.config = {}


def _windowed_modules(model) -> List[torch.nn.Module]:
    return [m for m in model.modules() if hasattr(m, 'left_window') and hasattr(m, 'right_window')]


@contextlib.contextmanager
def _evaluation_mode(model, evaluation_mode: str, seq_len: int, args):
    """(eval_fn, seq_len) of a mode.  'windowed_attention' limits every attention module for the duration of the block and restores
    the windows afterwards, also when the model raises."""
    if evaluation_mode not in MODES:
        raise ValueError(f'evaluation_mode must be one of {MODES}, got {evaluation_mode!r}')
    eval_fn = buffered_eval if evaluation_mode == 'buffered' else moving_average_eval
    modules = _windowed_modules(model) if evaluation_mode == 'windowed_attention' else []
    saved = [(m.left_window, m.right_window) for m in modules]
    try:
        if evaluation_mode == 'windowed_attention':
            window = seq_len // model.subsampling.subsampling_factor // 2      # // 2: applied in both directions
            for m in modules:
                m.left_window = m.right_window = window
            seq_len = int(getattr(args, 'max_sequence_length', 3600000))       # 10 hours
        yield eval_fn, seq_len
    finally:
        for m, (lw, rw) in zip(modules, saved):
            m.left_window, m.right_window = lw, rw


def evaluate(model, recordings: Iterable[Tuple[str, torch.Tensor, str]], tokenizer, seq_len: int, overlap: int,
             evaluation_mode: str = 'averaged_moving_window', normalize: Optional[Callable[[str], str]] = None,
             include_per_recording_evaluations: bool = False, args=None, beam_width: int = 1, lm=None, alpha: float = 0.5,
             beta: float = 1.5, hotwords=None, hotword_weight: float = 10.0) -> List[dict]:
    """WER of `model` over recordings, an iterable of (id, spec (1, F, T), gold_text).  Returns the reference's wer_data: a list
    of dicts recording / wer / words / ins_rate / del_rate / sub_rate, one per recording if asked for, and 'all' last.
    beam_width > 1 decodes with decoding.beam.BeamSearchCTCDecoder instead of the per-frame argmax; lm (a decoding.lm.NGramLM) with
    alpha, beta fuses an n-gram language model into that search; hotwords (a list of strings or a decoding.hotwords.HotwordSet) with
    hotword_weight boosts them inside it (pyctcdecode's decode_beams keywords)."""
    args = _Args() if args is None else args
    normalize = (lambda s: s) if normalize is None else normalize
    all_texts, all_golds, wer_data = [], [], []
    with _evaluation_mode(model, evaluation_mode, seq_len, args) as (eval_fn, seq_len):
        decoder = _decoder(model, tokenizer, beam_width, lm, alpha, beta, hotwords, hotword_weight)
        for rec_id, spec, gold_text in recordings:
            logits = eval_fn(args=args, model=model, spec=spec, seq_len=seq_len, overlap=overlap, tokenizer=tokenizer,
                             use_tqdm=False, return_numpy=False)
            out = normalize(decoder(logits)).lower()
            all_texts.append(out)
            all_golds.append(gold_text)
            if include_per_recording_evaluations:
                wer, words, ins_rate, del_rate, sub_rate = word_error_rate_detail(hypotheses=[out], references=[gold_text])
                wer_data.append({'recording': rec_id, 'wer': wer, 'words': words, 'ins_rate': ins_rate, 'del_rate': del_rate,
                                 'sub_rate': sub_rate})
    wer, words, ins_rate, del_rate, sub_rate = word_error_rate_detail(hypotheses=all_texts, references=all_golds)
    wer_data.append({'recording': 'all', 'wer': wer, 'words': words, 'ins_rate': ins_rate, 'del_rate': del_rate, 'sub_rate': sub_rate})
    return wer_data


def _left_at_16k(waveform: torch.Tensor, sample_rate: int, corrupt=None) -> torch.Tensor:
    """(1, L') left channel at 16 kHz: as it is, or through the resampler in one pass; then through `corrupt`, a callable
    (waveform, sample_rate=16000) -> waveform such as utils.augmentation.AddGaussianSNR, if one is given."""
    left = grab_left_channel(waveform) if sample_rate == SR else resample(waveform, sample_rate, SR, mix='left')
    return left if corrupt is None else corrupt(left, sample_rate=SR)


def transcribe(model, waveform: torch.Tensor, tokenizer, seq_len: int, overlap: int, evaluation_mode: str = 'averaged_moving_window',
               normalise: bool = True, args=None, beam_width: int = 1, lm=None, alpha: float = 0.5, beta: float = 1.5,
               sample_rate: int = SR, corrupt=None, hotwords=None, hotword_weight: float = 10.0) -> str:
    """Waveform to transcript: waveform (L,) or (channels, L) on the GPU at `sample_rate` Hz (16 kHz, or any rate
    utils.audio_tools.resample takes: its left channel is resampled to 16 kHz on the device first) -> `corrupt`, if given (a callable on the 16 kHz waveform:
    utils.augmentation.AddGaussianSNR / AddBackgroundNoise, the reference's noise experiments) -> spectrogram
    (utils.audio_tools.to_spectogram of the left channel) -> log-probs in `evaluation_mode` -> greedy CTC decoding (beam_width 1) or prefix beam search, with the n-gram LM `lm`
    fused in if one is given and `hotwords` (a list of strings or a decoding.hotwords.HotwordSet) boosted by hotword_weight inside it if any are given.  The text is returned as decoded (evaluate's `normalize` and lower() belong to scoring)."""
    args = _Args() if args is None else args
    spec = to_spectogram(_left_at_16k(waveform, sample_rate, corrupt), global_normalisation=normalise)
    with _evaluation_mode(model, evaluation_mode, seq_len, args) as (eval_fn, seq_len):
        logits = eval_fn(args=args, model=model, spec=spec, seq_len=seq_len, overlap=overlap, tokenizer=tokenizer, use_tqdm=False,
                         return_numpy=False)
        return _decoder(model, tokenizer, beam_width, lm, alpha, beta, hotwords, hotword_weight)(logits)


def transcribe_detail(model, waveform: torch.Tensor, tokenizer, seq_len: int, overlap: int, evaluation_mode: str = 'averaged_moving_window',
                      normalise: bool = True, args=None, beam_width: int = 1, lm=None, alpha: float = 0.5, beta: float = 1.5,
                      sample_rate: int = SR, corrupt=None, hotwords=None, hotword_weight: float = 10.0,
                      confidence: ConfidenceConfig = ConfidenceConfig(), temperature: Optional[float] = None, posterior: bool = False) -> dict:
    """`transcribe` with what it knows about its answer: {'text', 'tokens', 'token_confidence', 'words': [{'word', 'startTime',
    'endTime', 'confidence'}]}, the times in word_timestamps' '12.34s' form.  The keywords are transcribe's; `confidence` (a
    decoding.confidence.ConfidenceConfig) chooses the measure and the aggregations; `temperature` (what `calibrate` chose, say) takes
    the confidences of softmax(log_probs / temperature) and leaves the decoding as it is.  beam_width 1: greedy decoding, a token's
    confidence over its run of frames and the blanks behind it (without them if exclude_blank), its times from its own run.
    beam_width > 1: the best beam, the LM and the hotwords acting inside the search as in transcribe; token i covers the frames from
    its own to the next token's, a word lasts from its first token's frame to one past its last token's.  Frame, token and word
    confidences are computed on the device (include/sconf_confid.h).
    posterior=True adds what decoding.posterior knows (include/sconf_post.h; at temperature 1, for a recording of any length through
    posterior_confidence_long with the decoded ids and their spans): 'token_posterior', the posterior of every token among the strings
    at edit distance 1 in its slot; 'token_alternative', per token {'token': the best competing id, None for "delete", 'posterior'};
    and a 'posterior' on every word, its tokens' posteriors through the word aggregation of `confidence`."""
    args = _Args() if args is None else args
    spec = to_spectogram(_left_at_16k(waveform, sample_rate, corrupt), global_normalisation=normalise)
    with _evaluation_mode(model, evaluation_mode, seq_len, args) as (eval_fn, seq_len):
        logits = eval_fn(args=args, model=model, spec=spec, seq_len=seq_len, overlap=overlap, tokenizer=tokenizer, use_tqdm=False,
                         return_numpy=False)
        decoder = _decoder(model, tokenizer, beam_width, lm, alpha, beta, hotwords, hotword_weight)
    blank = model.decoder.num_classes - 1
    if beam_width == 1:
        g = greedy_confidence(logits, blank, confidence, temperature=temperature)
        ids, conf, times = g.tokens, g.token_confidence, [s[:2] for s in g.spans]
    else:
        out = decoder._search(logits, nbest=1)
        n = min(int(out.lengths[0]), out.tokens.shape[-1]) if int(out.count) else 0
        frames = out.token_frames[0, :n]
        idx, frame_conf = frame_confidence(logits, confidence, temperature=temperature)
        conf = token_confidence(frame_conf, idx, spans_from_token_frames(frames, logits.shape[0]), confidence, blank).tolist() if n else []
        ids, times = out.tokens[0, :n].tolist(), [[f, f + 1] for f in frames.tolist()]
    word_start = getattr(decoder, 'word_start', None)
    words = word_timestamps(ids, times, tokenizer, model.subsampling.subsampling_factor * HOP_LENGTH / SR, word_start=word_start)
    for w, c in zip(words, word_confidence(ids, conf, tokenizer, confidence, word_start)):
        w['confidence'] = c
    out = {'text': tokenizer.decode(ids), 'tokens': ids, 'token_confidence': conf, 'words': words}
    if posterior:
        pc = posterior_confidence_long(logits, ids, times, blank)
        packed = torch.cat([pc.token_posterior.view(torch.int32), pc.alternative, pc.alternative_posterior.view(torch.int32)]).cpu()   # the one copy
        n = len(ids)
        out['token_posterior'] = packed[:n].view(torch.float32).tolist()
        out['token_alternative'] = [{'token': None if a == blank else a, 'posterior': p}
                                    for a, p in zip(packed[n:2 * n].tolist(), packed[2 * n:].view(torch.float32).tolist())]
        for w, c in zip(words, word_confidence(ids, out['token_posterior'], tokenizer, confidence, word_start)):
            w['posterior'] = c
    return out


def _word_confidence_sweep(logits: torch.Tensor, blank: int, temperatures: Sequence[float], cfg: ConfidenceConfig, tokenizer, word_start=None):
    """The greedy words of logits (N, C) with their confidences at every temperature: (word texts, (K, words) f32 on the device).
    One sweep launch for the frames, one collapse, and one aggregate launch each for tokens and words over all K rows at once
    (row k of the (K, N) confidences is addressed by spans shifted by k N)."""
    idx, conf = frame_confidence_sweep(logits, temperatures, cfg)
    K, N = conf.shape
    targets, spans, tl = confidence_module.confid_kernels.runs(idx[None].contiguous(), None, int(blank), N)
    packed = torch.cat([tl, targets.reshape(-1)]).cpu()                                              # the one copy
    n = int(packed[0])
    ids = packed[1:1 + n].tolist()
    if n == 0:
        return [], torch.zeros(K, 0, dtype=torch.float32, device=conf.device)
    shift = torch.arange(K, device=conf.device, dtype=torch.int32)[:, None, None]
    frames = (spans[0, :n][:, (0, 2)][None] + shift * N).reshape(-1, 2).contiguous()
    tok = confidence_module.confid_kernels.aggregate(conf.reshape(-1), frames, cfg.aggregation, idx.repeat(K) if cfg.exclude_blank else None, int(blank))
    groups = _word_groups(ids, tokenizer, word_start)
    first_last = torch.tensor([[g[0], g[-1] + 1] for g in groups], dtype=torch.int32).to(conf.device)
    words = confidence_module.confid_kernels.aggregate(tok, (first_last[None] + shift * n).reshape(-1, 2).contiguous(), cfg.words, None, 0)
    return [tokenizer.decode([ids[k] for k in g]) for g in groups], words.reshape(K, len(groups))


def _word_posteriors(logits: torch.Tensor, blank: int, cfg: ConfidenceConfig, tokenizer, word_start=None) -> torch.Tensor:
    """(words,) f32 on the device: the posterior of every greedy word of logits (N, C), its tokens' posteriors
    (decoding.posterior.posterior_confidence_long) through cfg's word aggregation; the words are _word_confidence_sweep's."""
    g = greedy_confidence(logits, blank, cfg)
    if not g.tokens:
        return torch.zeros(0, dtype=torch.float32, device=g.frame_confidence.device)
    pc = posterior_confidence_long(logits, g.tokens, [s[:2] for s in g.spans], blank)
    groups = _word_groups(g.tokens, tokenizer, word_start)
    first_last = torch.tensor([[w[0], w[-1] + 1] for w in groups], dtype=torch.int32).to(pc.token_posterior.device)
    return confidence_module.confid_kernels.aggregate(pc.token_posterior.contiguous(), first_last, cfg.words, None, 0)


def calibrate(model, recordings: Iterable[Tuple[str, torch.Tensor, str]], tokenizer, seq_len: int, overlap: int,
              temperatures: Sequence[float] = (0.5, 0.67, 0.8, 1.0, 1.25, 1.5, 2.0, 3.0), confidence: ConfidenceConfig = ConfidenceConfig(),
              evaluation_mode: str = 'averaged_moving_window', normalize: Optional[Callable[[str], str]] = None, args=None,
              n_bins: int = 10, word_start=None, posterior: bool = False) -> dict:
    """Are the word confidences calibrated, and at which softmax temperature are they best?  recordings: (id, spec (1, F, T),
    gold_text) triples as `evaluate` takes them.  Each recording is decoded once (greedy); ONE launch of the temperature sweep gives
    its frame confidences at all `temperatures`, the aggregation of `confidence` makes token and word confidences of every row, and
    the edit alignment of the hypothesis words against the reference words (both through `normalize` and lower(); all recordings
    in one launch) labels every hypothesis word correct (a hit) or wrong (substituted or inserted).  A word that `normalize` cuts
    into several carries its confidence to each piece; one that it deletes drops out.  The words of all recordings are pooled.
    Returns {'temperatures', 'metrics': decoding.calibration.calibration_metrics per temperature, 'temperature': the grid point
    fit_temperature chooses (highest NCE), 'labels': the pooled 1 / 0 labels, 'confusion_pairs': (reference word, hypothesis word,
    count) of the substitutions, 'words': the number of pooled hypothesis words}.  posterior=True adds 'posterior_metrics': the
    calibration_metrics of the pooled word posteriors (decoding.posterior, at temperature 1) against the same labels, to set
    beside the entry of 'metrics' at temperature 1."""
    args = _Args() if args is None else args
    normalize = (lambda s: s) if normalize is None else normalize
    temperatures = [float(t) for t in temperatures]
    blank = model.decoder.num_classes - 1
    hyps, golds, confs, posts = [], [], [], []
    with _evaluation_mode(model, evaluation_mode, seq_len, args) as (eval_fn, seq_len):
        for rec_id, spec, gold_text in recordings:
            logits = eval_fn(args=args, model=model, spec=spec, seq_len=seq_len, overlap=overlap, tokenizer=tokenizer, use_tqdm=False,
                             return_numpy=False)
            words, conf = _word_confidence_sweep(logits, blank, temperatures, confidence, tokenizer, word_start)
            pieces, source = [], []
            for w, text in enumerate(words):
                for piece in normalize(text).lower().split():
                    pieces.append(piece)
                    source.append(w)
            hyps.append(' '.join(pieces))
            golds.append(' '.join(normalize(gold_text).lower().split()))
            confs.append(conf[:, torch.tensor(source, dtype=torch.long, device=conf.device)])
            if posterior:
                wp = _word_posteriors(logits, blank, confidence, tokenizer, word_start)
                posts.append(wp[torch.tensor(source, dtype=torch.long, device=wp.device)])
    if not hyps:
        raise ValueError('calibrate: no recordings')
    alignments = word_error_alignment(hyps, golds)
    labels = []
    for hyp, ops in zip(hyps, alignments):
        lab = [0] * len(hyp.split())
        for o in ops:
            if o['op'] == 'hit':
                lab[o['hyp_index']] = 1
        labels += lab
    pooled = torch.cat(confs, dim=1)
    correct = torch.tensor(labels, dtype=torch.float64)
    metrics = [calibration_metrics(pooled[k], correct, n_bins) for k in range(len(temperatures))]
    out = {'temperatures': temperatures, 'metrics': metrics, 'temperature': fit_temperature(None, None, temperatures, metrics=metrics),
           'labels': labels, 'confusion_pairs': confusion_pairs(alignments), 'words': len(labels)}
    if posterior:
        out['posterior_metrics'] = calibration_metrics(torch.cat(posts), correct, n_bins)
    return out


def spectrograms_of(recordings: Iterable[Tuple[str, torch.Tensor, str]], normalise: bool = True, sample_rate: int = SR, corrupt=None):
    """(id, waveform, gold_text) -> the (id, spec (1, F, T), gold_text) triples `evaluate` takes, one recording at a time; waveforms
    at `sample_rate` Hz, resampled to 16 kHz on the device where that is another rate, then through `corrupt` if one is given."""
    for rec_id, waveform, gold_text in recordings:
        yield rec_id, to_spectogram(_left_at_16k(waveform, sample_rate, corrupt), global_normalisation=normalise), gold_text


def sweep_spectrograms(waveform: torch.Tensor, snrs: Sequence[float], noise='gaussian', seed: int = 17925, row: int = 0,
                       normalise: bool = True, sample_rate: int = SR) -> torch.Tensor:
    """(K, F, T): the spectrograms of one recording corrupted at each of the K levels of `snrs` - what snr_sweep feeds the model for
    its recording number `row`.  The power is taken once per group of sconf_noise_max_levels levels, one launch mixes the group
    and to_spectogram runs on the (K, L) batch; level k is bit-equal to to_spectogram of a separate add_gaussian_snr(x, snrs[k],
    seed=seed, first_row=row) (add_background_noise(x, noise, snrs[k]))."""
    if not (isinstance(noise, str) and noise == 'gaussian') and not (torch.is_tensor(noise) and noise.dim() == 1):
        raise ValueError("noise must be 'gaussian' or a 1-D tensor (a 16 kHz clip)")
    left = _left_at_16k(waveform, sample_rate)[0]
    group = noiser.max_levels()
    specs = []
    for k0 in range(0, len(snrs), group):
        levels = [float(s) for s in snrs[k0:k0 + group]]
        mixed = add_gaussian_snr(left, levels, seed=seed, first_row=row) if isinstance(noise, str) else add_background_noise(left, noise, levels)
        specs.append(to_spectogram(mixed, global_normalisation=normalise))
    return specs[0] if len(specs) == 1 else torch.cat(specs)


def snr_sweep(model, recordings: Iterable[Tuple[str, torch.Tensor, str]], tokenizer, seq_len: int, overlap: int, snrs: Sequence[float],
              noise='gaussian', seed: int = 17925, normalise: bool = True, sample_rate: int = SR, **evaluate_keywords) -> List[dict]:
    """WER against SNR: `evaluate` over `recordings`, (id, waveform, gold_text) triples with the waveform (L,) or (channels, L) on the
    GPU, once per level of `snrs` (dB), the left channel at 16 kHz corrupted at that level before the spectrogram.
    noise: 'gaussian' - recording n gets the normals of (seed, row id n), the same sequence at every level as the reference's
    per-file re-seeding gives them - or a 1-D device tensor, a 16 kHz background clip that starts at 0 and repeats.
    Per recording the waveform's power is taken once and ONE launch mixes all the levels (sweep_spectrograms; in groups of
    sconf_noise_max_levels where there are more); to_spectogram runs on the (K, L) batch and each level then goes the way of `evaluate`, whose keywords
    (evaluation_mode, normalize, args, beam_width, lm, alpha, beta, hotwords, hotword_weight) pass through.
    Returns one record per level, in the order of `snrs`: {'snr_db', 'wer', 'words', 'ins_rate', 'del_rate', 'sub_rate'}."""
    snrs = [float(s) for s in snrs]
    if not snrs:
        raise ValueError('snr_sweep: no SNR levels')
    if 'include_per_recording_evaluations' in evaluate_keywords:
        raise ValueError('snr_sweep returns one record per level: include_per_recording_evaluations is not taken')
    per_level = [[] for _ in snrs]
    for n, (rec_id, waveform, gold_text) in enumerate(recordings):
        specs = sweep_spectrograms(waveform, snrs, noise, seed, n, normalise, sample_rate)
        for k in range(len(snrs)):
            per_level[k].append((rec_id, specs[k:k + 1], gold_text))
    records = []
    for snr, recs in zip(snrs, per_level):
        total = evaluate(model, recs, tokenizer, seq_len, overlap, **evaluate_keywords)[-1]
        records.append({'snr_db': snr, **{key: total[key] for key in ('wer', 'words', 'ins_rate', 'del_rate', 'sub_rate')}})
    return records


def align(model, spec: torch.Tensor, text: str, tokenizer, seq_len: int, overlap: int, evaluation_mode: str = 'averaged_moving_window',
          args=None, confidence: Optional[ConfidenceConfig] = None) -> List[dict]:
    """Word timestamps of a known transcript: log-probs of spec (1, F, T) exactly as `evaluate` computes them in `evaluation_mode`,
    CTC forced alignment of tokenizer.encode(text) on the GPU, then decoding.align.word_timestamps - a list of
    {'word', 'startTime', 'endTime', 'logp'} with times in the reference's '12.34s' form (one frame of the log-probs is
    subsampling_factor * HOP_LENGTH / SR seconds).  Raises ValueError when the transcript has more labels than the frames can emit.
    A transcript of up to 65535 labels is taken: a whole recording (from 8192 labels on through the long form of the aligner).
    confidence (a decoding.confidence.ConfidenceConfig): each record gains 'confidence', the word's confidence from the frame
    confidences over the alignment's own token spans (every frame of a span is the token's, so none is excluded as blank); None: the
    records of today."""
    args = _Args() if args is None else args
    with _evaluation_mode(model, evaluation_mode, seq_len, args) as (eval_fn, seq_len):
        logits = eval_fn(args=args, model=model, spec=spec, seq_len=seq_len, overlap=overlap, tokenizer=tokenizer, use_tqdm=False,
                         return_numpy=False)
    ids = [int(i) for i in tokenizer.encode(text)]
    al = ctc_forced_align(logits, ids, blank=model.decoder.num_classes - 1)
    if not math.isfinite(float(al.score)):
        raise ValueError(f'transcript of {len(ids)} labels cannot be emitted in {logits.shape[0]} frames')
    words = word_timestamps(ids, al.spans, tokenizer, model.subsampling.subsampling_factor * HOP_LENGTH / SR, token_logp=al.token_logp)
    if confidence is not None:
        idx, frame_conf = frame_confidence(logits, confidence)
        conf = token_confidence(frame_conf, None, al.spans[:len(ids)], dataclasses.replace(confidence, exclude_blank=False))
        for w, c in zip(words, word_confidence(ids, conf, tokenizer, confidence)):
            w['confidence'] = c
    return words


def align_waveform(model, waveform: torch.Tensor, text: str, tokenizer, seq_len: int, overlap: int,
                   evaluation_mode: str = 'averaged_moving_window', normalise: bool = True, args=None, sample_rate: int = SR,
                   corrupt=None, confidence: Optional[ConfidenceConfig] = None) -> List[dict]:
    """`align` from a waveform (L,) or (channels, L) on the GPU at `sample_rate` Hz: the spectrogram of the left channel (resampled to
    16 kHz where the rate is another, then through `corrupt` if one is given) in front, as `transcribe`."""
    spec = to_spectogram(_left_at_16k(waveform, sample_rate, corrupt), global_normalisation=normalise)
    return align(model, spec, text, tokenizer, seq_len, overlap, evaluation_mode=evaluation_mode, args=args, confidence=confidence)


def segment(model, spec: torch.Tensor, utterances: Sequence[str], tokenizer, seq_len: int, overlap: int,
            evaluation_mode: str = 'averaged_moving_window', star_between: bool = True, star_ends: bool = True, star_logp: float = 0.0,
            window: int = 30, min_confidence: Optional[float] = None, words: bool = False, args=None) -> List[dict]:
    """CTC segmentation of a loose transcript: `utterances` are the texts of a recording in order, with unknown times; they may skip
    parts of it (intros, music, adverts, cross-talk) and some may be wrong.  Log-probs of spec (1, F, T) exactly as `align` computes
    them, then decoding.segment.ctc_segment over [*] u0 [*] u1 ... [*] on the GPU (blank = num_classes - 1, the star = num_classes).
    Returns one {'text', 'startTime', 'endTime', 'confidence', 'logp'} per utterance, times in the '12.34s' form: 'logp' the mean
    log-prob per frame of the utterance, 'confidence' its lowest mean over `window` consecutive frames (Kürzinger's
    score_min_mean_over_L = 30, adopted, not tuned here).  min_confidence drops the records below it; words=True adds 'words', the
    `word_timestamps` records of the utterance's tokens.  star_between / star_ends place the stars; star_logp = 0 lets a star also
    take the cheap frames of the tokens beside it (they shrink towards one frame, as with torchaudio's <star>), a negative value
    makes it win only over frames that match nothing; a star always takes at least one frame.  No value has been tuned on real
    recordings here.  Raises ValueError when the row does not fit the frames, as `align` does."""
    args = _Args() if args is None else args
    with _evaluation_mode(model, evaluation_mode, seq_len, args) as (eval_fn, seq_len):
        logits = eval_fn(args=args, model=model, spec=spec, seq_len=seq_len, overlap=overlap, tokenizer=tokenizer, use_tqdm=False,
                         return_numpy=False)
    ids = [[int(i) for i in tokenizer.encode(u)] for u in utterances]
    C = model.decoder.num_classes
    seg = ctc_segment(logits, ids, blank=C - 1, star_between=star_between, star_ends=star_ends, star_logp=star_logp, window=window)
    if not math.isfinite(float(seg.alignment.score)):
        raise ValueError(f'{len(ids)} utterances of {sum(len(u) for u in ids)} labels cannot be emitted in {logits.shape[0]} frames')
    spf = model.subsampling.subsampling_factor * HOP_LENGTH / SR
    ranges = build_targets(ids, star_id(C), star_between, star_ends)[1]
    frames, logp, conf = seg.utt_frames.tolist(), seg.utt_logp.tolist(), seg.utt_conf.tolist()
    spans, token_logp = seg.alignment.spans, seg.alignment.token_logp
    records = []
    for k, (text, (j0, j1)) in enumerate(zip(utterances, ranges)):
        if min_confidence is not None and not conf[k] >= min_confidence:
            continue
        r = {'text': text, 'startTime': f'{frames[k][0] * spf:.2f}s', 'endTime': f'{frames[k][1] * spf:.2f}s', 'confidence': conf[k],
             'logp': logp[k]}
        if words:
            r['words'] = word_timestamps(ids[k], spans[j0:j1], tokenizer, spf, token_logp=token_logp[j0:j1])
        records.append(r)
    return records


def segment_waveform(model, waveform: torch.Tensor, utterances: Sequence[str], tokenizer, seq_len: int, overlap: int,
                     evaluation_mode: str = 'averaged_moving_window', normalise: bool = True, sample_rate: int = SR, corrupt=None,
                     **kwargs) -> List[dict]:
    """`segment` from a waveform (L,) or (channels, L) on the GPU at `sample_rate` Hz: the spectrogram of the left channel (resampled
    to 16 kHz where the rate is another, then through `corrupt` if one is given) in front, as `align_waveform`."""
    spec = to_spectogram(_left_at_16k(waveform, sample_rate, corrupt), global_normalisation=normalise)
    return segment(model, spec, utterances, tokenizer, seq_len, overlap, evaluation_mode=evaluation_mode, **kwargs)


def search(model, spec: torch.Tensor, keywords, tokenizer, seq_len: int, overlap: int, evaluation_mode: str = 'averaged_moving_window',
           min_score_per_label: float = -0.5, max_hits: int = 64, args=None) -> List[dict]:
    """Keyword search: where in the recording is each of `keywords` (a list of strings, or a decoding.kws.KeywordSet) said?
    Log-probs of spec (1, F, T) exactly as `align` computes them, then decoding.kws.ctc_keyword_search on the GPU
    (blank = num_classes - 1).  Returns one {'keyword', 'startTime', 'endTime', 'score'} per hit, times in the '12.34s' form, sorted
    by start.  'score' is the total log-likelihood ratio of the keyword's best path over the span against the greedy path over the
    same frames: 0 means the keyword IS the greedy decode of that span.  A keyword is reported from min_score_per_label times its
    number of tokens on (the default is not tuned on real recordings; it is ignored for a KeywordSet, which carries its own).  A
    keyword with more than max_hits hits carries 'truncated': True on its records."""
    from ..decoding.kws import KeywordSet, ctc_keyword_search
    args = _Args() if args is None else args
    with _evaluation_mode(model, evaluation_mode, seq_len, args) as (eval_fn, seq_len):
        logits = eval_fn(args=args, model=model, spec=spec, seq_len=seq_len, overlap=overlap, tokenizer=tokenizer, use_tqdm=False,
                         return_numpy=False)
    if not isinstance(keywords, KeywordSet):
        keywords = KeywordSet.from_text(keywords, tokenizer, min_score_per_label=min_score_per_label)
    hits = ctc_keyword_search(logits, keywords, blank=model.decoder.num_classes - 1, max_hits=max_hits)
    return hits.records(model.subsampling.subsampling_factor * HOP_LENGTH / SR)


def search_waveform(model, waveform: torch.Tensor, keywords, tokenizer, seq_len: int, overlap: int,
                    evaluation_mode: str = 'averaged_moving_window', normalise: bool = True, sample_rate: int = SR, corrupt=None,
                    **kwargs) -> List[dict]:
    """`search` from a waveform (L,) or (channels, L) on the GPU at `sample_rate` Hz: the spectrogram of the left channel (resampled
    to 16 kHz where the rate is another, then through `corrupt` if one is given) in front, as `align_waveform`."""
    spec = to_spectogram(_left_at_16k(waveform, sample_rate, corrupt), global_normalisation=normalise)
    return search(model, spec, keywords, tokenizer, seq_len, overlap, evaluation_mode=evaluation_mode, **kwargs)
