"""Dynamic evaluation: test-time adaptation on CTC pseudo-labels — mirror of lcasr/eval/dynamic_eval.py:11-142.

For every window of a long recording: `num_negatives` SpecAugment-ed copies plus the clean one go through ONE forward, the
clean copy is greedy-decoded into pseudo-labels, the augmented copies take a CTC loss against them, MADGRAD takes one step,
and the clean copy's posteriors (those of the forward BEFORE that step) are overlap-averaged; at the end the parameters are
put back.  Same signature, window arithmetic and loss scaling as the reference; what changes is the execution:

  * repeat + clone + the masked_fill sequence are one kernel (ops.spec_mask), the fill value (spectrogram mean) is a device
    scalar (ops.mean_f32): no host sync before the forward;
  * the posteriors never leave the GPU.  retokenize=True reproduces `tokenizer.encode(decoder(...))` (:92-93): only the
    collapsed label ids cross to the host.  retokenize=False builds the targets on the device (ops.ctc_collapse): one scalar per
    window crosses (the number of labels, to size the target tensor);
  * the overlap-average is ops.overlap_add_exp_ / ops.overlap_finalize, as in fetch_logits.

Deliberate differences from the reference:
  * buffers (BatchRenorm running statistics) are snapshotted and restored with the parameters, so a model left in train mode
    does not leak one recording's statistics into the next; the restore also runs when the loop raises;
  * the optimiser built here re-points the parameters into flat buffers of its own (optim.FlatParams); before returning every
    parameter's `.data` / `.grad` is moved back to exactly where it was, so a Trainer that owned the model goes on training it;
  * the mean used as fill value is taken over the window once instead of over its `num_negatives` identical copies.
The model's train/eval mode is left as the caller set it (the reference never touches it).
"""
from __future__ import annotations

import random

import torch

from .. import functional as Fn          # Fn.ops: the HIP op layer (tests swap it for the CPU kernel references)
from ..decoding.greedy import GreedyCTCDecoder
from ..optim import MADGRAD
from ..utils.augmentation import SpecAugment
from .utils import resolve_windowing, window_plan

DEFAULT_SPEC_AUGMENT = {'n_time_masks': 2, 'n_freq_masks': 3, 'freq_mask_param': 42, 'time_mask_param': -1, 'min_p': 0.05,
                        'zero_masking': False}


def dynamic_eval_ctc_loss(args, model, spec: torch.Tensor, seq_len: int, overlap: int, tokenizer, use_tqdm=True, optim=MADGRAD,
                          num_negatives: int = 2, lr_args: dict = {'lr': 8e-5}, spec_augment_config=DEFAULT_SPEC_AUGMENT,
                          augmentation=None, retokenize: bool = True, return_numpy: bool = True):
    """Overlap-averaged log-probs (N, vocab+1) of spec (1, F, T) while adapting the model window by window; the model is
    returned to its state before the call.  augmentation: an object with draw(shape) / apply(...)
    (default SpecAugment(**spec_augment_config)); a `zero_masking` attribute selects 0 as fill value."""
    if spec.dim() != 3 or spec.shape[0] != 1:
        raise ValueError(f'spec must be (1, features, time), got {tuple(spec.shape)}')
    spec_n = spec.shape[-1]
    downsampling_factor = args.config.get('model', {}).get('subsampling_factor', model.subsampling.subsampling_factor)   # :33
    assert args.config.get('training', {}).get('max_seq_len', 0) == 0, 'caching is not used anymore'                      # :57
    seq_len, overlap = resolve_windowing(args, spec_n, seq_len, overlap, downsampling_factor)                             # :34, :52-55, :58

    dev = next(model.parameters()).device
    blank = model.decoder.num_classes - 1
    C = tokenizer.vocab_size() + 1
    decoder = GreedyCTCDecoder(tokenizer=tokenizer, blank_id=blank)
    if augmentation is None:
        augmentation = SpecAugment(**spec_augment_config)
    spec = spec.to(dev)
    training_data = {s: spec[:, :, s:s + n].to(torch.float32).contiguous() for s, n in window_plan(spec_n, seq_len, overlap)}   # :64-73
    epochs = getattr(args, 'epochs', 1)

    # Snapshot (:37-38).  Building the optimiser moves every trainable parameter into a new flat buffer, so where each
    # parameter and its gradient lived is remembered as well and handed back in the `finally`.
    home = [(p, p.data, p.grad) for p in model.parameters()]
    saved = [p.detach().clone() for p in model.parameters()]
    saved_buffers = [(b, b.detach().clone()) for b in model.buffers()]
    model_outputs = {}
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    try:
        optimizer = optim(model.parameters(), **lr_args)                                                                  # :48, fresh per call
        direct = hasattr(optimizer, 'flat')                       # flat gradient buffer attached: the kernels accumulate straight into it
        for epoch in range(epochs):
            model_outputs = {}                                                                                            # :78: only the last epoch is averaged
            keys = list(training_data.keys())
            keys = random.sample(keys, len(keys)) if getattr(args, 'shuffle', False) else keys                            # :80
            if use_tqdm:
                from tqdm import tqdm
                keys = tqdm(keys)
            for i in keys:
                window = training_data[i]                                                                                 # (1, F, u_len)
                u_len = window.shape[-1]
                # :84-86: augmented copies first, clean copy last (its rows get empty intervals: a plain copy)
                t_iv, f_iv = augmentation.draw((num_negatives,) + tuple(window.shape[1:]))
                t_iv = torch.cat([t_iv.to(dev), t_iv.new_zeros(1, *t_iv.shape[1:]).to(dev)]).contiguous()
                f_iv = torch.cat([f_iv.to(dev), f_iv.new_zeros(1, *f_iv.shape[1:]).to(dev)]).contiguous()
                # the fill value: 0, or the mean over the augmented copies' slice (augmentation.py:70-73) = the window's mean
                mask_value = zero if getattr(augmentation, 'zero_masking', False) else Fn.ops.mean_f32(window)
                audio_chunk = augmentation.apply(window, t_iv, f_iv, mask_value, batch=num_negatives + 1)
                posteriors = model(audio_signal=audio_chunk)['final_posteriors']                                          # :90
                clean = posteriors[-1].detach().float().contiguous()
                N = posteriors.shape[1]
                if retokenize:                                                                                            # :92-93
                    ids = tokenizer.encode(decoder(clean))
                    S = len(ids)
                    targets = torch.zeros(1, max(S, 1), dtype=torch.int32)
                    targets[0, :S] = torch.as_tensor(ids, dtype=torch.int32)
                    targets = targets.to(dev)
                else:
                    targets, tl = Fn.ops.ctc_collapse(clean[None], None, blank)
                    S = int(tl[0])                                          # the one scalar that crosses to the host
                    targets = targets[:, :max(S, 1)]
                # an all-blank window has S = 0: one padding label of length 0, the loss is then -sum log p(blank)
                targets = targets.expand(num_negatives, -1).contiguous()
                target_lengths = torch.full((num_negatives,), S, dtype=torch.int32, device=dev)
                input_lengths = torch.full((num_negatives,), N, dtype=torch.int32, device=dev)
                augmented_outs = posteriors[:num_negatives]                                                               # :94
                loss = Fn.ctc_nll(augmented_outs, targets, input_lengths, target_lengths, blank).sum() / (N * num_negatives)   # :96-100
                optimizer.zero_grad()                                                                                     # :109-111
                Fn.set_direct_grad(direct)
                try:
                    loss.backward()
                finally:
                    Fn.set_direct_grad(False)
                optimizer.step()                                            # no x100, no clipping (MADGRAD.step: max_norm = 0)
                ds_len = clean.shape[-2]                                                                                  # :113-118
                model_outputs[i] = {'logits': clean, 'ds_len': ds_len, 'overlap_ds': int(overlap / (u_len / ds_len))}
    finally:
        with torch.no_grad():                                                                                             # :138-139
            for (p, data, grad), s in zip(home, saved):
                data.copy_(s)
                p.data, p.grad = data, grad
            for b, s in saved_buffers:
                b.copy_(s)
        Fn.clear_weight_cache()                                   # bf16 shadows registered against the optimiser's flat buffer are stale

    acc = torch.zeros(spec_n // 4 + seq_len, C, dtype=torch.float32, device=dev)                                          # :61
    count = torch.zeros(spec_n // 4 + seq_len, dtype=torch.float32, device=dev)
    logit_position = 0
    for i in sorted(model_outputs.keys()):                                                                                # :122-127, window-start order
        o = model_outputs[i]
        logit_position -= o['overlap_ds'] if i != 0 else 0
        Fn.ops.overlap_add_exp_(o['logits'][None], acc, count, logit_position, o['ds_len'])
        logit_position += o['ds_len']
    logits = Fn.ops.overlap_finalize(acc, count, logit_position)                                                          # :129-135
    return logits.cpu().numpy() if return_numpy else logits


dynamic_eval = dynamic_eval_ctc_loss
