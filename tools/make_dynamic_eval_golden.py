"""Fixture generator for dynamic evaluation — TEST INFRASTRUCTURE ONLY (development container only).

Runs the reference implementation's own `dynamic_eval_ctc_loss` (imported at run time from REF, CPU, fp32) on a tiny,
pre-trained eval-mode model and writes tests/golden/dyneval_model.npz (config + weights) and tests/golden/dyneval_cases.npz
(per case: recorded SpecAugment intervals, pseudo-labels, per-step losses, final averaged log-probs, parameter-change norm,
and the reference's own bf16-autocast noise against its fp32 run).  Inert where REF does not exist.

Stand-ins written here, because the libraries are absent: `lcasr.utils.audio_tools`, a `madgrad` module whose MADGRAD is the
reference's lcasr.optim.madgrad.MADGRAD, a `torchaudio.functional` with mask_along_axis[_iid] written to the interval law
documented by torchaudio (see lcasr_amd/utils/augmentation.py) that records every interval it draws and can replay them,
and a one-character-per-id tokenizer.

Why pre-training: a random-init model's arg-max sits on near-ties, so bf16 noise would change the pseudo-labels and every
number after them.  The model is trained (eval mode, no augmentation) on exactly the windows the cases use, against fixed
random targets that are consistent across the overlapping windows, until the labels are decisive.  CONDITION asserted at
generation time: at every pseudo-label of every window and epoch the clean copy's top-1/top-2 log-prob gap is >= MIN_GAP,
and the bf16-autocast re-run with the recorded intervals gives identical pseudo-labels.  The ratio of the masked cases'
per-step loss to the no-mask case's is stored too (`loss_ratio`); with the default masks it came out far above 1 without
touching the masks or the amount of pre-training (neither was changed for that).

The two-epoch case must show adaptation (epoch-2 summed loss below epoch-1's).  With fresh iid masks in every epoch the summed
loss of five windows is dominated by where the masks fall: of the seeds 200..211 probed, six gave a lower second epoch and
four of those also kept the gap condition (200, 201, 203, 211); 203 is used (1.24 -> 0.33).

Usage:  python tools/make_dynamic_eval_golden.py [pretrain|cases|all]
"""
from __future__ import annotations

import os
import sys
import types
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = '/root/reference'
GOLD = os.path.join(ROOT, 'tests', 'golden')

TINY = dict(vocab_size=127, n_layers=2, d_model=64, n_heads=2, head_dim=32, subsampling_conv_channels=32, use_rotary=True,
            rotary_base_freq=1500000, decoder_norm=True, self_conditioning=True, bias_in_ff=False, default_norm='layer_norm')
MIN_GAP = 2.0
PRETRAIN_STEPS = 2000
PRETRAIN_LR = 1e-3
SPEC_AUG = dict(n_time_masks=2, n_freq_masks=3, freq_mask_param=42, time_mask_param=-1, min_p=0.05, zero_masking=False)
# (name, seq_len, overlap, epochs, spec-augment overrides, seed)
CASES = [('w256', 256, 64, 1, {}, 101), ('w256_e2', 256, 64, 2, {}, 203), ('single', 2048, 0, 1, {}, 103),
         ('zero_mask', 256, 64, 1, dict(zero_masking=True), 104), ('no_mask', 256, 64, 1, dict(n_time_masks=0, n_freq_masks=0), 105)]


# ---- stand-in torchaudio.functional: interval law + recorder / replayer ---------------------------------------------------
class MaskTape:
    """Every mask call appends (is_time, start (B,), end (B,)); with `replay` set the intervals are taken from it instead."""
    def __init__(self): self.rec, self.replay = [], None

    def intervals(self, B, size, mask_param, p, is_time):
        if self.replay is not None:
            t, s, e = self.replay.pop(0)
            assert t == is_time and s.numel() == B
        else:
            mp = mask_param if p == 1.0 else min(mask_param, int(size * p))
            if mp < 1:
                s = e = torch.zeros(B, dtype=torch.long)
            else:
                value = torch.rand(B) * mp
                min_value = torch.rand(B) * (size - value)
                s = min_value.floor().long()
                e = s + value.floor().long()
        self.rec.append((is_time, s.clone(), e.clone()))
        return s, e


TAPE = MaskTape()


def _fill(x, s, e, mask_value, axis):
    size = x.size(axis)
    pos = torch.arange(size)
    m = (pos[None, :] >= s[:, None]) & (pos[None, :] < e[:, None])          # (B, size)
    shape = [x.shape[0]] + [1] * (x.dim() - 1)
    shape[axis] = size
    return x.masked_fill(m.view(shape), mask_value)


def mask_along_axis_iid(specgrams, mask_param, mask_value, axis, p=1.0):
    assert specgrams.dim() == 4 and axis in (2, 3)
    s, e = TAPE.intervals(specgrams.shape[0], specgrams.size(axis), mask_param, p, axis == 3)
    return _fill(specgrams, s, e, mask_value, axis)


def mask_along_axis(specgram, mask_param, mask_value, axis, p=1.0):
    is_time = axis == specgram.dim() - 1
    s, e = TAPE.intervals(1, specgram.size(axis), mask_param, p, is_time)
    x = specgram.reshape(1, *specgram.shape)
    return _fill(x, s, e, mask_value, axis + 1).reshape(specgram.shape)


class Tok:
    """One character per id, so encode(decode(ids)) == ids; `seen` keeps what the reference asked to encode."""
    def __init__(self, V): self.V, self.seen = V, []
    def vocab_size(self): return self.V
    def decode(self, ids): return ''.join(chr(0x100 + int(i)) for i in ids)
    def encode(self, s):
        ids = [ord(c) - 0x100 for c in s]
        self.seen.append(ids)
        return ids


def load_reference():
    sys.path.insert(0, REF)
    for name in ('lcasr', 'lcasr.utils', 'lcasr.models', 'lcasr.optim', 'lcasr.eval', 'lcasr.decoding'):
        m = types.ModuleType(name); m.__path__ = [os.path.join(REF, *name.split('.'))]; sys.modules[name] = m
    oc = types.ModuleType('omegaconf'); oc2 = types.ModuleType('omegaconf.omegaconf')
    oc2.OmegaConf = object; oc.omegaconf = oc2; oc.OmegaConf = object
    sys.modules['omegaconf'] = oc; sys.modules['omegaconf.omegaconf'] = oc2
    at = types.ModuleType('lcasr.utils.audio_tools'); at.total_frames = lambda s: int(s * 100); at.total_seconds = lambda f: f / 100
    sys.modules['lcasr.utils.audio_tools'] = at
    ta = types.ModuleType('torchaudio'); taf = types.ModuleType('torchaudio.functional')
    taf.mask_along_axis_iid, taf.mask_along_axis = mask_along_axis_iid, mask_along_axis
    ta.functional = taf
    sys.modules['torchaudio'] = ta; sys.modules['torchaudio.functional'] = taf
    warnings.filterwarnings('ignore')
    from lcasr.optim.madgrad import MADGRAD
    mg = types.ModuleType('madgrad'); mg.MADGRAD = MADGRAD
    sys.modules['madgrad'] = mg
    from lcasr.models.sconformer_xl import SCConformerXL
    from lcasr.eval.dynamic_eval import dynamic_eval_ctc_loss
    return SCConformerXL, MADGRAD, dynamic_eval_ctc_loss


def the_spec():
    """The recording of infer_tiny.npz (randn(1, 80, 1000)): shared so that it is stored once."""
    return torch.from_numpy(np.load(os.path.join(GOLD, 'infer_tiny.npz'))['spec'].copy())


def min_gap(lp):
    top = lp.float().topk(2, dim=-1).values
    return float((top[..., 0] - top[..., 1]).min())


# ---- stage 1: pre-train until the labels are decisive ---------------------------------------------------------------------
def pretrain(SC, MADGRAD):
    torch.manual_seed(12345)
    model = SC(**TINY)
    model.eval(); model.device = 'cpu'
    spec = the_spec()
    g = torch.Generator().manual_seed(2024)
    glob = torch.randint(0, TINY['vocab_size'], (31,), generator=g)            # one token per 4 output frames of the recording
    starts = [0, 192, 384, 576]
    full = torch.cat([spec[:, :, s:s + 256] for s in starts])                    # (4, 80, 256) -> 32 frames each
    full_tg = torch.stack([glob[6 * k:6 * k + 8] for k in range(4)])             # tokens whose place falls inside the window
    items = [(full, full_tg), (spec[:, :, 768:1000], glob[24:31][None]), (spec, glob[None])]
    opt = MADGRAD(model.parameters(), lr=PRETRAIN_LR)
    ctc = torch.nn.CTCLoss(blank=TINY['vocab_size'], reduction='sum')
    for step in range(PRETRAIN_STEPS):
        opt.zero_grad()
        tot, gaps = 0.0, []
        for x, tg in items:
            lp = model(audio_signal=x)['final_posteriors']
            B, N, _ = lp.shape
            loss = ctc(lp.transpose(0, 1), tg, torch.full((B,), N), torch.full((B,), tg.shape[1])) / tg.numel()
            loss.backward(); tot += float(loss); gaps.append(min_gap(lp.detach()))
        opt.step()
        if step % 50 == 0 or step == PRETRAIN_STEPS - 1:
            print(f'[pretrain {step}] loss/token {tot / 3:.5f} min gaps full/ragged/whole {gaps[0]:.2f} {gaps[1]:.2f} {gaps[2]:.2f}', flush=True)
    fx = {'cfg.' + k: np.array(v) for k, v in TINY.items()}
    for k, v in model.state_dict().items(): fx['w.' + k] = v.detach().numpy()
    np.savez_compressed(os.path.join(GOLD, 'dyneval_model.npz'), **fx)


# ---- stage 2: the reference's dynamic_eval_ctc_loss, fp32 and under bf16 autocast -----------------------------------------
def run_reference(SC, MADGRAD, dyn, sd, case, replay=None, autocast=False):
    name, seq_len, overlap, epochs, aug_over, seed = case
    model = SC(**TINY); model.load_state_dict(sd); model.eval(); model.device = 'cpu'
    tok = Tok(TINY['vocab_size'])
    rec = dict(gaps=[], sums=[], dnorm=[])
    model.register_forward_hook(lambda _m, _i, out: rec['gaps'].append(min_gap(out['final_posteriors'][-1].detach())))

    class RecCTC(torch.nn.CTCLoss):                                                 # the summed loss and its normaliser, per step
        def forward(self, lp, tg, il, tl):
            out = super().forward(lp, tg, il, tl)
            rec['sums'].append(float(out.detach().float()) / float(il.sum()))
            return out

    class RecOpt(MADGRAD):                                                          # parameter-change norm after every step
        def __init__(self, params, **kw):
            params = list(params)
            super().__init__(params, **kw)
            self._all, self._p0 = params, [p.detach().clone() for p in params]
        def step(self, closure=None):
            r = super().step(closure)
            rec['dnorm'].append(float(sum(float((p.detach() - q).double().pow(2).sum()) for p, q in zip(self._all, self._p0)) ** 0.5))
            return r

    args = types.SimpleNamespace(config={'model': {'subsampling_factor': 8}, 'audio_chunking': {'size': 512, 'overlap': 128}, 'training': {}},
                                 epochs=epochs, shuffle=False)
    TAPE.rec, TAPE.replay = [], (list(replay) if replay is not None else None)
    torch.manual_seed(seed)
    real = torch.nn.CTCLoss
    torch.nn.CTCLoss = RecCTC
    try:
        with torch.autocast('cpu', dtype=torch.bfloat16, enabled=autocast):
            logp = dyn(args, model, the_spec(), seq_len, overlap, tok, use_tqdm=False, optim=RecOpt, spec_augment_config=dict(SPEC_AUG, **aug_over))
    finally:
        torch.nn.CTCLoss = real
    for (k, v) in model.state_dict().items():
        assert torch.equal(v, sd[k]), f'reference did not restore {k}'
    return dict(logp=logp, labels=tok.seen, losses=rec['sums'], gaps=rec['gaps'], dnorm=rec['dnorm'][-1], tape=TAPE.rec)


def cases(SC, MADGRAD, dyn):
    mf = np.load(os.path.join(GOLD, 'dyneval_model.npz'))
    sd = {k[2:]: torch.from_numpy(mf[k].copy()) for k in mf.files if k.startswith('w.')}
    fx, mean_loss = {'names': np.array([c[0] for c in CASES])}, {}
    for case in CASES:
        name, seq_len, overlap, epochs, aug_over, seed = case
        aug = dict(SPEC_AUG, **aug_over)
        a = run_reference(SC, MADGRAD, dyn, sd, case)
        b = run_reference(SC, MADGRAD, dyn, sd, case, replay=a['tape'], autocast=True)
        visits = len(a['labels'])
        assert min(a['gaps']) >= MIN_GAP, f"{name}: top-1/top-2 gap {min(a['gaps']):.3f} below {MIN_GAP}: change the case"
        assert a['labels'] == b['labels'], f'{name}: bf16 autocast changed the pseudo-labels: change the case'
        n_t, n_f, nn_ = aug['n_time_masks'], aug['n_freq_masks'], 2
        assert len(a['tape']) == visits * (n_t + n_f)
        t_iv = np.zeros((visits, nn_, n_t, 2), np.int32); f_iv = np.zeros((visits, nn_, n_f, 2), np.int32)
        for v in range(visits):
            calls = a['tape'][v * (n_t + n_f):(v + 1) * (n_t + n_f)]
            assert all(c[0] for c in calls[:n_t]) and not any(c[0] for c in calls[n_t:])
            for j, (_, s, e) in enumerate(calls[:n_t]): t_iv[v, :, j, 0], t_iv[v, :, j, 1] = s.numpy(), e.numpy()
            for j, (_, s, e) in enumerate(calls[n_t:]): f_iv[v, :, j, 0], f_iv[v, :, j, 1] = s.numpy(), e.numpy()
        smax = max(1, max(len(l) for l in a['labels']))
        labels = np.full((visits, smax), -1, np.int32)
        for v, l in enumerate(a['labels']): labels[v, :len(l)] = l
        la, lb = np.array(a['losses']), np.array(b['losses'])
        per_epoch = la.reshape(epochs, -1).sum(1)
        if epochs > 1:
            assert per_epoch[-1] < per_epoch[0], f'{name}: no adaptation: epoch losses {per_epoch}'
        d = np.abs(a['logp'].astype(np.float64) - b['logp'].astype(np.float64))
        noise = np.array([d.max(), d.mean(), np.abs(np.exp(a['logp'].astype(np.float64)) - np.exp(b['logp'].astype(np.float64))).max(),
                          (np.abs(la - lb) / np.abs(la)).max(), abs(a['dnorm'] - b['dnorm']) / a['dnorm']])
        mean_loss[name] = la.mean()
        p = f'case.{name}.'
        fx.update({p + 'cfg': np.array([seq_len, overlap, epochs, int(aug['zero_masking']), n_t, n_f, nn_], np.int64), p + 't_iv': t_iv, p + 'f_iv': f_iv,
                   p + 'labels': labels, p + 'label_len': np.array([len(l) for l in a['labels']], np.int32), p + 'losses': la,
                   p + 'logp': a['logp'].astype(np.float32), p + 'dnorm': np.array(a['dnorm']), p + 'min_gap': np.array(min(a['gaps'])),
                   p + 'noise': noise, p + 'epoch_loss': per_epoch})
        print(f"[{name}] visits {visits} rows {a['logp'].shape[0]} min gap {min(a['gaps']):.2f} labels/window {[len(l) for l in a['labels']]} "
              f"loss {la.min():.4g}..{la.max():.4g} epoch sums {per_epoch} dnorm {a['dnorm']:.4e}\n    autocast noise: logp max {noise[0]:.3f} mean {noise[1]:.4f} "
              f"prob max {noise[2]:.3e} loss rel {noise[3]:.3e} dnorm rel {noise[4]:.3e}", flush=True)
    for name, v in mean_loss.items():
        fx[f'loss_ratio.{name}'] = np.array(v / mean_loss['no_mask'])
        print(f'[{name}] mean per-step loss / no-mask case: {v / mean_loss["no_mask"]:.1f}')
    assert all(fx[f'loss_ratio.{n}'] > 10 for n in ('w256', 'w256_e2', 'single', 'zero_mask')), 'the augmentation does not bite'
    np.savez_compressed(os.path.join(GOLD, 'dyneval_cases.npz'), **fx)


def main():
    if not os.path.isdir(REF):
        print('reference not present: nothing to do'); return
    what = sys.argv[1] if len(sys.argv) > 1 else 'all'
    torch.set_num_threads(8)
    SC, MADGRAD, dyn = load_reference()
    if what in ('pretrain', 'all'): pretrain(SC, MADGRAD)
    if what in ('cases', 'all'): cases(SC, MADGRAD, dyn)


if __name__ == '__main__':
    main()
