"""Plain-PyTorch references of the SpecAugment / dynamic-evaluation ops (same signatures as lcasr_amd.hip.ops) and the
helpers the CPU and GPU dynamic-evaluation tests share: fixture access, an augmentation that replays recorded intervals,
recorders for pseudo-labels / losses / parameter change, and the comparison against the fixture.

Bounds (set by the issue, not by the code under test): pseudo-labels and restored state are exact; final log-probs,
probabilities, per-step losses and the parameter-change norm may differ from the reference's fp32 run by at most 2x the
reference's OWN fp32-vs-bf16-autocast difference on the same case (`case.<name>.noise` in the fixture)."""
import numpy as np
import torch

from conftest import golden_cfg, golden_state_dict, load_golden

f32 = torch.float32


# ---- op references ---------------------------------------------------------------------------------------------------------
def spec_mask(src, t_iv, f_iv, mask_value, batch=None):
    Bs, Fq, T = src.shape
    B = Bs if batch is None else int(batch)
    x = src.expand(B, Fq, T).clone()
    t, f = torch.arange(T, device=src.device), torch.arange(Fq, device=src.device)
    for j in range(t_iv.shape[1]):                             # the reference's order: one masked_fill per mask
        m = (t[None, :] >= t_iv[:, j, 0:1]) & (t[None, :] < t_iv[:, j, 1:2])
        x = x.masked_fill(m[:, None, :], mask_value)
    for j in range(f_iv.shape[1]):
        m = (f[None, :] >= f_iv[:, j, 0:1]) & (f[None, :] < f_iv[:, j, 1:2])
        x = x.masked_fill(m[:, :, None], mask_value)
    return x


def mean_f32(x, lengths=None):
    if lengths is None:
        return x.double().mean().to(f32)
    T = x.shape[-1]
    keep = torch.arange(T, device=x.device)[None, :] < lengths[:, None]                       # (B, T)
    keep = keep.view(x.shape[0], *([1] * (x.dim() - 2)), T).expand(x.shape)
    return x[keep].double().mean().to(f32)


def greedy_ids(emission, blank):
    """lcasr/decoding/greedy.py:19-21 on one (N, C) sequence."""
    if emission.shape[0] == 0:
        return []
    idx = torch.unique_consecutive(torch.argmax(emission, dim=-1), dim=-1).tolist()
    return [i for i in idx if i != blank]


def ctc_collapse(x, lengths, blank, s_cap=None):
    B, N, _ = x.shape
    s_cap = N if s_cap is None else int(s_cap)
    targets = torch.zeros(B, s_cap, dtype=torch.int32, device=x.device)
    tl = torch.zeros(B, dtype=torch.int32, device=x.device)
    for b in range(B):
        n = N if lengths is None else int(lengths[b])
        ids = greedy_ids(x[b, :n], blank)
        tl[b] = len(ids) if len(ids) <= s_cap else -1
        k = min(len(ids), s_cap)
        targets[b, :k] = torch.tensor(ids[:k], dtype=torch.int32)
    return targets, tl


def attach(monkeypatch, kernel_refs):
    """kernel_refs.py has no entry for the new ops: hang these on it for the duration of a test."""
    for name, fn in (('spec_mask', spec_mask), ('mean_f32', mean_f32), ('ctc_collapse', ctc_collapse)):
        monkeypatch.setattr(kernel_refs, name, fn, raising=False)


# ---- fixture access --------------------------------------------------------------------------------------------------------
CASES = ['w256', 'w256_e2', 'single', 'zero_mask', 'no_mask']
SPEC_AUG = dict(n_time_masks=2, n_freq_masks=3, freq_mask_param=42, time_mask_param=-1, min_p=0.05, zero_masking=False)


class Tok:
    """One character per id: encode(decode(ids)) == ids."""
    def __init__(self, V): self.V = V
    def vocab_size(self): return self.V
    def decode(self, ids): return ''.join(chr(0x100 + int(i)) for i in ids)
    def encode(self, s): return [ord(c) - 0x100 for c in s]


class Args:
    def __init__(self, epochs=1, shuffle=False):
        self.config = {'model': {'subsampling_factor': 8}, 'audio_chunking': {'size': 512, 'overlap': 128}, 'training': {}}
        self.epochs, self.shuffle = epochs, shuffle


def fixture_model(device='cpu'):
    from lcasr_amd.models.sconformer_xl import SCConformerXL
    fx = load_golden('dyneval_model')
    m = SCConformerXL(**golden_cfg(fx))
    m.load_state_dict(golden_state_dict(fx))
    return m.to(device).eval()


def fixture_spec():
    return torch.from_numpy(load_golden('infer_tiny')['spec'].copy())


def case_cfg(fx, name):
    seq_len, overlap, epochs, zero, n_t, n_f, nn = (int(v) for v in fx[f'case.{name}.cfg'])
    return dict(seq_len=seq_len, overlap=overlap, epochs=epochs, num_negatives=nn,
                aug=dict(SPEC_AUG, zero_masking=bool(zero), n_time_masks=n_t, n_freq_masks=n_f))


def make_replay(fx, name, fail_at=None):
    """A SpecAugment whose draw() hands out the intervals the fixture recorded, visit by visit (fail_at: raise in that visit)."""
    from lcasr_amd.utils.augmentation import SpecAugment

    class Replay(SpecAugment):
        visit = 0

        def draw(self, shape, generator=None, device=None):
            v = self.visit
            self.visit += 1
            if fail_at is not None and v == fail_at:
                raise RuntimeError('injected failure')
            t_iv, f_iv = torch.from_numpy(fx[f'case.{name}.t_iv'][v].copy()), torch.from_numpy(fx[f'case.{name}.f_iv'][v].copy())
            assert t_iv.shape[0] == shape[0]
            return t_iv, f_iv

    return Replay(**case_cfg(fx, name)['aug'])


def run_case(fx, name, model, monkeypatch, retokenize, fail_at=None):
    """dynamic_eval on one fixture case with the recorded intervals; returns labels / losses per visit, the final log-probs and
    the parameter-change norm just before the restore.  Asserts the bit-exact restore of parameters and buffers."""
    import lcasr_amd.functional as Fn
    import lcasr_amd.optim as OPT
    from lcasr_amd.eval.dynamic_eval import dynamic_eval
    cfg = case_cfg(fx, name)
    rec = dict(labels=[], losses=[], dnorm=None)
    real_nll = Fn.ctc_nll

    def nll_rec(lp, targets, input_lengths, target_lengths, blank):
        out = real_nll(lp, targets, input_lengths, target_lengths, blank)
        rec['labels'].append(targets[0, :int(target_lengths[0])].tolist())
        rec['losses'].append(float(out.detach().double().sum()) / float(input_lengths.sum()))
        return out

    class RecOpt(OPT.MADGRAD):
        def __init__(self, params, **kw):
            params = list(params)
            super().__init__(params, **kw)
            self._all, self._p0 = params, [p.detach().clone() for p in params]

        def step(self, *a, **kw):
            r = super().step(*a, **kw)
            rec['dnorm'] = float(sum(float((p.detach() - q).double().pow(2).sum()) for p, q in zip(self._all, self._p0)) ** 0.5)
            return r

    monkeypatch.setattr(Fn, 'ctc_nll', nll_rec)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    homes = [p.data_ptr() for p in model.parameters()]
    dev = next(model.parameters()).device
    try:
        logp = dynamic_eval(Args(cfg['epochs']), model, fixture_spec().to(dev), cfg['seq_len'], cfg['overlap'], Tok(127), use_tqdm=False,
                            optim=RecOpt, num_negatives=cfg['num_negatives'], augmentation=make_replay(fx, name, fail_at),
                            retokenize=retokenize)
    finally:
        monkeypatch.setattr(Fn, 'ctc_nll', real_nll)
        for k, v in model.state_dict().items():
            assert torch.equal(v, before[k]), f'{k} not restored'
        assert homes == [p.data_ptr() for p in model.parameters()], 'parameters were not moved back to their storage'
    rec['logp'] = logp
    return rec


def compare(fx, name, rec):
    """Exact pseudo-labels; the rest within 2x the reference's own autocast noise.  Returns the measured figures."""
    p = f'case.{name}.'
    labels, ll = fx[p + 'labels'], fx[p + 'label_len']
    want = [labels[v, :ll[v]].tolist() for v in range(len(ll))]
    assert rec['labels'] == want, f'{name}: pseudo-labels differ from the reference'
    noise = fx[p + 'noise']
    ref, got = fx[p + 'logp'].astype(np.float64), np.asarray(rec['logp'], dtype=np.float64)
    assert got.shape == ref.shape
    d = np.abs(got - ref)
    la, lr = np.array(rec['losses']), fx[p + 'losses']
    fig = dict(logp_max=d.max(), logp_mean=d.mean(), prob_max=np.abs(np.exp(got) - np.exp(ref)).max(),
               loss_rel=(np.abs(la - lr) / np.abs(lr)).max(), dnorm_rel=abs(rec['dnorm'] - float(fx[p + 'dnorm'])) / float(fx[p + 'dnorm']))
    print(f'[dynamic_eval {name}] ' + '  '.join(f'{k} {fig[k]:.3e} (reference autocast noise {n:.3e})' for k, n in zip(fig, noise)))
    for k, n in zip(fig, noise):
        assert fig[k] <= 2 * n, f'{name}: {k} = {fig[k]:.3e} exceeds 2 x the reference autocast noise {n:.3e}'
    epochs = int(fx[p + 'cfg'][2])
    if epochs > 1:
        sums = la.reshape(epochs, -1).sum(1)
        assert sums[-1] < sums[0], f'{name}: no adaptation, epoch losses {sums}'
    return fig
