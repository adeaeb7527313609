"""Per-block gradient parity on the CPU: the autograd wiring of lcasr_amd.functional over the emulated ops (conftest's
`emulated_ops`) against float64, the anchor of the restatements to the reference's captures, and the checker's own sensitivity.

The cases, the checker and the bound are those of tests/test_blocks_gpu.py (block_cases.py, block_parity.py); what this file adds
is what needs no GPU: the anchor and the self-check."""
import pytest
import torch

import block_cases as C
import block_parity as P
import block_refs as R
from conftest import golden_cfg, golden_state_dict, load_golden

pytestmark = pytest.mark.filterwarnings('ignore::UserWarning')


# =============================================================================================================================
# anchor: in f32 the restatements reproduce the reference's captures stored in the tiny_* fixtures
# =============================================================================================================================
ANCHOR_TOL = 1e-4                       # same formula, same precision: only the summation order differs


def _rel(a, ref):
    a, ref = torch.as_tensor(a).double(), torch.as_tensor(ref).double()
    return float((a - ref).norm() / ref.norm())


class _Tiny:
    """A tiny_* fixture as the arguments of the restatements (weights in the reference's state_dict layout)."""

    def __init__(self, name):
        fx = self.fx = load_golden(name)
        self.cfg = cfg = golden_cfg(fx)
        if any(k.startswith('w.') for k in fx.files):
            self.sd, self.audio = golden_state_dict(fx), torch.from_numpy(fx['x'])
        else:                                                   # seed-built fixture (tools/make_subsample4_golden.py)
            from subsample4_cases import tiny_batch, tiny_model
            self.sd = {k: v.detach().clone() for k, v in tiny_model(fx).state_dict().items()}
            self.audio = torch.from_numpy(tiny_batch(fx)['x'])
        self.mode = cfg.get('default_norm', 'layer_norm')
        self.eps = 1e-8 if self.mode == 'rms_norm' else 1e-5
        self.factor = cfg.get('subsampling_factor', 8)
        self.H, self.D = cfg['n_heads'], cfg['head_dim']
        self.length = R.out_lengths(torch.from_numpy(fx['lengths']).long(), 3 if self.factor == 8 else 2)
        assert torch.equal(self.length, torch.from_numpy(fx['out_length']).long())
        self.mlen = None if int(self.length.max()) == int(self.length.min()) else self.length      # sconformer_xl.py:204-205

    def nrm(self, prefix):
        sd = self.sd
        return (sd[prefix + '.weight'], sd[prefix + '.bias']) if self.mode == 'layer_norm' else (sd[prefix + '.scale'], None)

    def sub(self):
        sd, p = self.sd, 'subsampling.'
        names = ['conv.0', 'conv.2', 'conv.3'] + (['conv.5', 'conv.6'] if self.factor == 8 else []) + ['out']
        args = [sd.get(p + n + s) for n in names for s in ('.weight', '.bias')]
        return (R.subsample if self.factor == 8 else R.subsample4)(self.audio, *args)

    def rot(self, N):
        if not self.cfg.get('use_rotary', False):
            return None, None
        return R.rotary_tables(N, self.D, float(self.cfg.get('rotary_base_freq', 10000)))

    def ff(self, x, L, residual):
        sd = self.sd
        return R.ff(x, *self.nrm(L + '.fn.norm'), sd[L + '.fn.fn.fc1.weight'], sd[L + '.fn.fn.fc2.weight'], sd.get(L + '.fn.fn.fc1.bias'),
                    sd.get(L + '.fn.fn.fc2.bias'), 0.5, self.mode, self.eps, residual)

    def attn(self, x, L, B, N, residual):
        sd = self.sd
        return R.attn(x, *self.nrm(L + '.norm'), sd[L + '.fn.qkv_proj.weight'], sd[L + '.fn.out_proj.weight'], sd.get(L + '.fn.qkv_proj.bias'),
                      sd.get(L + '.fn.out_proj.bias'), *self.rot(N), self.mlen, B, N, self.H, self.D, (-1, -1), self.mode, self.eps, residual)

    def conv(self, x, L, B, N, residual, buffers=None):
        sd, p = (self.sd if buffers is None else {**self.sd, **buffers}), L + '.fn.'
        return R.conv(x, *self.nrm(L + '.norm'), sd[p + 'pointwise_conv1.weight'], sd[p + 'pointwise_conv1.bias'], sd[p + 'depthwise_conv.weight'],
                      sd[p + 'depthwise_conv.bias'], sd[p + 'batch_norm.weight'], sd[p + 'batch_norm.bias'], sd[p + 'batch_norm.running_mean'],
                      sd[p + 'batch_norm.running_std'], int(sd[p + 'batch_norm.num_batches_tracked']), sd[p + 'pointwise_conv2.weight'],
                      sd[p + 'pointwise_conv2.bias'], self.mlen, B, N, True, self.mode, self.eps, residual)

    def dec(self):
        sd = self.sd
        nw, nb = self.nrm('decoder.norm') if self.cfg.get('decoder_norm', False) else (None, None)
        return nw, nb, sd['decoder.ff.weight'], sd['decoder.ff.bias']


# fixture -> whether it holds the reference's per-block captures (cap.*).  tiny_ss4_ragged is seed-built and holds none: its
# subsample4 restatement is anchored through the chained log-probs, buffers and loss only.
ANCHOR_CASES = {'tiny_ln_ragged': True, 'tiny_rms_ragged': True, 'tiny_ln_odd': True, 'tiny_ss4_ragged': False}
CAPTURES = ('sub.out', 'layers.0.ff1.branch', 'layers.0.attend.branch', 'layers.0.conv.branch', 'layers.0.out')


@pytest.mark.parametrize('name', ANCHOR_CASES)
def test_restatements_reproduce_the_reference_captures(name):
    """Each block restatement, fed the captured residual stream, gives the reference's capture (the fixtures ANCHOR_CASES marks:
    a fixture that loses its captures fails here), and the restatements chained into the whole model give the reference's
    log-probabilities, BatchRenorm buffers and CTC loss (every fixture): relative L2 <= 1e-4 in f32.

    Not anchored: all four fixtures have bias_in_ff False and the window (-1, -1), so the ff biases b1 / b2 and the two-sided window
    convention of R.attn are tied to the reference by no capture; they are checked only by the agreement of the fused blocks with the
    restatement."""
    tn = _Tiny(name)
    fx, cfg, sd = tn.fx, tn.cfg, tn.sd
    errs = {}
    with torch.no_grad():
        x3 = tn.sub()
        B, N, d = x3.shape
        caps = {k[4:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith('cap.')}
        assert all(k in caps for k in CAPTURES) if ANCHOR_CASES[name] else not caps, (name, sorted(caps))
        if caps:
            errs['sub.out'] = _rel(x3, caps['sub.out'])
            s = caps['sub.out'].reshape(B * N, d)
            L = 'layers.0'
            errs['ff1.branch'] = _rel(tn.ff(s, L + '.ff1', False), caps[L + '.ff1.branch'].reshape(B * N, d))
            s = s + caps[L + '.ff1.branch'].reshape(B * N, d)
            errs['attend.branch'] = _rel(tn.attn(s, L + '.attend', B, N, False), caps[L + '.attend.branch'].reshape(B * N, d))
            s = s + caps[L + '.attend.branch'].reshape(B * N, d)
            errs['conv.branch'] = _rel(tn.conv(s, L + '.conv', B, N, False)[0], caps[L + '.conv.branch'].reshape(B * N, d))
            s = s + caps[L + '.conv.branch'].reshape(B * N, d)
            s = tn.ff(s, L + '.ff2', True)
            out = caps[L + '.out'].reshape(B * N, d)
            errs['out'] = _rel(R.norm(s, *tn.nrm(L + '.norm_out'), tn.mode, tn.eps), out)
            if tn.mode == 'layer_norm' and cfg.get('decoder_norm', False):
                y1, h2 = R.norm2(s, *tn.nrm(L + '.norm_out'), *tn.nrm('decoder.norm'))
                errs['out(norm2)'] = _rel(y1, out)
                errs['norm2.h2'] = _rel(h2, R.norm(out, *tn.nrm('decoder.norm'), tn.mode, tn.eps))
        # the whole model from the restatements
        x = x3.reshape(B * N, d)
        nw, nb, wff, bff = tn.dec()
        has_norm = nw is not None
        n_layers = cfg['n_layers']
        for i in range(n_layers):
            L = f'layers.{i}'
            x = tn.ff(x, L + '.ff1', True)
            x = tn.attn(x, L + '.attend', B, N, True)
            x, (rm, rs, nbt) = tn.conv(x, L + '.conv', B, N, True)
            for key, v in (('running_mean', rm), ('running_std', rs)):
                errs[f'{L}.{key}'] = _rel(v, fx[f'buf.{L}.conv.fn.batch_norm.{key}'])
            assert nbt == int(fx[f'buf.{L}.conv.fn.batch_norm.num_batches_tracked'])
            x = tn.ff(x, L + '.ff2', True)
            x = R.norm(x, *tn.nrm(L + '.norm_out'), tn.mode, tn.eps)
            if caps:
                errs[f'{L}.out(chained)'] = _rel(x, caps[L + '.out'].reshape(B * N, d))
            if i != n_layers - 1 and cfg.get('self_conditioning', True):
                x = R.selfcond(x, nw, nb, wff, bff, sd['decoder.reprojection.weight'], sd['decoder.reprojection.bias'], has_norm, tn.mode, tn.eps)
        n_norms = (2 if cfg.get('legasee_double_norm', True) else 1) if has_norm else 0
        errs['logp'] = _rel(R.head(x, nw, nb, wff, bff, n_norms, tn.mode, tn.eps), torch.from_numpy(fx['logp']).reshape(B * N, -1))
        errs['logits'] = _rel(R.head(x, nw, nb, wff, bff, n_norms, tn.mode, tn.eps, True).log_softmax(-1), torch.from_numpy(fx['logp']).reshape(B * N, -1))
        nll = R.head_ctc(x, nw, nb, wff, bff, B, torch.from_numpy(fx['targets']), tn.length, torch.from_numpy(fx['target_lengths']),
                         wff.shape[0] - 1, n_norms, tn.mode, tn.eps)
        errs['ctc loss'] = abs(float(nll.sum()) - float(fx['loss'])) / float(fx['loss'])
    print(f'[anchor {name}] ' + ', '.join(f'{k} {v:.1e}' for k, v in errs.items()))
    assert max(errs.values()) <= ANCHOR_TOL, {k: v for k, v in errs.items() if v > ANCHOR_TOL}


def test_restatements_reproduce_the_reference_gradients():
    """The f32 gradients of the restatements chained into the whole model against the reference's (tiny_ln_ragged holds them in
    full): per-tensor relative L2 <= 1e-4, the anchor's bound.  The depthwise-conv biases in front of the training BatchRenorms are
    analytically zero - cancellation noise on both sides: they stay below common_model's floor (error <= 1 against it)."""
    from common_model import rel_l2_errors
    tn = _Tiny('tiny_ln_ragged')
    fx, cfg = tn.fx, tn.cfg
    tn.sd = sd = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and 'running' not in k and 'rotary' not in k else v) for k, v in tn.sd.items()}
    x3 = tn.sub()
    B, N, d = x3.shape
    x = x3.reshape(B * N, d)
    nw, nb, wff, bff = tn.dec()
    for i in range(cfg['n_layers']):
        L = f'layers.{i}'
        x = tn.ff(tn.conv(tn.attn(tn.ff(x, L + '.ff1', True), L + '.attend', B, N, True), L + '.conv', B, N, True)[0], L + '.ff2', True)
        x = R.norm(x, *tn.nrm(L + '.norm_out'))
        if i != cfg['n_layers'] - 1:
            x = R.selfcond(x, nw, nb, wff, bff, sd['decoder.reprojection.weight'], sd['decoder.reprojection.bias'])
    nll = R.head_ctc(x, nw, nb, wff, bff, B, torch.from_numpy(fx['targets']), tn.length, torch.from_numpy(fx['target_lengths']), wff.shape[0] - 1, 2)
    T = tn.audio.shape[-1]
    (nll.sum() / (T * B) * 100).backward()
    ref = {k[2:]: fx[k] for k in fx.files if k.startswith('g.')}
    errs = rel_l2_errors({k: sd[k].grad for k in ref}, ref)
    print('[anchor gradients] worst ' + ', '.join(f'{k} {v:.1e}' for k, v in sorted(errs.items(), key=lambda kv: -kv[1])[:4]))
    bad = {k: v for k, v in errs.items() if v > (1.0 if k.endswith('depthwise_conv.bias') else ANCHOR_TOL)}
    assert not bad, bad


# =============================================================================================================================
# the cases over the emulated ops
# =============================================================================================================================
@pytest.mark.parametrize('case', C.ALL, ids=repr)
def test_block_returned_gradients(case, emulated_ops):
    import lcasr_amd.functional as Fn
    P.check_block(case, Fn)


@pytest.mark.parametrize('case', C.SMALL + C.CHAINS[:2] + C.BIG[3:4], ids=repr)
def test_block_direct_gradients(case, emulated_ops):
    import lcasr_amd.functional as Fn
    P.check_block_direct(case, Fn)
    assert not Fn._direct['on'] and Fn._direct['hook'] is None


def test_direct_gradients_reach_the_leaf_behind_a_non_leaf_weight(emulated_ops):
    """wff is torch.cat(leaf, zero rows) (the class-padded decoder weights): no direct write, no hook, and the leaf still gets its
    gradient - added to the pre-fill by autograd."""
    import lcasr_amd.functional as Fn
    case = C.BY_NAME['selfcond-layer_norm-norm1-pre0-M231-d64-V129']
    assert case.nondirect == {'wff', 'bff', 'wre'}
    res, fired = P.run_fused(case, Fn, direct=True)
    assert sorted(fired) == ['bre', 'nb', 'nw']
    assert all(res.grads[k] is not None and float(res.grads[k].norm()) > 0 for k in case.nondirect)
    P.check_result(case, res, 'direct, non-leaf wff')


@pytest.mark.parametrize('case', C.NONCONTIG, ids=repr)
def test_block_noncontiguous_dy(case, emulated_ops):
    import lcasr_amd.functional as Fn
    P.check_noncontiguous_dy(case, Fn)


def test_ff_checkpoint_recompute_is_bit_equal(emulated_ops):
    import lcasr_amd.functional as Fn
    a, b = P.run_fused(C.FF_CKPT[0], Fn), P.run_fused(C.FF_CKPT[1], Fn)
    P.same_results(a, b, 'ff ckpt 0 / 1', exact=True)
    P.check_result(C.FF_CKPT[1], b, 'ckpt=1')


@pytest.mark.parametrize('case', C.CHAINS[:2], ids=repr)
def test_chain_twin_on_off(case, emulated_ops, monkeypatch):
    import lcasr_amd.functional as Fn
    P.check_twin_on_off(case, Fn, 'cpu', monkeypatch, C.CHAIN_COLSUM_BIASES)


def test_stale_twin_is_not_taken(emulated_ops, monkeypatch):
    import lcasr_amd.functional as Fn
    P.check_stale_twin(C.SMALL_BY_BLOCK['ff'][0], Fn, 'cpu', monkeypatch)


def test_sc_delta_route_of_the_cases(emulated_ops, monkeypatch):
    """Which self-conditioning cases take the sc_delta backward (the emulation states the kernels' shape rule); with SCONF_SC_DELTA=0
    the same cases take the two-pass backward and still meet the bound."""
    import lcasr_amd.functional as Fn
    assert all('M3072-d64-V4096' in c.name for c in C.DELTA) and Fn.sc_delta_enabled(3072, 4096, 64)
    assert not Fn.sc_delta_enabled(512, 1024, 256) and not Fn.sc_delta_enabled(231, 144, 64)
    monkeypatch.setenv('SCONF_SC_DELTA', '0')
    assert not Fn.sc_delta_enabled(3072, 4096, 64)
    for case in C.SC_DELTA_OFF:
        P.check_result(case, P.run_fused(case, Fn), 'SCONF_SC_DELTA=0')


# =============================================================================================================================
# self-check: the checker fails on a 5 % error in any one gradient tensor, and on each glue mutation
# =============================================================================================================================
@pytest.mark.parametrize('case', C.SMALL + C.CHAINS[:2], ids=repr)
def test_checker_fails_on_five_percent_in_any_tensor(case, emulated_ops):
    """Every d_model 64 case, the two S64 chains with their cap of 5e-2 included."""
    import lcasr_amd.functional as Fn
    truth, ac = P.plain_results(case)
    res = P.run_fused(case, Fn)
    assert not P.assess(case, truth, ac, res)[1]
    rms = P.grad_rms(truth)
    checked = 0
    for k in case.diff:
        if res.grads[k] is None:
            continue
        bad = P.Result(res.outs, dict(res.grads), res.extras)
        if P.is_zero_grad(truth, k):
            bad.grads[k] = res.grads[k] + 0.05 * rms              # analytically zero: 5 % of the block's gradient rms instead
        else:
            bad.grads[k] = res.grads[k] * 1.05
        fails = P.assess(case, truth, ac, bad)[1]
        assert fails and all(f.startswith(k + ':') for f in fails), (case.name, k, fails)
        checked += 1
    assert checked


def _must_fail(case, Fn, needles):
    truth, ac = P.plain_results(case)
    fails = P.assess(case, truth, ac, P.run_fused(case, Fn))[1]
    for n in needles:
        assert any(f.startswith(n + ':') for f in fails), (case.name, n, fails)


def test_checker_fails_when_bgrad_ignores_alpha(emulated_ops, monkeypatch):
    import lcasr_amd.functional as Fn
    orig = Fn._bgrad
    monkeypatch.setattr(Fn, '_bgrad', lambda dy16, bias, alpha=1.0, colsum=None: orig(dy16, bias, 1.0, colsum))
    _must_fail(C.SMALL_BY_BLOCK['ff'][0], Fn, ['b2'])
    _must_fail(C.CHAINS[0], Fn, ['f1.b2', 'f2.b2'])


def test_checker_fails_when_colsum_is_five_percent_off(emulated_ops, monkeypatch):
    import lcasr_amd.functional as Fn
    orig = emulated_ops.colsum_
    monkeypatch.setattr(emulated_ops, 'colsum_', lambda x, out, alpha=1.0: orig(x, out, 1.05 * alpha))
    _must_fail(C.SMALL_BY_BLOCK['ff'][0], Fn, ['b1', 'b2'])
    _must_fail(C.SMALL_BY_BLOCK['attn'][0], Fn, ['bqkv', 'bout'])


def test_checker_fails_when_the_residual_gradient_is_dropped(emulated_ops, monkeypatch):
    import lcasr_amd.functional as Fn
    orig = Fn._norm_bwd_res
    monkeypatch.setattr(Fn, '_norm_bwd_res', lambda dh, x, nw, mean, rstd, mode, eps, dres, dnw, dnb, twin=True:
                        orig(dh, x, nw, mean, rstd, mode, eps, None, dnw, dnb, twin))
    for block in ('ff', 'attn', 'conv', 'selfcond'):
        _must_fail(C.SMALL_BY_BLOCK[block][0], Fn, ['x'])


def test_checker_fails_when_a_block_takes_another_tensors_twin(emulated_ops, monkeypatch):
    import lcasr_amd.functional as Fn
    orig, last = Fn._take_twin, []

    def wrong(dy):
        r = orig(dy)
        if r[1] is not None:
            last.append(r)
            if len(last) > 1 and last[-2][0].shape == r[0].shape:
                return last[-2]                                   # the twin parked for the block behind
        return r

    monkeypatch.setattr(Fn, '_take_twin', wrong)
    _must_fail(C.CHAINS[0], Fn, ['x'])
    assert len(last) >= 3
