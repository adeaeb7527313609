"""GPU tests of the evaluation loop through the C ABI (lcasr_amd.hip.ops -> libsconf_hip.so): sconf_edit_counts and
sconf_copy_row_spans against tests/eval_refs.py, the buffered fetch_logits on the HIP path against the reference's own output
(tests/golden/buffered_tiny.npz) and against the product's own one-window forward, and the scoring end to end.

Bounds (set by the issue): edit counts are exact integers; copy_row_spans_ and the rows of the buffered output are bit-equal to
their source; the buffered output stays within max 0.3 / mean 0.03 of the reference's fp32 run (the bounds infer_tiny already
uses) and within 2e-3 of itself at another batch size."""
import numpy as np
import pytest
import torch

import eval_refs as E
from common_model import build_from_fixture
from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import lcasr_amd.hip.ops as o
    o._lib.load()
    return o


def geometry(ops):
    lib = ops._lib.load()
    return lib.sconf_edit_strip_cols(), lib.sconf_edit_pass_cols(), lib.sconf_edit_block_rows()


def branch(ops, m, n):
    """(passes over the reference, waves with columns in the last pass, row blocks) the kernel takes for an m x n pair."""
    S, Pc, R = geometry(ops)
    if m == 0 or n == 0:
        return (0, 0, 0)
    last = n - (n - 1) // Pc * Pc
    return (-(-n // Pc), -(-last // S), -(-m // R))


@pytest.fixture(scope='module')
def batch(ops):
    """One ragged batch over every size at which the launch geometry changes, with the branch each pair must reach, the
    reference counts (computed once) and the kernel's counts from one launch."""
    S, Pc, R = geometry(ops)
    W = Pc // S
    rng = np.random.default_rng(7)
    pairs, want_branch = [], []

    def add(h, r, br):
        pairs.append((h, r)); want_branch.append(br)

    for i, (m, n) in enumerate((m, n) for m in (0, 1, 63, 64, 65) for n in (0, 1, 63, 64, 65)):
        add(*E.random_pair(rng, m, n, 2 + i % 2), (1, 1, 1) if m and n else (0, 0, 0))
    for n, br in ((S - 1, (1, 1, 1)), (S, (1, 1, 1)), (S + 1, (1, 2, 1)), (Pc - 1, (1, W, 1)), (Pc, (1, W, 1)), (Pc + 1, (2, 1, 1)),
                  (2 * Pc + 3, (3, 1, 1))):
        add(*E.random_pair(rng, 70, n, 2), br)
        add(*E.random_pair(rng, 71, n, 3), br)
    for m, blocks in ((R - 1, 1), (R, 1), (R + 1, 2), (2 * R + 5, 3)):
        add(*E.random_pair(rng, m, 70, 3), (1, 1, blocks))
        add(*E.random_pair(rng, m, 69, 2), (1, 1, blocks))
    add(*E.random_pair(rng, 2 * R + 5, Pc + S + 1, 2), (2, 2, 3))
    add(*E.random_pair(rng, R + 44, S - 232, 5000), (1, 1, 2))                         # nearly all substitutions
    add(*E.planted_pair(rng, Pc + 40, 5000, 60), (2, 1, None))                         # long matching runs, few edits
    add(*E.planted_pair(rng, S - 12, 3, 40), (1, 1, None))
    add(np.zeros(0, np.int32), np.zeros(0, np.int32), (0, 0, 0))
    for (h, r), br in zip(pairs, want_branch):                                         # each case reaches the branch it is there for
        got = branch(ops, len(h), len(r))
        assert all(b is None or a == b for a, b in zip(got, br)), (len(h), len(r), got, br)
    hyp, ho = E.ragged([p[0] for p in pairs]); ref, ro = E.ragged([p[1] for p in pairs])
    want = E.edit_counts(hyp, ho, ref, ro)
    dev = [t.cuda() for t in (hyp, ho, ref, ro)]
    got = ops.edit_counts(*dev)
    return dict(pairs=pairs, want=want, dev=dev, got=got)


def test_edit_counts_ragged_batch_is_exact(ops, batch):
    got, want = batch['got'].cpu(), batch['want']
    assert got.dtype == torch.int64 and got.shape == want.shape
    bad = [(len(h), len(r), g, w) for (h, r), g, w in zip(batch['pairs'], got.tolist(), want.tolist()) if g != w]
    assert not bad, bad[:8]
    # ties at almost every cell with 2 and 3 symbols: the split is the one with the fewest substitutions, not merely a valid one
    assert (got[:, 0] == got[:, 1:].sum(1)).all()
    again = ops.edit_counts(*batch['dev'])
    assert torch.equal(again, batch['got'])                                            # two launches: bit-equal


def test_edit_counts_pair_by_pair_equals_the_batch(ops, batch):
    got = batch['got'].cpu()
    for p, (h, r) in enumerate(batch['pairs']):
        one = ops.edit_counts(*(t.cuda() for t in E.ragged([h]) + E.ragged([r])))
        assert one.shape == (1, 4) and one[0].tolist() == got[p].tolist(), (p, len(h), len(r))
    assert ops.edit_counts(*(t.cuda() for t in E.ragged([]) + E.ragged([]))).shape == (0, 4)      # P == 0: nothing launched


def test_edit_counts_one_large_pair_and_a_short_workspace(ops):
    rng = np.random.default_rng(11)
    h, r = E.planted_pair(rng, 2900, 40, 0)
    h = np.concatenate([h, rng.integers(0, 40, 100).astype(np.int32)])                 # 3000 x 2900
    rng.shuffle(h[1000:1400])
    assert (len(h), len(r)) == (3000, 2900) and branch(ops, 3000, 2900)[0] == 2
    hyp, ho = E.ragged([h]); ref, ro = E.ragged([r])
    want = E.edit_counts(hyp, ho, ref, ro)
    dev = [t.cuda() for t in (hyp, ho, ref, ro)]
    assert ops.edit_counts(*dev).cpu().tolist() == want.tolist()
    # straight through the C ABI with a workspace one key short of the pair's need: reported as -1, nothing overrun
    import ctypes as C
    vp = lambda t: C.c_void_p(t.data_ptr())
    need = 8 * (len(h) + 1)
    assert ops._lib.load().sconf_edit_counts_workspace(1, len(h), len(r)) == need
    ws = torch.zeros(need + 64, dtype=torch.uint8, device='cuda')
    out = torch.zeros(1, 4, dtype=torch.int64, device='cuda')
    ops._lib.call('sconf_edit_counts', vp(dev[0]), vp(dev[1]), vp(dev[2]), vp(dev[3]), 1, vp(out), vp(ws), need - 8, ops._stream())
    assert out.cpu().tolist() == [[-1, -1, -1, -1]] and int(ws[need - 8:].sum()) == 0
    ops._lib.call('sconf_edit_counts', vp(dev[0]), vp(dev[1]), vp(dev[2]), vp(dev[3]), 1, vp(out), vp(ws), need, ops._stream())
    assert out.cpu().tolist() == want.tolist() and int(ws[need:].sum()) == 0


@pytest.mark.parametrize('W,n,C,N', [(1, 9, 8, 20), (5, 33, 128, 200), (3, 700, 4, 2000)])
def test_copy_row_spans_is_bit_equal_to_slicing(ops, W, n, C, N):
    g = torch.Generator().manual_seed(W * 100 + n)
    src = torch.randn(W, n, C, generator=g)
    spans = [[0, n, 0]] if W == 1 else [[int(torch.randint(0, n // 2, (1,), generator=g)), 0, 0] for _ in range(W)]
    pos = 3
    for w in range(W if W > 1 else 0):
        rows = 0 if w == 1 else int(torch.randint(1, n - spans[w][0] + 1, (1,), generator=g))      # one span of 0 rows
        spans[w][1:] = [rows, pos]
        pos += rows
    if W > 2:
        spans[2] = [n - 1, 2, 0]                                # runs past its window: refused, copies nothing
    assert pos <= N
    want = torch.full((N, C), -7.0)
    E.copy_row_spans_(src, torch.tensor(spans, dtype=torch.int32), want)
    got = torch.full((N, C), -7.0).cuda()
    ops.copy_row_spans_(src.cuda(), torch.tensor(spans, dtype=torch.int32).cuda(), got)
    assert torch.equal(got.cpu(), want)
    for w, (s0, rows, d0) in enumerate(spans):
        if not (W > 2 and w == 2):
            assert torch.equal(got[d0:d0 + rows].cpu(), src[w, s0:s0 + rows])
    past = torch.tensor([[0, n, N - n + 1]] + [[0, 0, 0]] * (W - 1), dtype=torch.int32).cuda()     # runs past dst: refused
    ops.copy_row_spans_(src.cuda(), past, got)
    assert torch.equal(got.cpu(), want)


def test_buffered_fetch_logits_on_device(ops):
    from lcasr_amd.eval.buffered_transcription import buffer_plan, buffer_spans, fetch_logits
    fx, bx = load_golden('infer_tiny'), load_golden('buffered_tiny')
    m = build_from_fixture(fx, 'cuda').eval()

    class Tok:
        def vocab_size(self): return int(fx['cfg.vocab_size'])

    spec = torch.from_numpy(fx['spec'].copy())
    for ci, (sl, ov) in enumerate(bx['tiny.cases'].tolist()):
        one = fetch_logits(E.Args, m, spec, sl, ov, Tok(), use_tqdm=False, max_batch=1, return_numpy=False)
        bat = fetch_logits(E.Args, m, spec, sl, ov, Tok(), use_tqdm=False, max_batch=3)
        ref = bx[f'tiny.logits.{ci}']
        assert tuple(one.shape) == ref.shape == bat.shape, (sl, ov)
        d = np.abs(one.cpu().numpy() - ref)
        print(f'[buffered tiny gpu seq_len={sl} overlap={ov}] max {float(d.max()):.3f} mean {float(d.mean()):.4f} '
              f'batched vs one {float(np.abs(one.cpu().numpy() - bat).max()):.2e}')
        assert float(d.max()) < 0.3 and float(d.mean()) < 0.03, (sl, ov, float(d.max()), float(d.mean()))
        assert float(np.abs(one.cpu().numpy() - bat).max()) < 2e-3                     # same kernels, other batch size
        # every output row is the same row of the model's own forward of that one window, bit for bit
        sl_r, ov_r = (512, 128) if sl == -1 else (min(sl, 1000), ov if sl <= 1000 else 0)
        plan = buffer_plan(1000, sl_r, ov_r)
        sizes, outs = [], []
        with torch.no_grad():
            for b0, b1, _, _ in plan:
                outs.append(m(spec[:, :, b0:b1].contiguous().cuda())['final_posteriors'].float()[0])
                sizes.append(outs[-1].shape[0])
        spans, total = buffer_spans(plan, sizes, 1000 // 4 + sl_r)
        assert total == one.shape[0]
        for lp, (s0, rows, d0) in zip(outs, spans):
            assert torch.equal(one[d0:d0 + rows], lp[s0:s0 + rows]), (sl, ov, s0, rows, d0)


def test_scoring_end_to_end_on_device(ops):
    from lcasr_amd.eval.wer import token_error_counts, word_error_rate_detail
    rng = np.random.default_rng(5)
    vocab = [f'w{i}' for i in range(30)]
    S, Pc, R = geometry(ops)
    hyps, refs, tot, words = [], [], np.zeros(4, dtype=np.int64), 0
    for n in (0, 5, 400, Pc + 100):
        h, r = E.planted_pair(rng, n, len(vocab), n // 10)
        hyps.append(' '.join(vocab[i] for i in h)); refs.append(' '.join(vocab[i] for i in r))
        tot += np.array(E._split(E.edit_key_rows(h, r), len(h), len(r))); words += len(r)
    got = word_error_rate_detail(hyps, refs)
    assert got == (tot[0] / words, words, tot[3] / words, tot[2] / words, tot[1] / words)
    assert word_error_rate_detail(['abc d'], ['abd  d'], use_cer=True) == (2 / 6, 6, 0.0, 1 / 6, 1 / 6)

    import dyneval_refs
    g = torch.Generator().manual_seed(9)
    B, N, V = 4, 300, 128
    lp = (3 * torch.randn(B, N, V, generator=g)).log_softmax(-1)
    lengths = torch.tensor([300, 211, 1, 0], dtype=torch.int32)
    targets = torch.randint(0, V - 1, (B, 90), generator=g)
    tl = torch.tensor([90, 64, 0, 5])
    out = token_error_counts(lp.cuda(), lengths.cuda(), targets.cuda(), tl.cuda(), blank=V - 1)
    assert out.is_cuda and out.shape == (B, 4) and out.dtype == torch.int64
    for b in range(B):
        ids = dyneval_refs.greedy_ids(lp[b, :int(lengths[b])], V - 1)
        tg = targets[b, :int(tl[b])].tolist()
        assert out[b].tolist() == E._split(E.edit_key_rows(ids, tg), len(ids), len(tg)), b
    none = token_error_counts(lp.cuda(), None, targets.cuda(), tl.cuda(), blank=V - 1)
    assert none[0].tolist() == out[0].tolist()
