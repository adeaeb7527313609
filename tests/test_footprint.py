"""CPU self-check of the write-footprint harness (tests/footprint.py) and of its case table (tests/footprint_cases.py).

The harness must fail on what it is for - without a GPU and without ever provoking a device fault: it runs here on CPU tensors
against small Python "kernels", one per defect, and each must be flagged with the right region in the message while the correct
kernel passes.  Every case of the table is then laid out on a CPU arena (the size and routing queries are host-only; the library
builds here as test_cabi.py builds it), and the set of entry points with a case must be the set the binding declares."""
import pytest
import torch

import footprint as FP
import footprint_cases as FC
from footprint import ACC, IN, OUT, SCRATCH

M, K, N, LD = 40, 8, 12, 16


def toy_case():
    """out (M,N) at row stride LD = a (M,K) @ w (K,N); scratch[:N] = column sums of out; acc += scratch[:N]."""
    g = torch.Generator().manual_seed(0)
    a = FP.Arena()
    ra = a.take('a', (M, K), torch.float32, IN, init=torch.randn(M, K, generator=g))
    rw = a.take('w', (K, N), torch.float32, IN, init=torch.randn(K, N, generator=g))
    out = a.take('out', (M, N), torch.float32, OUT, ld=LD)
    acc = a.take('acc', N, torch.float32, ACC, init=torch.randn(N, generator=g) + 3.0, order='fixed')
    scr = a.take('scratch', 64, torch.float32, SCRATCH)

    def restate(v):
        o = v['a'].double() @ v['w'].double()
        return {'out': o, 'acc': v['acc'].double() + o.sum(0)}
    return FP.Case('toy', 'toy_kernel', a, [ra, rw, out, acc, scr], 'toy', restate)


def correct(v, buf, regs):
    v['out'].copy_(v['a'] @ v['w'])
    v['scratch'][:N] = v['out'].sum(0)
    v['acc'] += v['scratch'][:N]


def _raw_f32(buf, lo, hi):
    return buf[lo:hi].view(torch.float32)


def one_past(v, buf, regs):
    correct(v, buf, regs)
    r = regs['out']
    _raw_f32(buf, r.offset + r.extent, r.offset + r.extent + 4)[0] = 1.0


def one_before(v, buf, regs):
    correct(v, buf, regs)
    r = regs['out']
    _raw_f32(buf, r.offset - 4, r.offset)[0] = 1.0


def into_ld_gap(v, buf, regs):
    correct(v, buf, regs)
    r = regs['out']
    _raw_f32(buf, r.offset, r.offset + r.extent).as_strided((M - 1, LD), (LD, 1))[3, N] = 1.0


def block_unwritten(v, buf, regs):
    o = v['a'] @ v['w']
    v['out'][:16] = o[:16]; v['out'][32:] = o[32:]                          # rows 16..31: one 16-row block never stored
    v['scratch'][:N] = o.sum(0)
    v['acc'] += v['scratch'][:N]


def adds_into_out(v, buf, regs):
    v['out'] += v['a'] @ v['w']
    v['scratch'][:N] = (v['a'] @ v['w']).sum(0)
    v['acc'] += v['scratch'][:N]


def modifies_input(v, buf, regs):
    correct(v, buf, regs)
    v['a'][0, 0] += 1.0


def reads_scratch(v, buf, regs):
    stale = v['scratch'][N:2 * N].clone()                                   # never written by the kernel
    v['out'].copy_(v['a'] @ v['w'])
    v['scratch'][:N] = v['out'].sum(0)
    v['acc'] += v['scratch'][:N] + torch.nan_to_num(stale, nan=0.0, posinf=0.0, neginf=0.0).clamp(-1, 1) * 1e-3


def overwrites_acc(v, buf, regs):
    v['out'].copy_(v['a'] @ v['w'])
    v['scratch'][:N] = v['out'].sum(0)
    v['acc'].copy_(v['scratch'][:N])


def _run(kernel):
    c = toy_case()
    return FP.run_case(c, 'cpu', launch=lambda name, args, buf, views: kernel(views, buf, c.arena.regions))


def test_a_correct_kernel_passes_and_reports_its_figures():
    fig = _run(correct)
    assert fig['arena_bytes'] > 0 and fig['guard_bytes'] >= 6 * FP.GUARD + M * (LD - N) * 4 - (LD - N) * 4
    assert [s.split('=')[0] for s in fig['valued']] == ['out', 'acc']


@pytest.mark.parametrize('kernel,needle', [
    (one_past, r"confinement.*1 byte\(s\) PAST the end of the OUT region 'out'"),
    (one_before, r"confinement.*byte\(s\) BEFORE the OUT region 'out'"),
    (into_ld_gap, r"confinement.*in a stride gap of the OUT region 'out'.*element offset " + str(3 * LD + N)),
    (block_unwritten, r"OUT region 'out' completeness: 192 element\(s\) are NaN.*first at \[16, 0\]"),
    (adds_into_out, r"OUT region 'out' completeness"),
    (modifies_input, r"confinement.*inside the IN region 'a', byte [0-3] "),
    (reads_scratch, r"ACC region 'acc' completeness: \d+ element\(s\) differ"),
    (overwrites_acc, r"ACC region 'acc' values: max err"),
], ids=lambda p: p.__name__ if callable(p) else None)
def test_every_seeded_defect_is_caught_with_the_region_named(kernel, needle):
    with pytest.raises(FP.FootprintError, match=needle):
        _run(kernel)


def test_an_unspecified_sub_extent_is_excluded_from_completeness_but_not_from_confinement():
    c = toy_case()
    c.arena.regions['out'].unspecified = torch.zeros(M, N, dtype=torch.bool)
    c.arena.regions['out'].unspecified[16:32] = True
    FP.run_case(c, 'cpu', launch=lambda n, a, buf, v: block_unwritten(v, buf, c.arena.regions))
    with pytest.raises(FP.FootprintError, match='stride gap'):
        FP.run_case(c, 'cpu', launch=lambda n, a, buf, v: into_ld_gap(v, buf, c.arena.regions))


def test_carving_is_16_byte_granular_with_guards_everywhere():
    a = toy_case().arena
    a.validate()
    offs = [r.offset for r in a.regions.values()]
    assert all(o % 16 == 0 for o in offs) and any(o % 32 for o in offs), offs          # nothing is rounded up to 256 or 512
    assert FP.GUARD >= 256


# ------------------------------------------------------------------------------------------------ the case table
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from lcasr_amd.hip import _lib
    return _lib.load()


def test_every_entry_point_has_a_case():
    """A new entry point cannot be bound without stating its footprint."""
    from lcasr_amd.hip import _lib
    assert FC.NO_LAUNCH == {'sconf_gemm_num_splits'}
    assert {entry for _, entry, _ in FC.CASES.values()} | FC.NO_LAUNCH == set(_lib.PROTOTYPES)
    assert not {entry for _, entry, _ in FC.CASES.values()} & FC.NO_LAUNCH


@pytest.mark.parametrize('id', list(FC.CASES))
def test_case_layout(lib, id, monkeypatch):
    """Regions disjoint, 16-byte aligned and guarded; argument list as long as the prototype; declared output shapes = the shapes
    the kernel_refs restatement returns."""
    from lcasr_amd.hip import _lib
    for k in ('SCONF_SUB_MFMA', 'SCONF_GEMM_NO_256', 'SCONF_ATTN_WIDE', 'SCONF_QKV_ROT_EPILOGUE_OFF'): monkeypatch.delenv(k, raising=False)
    if id in FC.MFMA_OFF: monkeypatch.setenv('SCONF_SUB_MFMA', '0')
    rec = _Recorder(lib)
    c = FC.build(id, rec)
    assert c.name == FC.CASES[id][1]
    FP.check_layout(c, _lib.PROTOTYPES)
    ws = c.arena.regions.get('workspace')
    if ws is not None:                               # exactly what the entry point's own query returned (in the query's unit), unpadded
        sizes = [n for q, n in rec.queries if q == c.name + '_workspace']
        assert ws.cls == SCRATCH and sizes and ws.numel == sizes[-1] and ws.extent == ws.numel * ws.itemsize, (ws, rec.queries)
    if c.name == 'sconf_attn_bwd':                   # sconf.h: delta is 2*B*H*N floats
        B, N, H = c.args[11:14]
        d = c.arena.regions['delta']
        assert d.cls == SCRATCH and d.dtype == torch.float32 and d.numel == 2 * B * H * N and d.extent == 4 * d.numel


class _Recorder:
    """The library with its *_workspace queries recorded, so that a case's workspace can be held to what the query returned."""

    def __init__(self, lib):
        self._lib, self.queries = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.endswith('_workspace'): return fn

        def query(*a):
            n = fn(*a)
            self.queries.append((name, int(n)))
            return n
        return query


def test_gemm_and_attention_strides_are_pairwise_different(lib):
    """What the cases promise about their strides, asserted on the argument lists themselves."""
    for id, (family, entry, _) in FC.CASES.items():
        if entry == 'sconf_gemm_bf16' and '-accum-' not in id:
            a = FC.build(id, lib).args
            lds = [a[7], a[8], a[9], a[12], a[14], a[16]]                       # lda, ldb, ldc, ldr, ldaux, ldpre
            assert len(set(lds)) == 6, (id, lds)
        if entry in ('sconf_attn_fwd', 'sconf_attn_bwd'):
            triples = [tuple(x) for x in FC.build(id, lib).args if not isinstance(x, (int, float, FP.Region, type(None)))]
            assert len(triples) == (8 if entry == 'sconf_attn_bwd' else 4) and len(set(triples)) == len(triples), (id, triples)
            assert len({t[0] for t in triples}) == len(triples) and len({t[1] for t in triples}) == len(triples), (id, triples)
            assert all(x % 8 == 0 for t in triples for x in t), (id, triples)
