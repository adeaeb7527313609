"""CPU tests of the long form of CTC forced alignment (include/sconf_align_long.h, lcasr_amd.hip.align_long): the header against the
binding, the exports, the typing in both import orders, the host-side queries and refusals, the routing of
decoding.align.ctc_forced_align between the two units with both op layers replaced by the numpy restatement, and the layout of the
write-footprint cases.  The kernels themselves are tested in test_align_long_gpu.py."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

import align_long_footprint_cases as LC
import align_refs as AR
import footprint as FP
from cabi_header import assert_binding_is_header, header_abi
from conftest import ROOT

HEADER, PREFIX = 'sconf_align_long.h', 'sconf_lalign_'
SLABS = (256, 512, 1024, 2048, 4096, 8192)
ILLEGAL = (-1, 1, 128, 255, 257, 300, 768, 3072, 8191, 16384, 1 << 20)


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from lcasr_amd.hip import align_long
    return align_long.load()


def _declared():
    src = open(os.path.join(ROOT, 'include', HEADER)).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(sconf_[a-z0-9_]+)\s*\(', src)))


# ---- 1. the unit: header, binding, exports, typing ---------------------------------------------------------------------------------
def test_binding_is_the_header_and_the_other_units_do_not_name_it(lib):
    from lcasr_amd.hip import _lib, align, align_long
    funcs, enums = header_abi(HEADER, PREFIX)
    assert sorted(funcs) == _declared() and not enums
    assert set(funcs) == {'sconf_lalign_max_labels', 'sconf_lalign_default_slab_states', 'sconf_lalign_threads', 'sconf_lalign_states_per_thread',
                          'sconf_lalign_slabs', 'sconf_lalign_workspace', 'sconf_lalign_ctc'}
    assert_binding_is_header(funcs, align_long.PROTOTYPES, align_long.PLAIN, 'hip/align_long.py')
    # sconf_align_ctc's argument list with slab_states (an int) in front of the stream
    assert align_long.PROTOTYPES['sconf_lalign_ctc'] == align.PROTOTYPES['sconf_align_ctc'][:-1] + [ctypes.c_int, ctypes.c_void_p]
    assert align_long.Alignment is align.Alignment
    assert not any(n.startswith(PREFIX) for u in (_lib, align) for n in list(u.PROTOTYPES) + list(u.PLAIN))
    for f in (os.path.join('include', 'sconf.h'), os.path.join('include', 'sconf_align.h'), os.path.join('long-context-asr_amd', 'hip', '_lib.py'),
              os.path.join('long-context-asr_amd', 'hip', 'align.py')):
        assert 'lalign' not in open(os.path.join(ROOT, f)).read(), f
    assert lib.sconf_version() == 220


def test_every_declared_name_is_exported(lib):
    from lcasr_amd.hip import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert len(_declared()) == 7
    for n in _declared():
        assert hasattr(raw, n), f'{n} declared in include/{HEADER} but not exported'


_ORDER_CHILD = '''
import ctypes, sys
from lcasr_amd.hip import _lib
if sys.argv[1] == 'load-first': _lib.load()
from lcasr_amd.hip import align_long
lib = _lib.load()
for name, args in align_long.PROTOTYPES.items():
    assert list(getattr(lib, name).argtypes) == args and getattr(lib, name).restype is ctypes.c_int, name
    assert _lib.bound()[name] == (args, ctypes.c_int), name
for name, (args, res) in align_long.PLAIN.items():
    assert list(getattr(lib, name).argtypes) == args and getattr(lib, name).restype is res, name
    assert _lib.bound()[name] == (args, res), name
assert lib.sconf_lalign_workspace.restype is ctypes.c_int64 and lib.sconf_lalign_workspace(1, 100000, 65535, 0) > 1 << 32
print('typed', sys.argv[1])
'''


def test_the_unit_is_typed_in_both_import_orders(lib):
    for order in ('import-first', 'load-first'):
        r = subprocess.run([sys.executable, '-c', _ORDER_CHILD, order], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True)
        assert r.returncode == 0 and f'typed {order}' in r.stdout, r.stdout + r.stderr


# ---- 2. queries ------------------------------------------------------------------------------------------------------------------
def test_geometry_queries(lib):
    from lcasr_amd.decoding import align as D
    from lcasr_amd.hip import align, align_long
    M = lib.sconf_lalign_max_labels()
    assert M == 65535 == align_long.max_labels() == align_long.MAX_LABELS
    assert D.SHORT_FORM_LABELS == align.max_labels() == 8191               # the routing constant is the short unit's limit
    assert lib.sconf_lalign_default_slab_states() == 8192
    for w in SLABS + (0,):
        ww = w or 8192
        nt, spt = lib.sconf_lalign_threads(w), lib.sconf_lalign_states_per_thread(w)
        assert nt == min(1024, ww) and spt == ww // nt and nt * spt == ww and spt in (1, 2, 4, 8)
        cells = ww + 2 if spt == 1 else 3 + nt * (spt + 1)                 # a row: guard cells, and a padding cell per thread from 2 states on
        assert 2 * cells * 8 <= 160 * 1024 and (w != 0 or 2 * cells * 8 == 147504)      # two f64 rows fit the LDS
        for S in (0, 1, 127, 128, 129, 300, 700, 4095, 4096, 8191, 8192, 12288, M):
            assert lib.sconf_lalign_slabs(S, w) == -(-(2 * S + 1) // ww) == align_long.slabs(S, w)
        assert lib.sconf_lalign_slabs(-1, w) == -1 and lib.sconf_lalign_slabs(M + 1, w) == -1
    for w in ILLEGAL:
        assert lib.sconf_lalign_threads(w) == -1 and lib.sconf_lalign_states_per_thread(w) == -1 and lib.sconf_lalign_slabs(100, w) == -1
        assert lib.sconf_lalign_workspace(1, 100, 100, w) == -1
    with pytest.raises(ValueError, match='65535'):
        align_long.slabs(M + 1)
    # L - 1 a multiple of the slab: the last slab holds one state
    assert lib.sconf_lalign_slabs(128, 256) == 2 and lib.sconf_lalign_slabs(8192, 0) == 3 and lib.sconf_lalign_slabs(12288, 0) == 4


def _formula(B, N, Smax):
    """The workspace formula as include/sconf_align_long.h states it."""
    r256 = lambda n: (n + 255) // 256 * 256
    r8, r48 = (Smax + 7) // 8 * 8, (2 * Smax + 1 + 47) // 48 * 48
    return r256(4 * B) + r256(16 * B) + r256(2 * 16 * B * N) + r256(4 * B * N * (r8 + 12)) + r256(B * N * r48)


def test_workspace_query(lib):
    from lcasr_amd.hip import align_long
    ws = lib.sconf_lalign_workspace
    M = lib.sconf_lalign_max_labels()
    big = ws(1, 100000, M, 0)
    assert big > 1 << 32 and big == _formula(1, 100000, M) == align_long.align_workspace(1, 100000, M)
    assert ws(1, 45000, 12288, 0) == 3323520768 == _formula(1, 45000, 12288)                 # the figure in the header
    for B, N, S in ((1, 1, 0), (2, 100, 7), (3, 2048, 512), (1, 16384, 4096), (1, 9000, 8192), (2, 20000, 30000)):
        for w in (0, 256, 8192):
            assert ws(B, N, S, w) == _formula(B, N, S)
            assert 0 < ws(B, N, S, w) <= ws(B + 1, N, S, w) and ws(B, N, S, w) <= ws(B, N + 1, S, w) and ws(B, N, S, w) <= ws(B, N, S + 1, w)
    assert ws(2, 4000, 300, 0) > ws(1, 4000, 300, 0) and ws(1, 4001, 300, 0) > ws(1, 4000, 300, 0) and ws(1, 4000, 324, 0) > ws(1, 4000, 300, 0)
    # what the long form adds to the short unit's workspace: the per-sample record and the two edge columns
    assert ws(1, 16384, 4096, 0) - lib.sconf_align_workspace(1, 16384, 4096) == 256 + 2 * 16 * 16384
    for bad in ((-1, 10, 10), (0, 10, 10), (1, -1, 10), (1, 0, 10), (1, 10, -1), (1, 10, M + 1), (1 << 16, 1 << 16, 10)):
        assert ws(*bad, 0) == -1
    with pytest.raises(ValueError):
        align_long.align_workspace(1, 10, M + 1)
    with pytest.raises(ValueError):
        align_long.align_workspace(1, 10, 10, 300)


# ---- 3. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_name_their_cause(lib):
    one = ctypes.c_void_p(16)                                              # never dereferenced: every call below is refused on the host
    need = lib.sconf_lalign_workspace(1, 10, 3, 0)
    call = lambda blank=31, ws=need, B=1, N=10, C=32, S=3, w=0: lib.sconf_lalign_ctc(one, one, None, None, one, one, one, one, one, one, ws, B, N, C, S,
                                                                                    blank, w, None)
    assert call(blank=32) != 0 and b'blank' in lib.sconf_last_error()
    assert call(blank=-1) != 0 and b'blank' in lib.sconf_last_error()
    assert call(ws=need - 1) != 0 and b'workspace' in lib.sconf_last_error()
    assert call(S=65536, ws=1 << 40) != 0 and b'65535' in lib.sconf_last_error()
    assert call(S=-1, ws=1 << 40) != 0 and b'65535' in lib.sconf_last_error()
    for w in ILLEGAL:
        assert call(w=w, ws=1 << 40) != 0 and b'slab_states' in lib.sconf_last_error()
    assert call(C=30) != 0 and b'multiple of 4' in lib.sconf_last_error()
    assert call(N=0) != 0 and b'sizes' in lib.sconf_last_error()
    assert call(B=-1) != 0 and b'sizes' in lib.sconf_last_error()
    assert call(B=1 << 16, N=1 << 16, ws=1 << 60) != 0 and b'sizes' in lib.sconf_last_error()
    for missing in (0, 4, 5, 8, 9):                                        # log_probs, path, labels, score, workspace
        args = [one] * 10 + [need, 1, 10, 32, 3, 31, 0, None]
        args[2] = args[3] = None
        args[missing] = None
        assert lib.sconf_lalign_ctc(*args) != 0 and b'null' in lib.sconf_last_error()
    assert call(B=0) == 0                                                  # nothing to do, nothing launched
    assert call(B=0, w=300) == 0


# ---- 4. the public interface routes between the two units ------------------------------------------------------------------------
@pytest.fixture
def routed(monkeypatch):
    """Both op layers replaced by the numpy restatement, each call recorded under its unit's name."""
    from lcasr_amd.decoding import align as D
    from lcasr_amd.hip import align_long
    calls = []

    def restated(unit):
        def op(lp, tg, il, tl, blank):
            calls.append((unit, tg.shape[1]))
            return AR.ctc_align(lp, tg, il, tl, blank)
        return op
    monkeypatch.setattr(D.align_kernels, 'ctc_align', restated('short'))
    monkeypatch.setattr(align_long, 'ctc_align', restated('long'))
    return D, calls


def test_forced_align_routes_by_the_widest_transcript(routed):
    D, calls = routed
    lp, tg = AR.random_case(4, 2, 24, 8, 6)
    for Smax, unit in ((8191, 'short'), (8192, 'long'), (65535, 'long')):
        wide = torch.zeros(2, Smax, dtype=torch.int32)
        wide[:, :6] = tg
        got = D.ctc_forced_align(lp, wide, input_lengths=[24, 20], target_lengths=[6, 4], blank=7)
        want = AR.ctc_align(lp, tg, torch.tensor([24, 20]), torch.tensor([6, 4]), 7)
        assert calls[-1] == (unit, Smax) and isinstance(got, D.CTCAlignment)
        assert torch.equal(got.path, want.path) and torch.equal(got.labels, want.labels) and torch.equal(got.score, want.score)
        assert torch.equal(got.spans[:, :6], want.spans) and bool((got.spans[:, 6:] == -1).all()) and got.spans.shape == (2, Smax, 2)
    single = D.ctc_forced_align(lp[0], [1, 2, 3] + [0] * 8189, target_lengths=[3], blank=7)
    assert calls[-1] == ('long', 8192) and single.path.shape == (24,) and single.spans.shape == (8192, 2)
    n = len(calls)
    with pytest.raises(ValueError, match='65535'):
        D.ctc_forced_align(lp, torch.zeros(2, 65536, dtype=torch.int32), target_lengths=[6, 4], blank=7)
    assert len(calls) == n


_SHORT_CHILD = '''
import sys
import torch
sys.path.insert(0, 'tests')
import align_refs as AR
from lcasr_amd.decoding import align as D
from lcasr_amd.hip import _lib
D.align_kernels.ctc_align = AR.ctc_align
lp, tg = AR.random_case(4, 1, 24, 8, 6)
a = D.ctc_forced_align(lp[0], tg[0], blank=7)
assert a.path.shape == (24,)
assert 'lcasr_amd.hip.align_long' not in sys.modules and _lib._lib is None
assert not any(n.startswith('sconf_lalign_') for u in _lib._units for t in u for n in t)
print('short only')
'''


def test_a_short_transcript_neither_binds_the_long_unit_nor_loads_the_library():
    r = subprocess.run([sys.executable, '-c', _SHORT_CHILD], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True)
    assert r.returncode == 0 and 'short only' in r.stdout, r.stdout + r.stderr


def test_a_cpu_tensor_is_refused_by_the_long_product_path(lib):
    from lcasr_amd.decoding.align import ctc_forced_align
    lp, _ = AR.random_case(1, 1, 8, 8, 3)
    with pytest.raises(RuntimeError, match='GPU'):
        ctc_forced_align(lp[0], [1] * 8192, target_lengths=[3], blank=7)


# ---- 5. footprint cases --------------------------------------------------------------------------------------------------------------
def test_every_entry_point_has_a_case_or_launches_nothing():
    from lcasr_amd.hip import align_long
    assert LC.NO_LAUNCH == set(align_long.PLAIN)
    assert {entry for entry, _ in LC.CASES.values()} == set(align_long.PROTOTYPES)


@pytest.mark.parametrize('id', list(LC.CASES))
def test_case_layout(lib, id):
    from lcasr_amd.hip import align_long
    c = LC.build(id, lib)
    assert c.name == LC.CASES[id][0]
    FP.check_layout(c, align_long.PROTOTYPES)
    B, N, C, Smax = c.args[11:15]
    ws = c.arena.regions['workspace']
    assert ws.cls == FP.SCRATCH and ws.dtype == torch.uint8
    assert ws.numel == ws.extent == c.args[10] == lib.sconf_lalign_workspace(B, N, Smax, c.args[16])
    want = {'path': ((B, N), torch.int32), 'labels': ((B, N), torch.int32), 'spans': ((B, Smax, 2), torch.int32),
            'token_logp': ((B, Smax), torch.float32), 'score': ((B,), torch.float64)}
    for name, (shape, dtype) in want.items():
        r = c.arena.regions[name]
        assert r.cls == FP.OUT and r.shape == shape and r.dtype == dtype and r.unspecified is None and r.order is None
    assert {n for n, r in c.arena.regions.items() if r.cls != FP.IN} == set(want) | {'workspace'}
    assert ('input_lengths' in c.arena.regions) == (c.args[2] is not None) and ('target_lengths' in c.arena.regions) == (c.args[3] is not None)


def test_the_cases_cover_seams_and_launch_forms(lib):
    built = [LC.build(id, lib) for id in LC.CASES]
    geo = {(lib.sconf_lalign_threads(c.args[16]), lib.sconf_lalign_states_per_thread(c.args[16])) for c in built}
    assert {(256, 1), (512, 1), (1024, 2), (1024, 8)} <= geo
    counts = {lib.sconf_lalign_slabs(c.args[14], c.args[16]) for c in built}
    assert {1, 2, 3} <= counts
    assert any(2 * c.args[14] % (c.args[16] or 8192) == 0 and c.args[14] > 0 for c in built)      # a last slab of one state
