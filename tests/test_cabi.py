"""CPU test: libsconf_hip.so builds (hipcc cross-compiles gfx950 without a GPU), loads, and exports exactly the
entry points include/sconf.h declares, each bound in hip/_lib.py with the header's signature.  No compute call is made."""
import ctypes
import os
import re

from conftest import ROOT


def _declared():
    src = open(os.path.join(ROOT, 'include', 'sconf.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(sconf_[a-z0-9_]+)\s*\(', src)))


def test_library_exports_every_declared_symbol():
    import __graft_entry__ as g
    g.build()
    from lcasr_amd.hip import _lib
    assert os.path.exists(_lib.LIB_PATH)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert len(names) >= 27
    for n in names:
        assert hasattr(lib, n), f'{n} declared in include/sconf.h but not exported'
    bound = set(_lib.PROTOTYPES) | set(_lib.PLAIN)
    assert bound == set(names), (bound ^ set(names))
    lib.sconf_version.restype = ctypes.c_int
    assert lib.sconf_version() >= 100
    lib.sconf_last_error.restype = ctypes.c_char_p
    assert isinstance(lib.sconf_last_error(), bytes)


_CTYPE = {'sconf_stream_t': ctypes.c_void_p, 'int64_t': ctypes.c_int64, 'int': ctypes.c_int, 'int32_t': ctypes.c_int, 'float': ctypes.c_float}
_RESTYPE = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'const char*': ctypes.c_char_p}


def _header_abi():
    """(name -> (argtypes, restype), enumerator -> value) of include/sconf.h.  Every statement between the extern "C" braces must be
    the stream typedef, an anonymous enum or a function declaration over the types above: anything else raises."""
    src = open(os.path.join(ROOT, 'include', 'sconf.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    body = re.search(r'extern "C" \{\s*#endif(.*)#ifdef __cplusplus\s*\}', src, flags=re.S).group(1)
    funcs, enums = {}, {}
    for stmt in (' '.join(s.split()) for s in body.split(';')):
        if not stmt or stmt == 'typedef struct ihipStream_t* sconf_stream_t':
            continue
        m = re.fullmatch(r'enum \{(.*)\}', stmt)
        if m:
            for item in m.group(1).split(','):
                k, v = re.fullmatch(r'\s*(SCONF_[A-Z0-9_]+) = (\d+)\s*', item).groups()
                assert k not in enums, k
                enums[k] = int(v)
            continue
        m = re.fullmatch(r'(const char\*|int64_t|int) (sconf_[a-z0-9_]+) ?\((.*)\)', stmt)
        assert m, f'include/sconf.h: cannot classify the statement {stmt!r}'
        ret, name, params = m.groups()
        args = []
        for p in ([] if params.strip() == 'void' else params.split(',')):
            p = p.strip()
            pm = re.fullmatch(r'(?:const )?([a-z0-9_]+) ?(\*?) ?[A-Za-z_][A-Za-z0-9_]*', p)
            assert pm and (pm.group(2) or pm.group(1) in _CTYPE), f'include/sconf.h: {name}: cannot classify the parameter {p!r}'
            args.append(ctypes.c_void_p if pm.group(2) else _CTYPE[pm.group(1)])
        assert name not in funcs, f'{name} declared twice'
        funcs[name] = (args, _RESTYPE[ret])
    return funcs, enums


def test_bindings_and_enums_match_the_header_signature_for_signature():
    """hip/_lib.py types every call by hand: each argument list and return type must be the header's, and the op layer's enum
    values the header's enumerators.  (A swapped int / int64_t or a dropped argument would be a miscall into a kernel.)"""
    from lcasr_amd.hip import _lib, ops
    funcs, enums = _header_abi()
    assert sorted(funcs) == _declared()
    bound = {n: (a, ctypes.c_int) for n, a in _lib.PROTOTYPES.items()}
    assert not set(bound) & set(_lib.PLAIN)
    bound.update(_lib.PLAIN)
    assert set(bound) == set(funcs)
    for name, (args, res) in funcs.items():
        got_args, got_res = bound[name]
        assert got_res is res, f'{name}: returns {res.__name__} in the header, {got_res.__name__} in _lib.py'
        assert len(got_args) == len(args), f'{name}: {len(args)} arguments in the header, {len(got_args)} in _lib.py'
        for i, (g, w) in enumerate(zip(got_args, args)):
            assert g is w, f'{name}: argument {i} is {w.__name__} in the header, {g.__name__} in _lib.py'
    assert (ops.F32, ops.BF16) == (enums['SCONF_F32'], enums['SCONF_BF16'])
    assert ops.ACT and all(v == enums['SCONF_ACT_' + k.upper()] for k, v in ops.ACT.items())
    assert ops.LAYOUT == {k[len('SCONF_GEMM_'):].lower(): v for k, v in enums.items() if k.startswith('SCONF_GEMM_')}
    names = {'layer_norm': 'SCONF_NORM_LAYER', 'rms_norm': 'SCONF_NORM_RMS', 'rms_norm_apex': 'SCONF_NORM_RMS_APEX'}
    assert ops.NORM_MODE == {k: enums[n] for k, n in names.items()}
    assert len(names) == sum(k.startswith('SCONF_NORM_') for k in enums)


def test_host_side_argument_validation_sets_error():
    """Entry points validate shapes on the host before any launch (no GPU needed for the failure path)."""
    from lcasr_amd.hip import _lib
    lib = _lib.load()
    rc = lib.sconf_gemm_bf16(7, None, None, None, 8, 8, 8, 8, 8, 8, None, None, 8, None, 8, None, 8, 1.0, 0, 0, 1, None)
    assert rc != 0 and b'bad layout' in lib.sconf_last_error()
    rc = lib.sconf_norm_fwd(0, None, 0, None, None, None, 0, None, None, 4, 4096, 1e-5, None)
    assert rc != 0 and b'2048' in lib.sconf_last_error()


def test_convmod_geometry_queries_answer_on_the_host():
    """sconf_convmod_tile_frames / sconf_convmod_bwd_rows_per_thread: the launch geometry of the conv-module kernels, decided on the
    host from the problem size alone (8 for small problems, doubling up to 64 as B * ceil(N / TN) * d / 4 reaches 131072)."""
    from lcasr_amd.hip import _lib
    lib = _lib.load()
    assert lib.sconf_convmod_tile_frames(2, 100, 64) == 8 and lib.sconf_convmod_bwd_rows_per_thread(2, 100, 64) == 8
    assert lib.sconf_convmod_tile_frames(2, 16500, 256) == 16 and lib.sconf_convmod_bwd_rows_per_thread(2, 16500, 256) == 16
    assert lib.sconf_convmod_tile_frames(2, 33000, 256) == 32 and lib.sconf_convmod_bwd_rows_per_thread(2, 33000, 256) == 32
    assert lib.sconf_convmod_tile_frames(128, 2048, 768) == 64 and lib.sconf_convmod_bwd_rows_per_thread(128, 2048, 768) == 64
    assert lib.sconf_convmod_tile_frames(2, 100, 66) == -1 and lib.sconf_convmod_bwd_rows_per_thread(0, 100, 64) == -1


def test_attention_kernel_set_query_answers_on_the_host(monkeypatch):
    """sconf_attn_waves: 8-wave kernels for head_dim 128 from N = 256 on while a view fits 32-bit byte offsets, else the 4-wave ones."""
    from lcasr_amd.hip import _lib
    lib = _lib.load()
    monkeypatch.delenv('SCONF_ATTN_WIDE', raising=False)
    assert lib.sconf_attn_waves(128, 2048, 256) == 8 and lib.sconf_attn_waves(128, 255, 256) == 4
    assert lib.sconf_attn_waves(64, 2048, 128) == 4 and lib.sconf_attn_waves(256, 2048, 512) == 4 and lib.sconf_attn_waves(32, 2048, 64) == 4
    assert lib.sconf_attn_waves(128, 2048, 1 << 21) == 4            # (N - 1) * stride * 2 bytes does not fit 32 bits
    assert lib.sconf_attn_waves(48, 2048, 96) == -1
    monkeypatch.setenv('SCONF_ATTN_WIDE', '0')
    assert lib.sconf_attn_waves(128, 2048, 256) == 4
