"""CPU test: libsconf_hip.so builds (hipcc cross-compiles gfx950 without a GPU), loads, and exports exactly the entry points the
headers under include/ declare, each unit's bound in its own module under hip/ with the header's signature and typed by the one
loader of hip/_lib.py.  No compute call is made."""
import ctypes
import importlib
import os
import re
import subprocess
import sys

import pytest

from cabi_header import assert_binding_is_header, header_abi
from conftest import ROOT

# unit -> (header, binding module under hip/, name prefix, least number of declared names, names that must be among them)
UNITS = {
    'core': ('sconf.h', '_lib', 'sconf_', 27, set()),
    'audio': ('sconf_audio.h', 'audio', 'sconf_audio_', 3, set()),
    'align': ('sconf_align.h', 'align', 'sconf_align_', 4, {'sconf_align_max_labels', 'sconf_align_state_bytes', 'sconf_align_workspace', 'sconf_align_ctc'}),
    'beam': ('sconf_beam.h', 'beam', 'sconf_beam_', 4, {'sconf_beam_max_width', 'sconf_beam_max_tokens', 'sconf_beam_workspace', 'sconf_beam_ctc'}),
}


def _declared(header):
    src = open(os.path.join(ROOT, 'include', header)).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(sconf_[a-z0-9_]+)\s*\(', src)))


def test_library_exports_every_declared_symbol():
    import __graft_entry__ as g
    g.build()
    from lcasr_amd.hip import _lib
    assert os.path.exists(_lib.LIB_PATH)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for header in (u[0] for u in UNITS.values()):
        for n in _declared(header):
            assert hasattr(lib, n), f'{n} declared in include/{header} but not exported'
    lib.sconf_version.restype = ctypes.c_int
    assert lib.sconf_version() == 220
    lib.sconf_last_error.restype = ctypes.c_char_p
    assert isinstance(lib.sconf_last_error(), bytes)


@pytest.mark.parametrize('unit', list(UNITS))
def test_bindings_and_enums_match_the_header_signature_for_signature(unit):
    """Every unit types its calls by hand: each argument list and return type must be the header's (every declared name is exported:
    the test above), and the op layer's enum values the header's enumerators.  The units add nothing to the first one: sconf.h, the
    core tables and the text of _lib.py name none of their entry points."""
    from lcasr_amd.hip import _lib, ops
    header, module, prefix, at_least, required = UNITS[unit]
    binding = importlib.import_module('lcasr_amd.hip.' + module)
    funcs, enums = header_abi(header, prefix)
    assert sorted(funcs) == _declared(header) and len(funcs) >= at_least and required <= set(funcs)
    assert_binding_is_header(funcs, binding.PROTOTYPES, binding.PLAIN, f'hip/{module}.py')
    if unit != 'core':
        assert not enums
        assert not any(n.startswith(prefix) for n in list(_lib.PROTOTYPES) + list(_lib.PLAIN))
        assert prefix not in open(os.path.join(ROOT, 'include', 'sconf.h')).read()
        assert prefix not in open(os.path.join(ROOT, 'long-context-asr_amd', 'hip', '_lib.py')).read()
        return
    assert (ops.F32, ops.BF16) == (enums['SCONF_F32'], enums['SCONF_BF16'])
    assert ops.ACT and all(v == enums['SCONF_ACT_' + k.upper()] for k, v in ops.ACT.items())
    assert ops.LAYOUT == {k[len('SCONF_GEMM_'):].lower(): v for k, v in enums.items() if k.startswith('SCONF_GEMM_')}
    names = {'layer_norm': 'SCONF_NORM_LAYER', 'rms_norm': 'SCONF_NORM_RMS', 'rms_norm_apex': 'SCONF_NORM_RMS_APEX'}
    assert ops.NORM_MODE == {k: enums[n] for k, n in names.items()}
    assert len(names) == sum(k.startswith('SCONF_NORM_') for k in enums)


_ORDER_CHILD = '''
import ctypes, sys
from lcasr_amd.hip import _lib
if sys.argv[1] == 'load-first': _lib.load()
from lcasr_amd.hip import align, audio, beam
lib = _lib.load()
for unit in (audio, align, beam):
    for name, args in unit.PROTOTYPES.items():
        assert list(getattr(lib, name).argtypes) == args and getattr(lib, name).restype is ctypes.c_int, name
        assert _lib.bound()[name] == (args, ctypes.c_int), name
    for name, (args, res) in unit.PLAIN.items():
        assert list(getattr(lib, name).argtypes) == args and getattr(lib, name).restype is res, name
assert list(lib.sconf_beam_ctc.argtypes) == beam.PROTOTYPES['sconf_beam_ctc'] and lib.sconf_beam_workspace.restype is ctypes.c_int64
assert set(_lib.bound()) == {n for u in (_lib, audio, align, beam) for n in list(u.PROTOTYPES) + list(u.PLAIN)}
print('typed', sys.argv[1])
'''


def test_units_are_typed_in_both_import_orders():
    """A unit imported before the library is loaded is typed by load(); one imported after it is typed by its register call.  Fresh
    child processes: this one has long imported everything.  No GPU is touched: loading the library and setting argtypes
    initialises nothing."""
    import __graft_entry__ as g
    g.build()
    for order in ('import-first', 'load-first'):
        r = subprocess.run([sys.executable, '-c', _ORDER_CHILD, order], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True)
        assert r.returncode == 0 and f'typed {order}' in r.stdout, r.stdout + r.stderr


def test_untyped_call_is_refused():
    from lcasr_amd.hip import _lib
    with pytest.raises(RuntimeError, match='sconf_version_no_such'):
        _lib.call('sconf_version_no_such')
    with pytest.raises(RuntimeError, match='sconf_num_cus_no_such'):
        _lib.call('sconf_num_cus_no_such', 1, 2)


def test_double_registration_is_refused():
    from lcasr_amd.hip import _lib, beam
    with pytest.raises(ValueError, match='sconf_beam_ctc'):
        _lib.register(beam.PROTOTYPES, {})
    with pytest.raises(ValueError, match='sconf_version'):
        _lib.register({}, {'sconf_version': ([], ctypes.c_int)})
    with pytest.raises(ValueError, match='sconf_new_a'):
        _lib.register({'sconf_new_a': []}, {'sconf_new_a': ([], ctypes.c_int)})
    assert 'sconf_new_a' not in _lib.bound() and not any('sconf_new_a' in t for u in _lib._units for t in u)


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
