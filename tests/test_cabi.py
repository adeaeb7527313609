"""CPU test: libsconf_hip.so builds (hipcc cross-compiles gfx950 without a GPU), loads, and exports exactly the
entry points include/sconf.h declares.  No compute call is made."""
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
