"""CPU checks of the write-footprint cases of the audio ABI unit (tests/audio_footprint_cases.py): every launching entry point of
lcasr_amd.hip.audio has a case, and every case is laid out on a CPU arena - regions disjoint, aligned and guarded, the argument list
as the binding types it, the declared output shape the shape the restatement returns, the workspace exactly what the query says.
The library builds here as test_cabi.py builds it; the two queries are host-only."""
import pytest
import torch

import audio_footprint_cases as AC
import footprint as FP


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from lcasr_amd.hip import audio
    return audio.load()


def test_every_audio_entry_point_has_a_case_or_launches_nothing():
    from lcasr_amd.hip import audio
    assert AC.NO_LAUNCH == set(audio.PLAIN)
    assert {entry for entry, _ in AC.CASES.values()} == set(audio.PROTOTYPES)


@pytest.mark.parametrize('id', list(AC.CASES))
def test_audio_case_layout(lib, id):
    from lcasr_amd.hip import audio
    c = AC.build(id, lib)
    assert c.name == AC.CASES[id][0]
    FP.check_layout(c, audio.PROTOTYPES)
    ws = c.arena.regions['workspace']
    B, T, n_mels = c.args[12:15]
    assert ws.cls == FP.SCRATCH and ws.dtype == torch.uint8 and ws.numel == ws.extent == lib.sconf_audio_melspec_workspace(B, T, n_mels)
    spec = c.arena.regions['spec']
    assert spec.cls == FP.OUT and spec.shape == (B, n_mels, T) and T == lib.sconf_audio_tile_frames() + 1
    raw = c.arena.regions.get('raw')
    assert (raw is not None) == (bool(c.args[9]) and spec.dtype == torch.bfloat16)          # scratch only for normalised bf16 output


def test_workspace_grows_with_rows_mels_and_tiles_not_with_bins(lib):
    F = lib.sconf_audio_tile_frames()
    q = lib.sconf_audio_melspec_workspace
    base = q(1, F, 80)
    per_tile = q(1, 2 * F, 80) - base
    assert per_tile == 80 * 24 and q(1, F + 1, 80) == q(1, 2 * F, 80)                       # one (n, mean, M2) f64 triple per (mel, tile)
    assert q(3, 5 * F, 80) - q(3, 4 * F, 80) == 3 * per_tile
    assert q(1, 2 * F, 40) - q(1, F, 40) == per_tile // 2
    hour = q(1, 360001, 80)
    assert hour < 360001 * 80 * 4 // 4 and hour < 360001 * 257 * 4 // 10        # under a quarter of the f32 output, a tenth of a (T, 257) spectrum
    assert q(0, F, 80) == -1 and q(1, 0, 80) == -1 and q(1, F, 0) == -1 and q(1, F, 129) == -1
