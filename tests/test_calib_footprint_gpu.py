"""Write-footprint tests of the calibration unit on the device: every case of tests/calib_footprint_cases.py runs twice out of one
guarded arena (0xFF fill, random fill) through tests/footprint.py - guards intact, only the outputs and the alignment's workspace
written, the workspace at exactly ws_off[P] bytes, every element of the outputs written from the inputs alone (bit-equal between the
fills, whatever the workspace and the columns behind `classes` held), the integers equal to the numpy restatement and the
confidences within the confidence unit's own tolerance of it."""
import pytest
import torch

import calib_footprint_cases as KC
import footprint as FP

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def calib():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from lcasr_amd.hip import calib as k
    k.load()
    return k


@pytest.mark.parametrize('id', list(KC.CASES))
def test_calib(calib, id):
    FP.run_on_device(KC.build(id, calib.load()), calib.PROTOTYPES)
