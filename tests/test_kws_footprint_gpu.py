"""Write-footprint tests of the keyword-search unit on the device: every case of tests/kws_footprint_cases.py runs twice out of one
guarded arena (0xFF fill, random fill) through tests/footprint.py - guards intact, only the three outputs and the workspace written,
the workspace at exactly the queried size, every element of the outputs written from the inputs alone (bit-equal between the
fills, whatever the workspace and the columns behind `classes` held) and equal to the numpy restatement at tol = 0."""
import pytest
import torch

import footprint as FP
import kws_footprint_cases as KC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def kws():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from lcasr_amd.hip import kws as k
    k.load()
    return k


@pytest.mark.parametrize('id', list(KC.CASES))
def test_kws(kws, id):
    FP.run_on_device(KC.build(id, kws.load()), kws.PROTOTYPES)
