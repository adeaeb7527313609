"""Write-footprint tests of the confidence unit on the device: every case of tests/confid_footprint_cases.py runs twice out of one
guarded arena (0xFF fill, random fill) through tests/footprint.py - guards intact (the NaN in the columns behind `classes` never
reaches an output), only idx and conf, or targets, spans and target_lengths, or out written - nothing past S_cap labels of a
sequence that has more - every element of them written from the inputs alone (bit-equal between the fills), integers equal to the
float64 restatement's and confidences within confid_refs.tolerance of it."""
import pytest
import torch

import confid_footprint_cases as CC
import footprint as FP

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def confid():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from lcasr_amd.hip import confid as c
    c.load()
    return c


@pytest.mark.parametrize('id', list(CC.CASES))
def test_confid(confid, id):
    FP.run_on_device(CC.build(id, confid.load()), confid.PROTOTYPES)
