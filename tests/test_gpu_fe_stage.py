"""The front end's shared load stage (csrc/fe_stage.hpp) on the GPU: the case table of tests/fe_stage_cases.py -- every
instantiation of K0, K0r and K0w that differs in the load stage, in all eight device formats, fed whole, in ragged feeds and
after a reset, against the plain C models bit for bit."""
import pytest

import fe_stage_cases as fc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("row", sorted(fc.ROWS))
def test_load_stage_equals_the_models_in_every_format(row):
    res = fc.check(row)
    assert len(res) == len(fc.FORMATS) * len(fc.Q_LIST) and all(v > 0 for v in res.values()), res
