"""-m gpu: the band scan's decline and redo paths in MID-STREAM, on the card -- where the chained launch, the speculation
stream, the pinned control words and the device-side "predecessor committed" check run concurrently for real.  Cases, runners
and every assertion are tests/decline_checks.py's (its docstring says what each case is and what the runs took), shared with
tests/test_decline_emul.py: the oracle's records in its order, the path claimed, and the carried state of a dense-kernel run."""
import pytest

import decline_checks as dc

pytestmark = pytest.mark.gpu

RUNS = [(name, config, packed) for name, c in dc.CASES.items() for config in c.configs for packed in (False, True)]


@pytest.mark.parametrize("name,config,packed", RUNS, ids=["%s-%s-%s" % (n, c, "packed" if p else "full") for n, c, p in RUNS])
def test_decline(name, config, packed):
    s = dc.check(name, config, packed=packed)
    assert s["bursts"] >= 10, s
