"""TEST INFRASTRUCTURE: option scrub / irdm_scrub_device (csrc/scrub.hpp) restated in numpy, on interleaved float32."""
import numpy as np


def scrub(x, e=40):
    """x: float32 [2 n], I and Q interleaved (any bit patterns).  Returns (the scrubbed copy, the six figures): a component is
    good iff |c| <= 2^e, a sample with a component that is not good becomes +0, +0, every other sample keeps its bits"""
    c = np.ascontiguousarray(x, np.float32).reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        good = np.abs(c) <= np.ldexp(np.float32(1), e)
    bad, fin = ~good.all(axis=1), np.isfinite(c)
    y = c.view(np.uint32).copy()
    y[bad] = 0
    at = np.flatnonzero(bad)
    return y.view(np.float32).reshape(-1), dict(n_zeroed=len(at), n_nonfinite=int((~fin).sum()), n_over=int((fin & ~good).sum()),
                                                first=int(at[0]) if len(at) else 0, last=int(at[-1]) if len(at) else 0)
