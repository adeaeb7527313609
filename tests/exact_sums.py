"""Exact tensor checksums of the seed-built fixtures.  Standalone (math, numpy and a tensor's own methods only), so that both the
tests and the fixture generator tools/make_subsample4_golden.py can import it without any pytest module."""
import math

import numpy as np


def checksums(t):
    """[sum, sum of squares] of a tensor, exact in float64 up to the final rounding: a float32 (or integer) value and its square are
    exact in float64 and math.fsum adds without intermediate rounding."""
    v = t.detach().double().reshape(-1)
    return np.array([math.fsum(v.tolist()), math.fsum((v * v).tolist())], dtype=np.float64)
