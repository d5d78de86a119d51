"""The two number checkers that the argument checks of the host modules share."""
import math

import numpy as np


def int_in(name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError("%s must be an integer in %d .. %d: got %r" % (name, lo, hi, v))
    return int(v)


def number(name, v):
    try:
        f = float(v)
    except (TypeError, ValueError):
        f = float("nan")
    if isinstance(v, bool) or not math.isfinite(f):
        raise ValueError("%s must be a finite number: got %r" % (name, v))
    return f
