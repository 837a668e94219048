"""Writes tests/golden/ref_sincos.npz: the arguments of tests/sincos_args.py with their exact sin and cos.

    python tests/golden/make_golden_sincos.py

Needs mpmath (any sympy brings it).  For every argument: sin and cos at 200 bits — mpmath reduces the argument at a working
precision raised by the cancellation, so the doubles nearest k pi/2 get all 200 bits too — stored as a double-double: hi the
correctly rounded double, lo the double nearest exact - hi.  compute() is what tests/test_sincos.py compares the committed file with.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sincos_args as A  # noqa: E402

PREC = 200


def _split(x, mp):
    """(hi, lo) of the mpf x; checks that hi is the nearest double"""
    hi = float(x)
    rest = x - mp.mpf(hi)
    lo = float(rest)
    if hi != 0.0 and np.isfinite(hi):
        half = mp.ldexp(mp.mpf(float(np.spacing(abs(hi)))), -1)  # half the gap above |hi|; the gap below a power of two is smaller
        if np.frexp(abs(hi))[0] == 0.5 and mp.sign(rest) * mp.sign(x) < 0 and abs(hi) > 2.3e-308:
            half = half / 2
        assert abs(rest) <= half, (hi, lo)
    return hi, lo


def compute():
    """the fixture's arrays"""
    import mpmath
    mp = mpmath.mp
    a, fam, k = A.build()
    out = {"a": a, "family": fam, "k": k}
    cols = {name: np.empty(len(a)) for name in ("sin_hi", "sin_lo", "cos_hi", "cos_lo")}
    with mp.workprec(PREC):
        # the args module's rational pi, and the multiples its k columns name
        assert abs(mp.mpf(A.PI.numerator) / A.PI.denominator - mp.pi) < mp.mpf(10) ** -49
        for i in np.nonzero((fam == 1) | (fam == 2))[0]:
            t = mp.pi * int(k[i]) / 2 if fam[i] == 1 else mp.pi * (2 * abs(int(k[i])) + 1) / 4 * (1 if a[i] > 0 else -1)
            assert abs(mp.mpf(float(a[i])) - t) <= 2.5 * float(np.spacing(abs(a[i]))), (a[i], k[i])
        for i, x in enumerate(a):
            x = mp.mpf(float(x))
            cols["sin_hi"][i], cols["sin_lo"][i] = _split(mp.sin(x), mp)
            cols["cos_hi"][i], cols["cos_lo"][i] = _split(mp.cos(x), mp)
    out.update(cols)
    return out


if __name__ == "__main__":
    arrays = compute()
    np.savez(A.GOLDEN, **arrays)
    print("%s: %d arguments, %d bytes" % (A.GOLDEN, len(arrays["a"]), os.path.getsize(A.GOLDEN)))
