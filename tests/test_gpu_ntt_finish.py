"""The passes that finish a 60-bit transform -- N^-1 by shift in the last inverse stage, the one-step final reduction of the forward
transform (csrc/ntt_finish.h) -- against the CPU oracle, bit for bit.  Sizes: logn 12 (the strided passes' branch without phase
B), 13 (odd split) and 16.  Rows: those of test_gpu_ntt_lazy16.py -- the largest prime below 2^60, the smallest above 2^59, a 52-bit
and a 58-bit prime, and a 61-bit prime as the control the lazy kernels never see -- plus the smallest prime above 2^20 the lazy
modes can meet, which reaches them in the inverse once MOAI_NTT_FP=0 keeps it off the FP64 units.  Inputs: all q-1, all 0,
alternating 0 / q-1, random; for the inverse also the same residues raised by 3q on every row below 2^60, the [0, 4q) input
contract of the lazy integer butterflies (the FP64 rows accept it too; the 61-bit row's exact butterflies take [0, 2q) and stay
canonical).  With MOAI_NTT_LAZY16 on and off (off: M_LAZY8, a guard in every stage)."""
import numpy as np
import pytest

import oracle as O
from test_gpu_ntt_lazy16 import NPOLY, PATTERNS, ntt_prime, primes_for

pytestmark = pytest.mark.gpu

_cases = {}


def case(logn):
    """inputs [pattern][NPOLY][L][N] and the oracle's transforms of them, computed once per size and never written to"""
    if logn in _cases:
        return _cases[logn]
    n = 1 << logn
    primes = primes_for(logn) + [ntt_prime(logn, (1 << 20) + 1, +1)]
    L = len(primes)
    assert (1 << 20) < primes[5] < (1 << 24) and primes[4] > (1 << 60) and all((q - 1) % (2 * n) == 0 for q in primes)
    rng = np.random.default_rng(2600 + logn)
    qcol = np.array(primes, dtype=np.uint64)[None, :, None]
    x = np.zeros((len(PATTERNS), NPOLY, L, n), dtype=np.uint64)
    x[0] = qcol - np.uint64(1)
    x[2, 0, :, 1::2] = (qcol - np.uint64(1))[0]
    x[2, 1, :, 0::2] = (qcol - np.uint64(1))[0]
    x[3] = O.uniform_rns(rng, primes, (NPOLY,), n)
    # + 3q on the rows below 2^60 (4q < 2^62 there)
    raise3 = np.array([3 * q if q < (1 << 60) else 0 for q in primes], dtype=np.uint64)[None, :, None]
    octx = O.Context(logn, primes)
    flat = x.reshape(-1, L, n)
    c = dict(primes=primes, x=x, raised=x + raise3, fwd=octx.ntt(flat, L).reshape(x.shape),
             inv=octx.ntt(flat, L, inverse=True).reshape(x.shape))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _cases[logn] = c
    return c


@pytest.mark.parametrize("lazy16", [1, 0])
@pytest.mark.parametrize("logn", [12, 13, 16])
def test_finishing_passes_match_oracle(moai, logn, lazy16):
    c = case(logn)
    primes, L = c["primes"], len(c["primes"])
    ctx = moai.Context(logn, primes)
    try:
        for fp in (1, 0):
            moai.hip.set_tuning("MOAI_NTT_LAZY16", lazy16)
            moai.hip.set_tuning("MOAI_NTT_FP", fp)
            for k, name in enumerate(PATTERNS):
                what = "%s, MOAI_NTT_FP=%d" % (name, fp)
                x = c["x"][k]
                d = moai.DeviceBuffer.from_numpy(x)
                ctx.ntt_forward(d, NPOLY, L)
                assert (d.to_numpy(x.shape) == c["fwd"][k]).all(), "forward, " + what
                ctx.ntt_inverse(d, NPOLY, L)
                assert (d.to_numpy(x.shape) == x).all(), "round trip, " + what
                ctx.ntt_inverse(d, NPOLY, L)  # canonical data that is no transform of anything in particular
                assert (d.to_numpy(x.shape) == c["inv"][k]).all(), "inverse, " + what
                d = moai.DeviceBuffer.from_numpy(c["raised"][k])
                ctx.ntt_inverse(d, NPOLY, L)
                assert (d.to_numpy(x.shape) == c["inv"][k]).all(), "inverse of residues raised by 3q, " + what
    finally:
        moai.hip.reset_tuning()
