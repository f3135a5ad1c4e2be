"""The arguments on which sq::facos is held to the oracle (tests/test_acos_series.py on the host, tests/test_gpu_acos_series.py on the
device), and the oracle's values of them, computed once per process.

crd::acos_ has two ranges, |x| <= 0.5 and beyond, which share one evaluation of the arcsine series: the arguments crowd the places where
the range, the sign or the domain changes, and cover what randomVector feeds it.
* every binary32 within 4096 ulps of 0, +-0.5 and +-1, on both sides of each;
* +-0.5, +-1, +-0, 1.0000001 (the first binary32 above 1), NaN and +-inf;
* 2 * unit_float(n) - 1 in binary32, as randomVector forms it (oracle/sq_oracle.c, sqo_random_vector), for 2^18 seeded words n."""
import functools

import numpy as np

from bitcmp import nan_eq

f32 = np.float32
ULPS = 4096
N_WORDS = 1 << 18


def around(value):
    """Every binary32 within ULPS ulps of `value` (value != 0): its bit pattern +- ULPS."""
    b = int(np.array([value], f32).view(np.uint32)[0])
    return np.arange(b - ULPS, b + ULPS + 1, dtype=np.int64).astype(np.uint32).view(f32)


@functools.lru_cache(maxsize=None)
def arguments():
    zero = np.arange(0, ULPS + 1, dtype=np.uint32)                    # +0 and the 4096 values above it; with the sign bit, those below -0
    near = [zero.view(f32), (zero | np.uint32(0x80000000)).view(f32)] + [around(v) for v in (0.5, -0.5, 1.0, -1.0)]
    special = np.array([0.5, -0.5, 1.0, -1.0, 0.0, -0.0, 1.0000001, np.nan, np.inf, -np.inf], f32)
    n = np.random.default_rng(20261020).integers(0, 1 << 32, N_WORDS, dtype=np.uint64).astype(np.uint32)
    v = (f32(0) + f32(1) * (n.astype(f32) / f32(4294967296.0))).astype(f32)          # unit_float
    x = (f32(2) * v - f32(1)).astype(f32)
    out = np.concatenate(near + [special, x]).astype(f32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected():
    """sqo_acosf(x, TRIG_CRD) of every argument: the oracle's own code, never sq_math.h."""
    import pyoracle as O
    f = O.lib().sqo_acosf
    out = np.array([f(float(v), O.TRIG_CRD) for v in arguments()], f32)
    out.setflags(write=False)
    return out


def assert_bit_equal(got, what):
    """Exact on bits; where the oracle's value is a NaN (beyond +-1, NaN), a NaN: x86 and gfx950 choose the sign and payload of the
    NaN an invalid operation returns differently (tests/bitcmp.py, nan_eq), and the spec defines none."""
    got = np.asarray(got, f32)
    want, x = expected(), arguments()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isnan(want).sum() == 2 * ULPS + 4                         # beyond 1 and -1; 1.0000001, NaN, +-inf: nothing else may hide behind NaN = NaN
    bad = np.flatnonzero(~nan_eq(got, want))
    assert len(bad) == 0, "%s: %d of %d differ from the oracle, first at x = %r (bits %08x): got %r, oracle %r" % (
        what, len(bad), len(x), float(x[bad[0]]), int(x.view(np.uint32)[bad[0]]), float(got[bad[0]]), float(want[bad[0]]))
