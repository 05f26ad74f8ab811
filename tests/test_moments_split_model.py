"""The arithmetic of the half-wave split of SolverWF::moments() (faster_amd/csrc/fh_solve.hip.hpp), restated in numpy: no device needed.

moments() carries the contribution of the jerks x_s to the state at the start of segment tt in three sums over the segments s < tt,
S_k = sum m^k x_s with m = tt - 1 - s.  In the N = 6 and N = 10 buckets the rows (tt >= 1, axis) sit in half a wavefront: lane j adds
the segments s < NSEG / 2, lane j + 32 the segments s >= NSEG / 2, each in ascending s, and one addition joins the two partial sums
of each moment.  Two claims are pinned here:

  * the mask "segment s lies before tt" as a compare-and-select gives the bits of the former clamp-and-multiply
    (x_s * min(max(m + 1, 0), 1)), signs of zeros included: the sums start at +0 and a sum that starts at +0 is never -0;
  * the split order of the additions changes the states by rounding only: 1e-13 relative.  An N-term sum in any order is within
    (N - 1) eps of the exact sum relative to the sum of the absolute terms, so two orders differ by at most 2 * 9 * 1.1e-16 = 2e-15 of
    that scale: the bound is checked against the absolute terms of each state (its condition), 50 times above what can occur.
"""
import numpy as np
import pytest

J_MAX = 50.0
H = 0.37           # a step that is not a power of two: the h^2 and h^3 weights round


def fma(a, b, c):
    """a * b + c with one rounding for |a| <= 16 an integer: the product is exact in the 64-bit mantissa of a long double."""
    return (np.longdouble(a) * np.longdouble(b) + np.longdouble(c)).astype(np.float64)


def mask_multiply(x, dm):
    return x * np.minimum(np.maximum(dm + 1.0, 0.0), 1.0)


def mask_select(x, s, tt):
    return np.where(s < tt, x, 0.0)


def partial_sums(x, tt, segs, mask):
    """The loop of moments() over the segments `segs` (ascending) of the jerks x [B, N], for the state at the start of segment tt."""
    B = len(x)
    s0, s1, s2 = np.zeros(B), np.zeros(B), np.zeros(B)
    for s in segs:
        dm = float(tt - 1 - s)
        xv = mask_multiply(x[:, s], dm) if mask == "multiply" else mask_select(x[:, s], s, tt)
        t1 = dm * xv
        s0 = s0 + xv
        s1 = s1 + t1
        s2 = fma(dm, t1, s2)
    return s0, s1, s2


def states(s0, s1, s2, h=H):
    h2 = h * h
    h3 = h2 * h
    return h3 * (s0 * (1.0 / 6.0) + 0.5 * s1 + 0.5 * s2), h2 * (0.5 * s0 + s1), h * s0


def jerks(n_seg, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-J_MAX, J_MAX, size=(10000, n_seg))
    x[::7, rng.integers(0, n_seg)] = 0.0          # exact zeros and negative zeros among the jerks
    x[3::11, rng.integers(0, n_seg)] = -0.0
    return x


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("n_seg", [6, 10])
def test_select_mask_gives_the_bits_of_the_multiply_mask(n_seg):
    x = jerks(n_seg, seed=n_seg)
    for tt in range(0, n_seg + 1):
        a = partial_sums(x, tt, range(n_seg), "multiply")
        b = partial_sums(x, tt, range(n_seg), "select")
        for u, v in zip(a, b):
            assert np.array_equal(bits(u), bits(v)), tt
        for u, v in zip(states(*a), states(*b)):
            assert np.array_equal(bits(u), bits(v)), tt


@pytest.mark.parametrize("n_seg", [6, 10])
def test_split_sum_agrees_with_the_sequential_sum(n_seg):
    x = jerks(n_seg, seed=100 + n_seg)
    half = n_seg // 2
    worst = 0.0
    differing = 0
    for tt in range(1, n_seg + 1):
        seq = partial_sums(x, tt, range(n_seg), "multiply")                  # the unsplit loop, as the N = 15 / 16 buckets keep it
        lo = partial_sums(x, tt, range(half), "select")                      # lane j
        hi = partial_sums(x, tt, range(half, n_seg), "select")               # lane j + 32
        spl = tuple(a + b for a, b in zip(lo, hi))                           # halves_sum: commutative, the same value in both halves
        m = np.array([tt - 1 - s for s in range(n_seg)], dtype=np.float64)
        live = (m >= 0).astype(np.float64)
        ax = np.abs(x) * live
        # the absolute terms of each state: |c(m)| |x_s| with cP = h^3 (1/6 + m/2 + m^2/2), cV = h^2 (1/2 + m), cA = h
        scale = (H**3 * (ax @ (1.0 / 6.0 + 0.5 * m + 0.5 * m * m)), H**2 * (ax @ (0.5 + m)), H * ax.sum(axis=1))
        for a, b, sc in zip(states(*seq), states(*spl), scale):
            err = np.abs(a - b)
            differing += int((err > 0).sum())
            ok = sc > 0
            assert (err[~ok] == 0).all()
            worst = max(worst, float((err[ok] / sc[ok]).max()))
            assert (err <= 1e-13 * sc).all(), (tt, float((err[ok] / sc[ok]).max()))
    print("N = %d: worst difference %.2e of the absolute terms; %d of %d states differ in their last bits" % (
        n_seg, worst, differing, 3 * n_seg * len(x)))
    assert differing > 0       # the two orders ARE different sums (the test would pass vacuously on equal code)
    assert worst < 1e-14       # ... and the reasoning above (2e-15) holds with room
