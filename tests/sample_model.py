"""The sample clock of resetX() + fillX() (solverGurobi.cpp:382-388, :122-168) and what consumes its samples — appendToPlan
(faster.cpp:606-648) and getNextGoal (faster.cpp:699-723) — restated in plain Python, for the tests that compare the device with a
reference of higher precision.  Not a test file.

The clock is the loop itself in Python floats (IEEE doubles: the same bits as the reference's `t = t + DC`).  The state of a sample is
the cubic of its segment and its derivatives at tau = t - interval dt, evaluated EXACTLY in fractions.Fraction from the double inputs;
next to it goes a bound on what a double evaluation may differ by, derived from the number formats (never measured).

The trajectories the tests pose are synthetic and DISCONTINUOUS on purpose (synthetic_result): segment s carries 1000 s, 100 s, 10 s in its
constant, linear and quadratic rows and a cubic row of its own per axis, so a sample evaluated in the wrong segment is wrong in every
field by many orders of magnitude more than any bound — a solved trajectory is C2 and would show it in the jerk alone."""
import collections
import math
from fractions import Fraction

import numpy as np

from faster_amd import abi

U = Fraction(1, 2 ** 53)   # unit roundoff of a double


def clock(n, DC, dt, N):
    """fillX's clock (:131-135) for samples 0 .. n - 1: (t[i], interval[i]) as lists of Python floats / ints."""
    t, interval, ts, ivs = 0.0, 0, [], []
    for _ in range(n):
        t = t + DC
        if t > dt * (interval + 1):
            interval = min(interval + 1, N - 1)
        ts.append(t)
        ivs.append(interval)
    return ts, ivs


def closed_form_intervals(n, DC, dt, N):
    """What a clock WITHOUT the running sum would say: t = (i + 1) DC, interval = ceil(t / dt) - 1 (clamped).  Only used to count the
    samples such a clock would put into another segment: the cases the tests pose must have some."""
    return [min(max(math.ceil(((i + 1) * DC) / dt) - 1, 0), N - 1) for i in range(n)]


def count(N, dt, DC):
    """resetX's size (:384-385), in this operation order."""
    return max(2, int(N * dt / DC))


def usable(problem, result):
    return bool(result["solved"]) and 1 <= int(problem["n_seg"]) <= abi.FH_MAX_SEG


def _components(c, tau):
    """The terms of pos / vel / accel of one axis at tau (Fractions): [[terms of pos], [terms of vel], [terms of accel]]; c = (a, b, c, d) of
    a tau^3 + b tau^2 + c tau + d."""
    a, b, cc, d = c
    return [[a * tau ** 3, b * tau ** 2, cc * tau, d], [3 * a * tau ** 2, 2 * b * tau, cc], [6 * a * tau, 2 * b]]


def states(problem, result):
    """(ref, bound, intervals): ref[i] the exact state of sample i rounded once (abi.state_dtype, count(N, dt, DC) of them; none for an
    unsolved result or a bad n_seg), bound[i] ([12] doubles in the order pos, vel, accel, jerk) such that a correct double evaluation g
    satisfies |g - ref| <= bound in double arithmetic, intervals[i] the segment of sample i.

    bound = 8 u sum |term| + 2 u max(|t|, |interval dt|) |d/dtau of the component| (+ the rounding of ref itself), u = 2^-53: the first
    part covers the roundings of a cubic evaluated with or without fused multiply-adds (at most six roundings on any term), the second
    the one or two roundings of tau = t - interval dt.  The jerk is 6 c: one multiplication, nothing to contract — its bound is zero, its
    bits are the reference's.  Sample size - 1 has vel = accel = jerk = 0 (:165-167)."""
    if not usable(problem, result):
        return np.zeros(0, dtype=abi.state_dtype), np.zeros((0, 12)), []
    N, dt, DC = int(problem["n_seg"]), float(result["dt"]), float(problem["dc"])
    size = count(N, dt, DC)
    ts, ivs = clock(size, DC, dt, N)
    ref = np.zeros(size, dtype=abi.state_dtype)
    bound = np.zeros((size, 12))
    coef = [[[Fraction(float(result["coeff"][s][3 * r + a])) for r in range(4)] for a in range(3)] for s in range(N)]
    fdt = Fraction(dt)
    for i in range(size):
        exact, bnd = state_in_segment(coef[ivs[i]], Fraction(ts[i]), ivs[i], fdt)
        for a in range(3):
            for f, name in enumerate(("pos", "vel", "accel")):
                zero = f > 0 and i == size - 1
                ref[name][i, a], bound[i, 3 * f + a] = (0.0, 0.0) if zero else _round_with_bound(exact[a][f], bnd[a][f])
            ref["jerk"][i, a] = 0.0 if i == size - 1 else 6.0 * float(result["coeff"][ivs[i]][a])
    return ref, bound, ivs


def state_in_segment(coef_s, t, interval, dt):
    """Exact pos / vel / accel per axis ([3][3] Fractions) of the segment with coefficients coef_s ([axis][a, b, c, d], Fractions) at the
    clock value t when the clock says `interval`, and the bound of each (Fractions, without the rounding of the reference)."""
    tau = t - interval * dt
    span = max(abs(t), abs(interval * dt))
    exact, bnd = [], []
    for a in range(3):
        terms = _components(coef_s[a], tau)
        vals = [sum(tt) for tt in terms]
        slope = [vals[1], vals[2], 6 * coef_s[a][0]]   # d/dtau of pos, vel, accel
        exact.append(vals)
        bnd.append([8 * U * sum(abs(x) for x in terms[f]) + 2 * U * span * abs(slope[f]) for f in range(3)])
    return exact, bnd


def _round_with_bound(exact, bnd):
    """(r, b): r = the double nearest to `exact`; b a double with |g - exact| <= bnd  =>  fl(|g - r|) <= b for any double g (rounding to
    nearest is monotone, so the comparison may be made in doubles)."""
    r = float(exact)
    b = float(bnd + abs(exact - Fraction(r)))
    return r, float(np.nextafter(b, np.inf))


def as12(s):
    return np.concatenate([s["pos"], s["vel"], s["accel"], s["jerk"]], axis=-1)


def check_states(got, ref, bound, where=""):
    """got[i] against ref[i] for the same samples: the jerk bit for bit (that is the interval, exactly: every segment and axis has a
    cubic coefficient of its own), pos / vel / accel within the derived bound."""
    assert len(got) == len(ref) == len(bound), (where, len(got), len(ref))
    if not len(got):
        return
    assert got["jerk"].tobytes() == ref["jerk"].tobytes(), (where, "jerk bits (the segment of a sample)",
                                                              np.nonzero((got["jerk"] != ref["jerk"]).any(axis=1))[0][:8])
    err = np.abs(as12(got) - as12(ref))
    bad = np.nonzero(~(err <= bound))   # (a NaN fails)
    assert not len(bad[0]), (where, "sample %d component %d: |%r - %r| = %.3e > %.3e" % (
        bad[0][0], bad[1][0], as12(got)[bad[0][0], bad[1][0]], as12(ref)[bad[0][0], bad[1][0]], err[bad[0][0], bad[1][0]],
        bound[bad[0][0], bad[1][0]]))


def next_goal(plan, ticks):
    """getNextGoal `ticks` times on a deque (faster.cpp:699-723, without yaw): (the goal of the last call or None for an empty plan, the
    number of states popped).  `next_goal = plan_.front(); if (plan_.size() > 1) plan_.pop_front()`."""
    dq = collections.deque(plan)
    goal, popped = None, 0
    if not dq:
        return None, 0
    for _ in range(ticks):
        goal = dq[0]
        if len(dq) == 1:
            break            # (every further call returns the same state and pops nothing)
        dq.popleft()
        popped += 1
    return goal, popped


def append_to_plan(kept_prefix, whole, k_safe, safe):
    """appendToPlan for a given k_safe (:617-640): what is kept of the old plan, whole samples 0 .. k_safe, then every safe sample."""
    return np.concatenate([kept_prefix, whole[:k_safe + 1], safe])


# ---- synthetic records and the shared case list ----
def synthetic_result(N, dt, seed, solved=1):
    """An fh_result written by hand: `solved`, the chosen dt, and for segment s a cubic row of its own per axis, the quadratic row 10 s +
    noise, the linear row 100 s + noise, the constant row 1000 s + noise (noise in [-1, 1): full mantissas, so roundings are real)."""
    rng = np.random.default_rng(seed)
    rs = np.zeros((), dtype=abi.result_dtype)
    rs["solved"], rs["dt"], rs["factor"] = solved, dt, 1.0 + (seed % 7)
    for s in range(N):
        for a in range(3):
            rs["coeff"][s, 0 + a] = (3 * s + a + 1) * 1.1 + 0.25 * rng.uniform(-1, 1)
            rs["coeff"][s, 3 + a] = 10.0 * s + rng.uniform(-1, 1)
            rs["coeff"][s, 6 + a] = 100.0 * s + rng.uniform(-1, 1)
            rs["coeff"][s, 9 + a] = 1000.0 * s + rng.uniform(-1, 1)
    return rs


def synthetic_problem(N, DC):
    pr = np.zeros((), dtype=abi.problem_dtype)
    pr["n_seg"], pr["dc"], pr["a_max"], pr["v_max"], pr["j_max"] = N, DC, 5.0, 5.0, 8.0
    return pr


Case = collections.namedtuple("Case", "name DC dt N misplaced")

# (DC, dt / DC, N, the samples a closed-form clock puts into another segment): the table of the sample clock's knot cases
_TABLE = [(0.01, 24.494897, 10, 0), (0.01, 7, 10, 7), (0.01, 50, 10, 4), (0.01, 100, 6, 2), (0.02, 2.5, 16, 4), (0.1, 3, 15, 7),
          (0.005, 73, 10, 3), (0.05, 20, 10, 2), (0.0078125, 24, 10, 0)]


def cases():
    """The cases of the CPU and the GPU tests.  `misplaced`: how many samples t = (i + 1) DC, interval = ceil(t / dt) - 1 puts into another
    segment than the loop does (tests/test_sample_model.py holds the model to these numbers: a case that stops discriminating fails there)."""
    out = [Case("table DC=%g dt=%g DC N=%d" % (DC, m, N), DC, DC * m, N, mis) for DC, m, N, mis in _TABLE]
    # short hops: dt = factor max(dt_init, 2 DC) = 2 DC f, an exact multiple of DC
    out += [Case("short hop f=%g" % f, 0.01, 2 * 0.01 * f, 6, mis) for f, mis in ((1, 1), (1.5, 1), (2, 1), (3.5, 3))]
    out += [Case("N=%d" % N, 0.01, 0.01 * 7, N, mis) for N, mis in ((1, 0), (2, 0), (6, 3), (15, 12), (16, 13))]   # (N = 10: a table row)
    out.append(Case("clamp: dt = 0.4 DC", 0.01, 0.4 * 0.01, 3, 1))          # size 2 through the clamp, one interval per step at most
    out.append(Case("long: 75 tiles", 0.01, 3.0, 16, 9))                      # 4800 samples
    return out


def sized(target):
    """(DC, dt, N) whose trajectory has exactly `target` samples, with knots on samples (tests place ends of plans on tile edges)."""
    DC, dt, N = {2: (0.01, 0.004, 3), 64: (0.0078125, 0.0078125 * 8, 8), 65: (0.01, 0.05, 13), 128: (0.0078125, 0.0078125 * 8, 16),
                 129: (0.01, 0.43, 3), 200: (0.05, 1.0, 10)}[target]
    assert count(N, dt, DC) == target, (target, count(N, dt, DC))
    return DC, dt, N


def case_records(case, seed):
    """The four records of a case: the trajectory itself, an unsolved result, n_seg = 0 and n_seg = 17 (problems, results)."""
    pr = np.zeros(4, dtype=abi.problem_dtype)
    rs = np.zeros(4, dtype=abi.result_dtype)
    for j in range(4):
        pr[j] = synthetic_problem(case.N, case.DC)
        rs[j] = synthetic_result(case.N, case.dt, seed + j)
    rs["solved"][1] = 0
    pr["n_seg"][2] = 0
    pr["n_seg"][3] = abi.FH_MAX_SEG + 1
    return pr, rs
