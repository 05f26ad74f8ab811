"""The model the GPU tests of the sample clock compare against (tests/sample_model.py), checked on the CPU before anything goes to a GPU:
(a) against the oracle's C restatement of resetX + fillX (orc_sample), (b) its clock against fh::clock_loop / fh::clock_at as g++ compiles
them, (c) the condition that makes the GPU tests worth running — the cases contain samples that a clock without the running sum
(t = (i + 1) DC, interval = ceil(t / dt) - 1) puts into another segment, and at those samples the neighbouring segment's state is far
outside every bound."""
import os
import struct
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_model as sm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sm.cases()


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


@pytest.mark.parametrize("ci", range(len(CASES)), ids=[c.name for c in CASES])
def test_model_equals_the_oracle_sampler(oracle, ci):
    """(a) counts exact, the jerk of every sample bit for bit (the interval), pos / vel / accel within the model's own bound; the unsolved
    record gives no samples.  Also with a capacity below the count: the zeroed tail belongs to sample size - 1 only."""
    case = CASES[ci]
    pr, rs = sm.case_records(case, 100 * ci)
    ref, bound, ivs = sm.states(pr[0], rs[0])
    size = sm.count(case.N, case.dt, case.DC)
    assert len(ref) == size <= 8192
    got = oracle.sample(pr[0], rs[0])
    sm.check_states(got, ref, bound, case.name)
    assert ivs[-1] <= case.N - 1 and ivs[0] >= 0 and all(b - a in (0, 1) for a, b in zip(ivs, ivs[1:]))   # one interval per step at most
    assert not ref["vel"][-1].any() and not ref["accel"][-1].any() and not ref["jerk"][-1].any()
    assert ref["jerk"][:-1].all()   # (only the last sample has a zero jerk: every cubic coefficient is non-zero)
    cut = oracle.sample(pr[0], rs[0], max_samples=size - 1)
    sm.check_states(cut, ref[:size - 1], bound[:size - 1], case.name + " (truncated)")
    assert len(oracle.sample(pr[1], rs[1])) == 0 and len(sm.states(pr[1], rs[1])[0]) == 0
    for j in (2, 3):   # n_seg = 0 / 17: the library's entry points refuse them (count 0); the model has no samples for them
        assert len(sm.states(pr[j], rs[j])[0]) == 0


def test_model_clock_equals_clock_loop_and_clock_at(tmp_path):
    """(b) every sample of every case: t bit for bit and the interval, for the loop and for the short cut, without and with contraction
    into fused multiply-adds."""
    src = os.path.join(ROOT, "tests", "cpp", "test_clock_cases.cpp")
    lines, want = [], []
    for case in CASES + [sm.Case("sized %d" % n, *sm.sized(n), None) for n in (2, 64, 65, 128, 129, 200)]:
        n = sm.count(case.N, case.dt, case.DC)
        lines.append("%x %x %d %d" % (bits(case.DC), bits(case.dt), case.N, n))
        ts, ivs = sm.clock(n, case.DC, case.dt, case.N)
        want += ["%x %d %x %d" % (bits(t), iv, bits(t), iv) for t, iv in zip(ts, ivs)]
    for flags in (["-ffp-contract=off"], ["-ffp-contract=fast", "-mfma"]):
        exe = str(tmp_path / "test_clock_cases")
        subprocess.check_call(["g++", "-O2", "-std=c++14"] + flags + [src, "-o", exe])
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        got = r.stdout.split("\n")[:-1]
        assert len(got) == len(want)
        bad = [i for i in range(len(want)) if got[i] != want[i]]
        assert not bad, (flags, bad[:5], got[bad[0]], want[bad[0]])


def test_cases_tell_the_running_sum_from_a_closed_form():
    """(c) per case, the number of samples a closed-form clock misplaces is the recorded one (the table of the knot cases: at least 2 in
    every knot row, 0 in the controls); at each such sample the state evaluated in the closed form's segment is more than 10^6 bounds
    away from the model in pos, vel and accel of every axis, and its jerk has other bits."""
    controls = 0
    for ci, case in enumerate(CASES):
        n = sm.count(case.N, case.dt, case.DC)
        _, ivs = sm.clock(n, case.DC, case.dt, case.N)
        other = sm.closed_form_intervals(n, case.DC, case.dt, case.N)
        differ = [i for i in range(n) if ivs[i] != other[i]]
        assert len(differ) == case.misplaced, (case.name, len(differ), case.misplaced)
        controls += int(not differ)
        if case.name.startswith("table") and case.misplaced:
            assert len(differ) >= 2, case.name
        pr, rs = sm.case_records(case, 100 * ci)
        ts, _ = sm.clock(n, case.DC, case.dt, case.N)
        coef = [[[Fraction(float(rs[0]["coeff"][s][3 * r + a])) for r in range(4)] for a in range(3)] for s in range(case.N)]
        for i in differ:
            assert abs(other[i] - ivs[i]) == 1, (case.name, i)
            good, bnd = sm.state_in_segment(coef[ivs[i]], Fraction(ts[i]), ivs[i], Fraction(case.dt))
            wrong, _ = sm.state_in_segment(coef[other[i]], Fraction(ts[i]), other[i], Fraction(case.dt))
            for a in range(3):
                for f in range(3):
                    assert abs(wrong[a][f] - good[a][f]) > 10 ** 6 * bnd[a][f] > 0, (case.name, i, a, f)
                assert rs[0]["coeff"][other[i]][a] != rs[0]["coeff"][ivs[i]][a]
    assert controls >= 1
    assert sum(c.misplaced for c in CASES) >= 50


def test_sized_trajectories_and_the_consumer_models():
    """The trajectories the GPU tests use to put plan ends on tile edges have the sample counts they are named after; the deque model of
    getNextGoal and the concatenation of appendToPlan on cases worked by hand."""
    for n in (2, 64, 65, 128, 129, 200):
        DC, dt, N = sm.sized(n)
        assert sm.count(N, dt, DC) == n
    plan = list(range(10, 15))
    assert sm.next_goal(plan, 1) == (10, 1) and sm.next_goal(plan, 2) == (11, 2)
    assert sm.next_goal(plan, 4) == (13, 4)        # four calls: 10, 11, 12, 13 go out; 14 is left
    assert sm.next_goal(plan, 5) == (14, 4)        # the fifth call returns the last state and keeps it
    assert sm.next_goal(plan, 2 ** 31 - 1) == (14, 4)
    assert sm.next_goal([7], 3) == (7, 0) and sm.next_goal([], 3) == (None, 0)
    a = np.arange(20)
    assert sm.append_to_plan(a[3:5], a[10:], 2, a[:2]).tolist() == [3, 4, 10, 11, 12, 0, 1]
