"""The numpy model of the separation of committed plans (tests/separation_model.py, the restatement of include/fasterhip_separation.h) on
hand cases whose answers are worked out by hand, and five wrong variants of the model, each of which changes the case that is named for
it.  tests/test_gpu_separation.py runs the same cases on the device.  Coordinates are multiples of 0.25 and r = 0.5, cap = 1: every
square and every sum below is exact."""
import numpy as np
import pytest

import separation_model as sm
from faster_amd import abi

INF = float("inf")
R, CAP = 0.5, 1.0
NEAR = abi.FH_SEP_NEAR


def line(n, x0=0.0, y=0.0, z=0.0, step=0.25):
    return [(x0 + step * j, y, z) for j in range(n)]


def rec(flags=0, n_tested=0, first=-1, first_other=-1, worst=-1, worst_other=-1, n_near=0, min_d2=INF):
    return dict(flags=flags, n_tested=n_tested, first=first, first_other=first_other, worst=worst, worst_other=worst_other, n_near=n_near,
                min_d2=min_d2)


def _bad_record_fleet():
    v, pl = sm.fleet([[(0, 0, 0)], [(0.25, 0, 0)], [(0, 0, 0)]])
    v["plan_head"][1] = -1          # bad: nothing of it is read, and it is not an other of anyone
    pl["pos"][1, 0] = (0.25, 0, 0)
    v["plan_head"][2], v["plan_size"][2] = 1, 1   # bad too: head + size > max_states = 1
    return v, pl


def hand_cases():
    """name -> (params, vehicles, plans, {vehicle: expected record})."""
    c = {}
    par = sm.params(R, CAP)
    # two vehicles on parallel lines 0.25 apart, in step: d2 = 0.0625 at every instant, in both records
    v, pl = sm.fleet([line(8), line(8, y=0.25)])
    c["parallel"] = (par, v, pl, {0: rec(NEAR, 8, 0, 1, 0, 1, 1, 0.0625), 1: rec(NEAR, 8, 0, 0, 0, 0, 1, 0.0625)})
    # vehicle 0 flies past vehicle 1, whose plan has ended at j = 1 and which stands at (1.5, 0.25, 0): at j = 6 vehicle 0 is at (1.5, 0, 0).
    # Record 1 tests j = 0, 1 only, where vehicle 0 is still 1.25 and more away: the pair's closest approach is in record 0 alone.
    v, pl = sm.fleet([line(8), [(1.5, 0.25, 0)] * 2])
    c["passing_one_that_ended"] = (par, v, pl, {0: rec(NEAR, 8, 5, 1, 6, 1, 1, 0.0625), 1: rec(0, 2)})
    # two others at the same distance at the same instant: the smaller number
    v, pl = sm.fleet([[(0, 0, 0)], [(0.5, 0.5, 0)], [(0.25, 0, 0)], [(-0.25, 0, 0)]])
    c["tie_between_two_k"] = (par, v, pl, {0: rec(NEAR, 1, 0, 2, 0, 2, 2, 0.0625)})
    # the same distance at two instants: the smaller instant (a standing other between two positions of the subject)
    v, pl = sm.fleet([[(0.75, 0, 0), (0, 0, 0), (0.5, 0, 0), (0, 0, 0)], [(0.25, 0, 0)]])
    c["tie_between_two_j"] = (par, v, pl, {0: rec(NEAR, 4, 1, 1, 1, 1, 1, 0.0625), 1: rec(0, 1, -1, -1, 0, 0, 0, 0.25)})
    # an other at exactly r: looked at, not near
    v, pl = sm.fleet([[(0, 0, 0)], [(0.5, 0, 0)]])
    c["exactly_r"] = (par, v, pl, {0: rec(0, 1, -1, -1, 0, 1, 0, 0.25), 1: rec(0, 1, -1, -1, 0, 0, 0, 0.25)})
    # an other at exactly cap: not looked at
    v, pl = sm.fleet([[(0, 0, 0)], [(0, 1.0, 0)]])
    c["exactly_cap"] = (par, v, pl, {0: rec(0, 1), 1: rec(0, 1)})
    # alone: no others, and never itself
    v, pl = sm.fleet([line(3)])
    c["alone"] = (par, v, pl, {0: rec(0, 3)})
    # bad records beside a good one: the flag alone, and invisible to the good one although their memory holds a position next to it
    v, pl = _bad_record_fleet()
    c["bad_record"] = (par, v, pl, {0: rec(0, 1), 1: rec(abi.FH_SEP_BAD_PLAN), 2: rec(abi.FH_SEP_BAD_PLAN)})
    # an empty plan is not bad, tests nothing and is nobody's other; a NaN of the subject is skipped and flagged, a NaN of the other
    # fails d2 < cap cap by itself; at j = 3 vehicle 0 has ended and stands at (0.25, 0, 0), 0.25 below vehicle 2
    v, pl = sm.fleet([[(0, 0, 0), (np.nan, 0, 0), (0.25, 0, 0)], [], [(np.inf, 0, 0), (0, 0.25, 0), (np.nan, 0, 0), (0.25, 0.25, 0)]])
    c["empty_and_not_finite"] = (par, v, pl, {0: rec(abi.FH_SEP_NOT_FINITE, 3), 1: rec(0, 0),
                                              2: rec(abi.FH_SEP_NOT_FINITE | NEAR, 4, 3, 0, 3, 0, 1, 0.0625)})
    return c


CASES = hand_cases()
# the case each wrong variant changes
CHANGED_BY = {"no_hover": "passing_one_that_ended", "le": "exactly_r", "larger_k_on_ties": "tie_between_two_k", "self_pair": "alone",
              "bad_as_other": "bad_record"}


def check(records, expected, name):
    for i, want in expected.items():
        for k, val in want.items():
            assert records[k][i] == val, (name, i, k, records[k][i], val)
        assert records["reserved"][i] == 0 and not records["reserved_d"][i].any()


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_case(name):
    par, v, pl, expected = CASES[name]
    check(sm.separation(par, v, pl, pl.shape[1]), expected, name)


def test_not_finite_of_the_subject_is_skipped_not_propagated():
    """Vehicle 0 of empty_and_not_finite: its j = 1 is NaN; its other (vehicle 2) is at (inf, 0, 0) at j = 0 and NaN at j = 2, so nothing
    is within cap at any instant although both are finite and 0.25 apart at DIFFERENT instants."""
    par, v, pl, _ = CASES["empty_and_not_finite"]
    got = sm.separation(par, v, pl, pl.shape[1])
    assert got["min_d2"][0] == INF and got["n_tested"][0] == 3


def test_exactly_cap_with_le_is_seen():
    par, v, pl, _ = CASES["exactly_cap"]
    assert sm.separation(par, v, pl, 1, variant="le")["min_d2"][0] == 1.0


@pytest.mark.parametrize("variant", sm.VARIANTS)
def test_each_wrong_variant_changes_its_named_case(variant):
    assert set(CHANGED_BY) == set(sm.VARIANTS) and len(sm.VARIANTS) >= 5
    par, v, pl, expected = CASES[CHANGED_BY[variant]]
    right = sm.separation(par, v, pl, pl.shape[1])
    wrong = sm.separation(par, v, pl, pl.shape[1], variant=variant)
    check(right, expected, variant)
    assert right.tobytes() != wrong.tobytes(), variant
    with pytest.raises(AssertionError):
        check(wrong, expected, variant)


def test_variants_in_detail():
    par, v, pl, _ = CASES["passing_one_that_ended"]
    assert sm.separation(par, v, pl, 8, variant="no_hover")["min_d2"][0] == INF          # the standing vehicle has vanished
    par, v, pl, _ = CASES["exactly_r"]
    assert sm.separation(par, v, pl, 1, variant="le")["flags"][0] == NEAR
    par, v, pl, _ = CASES["tie_between_two_k"]
    w = sm.separation(par, v, pl, 1, variant="larger_k_on_ties")[0]
    assert (w["worst_other"], w["first_other"]) == (3, 3)
    par, v, pl, _ = CASES["alone"]
    w = sm.separation(par, v, pl, 3, variant="self_pair")[0]
    assert w["min_d2"] == 0.0 and w["worst_other"] == 0 and w["n_near"] == 1
    par, v, pl, _ = CASES["bad_record"]
    w = sm.separation(par, v, pl, 1, variant="bad_as_other")[0]
    assert w["flags"] == NEAR and w["first_other"] == 1


def random_fleet(rng, n, max_states, box=4.0, sizes=None, step=0.05):
    """n plans of random length that drift through a box: a start, a direction, `step` per state."""
    sizes = rng.integers(1, max_states + 1, size=n) if sizes is None else np.asarray(sizes)
    plans = []
    for i in range(n):
        start = rng.uniform(0.0, box, size=3) * (1.0, 1.0, 0.25)
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        plans.append(start[None, :] + step * np.arange(int(sizes[i]))[:, None] * d[None, :])
    return sm.fleet(plans, max_states=max_states)


def pair_min(par, v, pl, i, k):
    """The smallest d2 below cap cap of the pair as record i sees it: the fleet reduced to the two."""
    two = np.array([i, k])
    return sm.separation(par, v[two], pl[two], pl.shape[1])["min_d2"][0]


def test_equal_lengths_give_both_records_the_same_minimum():
    rng = np.random.default_rng(5)
    v, pl = random_fleet(rng, 12, 40, box=1.5, sizes=[40] * 12)
    par = sm.params(0.3, 0.9)
    seen = 0
    for i in range(12):
        for k in range(i + 1, 12):
            a, b = pair_min(par, v, pl, i, k), pair_min(par, v, pl, k, i)
            assert a == b
            seen += a < INF
    assert seen >= 5


def test_unequal_lengths_the_closest_approach_is_the_smaller_of_the_two_records():
    """Brute force over every instant either of the two tests, the other standing at its last state when it has ended."""
    rng = np.random.default_rng(6)
    v, pl = random_fleet(rng, 12, 40, box=1.5)
    par = sm.params(0.3, 0.9)
    differ = 0
    for i in range(12):
        for k in range(i + 1, 12):
            si, sk = int(v["plan_size"][i]), int(v["plan_size"][k])
            j = np.arange(max(si, sk))
            d = pl["pos"][k, np.minimum(j, sk - 1)] - pl["pos"][i, np.minimum(j, si - 1)]
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            truth = d2.min() if d2.min() < 0.9 * 0.9 else INF
            a, b = pair_min(par, v, pl, i, k), pair_min(par, v, pl, k, i)
            assert min(a, b) == truth
            differ += a != b
    assert differ >= 3


def test_abi_helpers():
    d = abi.default_separation_params(0.84)
    assert (d["r"], d["cap"], d["stride"], d["count"]) == (0.84, 1.68, 1, 0) and not d["reserved"].any()
    par, v, pl, _ = CASES["parallel"]
    assert np.array_equal(abi.separation_distances(sm.separation(par, v, pl, 8)), [0.25, 0.25])
