"""tests/rounds_model.py against hand cases that each of its wrong variants changes, the two consequences include/fasterhip_rounds.h
states (greedy colouring in index order; neighbours share only the last class) on random lattice fleets, and the chain that needs one
pass per vehicle.  No GPU: the device is compared with this model in tests/test_gpu_rounds.py."""
import numpy as np
import pytest

import rounds_model as rm
from faster_amd import abi


def _line(a, b, m):
    return np.linspace(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), m)


def _chain(n):
    """Vehicle i stands at x = i: with reach 1.5 it is a neighbour of i - 1 and i + 1 only."""
    return rm.fleet([[[float(i), 0.0, 0.0]] for i in range(n)])


def _triangle():
    return rm.fleet([[[0.0, 0.0, 0.0]], [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]]])


def _clump(n):
    """n vehicles within 0.64 of each other: all are neighbours at reach 1."""
    return rm.fleet([[[0.01 * i, 0.0, 0.0]] for i in range(n)])


def _case(name):
    """(par, vehicles, plans, the variants this case exposes)"""
    if name == "short_plan_in_a_long_ones_path":   # the long plan reaches the standing one at instant 7; the short plan ended at 1
        v, pl = rm.fleet([[[7.0, 0.0, 0.0], [7.0, 0.2, 0.0]], _line((0, 0.2, 0), (9, 0.2, 0), 10)])
        return rm.params(0.5, 4), v, pl, ("min_size", "vanish")
    if name == "exactly_reach":                    # (3, 4, 0): d2 = 25 = reach reach, in doubles
        v, pl = rm.fleet([[[0.0, 0.0, 0.0]], [[3.0, 4.0, 0.0]]])
        return rm.params(5.0, 4), v, pl, ("le",)
    if name == "only_instant_zero":
        v, pl = rm.fleet([_line((0, 0, 0), (8, 0, 0), 5), _line((0.1, 0, 0), (0.1, 40, 0), 5)])
        return rm.params(0.5, 4, stride=2), v, pl, ("from_stride",)
    if name == "a_pair":
        v, pl = rm.fleet([[[0.0, 0.0, 0.0]], [[0.1, 0.0, 0.0]]])
        return rm.params(0.5, 4), v, pl, ("any_index",)
    if name == "triangle_in_two_rounds":
        v, pl = _triangle()
        return rm.params(1.5, 2), v, pl, ("no_clip",)
    if name == "chain_of_three_one_pass":
        v, pl = _chain(3)
        return rm.params(1.5, 4, passes=1), v, pl, ("same_pass",)
    if name == "exactly_the_list":                 # the last of 65 has FH_ROUNDS_LIST lower neighbours: they fit
        v, pl = _clump(abi.FH_ROUNDS_LIST + 1)
        return rm.params(1.0, 64, passes=64), v, pl, ("overflow_ge",)
    raise KeyError(name)


CASES = ("short_plan_in_a_long_ones_path", "exactly_reach", "only_instant_zero", "a_pair", "triangle_in_two_rounds", "chain_of_three_one_pass",
         "exactly_the_list")


def test_hand_cases_by_hand():
    par, v, pl, _ = _case("short_plan_in_a_long_ones_path")
    r = rm.classes(par, v, pl, pl.shape[1])
    assert r["n_lower"].tolist() == [0, 1] and r["round_class"].tolist() == [0, 1] and r["decided_pass"].tolist() == [0, 1] and not r["flags"].any()
    par, v, pl, _ = _case("exactly_reach")
    assert rm.classes(par, v, pl, 1)["round_class"].tolist() == [0, 0]   # strict: not neighbours
    par, v, pl, _ = _case("only_instant_zero")
    assert rm.classes(par, v, pl, 5)["n_lower"].tolist() == [0, 1]
    par, v, pl, _ = _case("a_pair")
    assert rm.classes(par, v, pl, 1)["n_lower"].tolist() == [0, 1]
    par, v, pl, _ = _case("triangle_in_two_rounds")
    r = rm.classes(par, v, pl, 1)
    assert r["round_class"].tolist() == [0, 1, 1] and r["decided_pass"].tolist() == [0, 1, 2] and not r["flags"].any()
    par, v, pl, _ = _case("chain_of_three_one_pass")
    r = rm.classes(par, v, pl, 1)
    assert r["round_class"].tolist() == [0, 1, 3] and r["decided_pass"].tolist() == [0, 1, -1] and r["flags"].tolist() == [0, 0, abi.FH_ROUND_UNSETTLED]
    par, v, pl, _ = _case("exactly_the_list")
    r = rm.classes(par, v, pl, 1)
    assert r["n_lower"].tolist() == list(range(65)) and not r["flags"].any()
    assert r["round_class"].tolist() == list(range(64)) + [63] and r["decided_pass"].tolist() == list(range(65))


def test_every_wrong_variant_changes_its_hand_case_and_no_other_variant_is_unexposed():
    exposed = set()
    for name in CASES:
        par, v, pl, variants = _case(name)
        want = rm.classes(par, v, pl, pl.shape[1])
        for variant in rm.VARIANTS:
            got = rm.classes(par, v, pl, pl.shape[1], variant)
            if variant in variants:
                assert got.tobytes() != want.tobytes(), (name, variant)
                exposed.add(variant)
    assert exposed == set(rm.VARIANTS)


def test_overflow_goes_last_and_counts_exactly_and_the_one_above_treats_it_as_decided():
    for n in (66, 67):
        v, pl = _clump(n)
        r = rm.classes(rm.params(1.0, 3, passes=2), v, pl, 1)
        assert r["n_lower"].tolist() == list(range(n))
        over = r["flags"] == abi.FH_ROUND_OVERFLOW
        assert np.nonzero(over)[0].tolist() == list(range(65, n)) and (r["round_class"][over] == 2).all() and (r["decided_pass"][over] == 0).all()
    # a vehicle above an overflowed one, a neighbour of it alone: decided in pass 1 from the overflowed one's class
    ps = [[[0.01 * i, 0.0, 0.0]] for i in range(66)] + [[[0.65 + 0.995, 0.0, 0.0]]]   # (1.005 from vehicle 64)
    v, pl = rm.fleet(ps)
    r = rm.classes(rm.params(1.0, 3, passes=1), v, pl, 1)
    assert r["n_lower"][66] == 1 and r["flags"][65] == abi.FH_ROUND_OVERFLOW and r["round_class"][65] == 2
    assert (int(r["round_class"][66]), int(r["decided_pass"][66]), int(r["flags"][66])) == (0, 1, 0)


def test_bad_extents_and_positions_that_are_not_finite():
    v, pl = rm.fleet([[[0.0, 0.0, 0.0]], [[0.1, 0.0, 0.0]], [[0.2, 0.0, 0.0], [0.2, 0.0, 0.0]], [[0.3, 0.0, 0.0]], []], max_states=4)
    v["plan_head"][1] = 4   # bad: head + size > max_states
    pl["pos"][2, 1, 1] = np.nan
    r = rm.classes(rm.params(1.0, 4), v, pl, 4)
    assert r["flags"].tolist() == [0, abi.FH_ROUND_BAD_PLAN, abi.FH_ROUND_NOT_FINITE, 0, 0]
    assert r["n_lower"].tolist() == [0, 0, 1, 2, 0]   # the bad one and the empty one have no neighbours; instant 0 of vehicle 2 still counts
    assert r["round_class"].tolist() == [0, 0, 1, 2, 0]
    # count = 1 cuts the NaN off: the last state is readable only when an instant behind the plan can be tested
    r = rm.classes(rm.params(1.0, 4, count=1), v, pl, 4)
    assert r["flags"].tolist() == [0, abi.FH_ROUND_BAD_PLAN, 0, 0, 0]


def test_rounds_one_is_class_zero_everywhere():
    v, pl = _clump(70)
    for passes in (0, 3):
        r = rm.classes(rm.params(1.0, 1, passes=passes), v, pl, 1)
        assert not r["round_class"].any()


@pytest.mark.parametrize("seed", range(6))
def test_the_two_consequences_on_random_lattice_fleets(seed):
    """Positions on the integer lattice, reach 1.5: d2 is an integer, far from the roundings.  No flags, passes = n - 1."""
    rng = np.random.default_rng(seed)
    n, max_states = 40, 12
    ps = []
    for _ in range(n):
        size = int(rng.integers(1, max_states + 1))
        start = rng.integers(0, 7, size=3)
        steps = rng.integers(-1, 2, size=(size, 3))
        steps[0] = 0
        ps.append((start + np.cumsum(steps, axis=0)).astype(np.float64))
    v, pl = rm.fleet(ps, max_states=max_states)
    for rounds in (2, 3, 64):
        par = rm.params(1.5, rounds, passes=n - 1, stride=1 + seed % 2)
        adj, flags = rm.neighbours(par, v, pl, max_states)
        assert (adj == adj.T).all() and not adj.diagonal().any() and not flags.any()
        r = rm.classes(par, v, pl, max_states)
        assert not r["flags"].any()
        assert r["round_class"].tolist() == rm.greedy(adj, rounds).tolist()
        i, k = np.nonzero(adj)
        same = r["round_class"][i] == r["round_class"][k]
        assert (r["round_class"][i][same] == rounds - 1).all()
        if rounds == 64:
            assert not same.any()   # (no vertex of 40 needs colour 63)


@pytest.mark.parametrize("n", (2, 6, 9))
def test_a_chain_settles_in_exactly_n_minus_one_passes(n):
    v, pl = _chain(n)
    r = rm.classes(rm.params(1.5, 4, passes=n - 1), v, pl, 1)
    assert r["decided_pass"].tolist() == list(range(n)) and not r["flags"].any()
    assert r["round_class"].tolist() == [i % 2 for i in range(n)]
    for passes in range(n - 1):
        r = rm.classes(rm.params(1.5, 4, passes=passes), v, pl, 1)
        unsettled = (r["flags"] & abi.FH_ROUND_UNSETTLED) != 0
        assert np.nonzero(unsettled)[0].tolist() == list(range(passes + 1, n))
        assert (r["round_class"][unsettled] == 3).all() and (r["decided_pass"][unsettled] == -1).all()
        assert r["decided_pass"][:passes + 1].tolist() == list(range(passes + 1))


def test_gate():
    v, _ = _chain(5)
    v["stage"] = [abi.FH_FLEET_STAGE_CONFLICT, 4, abi.FH_FLEET_STAGE_CONFLICT, 0, abi.FH_FLEET_STAGE_CONFLICT]
    v["active"] = 9
    rec = rm.fixed_records(np.array([0, 1, 0, 1, 2]))
    begin = np.array([1, 1, 0, 7, 1], dtype=np.int32)
    for rnd, want in ((0, [1, 0, 0, 0, 0]), (1, [0, 1, 0, 1, 0]), (2, [0, 0, 0, 0, 1]), (3, [0] * 5), (abi.FH_ROUND_RETRY, [1, 0, 0, 0, 1]),
                      (abi.FH_ROUND_RESTORE, [1, 1, 0, 1, 1])):
        gv, act = rm.gate(rec, rnd, begin, v)
        assert act.tolist() == want and gv["active"].tolist() == want and act.dtype == np.int32
        gv["active"] = v["active"]
        assert gv.tobytes() == v.tobytes()   # nothing else of the records
