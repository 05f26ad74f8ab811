"""The Python model of include/fasterhip_spread.h (tests/spread_model.py) on its own: every named case has the property it is named
for, the model is reach_model's when every vehicle is a group of its own, the two consequences the header states hold on random small
fleets, and every deliberately wrong variant is told from the model by at least one named case — so kernels that made one of those
mistakes would not pass tests/test_gpu_spread.py, which compares them with this model in every byte."""
import numpy as np
import pytest

from faster_amd import abi

import reach_model as rm
import spread_model as sm

WANTED, FOUND = abi.FH_FRONTIER_WANTED, abi.FH_FRONTIER_FOUND
OVERFLOW, UNSETTLED, CLAIMED = abi.FH_SPREAD_OVERFLOW, abi.FH_SPREAD_UNSETTLED, abi.FH_SPREAD_CLAIMED
REACH_FIELDS = ("flags", "view", "cell", "hops", "candidates", "reachable", "reached", "levels", "d2")


def goal_cell(case, cell):
    return np.array(rm.centre(cell, case["grid"][1], case["grid"][0]))


def test_every_named_case_has_the_property_it_is_named_for():
    g, m, r = sm.expected("pair_same_voxel")
    alone = rm.model(dict(sm.case("pair_same_voxel"), par=sm.reach_par_of(sm.case("pair_same_voxel")["par"])))
    assert alone[2]["cell"][0] == alone[2]["cell"][1] == r["cell"][0] and r["cell"][1] != r["cell"][0]   # alone both take one voxel; the second yields
    assert m.tolist() == [1, 1] and r["decided_pass"].tolist() == [1, 2] and r["lower"].tolist() == [0, 1] and r["claims"].tolist() == [0, 1]
    assert sm.d2_of(g[0], g[1]) >= 1.0 and r["claimed"][1] > 0 and r["reachable"][1] == r["candidates"][1] - r["claimed"][1]
    g, m, r = sm.expected("pair_other_groups")
    assert r["cell"][0] == r["cell"][1] and r["decided_pass"].tolist() == [1, 1] and r["group"].tolist() == [0, 1] and not r["lower"].any()
    g, m, r = sm.expected("chain_passes_3")
    assert r["decided_pass"].tolist() == [1, 2, 3] and r["lower"].tolist() == [0, 1, 1] and m.tolist() == [1, 1, 1]
    g2, m2, r2 = sm.expected("chain_passes_2")
    assert r2["decided_pass"].tolist() == [1, 2, -1] and r2["flags"][2] == WANTED | UNSETTLED and m2.tolist() == [1, 1, 0]
    assert r2[:2].tobytes() == r[:2].tobytes() and g2[2].tobytes() == sm.case("chain_passes_2")["vehicles"]["g_term"][2].tobytes()
    # a traveling peer holds what the arrived vehicle would take: a standing claim.  Not from a non-peer, a GOAL_REACHED one, a NaN
    g, m, r = sm.expected("traveling_peer")
    free = sm.expected("traveling_non_peer")[2]
    c = sm.case("traveling_peer")
    assert np.array_equal(goal_cell(c, (4, 2, 0)), c["vehicles"]["g_term"][1]) and free["cell"][0] == rm.cell_index((4, 2, 0), c["grid"][2])
    assert r["claims"][0] == 1 and r["lower"][0] == 0 and r["cell"][0] != free["cell"][0] and r["claimed"][0] > 0 and r["flags"][1] == 0
    for name in ("traveling_non_peer", "reached_not_wanted", "nan_g_term"):
        _, _, q = sm.expected(name)
        assert q["claims"][0] == 0 and q["claimed"][0] == 0 and q["cell"][0] == free["cell"][0] and q["decided_pass"].tolist() == [1, 0], name
    assert sm.expected("nan_g_term")[2]["flags"][1] == abi.FH_FRONTIER_BAD_POS
    g, m, r = sm.expected("finds_nothing")
    assert m.tolist() == [0, 1] and r["flags"].tolist() == [WANTED, WANTED | FOUND] and r["lower"][1] == 1 and r["claims"][1] == 0 and r["claimed"][1] == 0
    assert r["decided_pass"].tolist() == [1, 2]
    assert sm.expected("outside_reach")[2]["lower"].tolist() == [0, 0] and sm.expected("inside_reach")[2]["lower"].tolist() == [0, 1]
    c = sm.case("outside_reach")
    assert sm.d2_of(c["vehicles"]["state"]["pos"][1], c["vehicles"]["state"]["pos"][0]) == 49.0   # exactly reach^2
    g, m, r = sm.expected("exactly_r_spread")
    assert sm.d2_of(g[0], g[1]) == 1.0 and r["hops"][1] == 2   # a candidate at exactly r_spread is not claimed, and is the choice
    g, m, r = sm.expected("all_claimed")
    assert r["flags"][1] == WANTED | CLAIMED and m.tolist() == [1, 0] and r["claimed"][1] == r["candidates"][1] == 5 and r["reachable"][1] == 0
    _, m, r = sm.expected("claims_32")
    assert r["claims"][0] == 32 and r["flags"][0] == WANTED | FOUND and r["decided_pass"][0] == 1
    _, m, r = sm.expected("claims_33")
    assert r["claims"][0] == 33 and r["lower"][0] == 0 and r["flags"][0] == WANTED | OVERFLOW and r["decided_pass"][0] == 0 and m[0] == 0
    for name, lo, hi in (("fleet_63", 0, 62), ("fleet_64", 0, 63), ("fleet_65", 63, 64), ("fleet_65_at_64", 0, 64), ("fleet_129", 0, 128),
                         ("fleet_129_at_64", 64, 128)):
        _, m, r = sm.expected(name)
        assert np.nonzero(m)[0].tolist() == [lo, hi] and r["lower"][hi] == 1 and r["decided_pass"][hi] == 2 and r["cell"][hi] != r["cell"][lo], name
    _, m, r = sm.expected("standing_at_128")
    assert r["claims"][0] == 1 and r["claimed"][0] > 0 and np.nonzero(m)[0].tolist() == [0]
    for name in ("labels", "labels_negative", "labels_large"):
        _, m, r = sm.expected(name)
        assert r["decided_pass"].tolist() == [1, 1, 2, 2] and r["cell"][0] == r["cell"][1] and r["cell"][2] == r["cell"][3] != r["cell"][0], name
        assert r["group"].tolist() == sm.case(name)["group"].tolist()
    _, m, r = sm.expected("shared_and_invalid")
    assert r["flags"][2] == WANTED | abi.FH_FRONTIER_NO_VIEW and r["group"][2] == 0 and r["lower"].tolist() == [0, 1, 0, 2] and r["decided_pass"].tolist() == [1, 2, 0, 3]
    _, m, r = sm.expected("one_vehicle")
    assert m.tolist() == [1] and r["decided_pass"].tolist() == [1]
    _, m, r = sm.expected("overflowed_lower_peer")
    assert r["flags"][0] == WANTED | OVERFLOW and r["lower"][34] == 1 and r["claims"][34] == 0 and r["claimed"][34] == 0 and r["decided_pass"][34] == 1


@pytest.mark.parametrize("name", rm.ALL_CASES)
def test_without_peers_the_model_is_reach_models(name):
    case = sm.own_groups(rm.case(name))
    want = rm.model(case)
    for passes in (1, 8):
        got = sm.model(case, par=sm.spread_par_of(case["par"], r_spread=1.0, passes=passes))
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), name
        for k in REACH_FIELDS:
            assert got[2][k].tobytes() == want[2][k].tobytes(), (name, k)
        searched = (want[2]["flags"] & ~(FOUND | abi.FH_REACH_CUT)) == WANTED
        assert np.array_equal(got[2]["decided_pass"], searched.astype(np.int32)) and not got[2]["lower"].any() and not got[2]["claims"].any()


def random_fleet(seed):
    """A floor of 30 x 12 voxels with a few walls, 10 vehicles in 3 views, labels that join two of the views; some arrived, some
    traveling to goals on the floor."""
    rng = np.random.default_rng(seed)
    nx, ny, n = 30, 12, 10
    view = np.zeros((2, ny, nx), dtype=np.uint8)
    view[1] = rng.random((ny, nx)) < 0.5
    occ = np.zeros((2, ny, nx), dtype=np.uint8)
    occ[1] = 100
    occ[0][rng.random((ny, nx)) < 0.08] = 100
    cells = [(int(rng.integers(nx)), int(rng.integers(ny)), 0) for _ in range(n)]
    g = np.array([rm.centre((int(rng.integers(nx)), int(rng.integers(ny)), 0)) for _ in range(n)])
    case = rm.make_case((nx, ny, 2), [view] * 3, [rm.centre(c) for c in cells], occ, sm.spread_params(2.5, 1.2, passes=n), view_of=rng.integers(0, 3, n),
                        g_term=g)
    case["vehicles"]["status"] = np.where(rng.random(n) < 0.7, sm.GOAL_REACHED, sm.TRAVELING)
    case["group"] = np.array([5, 5, -2], dtype=np.int32)
    return case


@pytest.mark.parametrize("seed", range(6))
def test_goals_of_peers_keep_r_spread_apart_and_off_the_standing_claims(seed):
    case = random_fleet(seed)
    g, m, r = sm.model(case)
    veh, par = case["vehicles"], case["par"]
    n = len(veh)
    r_spread2 = float(par["r_spread"]) ** 2
    reach2, near2 = (2 * float(par["r_max"]) + float(par["r_spread"])) ** 2, (float(par["r_max"]) + float(par["r_spread"])) ** 2
    assert not (r["flags"] & (OVERFLOW | UNSETTLED)).any() and m.sum() >= 2
    grp = case["group"][case["view_of"]]
    pos = veh["state"]["pos"]
    pairs = 0
    for i in range(n):
        for k in range(n):
            if i == k or grp[i] != grp[k] or not m[i]:
                continue
            if m[k] and sm.d2_of(pos[k], pos[i]) < reach2:
                pairs += 1
                assert sm.d2_of(g[k], g[i]) >= r_spread2, (i, k)
            if r["flags"][k] == 0 and veh["status"][k] != sm.GOAL_REACHED and sm.d2_of(veh["g_term"][k], pos[i]) < near2:
                assert sm.d2_of(veh["g_term"][k], g[i]) >= r_spread2, (i, k)
    assert pairs > 0


def test_every_wrong_variant_changes_a_named_case():
    told = {}
    for variant in sm.VARIANTS:
        told[variant] = [name for name in sm.CASES
                         if any(a.tobytes() != b.tobytes() for a, b in zip(sm.model(sm.case(name), variant), sm.expected(name)))]
        assert told[variant], variant
    # the case made for each of them is among those that tell it
    for variant, name in (("no_standing", "traveling_peer"), ("higher_peers", "pair_same_voxel"), ("le_spread", "exactly_r_spread"),
                          ("non_peers", "pair_other_groups"), ("group_by_view", "labels"), ("same_pass", "chain_passes_3"),
                          ("no_reach", "outside_reach"), ("overflow_claim", "overflowed_lower_peer")):
        assert name in told[variant], (variant, told[variant])
