"""The Python model of include/fasterhip_team.h (tests/team_model.py) on the CPU: every named case has the property it is named for,
every wrong variant of the model changes a named case, and the two reductions the header promises hold against the models of the two
choosers it composes (tests/spread_model.py on all of its cases, tests/gain_model.py on all of its cases)."""
import numpy as np
import pytest

from faster_amd import abi

import gain_model as gm
import reach_model as rm
import spread_model as sm
import team_model as tm

W, F = abi.FH_FRONTIER_WANTED, abi.FH_FRONTIER_FOUND


def run(name):
    d = {}
    c = tm.case(name)
    goals, mask, rec = tm.model(c, details=d)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((goals, mask, rec), tm.expected(name)))
    return c, goals, mask, rec, d


def cell(c, xyz):
    return rm.cell_index(xyz, c["grid"][2])


def xyz_of(c, cell_):
    nx, ny, _ = c["grid"][2]
    return (cell_ % nx, (cell_ // nx) % ny, cell_ // (nx * ny))


def ball(c, centre, r, info):
    """The unknown voxels of the box within r voxels of `centre`, as a set, one squared distance each."""
    lo, hi = info["lo"], info["hi"]
    return {(x, y, z) for z in range(lo[2], hi[2] + 1) for y in range(lo[1], hi[1] + 1) for x in range(lo[0], hi[0] + 1)
            if info["unknown"][z, y, x] and (x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2 <= r * r}


def covered_set(info):
    return {(int(x), int(y), int(z)) for z, y, x in zip(*np.nonzero(info["cov"]))}


def differs(name, variant):
    return any(a.tobytes() != b.tobytes() for a, b in zip(tm.model(tm.case(name), variant=variant), tm.expected(name)))


def test_two_searchers_before_a_wall_get_two_voxels_and_the_second_gain_excludes_the_first_ball():
    c, goals, mask, rec, d = run("wall_pair")
    alone = gm.gain_goals(tm.gain_par_of(c["par"]), c["grid"], c["flags"], c["stride"], c["view_of"], c["n_views"], c["vehicles"], c["occ"],
                          c["m_origin"], c["m_res"])
    # want is "reached" here and "all" there makes no difference: both have arrived
    assert alone[1].tolist() == [1, 1] and int(alone[2]["cell"][0]) == int(alone[2]["cell"][1])        # K17: both the same voxel
    assert mask.tolist() == [1, 1] and int(rec["cell"][0]) == int(alone[2]["cell"][0]) != int(rec["cell"][1])
    first, second = xyz_of(c, int(rec["cell"][0])), xyz_of(c, int(rec["cell"][1]))
    g, cr = int(c["par"]["gain_radius"]), int(c["par"]["claim_radius"])
    assert covered_set(d[1]) == ball(c, first, cr, d[1]) and int(rec["covered"][1]) == len(covered_set(d[1])) > 0
    assert int(rec["gain"][1]) == len(ball(c, second, g, d[1]) - covered_set(d[1]))
    assert rec["decided_pass"].tolist() == [1, 2] and rec["lower"].tolist() == [0, 1] and int(rec["claimed"][1]) == 1


def test_a_claim_ball_that_cuts_a_candidates_ball_leaves_the_exact_difference():
    c, _, mask, rec, d = run("cut_ball")
    g = int(c["par"]["gain_radius"])
    cut = 0
    for k, (hops, gain, utility, _) in d[1]["cands"].items():
        whole, rest = ball(c, xyz_of(c, k), g, d[1]), ball(c, xyz_of(c, k), g, d[1]) - covered_set(d[1])
        assert gain == len(rest) and utility == gain - hops
        cut += 0 < len(rest) < len(whole)
    assert cut > 0 and mask.tolist() == [1, 1]


def test_squared_distance_exactly_r2_is_covered_and_r2_plus_1_is_not():
    c, _, _, rec, d = run("exact_claim")
    r2 = tm.EXACT_R ** 2
    dist = lambda v: sum((v[k] - tm.EXACT_CLAIM[k]) ** 2 for k in range(3))   # noqa: E731
    assert sorted(dist(v) for v in tm.EXACT_IN) == [5, 6, r2, r2, r2] and sorted(dist(v) for v in tm.EXACT_OUT) == [r2 + 1, r2 + 1, r2 + 2]
    assert d[0]["voxels"] == [tm.EXACT_CLAIM] and covered_set(d[0]) == set(tm.EXACT_IN) and int(rec["covered"][0]) == len(tm.EXACT_IN)
    assert differs("exact_claim", "lt_claim")


def test_claim_radius_minus_1_0_and_31():
    seen = {}
    for name in ("claim_radius_none", "claim_radius_0", "claim_radius_31"):
        c, _, mask, rec, d = run(name)
        assert d[0]["voxels"] == [(10, 2, 1)] and d[0]["unknown"][1, 2, 10] and int(mask[0]) == 1   # a standing g_term that lies in unknown space
        seen[name] = (int(rec["covered"][0]), int(rec["best_gain"][0]), covered_set(d[0]))
    assert seen["claim_radius_none"][0] == 0 and not seen["claim_radius_none"][2]
    assert seen["claim_radius_0"][0] == 1 and seen["claim_radius_0"][2] == {(10, 2, 1)}
    n_unknown = int(d[0]["unknown"][d[0]["lo"][2]:d[0]["hi"][2] + 1, d[0]["lo"][1]:d[0]["hi"][1] + 1, d[0]["lo"][0]:d[0]["hi"][0] + 1].sum())
    assert seen["claim_radius_31"][0] == n_unknown > 0 and seen["claim_radius_31"][1] == 0   # everything in the box: every gain is 0
    assert seen["claim_radius_none"][1] > 0


def test_two_overlapping_claims_count_the_union_once():
    c, _, _, rec, d = run("two_claims")
    a, b = (ball(c, v, 3, d[0]) for v in d[0]["voxels"])
    assert a & b and int(rec["covered"][0]) == len(a | b) < len(a) + len(b) and int(rec["claims"][0]) == 2
    assert differs("two_claims", "covered_per_claim")


def test_claims_outside_the_box_and_outside_the_lattice_reach_in():
    c, _, _, rec, d = run("claim_outside_box")
    (k,) = d[0]["voxels"]
    assert k[0] > d[0]["hi"][0] and 0 <= k[0] < c["grid"][2][0] and int(rec["covered"][0]) == len(ball(c, k, 4, d[0])) > 0
    c, _, _, rec, d = run("claim_outside_lattice")
    (k,) = d[0]["voxels"]
    assert k[0] == -2 and int(rec["covered"][0]) == len(ball(c, k, 4, d[0])) > 0 and int(rec["claims"][0]) == 1
    for name in ("claim_outside_box", "claim_outside_lattice"):
        assert differs(name, "r_int_plain") and differs(name, "x_unclipped")   # K16's near would not list them; an unclipped row leaks


def test_claim_balls_across_a_word_boundary_and_at_the_ends_of_rows_do_not_leak():
    c, _, _, rec, d = run("word_edge_claim")
    info = d[0]
    assert (info["lo"][0], info["hi"][0]) == (0, 131) and (63, 2, 0) in info["voxels"] and (131, 2, 0) in info["voxels"] and (130, 4, 1) in info["voxels"]
    cov = covered_set(info)
    assert {(62, 2, 1), (63, 2, 1), (64, 2, 1), (65, 2, 1)} <= cov                       # across bits 63 | 64
    assert (131, 2, 1) in cov and (131, 4, 1) in cov
    assert info["unknown"][1, 3, 0] and (0, 3, 1) not in cov and (1, 3, 1) not in cov    # the start of the next row in y: unknown, not covered
    assert cov == set().union(*(ball(c, v, 5, info) for v in info["voxels"])) and int(rec["covered"][0]) == len(cov)
    assert differs("word_edge_claim", "x_unclipped")


def test_every_open_candidate_poor_only_because_of_the_discount():
    c, _, mask, rec, d = run("poor_by_discount")
    assert mask.tolist() == [1, 0] and int(rec["flags"][1]) & abi.FH_TEAM_ALL_POOR and not int(rec["flags"][1]) & F
    assert int(rec["poor"][1]) == int(rec["reachable"][1]) > 0 and int(rec["best_gain"][1]) < int(c["par"]["min_gain"])
    assert differs("poor_by_discount", "poor_before") and differs("poor_by_discount", "no_discount")   # without the discount it is not poor
    _, _, mask0, rec0, _ = run("poor_by_discount_min_0")
    assert mask0.tolist() == [1, 1] and int(rec0["poor"][1]) == 0 and not int(rec0["flags"][1]) & abi.FH_TEAM_ALL_POOR
    assert np.array_equal(rec0["covered"], rec["covered"])


def test_a_candidate_both_claimed_and_richest_is_not_chosen_and_not_in_best_gain():
    c, _, mask, rec, d = run("claimed_and_richest")
    richest = cell(c, (9, 2, 0))
    assert int(rec["cell"][0]) == richest and int(rec["gain"][0]) == 9 == int(rec["best_gain"][0])
    assert d[1]["claimed"] == [richest] and richest not in d[1]["cands"] and int(rec["cell"][1]) != richest
    assert int(rec["best_gain"][1]) == 6 == int(rec["gain"][1]) and int(rec["covered"][1]) == 0
    assert differs("claimed_and_richest", "claimed_in_best")


def test_a_chain_of_three_over_the_passes():
    c, _, mask, rec, d = run("chain_passes_3")
    assert rec["decided_pass"].tolist() == [1, 2, 3] and rec["lower"].tolist() == [0, 1, 2] and mask.tolist() == [1, 1, 1]
    assert rec["claims"].tolist() == [0, 1, 2] and len(d[2]["voxels"]) == 2
    a, b = (ball(c, v, 2, d[2]) for v in d[2]["voxels"])
    assert a and b and int(rec["covered"][2]) == len(a | b) > int(rec["covered"][1]) > 0   # the third sees both discounts
    _, _, mask2, rec2, _ = run("chain_passes_2")
    assert rec2["decided_pass"].tolist() == [1, 2, -1] and mask2.tolist() == [1, 1, 0]
    assert int(rec2["flags"][2]) == W | abi.FH_TEAM_UNSETTLED and (int(rec2["gain"][2]), int(rec2["best_gain"][2]), int(rec2["covered"][2])) == (-1, -1, 0)
    assert rec2[:2].tobytes() == rec[:2].tobytes()


def test_the_widened_reach_lists_a_peer_that_k16_does_not():
    c, _, _, rec, _ = run("widened_reach")
    assert rec["lower"].tolist() == [0, 1] and rec["decided_pass"].tolist() == [1, 2]
    _, _, _, plain, _ = run("widened_reach_plain")
    assert plain["lower"].tolist() == [0, 0] and plain["decided_pass"].tolist() == [1, 1]
    a = sm.spread_goals(sm.spread_params(1.0, 0.4), c["grid"], c["flags"], c["stride"], c["view_of"], c["n_views"], None, c["vehicles"], c["occ"],
                        c["m_origin"], c["m_res"])
    assert a[2]["lower"].tolist() == [0, 0]
    assert differs("widened_reach", "r_int_plain")


def test_overflow_reached_only_through_the_widened_near():
    _, _, mask, rec, _ = run("widened_overflow")
    assert int(rec["flags"][0]) == W | abi.FH_TEAM_OVERFLOW and int(rec["claims"][0]) == 33 and int(rec["decided_pass"][0]) == 0 and int(mask[0]) == 0
    assert (int(rec["gain"][0]), int(rec["best_gain"][0]), int(rec["utility"][0]), int(rec["poor"][0]), int(rec["covered"][0])) == (-1, -1, 0, 0, 0)
    _, _, mask, rec, _ = run("widened_overflow_plain")
    assert int(rec["flags"][0]) == W | F and int(rec["claims"][0]) == 0 and int(mask[0]) == 1


def test_a_lower_peer_that_found_nothing_claims_nothing_and_covers_nothing():
    c, _, mask, rec, d = run("empty_lower_peer")
    assert mask.tolist() == [0, 1] and rec["lower"].tolist() == [0, 1] and int(rec["claims"][1]) == 0 == int(rec["covered"][1]) == int(rec["claimed"][1])
    assert d[1]["voxels"] == [] and int(rec["decided_pass"][1]) == 2


def test_every_wrong_variant_changes_a_named_case():
    assert len(tm.VARIANTS) >= 10
    told = {v: [n for n in tm.CASES if differs(n, v)] for v in tm.VARIANTS}
    assert all(told.values()), told
    # and the cases named for a mistake tell it
    for name, v in (("wall_pair", "no_discount"), ("exact_claim", "lt_claim"), ("exact_claim", "cube_claim"), ("exact_claim", "round_voxel"),
                    ("two_claims", "covered_per_claim"), ("widened_reach", "r_int_plain"), ("wall_pair", "higher_peers"),
                    ("claimed_and_richest", "claimed_in_best"), ("word_edge_claim", "x_unclipped"), ("poor_by_discount", "poor_before")):
        assert name in told[v], (name, v, told[v])


def test_not_searched_vehicles_and_written_bytes():
    for name in tm.CASES:
        goals, mask, rec = tm.expected(name)
        idle = rec["decided_pass"] <= 0   # no searcher or OVERFLOW (0), UNSETTLED (-1)
        assert not (rec["flags"][idle] & F).any() and not rec["candidates"][idle].any() and not mask[idle].any()
        assert (rec["gain"][idle] == -1).all() and (rec["best_gain"][idle] == -1).all()
        assert not rec["utility"][idle].any() and not rec["poor"][idle].any() and not rec["covered"][idle].any()
        assert not rec["reserved"].any() and not rec["reserved0"].any()
        assert goals[mask == 0].tobytes() == tm.case(name)["vehicles"]["g_term"][mask == 0].tobytes()


# ---- the two reductions ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sm.CASES))
def test_reduction_a_is_the_model_of_the_chooser_with_point_claims(name):
    c = tm.case("A:" + name)
    p = c["par"]
    assert (int(p["claim_radius"]), int(p["gain_radius"]), int(p["hop_cost"]), int(p["min_gain"])) == (-1, 0, 1, 0)
    assert p.tobytes()[:52] == sm.case(name)["par"].tobytes()[:52]
    goals, mask, rec = tm.expected("A:" + name)
    k_goals, k_mask, k_rec = sm.expected(name)
    assert goals.tobytes() == k_goals.tobytes() and mask.tobytes() == k_mask.tobytes()
    assert all(rec[i].tobytes()[:64] == k_rec[i].tobytes() for i in range(len(rec)))
    found = mask == 1
    assert (rec["gain"][found] == 0).all() and np.array_equal(rec["utility"][found], -rec["hops"][found]) and not rec["poor"].any() and not rec["covered"].any()


@pytest.mark.parametrize("name", list(gm.CASES))
def test_reduction_b_is_the_model_of_the_chooser_by_gain_when_no_searcher_has_a_peer(name):
    c = tm.case("B:" + name)
    goals, mask, rec = tm.expected("B:" + name)
    k_goals, k_mask, k_rec = gm.expected(name)
    assert not rec["lower"].any() and not rec["claims"].any() and not rec["covered"].any() and (rec["decided_pass"] <= 1).all()
    assert goals.tobytes() == k_goals.tobytes() and mask.tobytes() == k_mask.tobytes()
    as_team = k_rec.copy()
    as_team["flags"] = tm.as_team_flags(k_rec["flags"])
    view = np.array([int(i if gm.case(name)["view_of"] is None else gm.case(name)["view_of"][i]) for i in range(len(rec))])
    assert np.array_equal(c["view_of"][(view >= 0) & (view < gm.case(name)["n_views"])], np.nonzero((view >= 0) & (view < gm.case(name)["n_views"]))[0])
    as_team["view"] = rec["view"]   # (every vehicle reads a copy of its view under an index of its own: the one word that differs)
    for i in range(len(rec)):
        assert rec[i].tobytes()[:40] == as_team[i].tobytes()[:40], (name, i, rec[i], k_rec[i])
        assert rec[i].tobytes()[64:80] == k_rec[i].tobytes()[40:56], (name, i, rec[i], k_rec[i])
