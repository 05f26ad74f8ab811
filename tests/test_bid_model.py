"""The Python model of include/fasterhip_bid.h (tests/bid_model.py) on the CPU: every named case has the property it is named for, every
wrong variant of the model changes a named case, and the consequences the header states hold: the rounds give the goals of the
sequential greedy rule, without rivals they give what tests/team_model.py gives (Reduction A), and renumbering the vehicles permutes
the outputs."""
import numpy as np
import pytest

from faster_amd import abi

import bid_model as bm
import gain_model as gm
import reach_model as rm
import team_model as tm

W, F = abi.FH_FRONTIER_WANTED, abi.FH_FRONTIER_FOUND
U, O = abi.FH_BID_UNSETTLED, abi.FH_BID_OVERFLOW


def run(name):
    d, tr = {}, {}
    c = bm.case(name)
    goals, mask, rec = bm.model(c, details=d, trace=tr)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((goals, mask, rec), bm.expected(name)))
    return c, goals, mask, rec, d, tr


def cell(c, xyz):
    return rm.cell_index(xyz, c["grid"][2])


def xyz_of(c, cell_):
    nx, ny, _ = c["grid"][2]
    return (cell_ % nx, (cell_ // nx) % ny, cell_ // (nx * ny))


def ball(centre, r, info):
    """The unknown voxels of the box within r voxels of `centre`, as a set, one squared distance each."""
    lo, hi = info["lo"], info["hi"]
    return {(x, y, z) for z in range(lo[2], hi[2] + 1) for y in range(lo[1], hi[1] + 1) for x in range(lo[0], hi[0] + 1)
            if info["unknown"][z, y, x] and (x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2 <= r * r}


def covered_set(info):
    return {(int(x), int(y), int(z)) for z, y, x in zip(*np.nonzero(info["cov"]))}


def differs(name, variant):
    return any(a.tobytes() != b.tobytes() for a, b in zip(bm.model(bm.case(name), variant=variant), bm.expected(name)))


# ---- 1 .. 12: the named cases ---------------------------------------------------------------------------------------------------------------
def test_the_nearer_vehicle_gets_the_rich_voxel_whatever_its_index_and_the_index_order_gives_it_to_vehicle_0():
    c, goals, mask, rec, d, tr = run("nearer_higher")
    rich = cell(c, (11, 2, 0))
    assert tr["offers"][1] == {0: (2, 7), 1: (5, 4)}                     # both ask for the same voxel; vehicle 1 is three steps nearer
    assert mask.tolist() == [1, 1] and int(rec["cell"][1]) == rich != int(rec["cell"][0])
    assert rec["decided_pass"].tolist() == [2, 1] and rec["searches"].tolist() == [2, 1] and rec["rivals"].tolist() == [1, 1]
    assert rec["claims"].tolist() == [1, 0] and int(rec["claimed"][0]) == 1
    g, cr = int(c["par"]["gain_radius"]), int(c["par"]["claim_radius"])
    winner = ball((11, 2, 0), cr, d[0])
    assert covered_set(d[0]) == winner and int(rec["covered"][0]) == len(winner) == int(rec["gain"][1]) > 0
    own = ball(xyz_of(c, int(rec["cell"][0])), g, d[0])
    assert int(rec["gain"][0]) == len(own - winner) and not (own - winner) & winner   # the loser's ball counts none of the winner's covered voxels
    # the chooser it stands beside gives the rich voxel to index 0, seven steps away
    t_goals, t_mask, t_rec = tm.model(bm.as_team(c))
    assert int(t_rec["cell"][0]) == rich != int(t_rec["cell"][1]) and t_rec["decided_pass"].tolist() == [1, 2] and int(t_rec["hops"][0]) == 7
    assert int(rec["hops"][0]) + int(rec["hops"][1]) < int(t_rec["hops"][0]) + int(t_rec["hops"][1]) or int(rec["utility"][1]) > int(t_rec["utility"][0])
    assert differs("nearer_higher", "index_order") and differs("nearer_higher", "lower_only")


def test_equal_utility_the_fewer_hops_win():
    c, _, mask, rec, _, tr = run("fewer_hops")
    assert int(c["par"]["hop_cost"]) == 0 and tr["offers"][1] == {0: (9, 7), 1: (9, 4)}
    assert rec["decided_pass"].tolist() == [2, 1] and int(rec["cell"][1]) == cell(c, (11, 2, 0)) and mask.tolist() == [1, 1]
    assert differs("fewer_hops", "ties_no_hops")


def test_equal_utility_and_equal_hops_the_lower_index_wins():
    c, _, mask, rec, _, tr = run("same_voxel")
    assert tr["offers"][1][0] == tr["offers"][1][1] and tr["ties"] == [(1, 0, 1)]
    assert rec["decided_pass"].tolist() == [1, 2] and mask.tolist() == [1, 1] and int(rec["cell"][0]) != int(rec["cell"][1])
    assert differs("same_voxel", "ties_high")


def test_a_chain_of_three_with_offers_falling_against_the_index():
    c, _, mask, rec, d, tr = run("chain")
    o = tr["offers"][1]
    assert o[2][0] > o[1][0] > o[0][0]
    assert rec["decided_pass"].tolist() == [3, 2, 1] and rec["searches"].tolist() == [3, 2, 1] and rec["claims"].tolist() == [2, 1, 0]
    assert mask.tolist() == [1, 1, 1] and len(set(rec["cell"].tolist())) == 3 and len(d[0]["voxels"]) == 2
    _, _, mask2, rec2, _, _ = run("chain_passes_2")
    assert rec2["decided_pass"].tolist() == [-1, 2, 1] and mask2.tolist() == [0, 1, 1]
    assert int(rec2["flags"][0]) == W | U and int(rec2["searches"][0]) == 2 and int(rec2["rivals"][0]) == 2 and int(rec2["claims"][0]) == 0
    assert (int(rec2["gain"][0]), int(rec2["best_gain"][0]), int(rec2["covered"][0]), int(rec2["candidates"][0])) == (-1, -1, 0, 0)
    assert rec2[1:].tobytes() == rec[1:].tobytes()


def test_a_path_of_four_settles_both_local_maxima_in_round_1():
    _, _, mask, rec, _, tr = run("path_four")
    assert rec["rivals"].tolist() == [1, 2, 2, 1]                        # 0 - 1 - 2 - 3
    assert [tr["offers"][1][i][0] for i in range(4)] == [7, -1, 7, -1]   # high, low, high, low
    assert tr["decided"] [1] == [0, 2] and tr["decided"][2] == [1, 3] and rec["decided_pass"].tolist() == [1, 2, 1, 2]
    assert rec["searches"].tolist() == [1, 2, 1, 2] and rec["claims"].tolist() == [0, 2, 0, 1] and mask.tolist() == [1, 1, 1, 1]
    assert differs("path_four", "sees_own_round")


def test_searches_1_2_and_3():
    # a loser none of whose rivals won with a goal keeps its offer, unsearched
    _, _, mask, rec, _, tr = run("keeps_offer")
    assert tr["searched"] [1] == [0, 1, 2, 3] and tr["searched"][2] == [1] and tr["searched"][3] == [2]
    assert tr["offers"][2][2] == tr["offers"][1][2] and tr["decided"][1] == [0, 3] and int(mask[3]) == 0
    assert rec["searches"].tolist() == [1, 2, 2, 1] and rec["decided_pass"].tolist() == [1, 2, 3, 1]
    _, _, _, rec2, _, _ = run("keeps_offer_passes_2")
    assert int(rec2["searches"][2]) == 1 and int(rec2["flags"][2]) == W | U and int(rec2["rivals"][2]) == 2   # it lost twice and was searched once
    assert differs("keeps_offer", "mask0_claims") and differs("keeps_offer", "stale_offers")
    # one rival's win gives 2; two rivals winning in different rounds give 3
    assert bm.expected("nearer_higher")[2]["searches"].tolist() == [2, 1]
    assert bm.expected("chain")[2]["searches"].tolist() == [3, 2, 1]


def test_the_order_flips_after_a_discount():
    c, _, mask, rec, d, tr = run("flip")
    assert rec["rivals"].tolist() == [1, 2, 1]                            # C is a rival of B only
    a, b, cc = (tr["offers"][1][i] for i in range(3))
    assert bm.beats(a, 0, b, 1) and bm.beats(b, 1, cc, 2)
    assert tr["offers"][2][2] == cc and bm.beats(cc, 2, tr["offers"][2][1], 1)   # C kept its offer; B's second falls below it
    assert rec["decided_pass"].tolist() == [1, 3, 2] and rec["searches"].tolist() == [1, 3, 1] and int(rec["claims"][1]) == 2
    assert len(d[1]["voxels"]) == 2 and mask.tolist() == [1, 1, 1]
    assert differs("flip", "stale_offers") and differs("flip", "decided_block")


def test_a_rival_without_an_offer_blocks_nobody_and_claims_nothing():
    for name, flag in (("no_offer_poor", abi.FH_BID_ALL_POOR), ("no_offer_unreachable", 0)):
        _, _, mask, rec, d, tr = run(name)
        assert tr["offers"][1][0] is None and tr["offers"][1][1] is not None and rec["rivals"].tolist() == [1, 1]
        assert rec["decided_pass"].tolist() == [1, 1] and mask.tolist() == [0, 1] and int(rec["flags"][0]) == W | flag
        assert rec["claims"].tolist() == [0, 0] and rec["searches"].tolist() == [1, 1]
        assert differs(name, "no_offer_blocks")
    rec = bm.expected("no_offer_poor")[2]
    assert int(rec["poor"][0]) == int(rec["reachable"][0]) > 0 and int(bm.expected("no_offer_unreachable")[2]["reachable"][0]) == 0


def test_lists_of_64_are_searched_and_65_overflow():
    c, _, mask, rec, d, _ = run("listed_64")
    assert (rec["rivals"][:3] + np.array([62, 62, 62])).tolist() == [64, 64, 64] == [abi.FH_BID_LIST] * 3
    last = int(np.argmax(rec["decided_pass"][:3]))
    assert int(rec["claims"][last]) == 64 and len(d[last]["voxels"]) == 64 and mask[:3].tolist() == [1, 1, 1]
    lo, hi, cr = d[last]["lo"], d[last]["hi"], int(c["par"]["claim_radius"])
    assert all(lo[a] - cr <= v[a] <= hi[a] + cr for v in d[last]["voxels"] for a in range(3))     # every claim ball touches the box
    c, _, mask, rec, _, tr = run("listed_65")
    far = len(rec) - 1
    assert (rec["flags"][:3] == W | O).all() and (rec["decided_pass"][:3] == 0).all() and (rec["searches"][:3] == 0).all() and not mask[:3].any()
    assert (rec["rivals"][:3] == 3).all() and (rec["claims"][:3] == 62).all()
    assert int(rec["rivals"][far]) == 3 and int(rec["decided_pass"][far]) == 1 and int(rec["claims"][far]) == 0 and int(mask[far]) == 1
    assert differs("listed_65", "overflow_blocks")
    # a list of 33: searched here, OVERFLOW for the chooser with lists of 32
    c, _, mask, rec, _, _ = run("listed_33")
    assert int(rec["claims"][0]) == 33 and int(mask[0]) == 1 and int(rec["flags"][0]) == W | F
    assert int(tm.expected("widened_overflow")[2]["flags"][0]) == W | abi.FH_TEAM_OVERFLOW


def test_a_rival_at_exactly_reach_is_listed_by_neither_and_just_inside_by_both():
    c, _, _, rec, _, _ = run("outside_reach")
    pos = c["vehicles"]["state"]["pos"]
    assert float(bm.sm.d2_of(pos[1], pos[0])) == 8.5 * 8.5 == float(bm.sm.d2_of(pos[0], pos[1]))
    assert rec["rivals"].tolist() == [0, 0] and rec["decided_pass"].tolist() == [1, 1]
    _, _, _, rec, _, _ = run("inside_reach")
    assert rec["rivals"].tolist() == [1, 1] and rec["decided_pass"].tolist() == [1, 2]


def test_standing_claims_above_and_below_and_the_goal_of_a_decided_rival_above():
    c, goals, mask, rec, d, _ = run("claims_both_sides")
    assert rec["decided_pass"].tolist() == [0, 2, 1, 0] and rec["rivals"].tolist() == [0, 1, 1, 0]
    assert rec["claims"].tolist() == [0, 3, 2, 0] and mask.tolist() == [0, 1, 1, 0]
    g_term = c["vehicles"]["g_term"]
    assert d[1]["claims"] == [tuple(g_term[0]), tuple(g_term[3]), tuple(goals[2])]    # below, above, and the goal of the rival above
    assert int(tm.model(bm.as_team(c))[2]["claims"][1]) == 2                       # the index order never reads a higher searcher's goal


def test_a_winners_claim_ball_across_a_word_boundary_and_at_a_row_end_does_not_leak():
    c, goals, mask, rec, d, _ = run("word_edge_winner")
    info = d[1]
    assert (info["lo"][0], info["hi"][0]) == (0, 131) and info["voxels"] == [(63, 2, 0), (131, 2, 0)]
    cov = covered_set(info)
    assert {(62, 2, 1), (63, 2, 1), (64, 2, 1), (65, 2, 1)} <= cov and (131, 2, 1) in cov and (131, 3, 1) in cov
    assert info["unknown"][1, 3, 0] and info["unknown"][1, 3, 1] and (0, 3, 1) not in cov and (1, 3, 1) not in cov and (0, 4, 1) not in cov
    assert cov == ball((63, 2, 0), 5, info) | ball((131, 2, 0), 5, info) and int(rec["covered"][1]) == len(cov) == 16
    assert rec["decided_pass"].tolist() == [1, 3, 2] and rec["searches"].tolist() == [1, 3, 2]


# ---- the wrong variants -----------------------------------------------------------------------------------------------------------------------
def test_every_wrong_variant_changes_a_named_case():
    assert len(bm.VARIANTS) == 10
    told = {v: [n for n in bm.CASES if differs(n, v)] for v in bm.VARIANTS}
    assert all(told.values()), told
    for name, v in (("nearer_higher", "index_order"), ("same_voxel", "ties_high"), ("fewer_hops", "ties_no_hops"), ("flip", "stale_offers"),
                    ("flip", "decided_block"), ("path_four", "sees_own_round"), ("no_offer_poor", "no_offer_blocks"),
                    ("no_offer_unreachable", "no_offer_blocks"), ("listed_65", "overflow_blocks"), ("nearer_higher", "lower_only"),
                    ("keeps_offer", "mask0_claims")):
        assert name in told[v], (name, v, told[v])


def test_not_searched_vehicles_and_written_bytes():
    for name in bm.CASES:
        goals, mask, rec = bm.expected(name)
        idle = rec["decided_pass"] <= 0   # no searcher or OVERFLOW (0), UNSETTLED (-1)
        assert not (rec["flags"][idle] & F).any() and not rec["candidates"][idle].any() and not mask[idle].any()
        assert (rec["gain"][idle] == -1).all() and (rec["best_gain"][idle] == -1).all()
        assert not rec["utility"][idle].any() and not rec["poor"][idle].any() and not rec["covered"][idle].any()
        assert not rec["reserved"].any() and not rec["searches"][rec["decided_pass"] == 0].any()
        assert (rec["searches"][rec["decided_pass"] != 0] >= 1).all()
        assert goals[mask == 0].tobytes() == bm.case(name)["vehicles"]["g_term"][mask == 0].tobytes()


# ---- consequence 1: progress --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(bm.CASES))
def test_every_round_decides_the_best_offer_of_each_connected_set(name):
    tr = {}
    bm.model(bm.case(name), trace=tr)
    fl = bm._Fleet(*bm._args(bm.case(name)))
    for p, offers in tr["offers"].items():
        left = set(offers)
        while left:   # a connected set of undecided rivals
            comp, edge = set(), [min(left)]
            while edge:
                i = edge.pop()
                if i in comp:
                    continue
                comp.add(i)
                edge += [k for k in fl.rivals[i] if k in left and k not in comp]
            left -= comp
            with_offer = [i for i in comp if offers[i] is not None]
            if with_offer:
                best = with_offer[0]
                for i in with_offer[1:]:
                    if bm.beats(offers[i], i, offers[best], best):
                        best = i
                assert best in tr["decided"][p], (name, p, comp)
            assert all(i in tr["decided"][p] for i in comp if offers[i] is None)


# ---- consequence 2: the sequential greedy rule ------------------------------------------------------------------------------------------------------
def test_the_rounds_give_the_goals_of_the_sequential_greedy_rule():
    checked = 0
    for name in bm.CASES:
        goals, mask, rec = bm.expected(name)
        if (rec["flags"] & U).any():
            continue
        g_goals, g_mask, g_rec = bm.greedy(bm.case(name))
        assert goals.tobytes() == g_goals.tobytes() and mask.tobytes() == g_mask.tobytes(), name
        a, b = rec.copy(), g_rec.copy()
        for r in (a, b):
            r["decided_pass"], r["searches"] = 0, 0
        assert a.tobytes() == b.tobytes(), name
        checked += 1
    assert checked == len(bm.CASES) - 2   # (the two cases with too few passes)


# ---- consequence 3: Reduction A -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bm.REDUCTIONS_A)
def test_reduction_a_without_rivals_it_is_the_chooser_it_stands_beside(name):
    c = bm.case(name)
    goals, mask, rec = bm.expected(name)
    t_goals, t_mask, t_rec = tm.model(bm.as_team(c))
    assert not rec["rivals"].any() and (rec["claims"] <= 32).all() and (rec["decided_pass"] <= 1).all()
    assert goals.tobytes() == t_goals.tobytes() and mask.tobytes() == t_mask.tobytes()
    assert bm.as_team_records(rec).tobytes() == t_rec.tobytes()
    assert np.array_equal(rec["searches"], (rec["decided_pass"] == 1).astype(np.int32))


def test_reduction_a_runs_over_all_cases_of_the_gain_model():
    assert len(gm.CASES) == 32 and sum(n.startswith("A:gain:") for n in bm.REDUCTIONS_A) == 32


# ---- consequence 4: relabelling ---------------------------------------------------------------------------------------------------------------------
def _perms(n):
    idx = np.arange(n)
    return [idx[::-1].copy(), np.roll(idx, 1), np.random.RandomState(20).permutation(n)]


def _tied(name):
    tr = {}
    bm.model(bm.case(name), trace=tr)
    return bool(tr["ties"])


def test_at_most_a_quarter_of_the_named_cases_is_tied():
    tied = [n for n in bm.CASES if _tied(n)]
    assert 4 * len(tied) <= len(bm.CASES) and "same_voxel" in tied, tied


@pytest.mark.parametrize("name", [n for n in bm.CASES])
def test_renumbering_the_vehicles_permutes_the_outputs(name):
    if _tied(name):
        return   # (ties fall to the index: counted by the test above)
    c = bm.case(name)
    goals, mask, rec = bm.expected(name)
    for perm in _perms(len(rec)):
        p_goals, p_mask, p_rec = bm.model(bm.relabelled(c, perm))
        assert p_goals.tobytes() == goals[perm].tobytes() and p_mask.tobytes() == mask[perm].tobytes(), (name, perm)
        a, b = p_rec.copy(), rec[perm].copy()
        a["decided_pass"], b["decided_pass"] = 0, 0
        assert a.tobytes() == b.tobytes(), (name, perm)
    if name == "nearer_higher":   # the index order does not have this property
        t = tm.model(bm.as_team(c))
        p = tm.model(bm.as_team(bm.relabelled(c, [1, 0])))
        assert p[2]["cell"].tolist() != t[2]["cell"][[1, 0]].tolist()
