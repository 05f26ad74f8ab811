"""The model of include/fasterhip_apart.h (tests/far_spread_model.py) on its named cases: every case has the property it is named
for, every case named for a claim differs from what tests/far_model.py gives on the same inputs, every wrong variant changes the case
named for it, and the two consequences the header states hold on all cases and on random small fleets — (a) without peers the outputs
are fh_far_goals_device's, (b) with enough passes no two peers' goals and no goal and a standing peer's g_term are nearer than r_spread,
asserted voxel by voxel."""
import numpy as np
import pytest

from faster_amd import abi

import far_model as fa
import far_spread_model as fs

FOUND, WANTED, SKIPPED = abi.FH_FRONTIER_FOUND, abi.FH_FRONTIER_WANTED, abi.FH_FAR_SKIPPED
NEAR, MID, END = (fs.centre((q[0], q[1], 0)) for q in (fs.NEAR, fs.MID, fs.END))


def goal(name, i):
    goals, mask, rec, _, _ = fs.expected(name)
    return tuple(goals[i]) if mask[i] == 1 else None


def rec_of(name, i):
    return fs.expected(name)[2][i]


def d2(a, b):
    e = [np.float64(a[k]) - np.float64(b[k]) for k in range(3)]
    return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]


# ---- what each case is named for ----------------------------------------------------------------------------------------------------------
def test_pairs():
    assert goal("pair_one_view", 0) == NEAR and goal("pair_one_view", 1) == MID and d2(NEAR, MID) >= 2.0 ** 2
    r = rec_of("pair_one_view", 1)
    assert (int(r["decided_pass"]), int(r["lower"]), int(r["standing"]), int(r["claims"]), int(r["claimed"]), int(r["targets"]), int(r["reachable"])) == \
        (2, 1, 0, 1, 1, 2, 1)
    assert goal("pair_two_groups", 0) == goal("pair_two_groups", 1) == NEAR
    assert [int(x) for x in fs.expected("pair_two_groups")[2]["group"]] == [0, 1]


def test_chains():
    assert [goal("chain_of_three", i) for i in range(3)] == [NEAR, MID, END]
    assert [int(x) for x in fs.expected("chain_of_three")[2]["decided_pass"]] == [1, 2, 3]
    assert [int(x) for x in fs.expected("chain_of_three")[2]["claims"]] == [0, 1, 2]
    rec = fs.expected("chain_two_passes")[2]
    assert [int(x) for x in rec["decided_pass"]] == [1, 2, -1] and int(rec["flags"][2]) == WANTED | fs.UNSETTLED
    assert goal("chain_two_passes", 2) is None and (int(rec["lower"][2]), int(rec["claims"][2]), int(rec["targets"][2]), int(rec["cell"][2])) == (2, 0, 0, -1)
    assert fs.expected("chain_two_passes")[0][2].tobytes() == fs.case("chain_two_passes")["vehicles"]["g_term"][2].tobytes()
    assert fs.expected("chain_two_passes")[4][0] == 1                                 # its view is needed all the same
    rec = fs.expected("lower_finds_nothing")[2]
    assert goal("lower_finds_nothing", 0) is None and goal("lower_finds_nothing", 1) == NEAR
    assert (int(rec["decided_pass"][1]), int(rec["lower"][1]), int(rec["claims"][1]), int(rec["claimed"][1])) == (2, 1, 0, 0)
    assert goal("higher_claims_nothing", 0) == NEAR and goal("higher_claims_nothing", 1) == MID


def test_who_claims():
    assert goal("standing_claim", 0) == MID and int(rec_of("standing_claim", 0)["standing"]) == 1
    r = rec_of("standing_claim", 1)
    assert (int(r["flags"]), int(r["decided_pass"]), int(r["lower"]), int(r["standing"]), int(r["claims"])) == (WANTED | SKIPPED, 0, 0, 0, 0)
    assert goal("standing_non_peer", 0) == NEAR and int(rec_of("standing_non_peer", 0)["standing"]) == 0
    assert goal("standing_reached", 0) == NEAR and int(rec_of("standing_reached", 0)["standing"]) == 0
    assert goal("standing_travels", 0) == MID and int(rec_of("standing_travels", 0)["standing"]) == 1
    assert goal("standing_nan", 0) == NEAR and int(rec_of("standing_nan", 1)["flags"]) & abi.FH_FRONTIER_BAD_POS
    assert goal("skipped_yawing", 0) == MID
    assert goal("skipped_reached", 0) == NEAR and int(rec_of("skipped_reached", 0)["standing"]) == 0


def test_radius_and_coverage():
    assert goal("radius_edge", 0) == NEAR and goal("radius_edge", 1) == MID
    assert [int(x) for x in fs.expected("radius_edge")[2]["claimed"][:2]] == [0, 1]
    r = rec_of("all_claimed", 0)
    assert goal("all_claimed", 0) is None and int(r["flags"]) == WANTED | fs.CLAIMED and (int(r["targets"]), int(r["claimed"]), int(r["reachable"])) == (1, 1, 0)
    r = rec_of("avoid_and_claim", 0)
    assert goal("avoid_and_claim", 0) == MID and (int(r["targets"]), int(r["claimed"]), int(r["claims"])) == (1, 0, 1)
    r = rec_of("route_through_claim", 0)
    assert goal("route_through_claim", 0) == MID and int(r["hops"]) == 8 and int(r["claimed"]) == 1 and int(r["reached"]) == 12
    assert goal("gap_not_centre", 0) == fs.centre((20, 0, 0)) and goal("block_not_voxel", 0) == fs.centre((20, 0, 0))


def test_counts_and_fleet_sizes():
    for name, m in (("standing_33", 33), ("standing_300", 300)):
        r = rec_of(name, 0)
        assert goal(name, 0) == MID and (int(r["standing"]), int(r["claims"]), int(r["claimed"]), int(r["decided_pass"])) == (m, m, 1, 1), name
        assert not int(r["flags"]) & ~(WANTED | FOUND), name                           # nothing overflows
    assert 33 > abi.FH_SPREAD_LIST and 300 > 256
    for n in (255, 256, 257, 513):
        goals, mask, rec, _, _ = fs.expected("fleet_%d" % n)
        chain = [k for k in (0, 64, 256, n - 1) if k < n]
        chain = sorted(set(chain))
        assert [int(rec["decided_pass"][k]) for k in chain] == list(range(1, len(chain) + 1)), n
        assert [int(rec["lower"][k]) for k in chain] == list(range(len(chain))), n
        standing = len({k for k in (63, 255, n - 2) if 0 <= k < n and k not in chain})
        assert all(int(rec["standing"][k]) == standing for k in chain) and all(mask[k] == 1 for k in chain), n
        assert int(mask.sum()) == len(chain) and len({tuple(goals[k]) for k in chain}) == len(chain), n


def test_bitmap_edges():
    goals, mask, rec, _, _ = fs.expected("two_words")
    assert int(rec["claimed"][0]) == 2 and int(rec["targets"][0]) == 4 and tuple(goals[0]) == fs.centre((63, 1, 0))
    goals, mask, rec, _, _ = fs.expected("partial_block")
    assert tuple(goals[0]) == fs.centre((12, 0, 0)) and tuple(goals[1]) == fs.centre((0, 0, 0)) and [int(x) for x in rec["claimed"][:2]] == [0, 1]
    assert goal("claim_outside", 0) == fs.centre((22, 0, 0)) and int(rec_of("claim_outside", 0)["claimed"]) == 1
    assert goal("block_1", 0) == NEAR and goal("block_1", 1) == MID and int(rec_of("block_1", 1)["claimed"]) == 1
    assert goal("block_16", 0) == fs.centre((20, 3, 0)) and goal("block_16", 1) == fs.centre((39, 17, 0))
    case = fs.case("cap")
    assert fa.blocks_of(case["grid"][2], 1)[2] == abi.FH_FAR_MAX_WORDS
    goals, mask, rec, _, _ = fs.expected("cap")
    assert mask.tolist() == [1, 1] and int(rec["claimed"][1]) == 3 and d2(goals[0], goals[1]) > 30.0 ** 2


def test_labels_and_views():
    assert [goal("labels", i) for i in range(3)] == [NEAR, NEAR, MID]
    assert [int(x) for x in fs.expected("labels")[2]["group"]] == [-7, 2 ** 31 - 1, -7]
    assert [goal("labels_null", i) for i in range(3)] == [NEAR] * 3 and [int(x) for x in fs.expected("labels_null")[2]["group"]] == [0, 1, 2]
    goals, mask, rec, _, _ = fs.expected("shared_and_invalid_view")
    assert [tuple(g) for g in goals[[0, 2, 3]]] == [NEAR, MID, NEAR] and int(mask[1]) == 0
    assert int(rec["flags"][1]) & abi.FH_FRONTIER_NO_VIEW and int(rec["group"][1]) == 0 and int(rec["view"][1]) == 5 and int(rec["standing"][0]) == 0
    assert goal("one_vehicle", 0) == NEAR and int(rec_of("one_vehicle", 0)["decided_pass"]) == 1


@pytest.mark.parametrize("name", fs.CLAIM_CASES)
def test_a_case_named_for_a_claim_differs_from_the_chooser_without_claims(name):
    goals, mask, rec, sums, need = fs.expected(name)
    f_goals, f_mask, f_rec, f_sums, f_need = fs.far_outputs(fs.case(name))
    assert goals.tobytes() != f_goals.tobytes() or mask.tobytes() != f_mask.tobytes(), name
    assert need.tobytes() == f_need.tobytes() and sorted(sums) == sorted(f_sums)        # the summary stage is that chooser's
    assert all(sums[v].tobytes() == f_sums[v].tobytes() for v in sums)


# ---- the wrong variants ------------------------------------------------------------------------------------------------------------------------
NAMED_FOR = {"no_standing": "standing_claim", "higher_peers": "higher_claims_nothing", "le": "radius_edge", "non_peers": "standing_non_peer",
             "group_by_view": "labels", "same_pass": "chain_two_passes", "centre": "gap_not_centre", "cut_links": "route_through_claim",
             "reached_claims": "skipped_reached", "voxel_only": "block_not_voxel"}


@pytest.mark.parametrize("variant", fs.VARIANTS)
def test_every_wrong_variant_changes_the_case_named_for_it(variant):
    assert sorted(NAMED_FOR) == sorted(fs.VARIANTS)
    name = NAMED_FOR[variant]
    want, got = fs.expected(name), fs.model(fs.case(name), variant)
    assert any(w.tobytes() != g.tobytes() for w, g in zip(want[:3], got[:3])), (variant, name)


# ---- the consequences ---------------------------------------------------------------------------------------------------------------------------
def consequence_a(case, out):
    """Without peers: goals, mask and the first 64 bytes of every record are the chooser's without claims."""
    goals, mask, rec, sums, need = out
    f_goals, f_mask, f_rec, f_sums, f_need = fs.far_outputs(case)
    assert goals.tobytes() == f_goals.tobytes() and mask.tobytes() == f_mask.tobytes()
    assert rec.view(np.uint8).reshape(len(rec), 96)[:, :64].tobytes() == f_rec.tobytes()
    assert need.tobytes() == f_need.tobytes() and all(sums[v].tobytes() == f_sums[v].tobytes() for v in f_sums)


def consequence_b(case, out):
    """No two peers' goals nearer than r_spread, no goal within r_spread of a standing peer's g_term.  -> the pairs tested."""
    goals, mask, rec, _, _ = out
    if int(rec["lower"].max()) >= int(case["par"]["passes"]):
        return 0
    s2 = np.float64(case["par"]["r_spread"]) * np.float64(case["par"]["r_spread"])
    who = fs.judge(case["par"], case["grid"], case["view_of"], case["n_views"], case["skip"], case["group"], case["vehicles"])
    pairs = 0
    for i in np.nonzero(mask == 1)[0]:
        for k in range(len(mask)):
            if k == i or who[k][2] == fs.NONE or who[k][3] != who[i][3]:
                continue
            if who[k][2] == fs.STANDING:
                assert not d2(goals[i], case["vehicles"]["g_term"][k]) < s2, (i, k)
                pairs += 1
            elif mask[k] == 1:
                assert not d2(goals[i], goals[k]) < s2, (i, k)
                pairs += 1
    return pairs


def test_the_consequences_hold_on_every_case_and_on_random_small_fleets():
    without, pairs = 0, 0
    for name in fs.CASES:
        case, out = fs.case(name), fs.expected(name)
        if not fs.has_peers(case):
            consequence_a(case, out)
            without += 1
        pairs += consequence_b(case, out)
    for seed in range(60):
        case = fs.random_fleet(seed)
        out = fs.model(case)
        if not fs.has_peers(case):
            consequence_a(case, out)
            without += 1
        pairs += consequence_b(case, out)
    assert without >= 8 and pairs >= 100, "consequence (a) on %d cases and fleets without peers, (b) on %d pairs of peers" % (without, pairs)
    print("consequence (a) on %d cases and fleets without peers, (b) on %d pairs of peers" % (without, pairs))
