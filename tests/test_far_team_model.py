"""The model of include/fasterhip_stake.h (tests/far_team_model.py) on its named cases: every case has the property it is named for, every
wrong variant of the model changes the case named for it, and the consequences (a) .. (e) of the header hold against the models of the
far chooser by gain, of the far chooser for a team and of the far chooser itself, on all of their cases and on 60 random small fleets."""
import numpy as np
import pytest

from faster_amd import abi

import far_gain_model as fg
import far_model as fa
import far_spread_model as fs
import far_team_model as ft

FOUND = abi.FH_FRONTIER_FOUND


def block_x(rec, i, cx=12):
    """The x of the chosen block in a lattice of one row of blocks a layer."""
    return int(rec["block_cell"][i]) % cx


def raw(rec, lo, hi):
    return np.ascontiguousarray(rec).view(np.uint8).reshape(len(rec), -1)[:, lo:hi]


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_layout_of_the_model_record():
    assert abi.far_team_record_dtype.itemsize == 128 and abi.far_team_params_dtype.itemsize == 96
    assert ft.work_bytes((24, 2, 2), 2, 1, 3) == 4 * 8 + 64 + 64 * 2 + 64 + 12 + 12
    assert ft.work_bytes((24, 2, 2), 2, 1, -1) == 0 and ft.work_bytes((24, 2, 2), 17, 1, 1) == 0 and ft.work_bytes(fa.OVER_CAP, 1, 1, 1) == 0


def test_two_teammates_two_halls():
    """K23's rule sends both to the rich hall; K22's parts them by r_spread inside the same hall where it is wider than r_spread; this
    chooser gives the lower index the rich hall and the other the poorer one."""
    case = ft.case("two_halls")
    goals, mask, rec = ft.expected("two_halls")[:3]
    g_rec = ft.gain_outputs(case)[2]
    assert [int(b) for b in g_rec["block_cell"]] == [7, 7] and [int(g) for g in g_rec["gain"]] == [16, 16]
    assert mask.tolist() == [1, 1] and block_x(rec, 0) == 7 and block_x(rec, 1) == 1
    assert (int(rec["gain"][0]), int(rec["utility"][0]), int(rec["hops"][0])) == (16, 13, 3)
    assert (int(rec["gain"][1]), int(rec["utility"][1]), int(rec["hops"][1])) == (8, 5, 3)
    assert (int(rec["covered"][0]), int(rec["removed"][0]), int(rec["covered"][1]), int(rec["removed"][1])) == (0, 0, 5, 16)
    assert (int(rec["claims"][1]), int(rec["claimed"][1]), int(rec["lower"][1]), int(rec["decided_pass"][1])) == (1, 1, 1, 2)
    wide = ft.case("wide_hall")
    w_goals, w_mask, w_rec = ft.expected("wide_hall")[:3]
    s_goals, s_mask, s_rec = ft.spread_outputs(wide)[:3]
    g2_rec = ft.gain_outputs(wide)[2]
    cx = 12
    assert int(g2_rec["block_cell"][0]) == int(g2_rec["block_cell"][1]) and int(g2_rec["block_cell"][0]) % cx == 7
    assert s_mask.tolist() == [1, 1] and [int(b) % cx for b in s_rec["block_cell"]] == [7, 7] and s_rec["block_cell"][0] != s_rec["block_cell"][1]
    assert float(np.sum((s_goals[0] - s_goals[1]) ** 2)) >= 1.0
    assert w_mask.tolist() == [1, 1] and int(w_rec["block_cell"][0]) % cx == 7 and int(w_rec["block_cell"][1]) % cx == 1
    assert int(w_rec["removed"][1]) > 0


def test_who_covers_and_who_does_not():
    rec = ft.expected("standing_covers")[2]
    assert block_x(rec, 0) == 1 and (int(rec["standing"][0]), int(rec["claims"][0]), int(rec["covered"][0]), int(rec["removed"][0])) == (1, 1, 5, 16)
    assert int(rec["decided_pass"][1]) == 0 and int(rec["gain"][1]) == -1 and int(rec["covered"][1]) == 0
    # a lower peer that found nothing
    goals, mask, rec = ft.expected("lower_mask0")[:3]
    assert mask.tolist() == [0, 1] and int(rec["lower"][1]) == 1 and int(rec["claims"][1]) == 0 and int(rec["covered"][1]) == 0
    assert block_x(rec, 1) == 7 and int(rec["gain"][1]) == 16
    # UNSETTLED vehicles.  The searching members of a group are one chain by index, so a searcher that IS decided never has an UNSETTLED
    # lower peer: "an UNSETTLED lower peer covers nothing" can only mean that whoever stands behind one is UNSETTLED itself, and that
    # its record carries covered = removed = 0 and gain = best_gain = -1.  That is what is checked here
    goals, mask, rec = ft.expected("lower_unsettled")[:3]
    assert [bool(f & ft.UNSETTLED) for f in rec["flags"]] == [False, True, True] and mask.tolist() == [1, 0, 0]
    assert rec["decided_pass"].tolist() == [1, -1, -1] and rec["gain"].tolist()[1:] == [-1, -1] and rec["best_gain"].tolist()[1:] == [-1, -1]
    assert rec["covered"].tolist() == [0, 0, 0] and rec["lower"].tolist() == [0, 1, 2] and rec["removed"].tolist() == [0, 0, 0]
    goals, mask, rec = ft.expected("chain_short")[:3]   # passes smaller than the chain: the third is not decided
    assert [bool(f & ft.UNSETTLED) for f in rec["flags"]] == [False, False, True] and mask.tolist() == [1, 1, 0]
    assert int(rec["covered"][1]) == 5 and block_x(rec, 1) == 1
    # a peer of another group
    rec = ft.expected("other_group")[2]
    assert [block_x(rec, i) for i in (0, 1)] == [7, 1] and int(rec["covered"][0]) == 0 and int(rec["standing"][0]) == 0
    assert int(rec["standing"][1]) == 1 and int(rec["covered"][1]) == 5
    rec = ft.expected("labels_join")[2]
    assert int(rec["standing"][0]) == 1 and int(rec["covered"][0]) == 5 and block_x(rec, 0) == 1 and rec["group"].tolist() == [-7, -7, -7]


def test_claim_voxels_at_and_beyond_the_faces():
    rec = ft.expected("claim_outside")[2]
    assert (int(rec["claims"][0]), int(rec["claimed"][0]), int(rec["covered"][0]), int(rec["removed"][0])) == (1, 1, 0, 0) and block_x(rec, 0) == 1
    rec = ft.expected("claim_on_face")[2]
    # the goal on the faces lies in voxel (16, 0, 0): block 8 alone is covered (k = 1); the one a nextafter below y = 0 covers nothing
    assert (int(rec["claims"][0]), int(rec["covered"][0]), int(rec["removed"][0])) == (2, 1, 8)
    rec = ft.expected("six_faces")[2]
    assert (rec["covered"][:6] > 0).all() and (np.diff(rec["covered"][:6]) > 0).all()   # every goal given adds a clipped cube
    base = fg.expected("faces")[2]
    assert (rec["gain"][:6] <= base["gain"]).all() and (rec["gain"][:6] < base["gain"]).any() and (rec["removed"][:6] > 0).all()


def test_words_rows_and_the_union():
    for name, cover in (("word_edge_65", (4, 8)), ("word_edge_130", (6, 12))):
        rec = ft.expected(name)[2]
        # the cubes 61 .. 65 and 62 .. 66 (clipped at block 64 where Cx = 65), all wholly unknown (2 voxels each); block 59's cube
        # 56 .. 62 loses 61 and 62
        assert (int(rec["covered"][0]), int(rec["removed"][0])) == cover, name
        assert int(rec["block_cell"][0]) == 59 and int(rec["gain"][0]) == 2 and int(rec["best_gain"][0]) == 2, name
        assert int(ft.gain_outputs(ft.case(name))[2]["gain"][0]) == 6
    rec = ft.expected("row_edge")[2]
    assert (int(rec["covered"][0]), int(rec["removed"][0])) == (4, 1) and int(rec["block_cell"][0]) == 0 and int(rec["gain"][0]) == 4
    rec = ft.expected("overlap")[2]
    assert (int(rec["claims"][0]), int(rec["covered"][0]), int(rec["removed"][0])) == (2, 4, 24)
    rec = ft.expected("cover_0")[2]
    assert (int(rec["claims"][0]), int(rec["covered"][0]), int(rec["removed"][0]), block_x(rec, 0), int(rec["gain"][0])) == (1, 0, 0, 7, 16)
    rec = ft.expected("cover_5")[2]
    assert (int(rec["covered"][0]), int(rec["removed"][0]), block_x(rec, 0)) == (7, 32, 1)
    rec = ft.expected("many_claims")[2]
    assert (int(rec["standing"][0]), int(rec["claims"][0]), int(rec["covered"][0]), int(rec["removed"][0])) == (299, 299, 4, 24)


def test_covered_targets_and_poor_blocks():
    rec = ft.expected("covered_target")[2]
    assert int(rec["claimed"][0]) == 0 and int(rec["targets"][0]) == int(rec["reachable"][0]) == 2 and block_x(rec, 0) == 1
    rec = ft.expected("covered_target_chosen")[2]
    assert block_x(rec, 0) == 7 and (int(rec["gain"][0]), int(rec["utility"][0]), int(rec["covered"][0]), int(rec["claimed"][0])) == (0, 0, 5, 0)
    rec = ft.expected("min_gain_equal")[2]
    assert block_x(rec, 0) == 7 and int(rec["gain"][0]) == 8 and not rec["flags"][0] & ft.ALL_POOR
    rec = ft.expected("min_gain_above")[2]
    assert rec["flags"][0] & ft.ALL_POOR and int(rec["cell"][0]) == -1 and int(rec["poor"][0]) == 2 and int(rec["best_gain"][0]) == 8
    goals, mask, rec = ft.expected("poor_and_claimed")[:3]
    assert mask[0] == 0 and rec["flags"][0] & ft.ALL_POOR and rec["flags"][0] & ft.CLAIMED and not rec["flags"][0] & FOUND
    assert int(rec["claimed"][0]) == 1 and int(rec["reachable"][0]) == int(rec["poor"][0]) > 0 and int(rec["gain"][0]) == -1 and int(rec["best_gain"][0]) == 1


def test_shapes_and_vehicles_that_are_not_searched():
    for name in ("block_1", "block_3", "block_16", "partial_block", "cap", "fleet_257"):
        goals, mask, rec = ft.expected(name)[:3]
        assert mask[0] == 1 and mask[1] == 1 and rec["block_cell"][0] != rec["block_cell"][1], name
        assert int(rec["covered"][1]) > 0, name
    rec = ft.expected("fleet_1")[2]
    assert len(rec) == 1 and block_x(rec, 0) == 7 and int(rec["covered"][0]) == 0
    rec = ft.expected("fleet_257")[2]
    assert int(rec["lower"][256]) == 256 and (rec["flags"][64:] & ft.UNSETTLED).all() and not (rec["flags"][:64] & ft.UNSETTLED).any()
    goals, mask, rec = ft.expected("not_searched")[:3]
    assert mask.tolist() == [0, 0, 0, 0, 0, 1, 1]
    assert [int(f) for f in rec["flags"][:5]] == [abi.FH_FRONTIER_WANTED | abi.FH_STAKE_SKIPPED, 0, abi.FH_FRONTIER_WANTED | abi.FH_FRONTIER_NO_VIEW,
                                                   abi.FH_FRONTIER_WANTED | abi.FH_FRONTIER_BAD_POS, abi.FH_FRONTIER_WANTED | abi.FH_REACH_START_OUTSIDE]
    for k, v in (("gain", -1), ("best_gain", -1), ("utility", 0), ("poor", 0), ("covered", 0), ("removed", 0), ("decided_pass", 0)):
        assert rec[k][:5].tolist() == [v] * 5, k
    need = ft.expected("unneeded_view")[4]
    assert need[:3].tolist() == [1, 0, 1] and sorted(ft.expected("unneeded_view")[5]) == [0, 2]


# the case that tells each wrong variant from the model, and the vehicle whose record differs
TELLS = {"cover_by_gap": "claim_outside", "cover_removes": "covered_target", "cover_non_peers": "other_group", "mask0_covers": "lower_mask0",
         "standing_no_cover": "standing_covers", "row_wrap": "row_edge", "union_twice": "overlap", "poor_uncovered": "min_gain_above",
         "own_block": "standing_covers", "removed_cube": "overlap"}


@pytest.mark.parametrize("variant", ft.VARIANTS)
def test_every_wrong_variant_changes_the_case_named_for_it(variant):
    assert sorted(TELLS) == sorted(ft.VARIANTS)
    name = TELLS[variant]
    right, wrong = ft.expected(name), ft.model(ft.case(name), variant)
    assert not same(right[2], wrong[2]), (variant, name)
    # and it is a variant of THIS rule: the tables that do not depend on claims stay
    assert same(right[4], wrong[4]) and same(right[6], wrong[6]) and same(right[7], wrong[7]) and same(right[8], wrong[8])


def test_several_variants_change_more_than_one_case():
    changed = {v: [n for n in ("two_halls", "standing_covers", "claim_outside", "overlap", "six_faces", "word_edge_65", "many_claims")
                   if not same(ft.expected(n)[2], ft.model(ft.case(n), v)[2])] for v in ("cover_by_gap", "standing_no_cover", "union_twice", "own_block")}
    assert all(len(c) >= 2 for c in changed.values()), changed


def unshared(case):
    """The case with a copy of its view for every vehicle: nobody has a peer.  A vehicle without a view keeps none."""
    n, stride, n_views = len(case["vehicles"]), case["stride"], case["n_views"]
    vo = np.arange(n) if case["view_of"] is None else np.asarray(case["view_of"])
    out = dict(case)
    flags = np.zeros(n * stride, dtype=np.uint8)
    view_of = np.full(n, -1, dtype=np.int32)
    for i in range(n):
        if 0 <= vo[i] < n_views:
            flags[i * stride:(i + 1) * stride] = case["flags"][vo[i] * stride:(vo[i] + 1) * stride]
            view_of[i] = i
    out["flags"], out["view_of"], out["n_views"], out["group"] = flags, view_of, n, None
    return out


def check_a(case, par):
    """Consequence (a) on a case in which no searcher has a peer."""
    probe = dict(case, par=par)
    assert not ft.has_peers(probe)
    mine = ft.model(probe)
    theirs = ft.gain_outputs(probe)
    assert same(mine[0], theirs[0]) and same(mine[1], theirs[1])
    assert same(raw(mine[2], 0, 64), raw(theirs[2], 0, 64))
    for k in ("gain", "utility", "poor", "best_gain"):
        assert same(np.ascontiguousarray(mine[2][k]), np.ascontiguousarray(theirs[2][k])), k
    assert not mine[2]["covered"].any() and not mine[2]["removed"].any() and not mine[2]["claims"].any()
    assert sorted(mine[3]) == sorted(theirs[3]) and all(same(mine[3][v], theirs[3][v]) for v in mine[3])
    assert same(mine[4], theirs[4])
    assert sorted(mine[5]) == sorted(theirs[5]) and all(same(mine[5][v], theirs[5][v]) for v in mine[5])


def check_b(case, par):
    """Consequence (b): gain_blocks 0, hop_cost >= 1, min_gain 0."""
    probe = dict(case, par=par)
    mine = ft.model(probe)
    theirs = ft.spread_outputs(probe)
    assert same(mine[0], theirs[0]) and same(mine[1], theirs[1])
    assert same(raw(mine[2], 0, 96), raw(theirs[2], 0, 96))
    who = fs.judge(par, case["grid"], case["view_of"], case["n_views"], case["skip"], case.get("group"), case["vehicles"])
    assert mine[6].tolist() == [w[2] for w in who] and mine[7].tolist() == [w[3] for w in who]
    assert same(mine[8], np.ascontiguousarray(theirs[2]["lower"]))
    assert all(same(mine[3][v], theirs[3][v]) for v in mine[3]) and sorted(mine[3]) == sorted(theirs[3]) and same(mine[4], theirs[4])
    searched = mine[2]["decided_pass"] > 0
    assert (mine[2]["gain"][searched & (mine[1] == 1)] == 0).all() and not mine[2]["poor"].any()


@pytest.mark.parametrize("name", sorted(fg.CASES))
def test_consequence_a_on_the_cases_of_the_far_chooser_by_gain(name):
    case = dict(fg.case(name), group=None)
    check_a(unshared(case), ft.from_gain_params(case["par"], r_spread=1.0, claim_blocks=3))
    if not ft.has_peers(dict(case, par=ft.from_gain_params(case["par"]))):
        check_a(case, ft.from_gain_params(case["par"], r_spread=2.0))


@pytest.mark.parametrize("name", sorted(fs.CASES))
def test_consequence_b_on_the_cases_of_the_far_chooser_for_a_team(name):
    case = fs.case(name)
    check_b(case, ft.from_spread_params(case["par"], claim_blocks=3))
    if name in ("pair_one_view", "standing_claim", "chain_of_three", "two_words"):
        check_b(case, ft.from_spread_params(case["par"], claim_blocks=0, hop_cost=7))
        check_b(case, ft.from_spread_params(case["par"], claim_blocks=5, hop_cost=16384))


def check_c(case, far_par, r_spread, claim_blocks, hop_cost=1):
    """Consequence (c) on a case in which no searcher has a peer: gain_blocks 0, hop_cost >= 1 and min_gain 0 give far_model's goals,
    mask, first 64 bytes of every record, summary words and need bytes."""
    par = ft.from_gain_params(fg.reduction_params(far_par, hop_cost), r_spread=r_spread, claim_blocks=claim_blocks)
    assert not ft.has_peers(dict(case, par=par))
    mine = ft.model(dict(case, par=par))
    theirs = fa.model(case, par=far_par)
    assert same(mine[0], theirs[0]) and same(mine[1], theirs[1]) and same(raw(mine[2], 0, 64), raw(theirs[2], 0, 64))
    assert sorted(mine[3]) == sorted(theirs[3]) and all(same(mine[3][v], theirs[3][v]) for v in mine[3]) and same(mine[4], theirs[4])
    for k in ("lower", "standing", "claims", "claimed", "poor", "covered", "removed"):
        assert not mine[2][k].any(), k


@pytest.mark.parametrize("name", sorted(fa.CASES))
def test_consequence_c_on_the_cases_of_the_far_chooser(name):
    check_c(unshared(dict(fa.case(name), group=None)), fa.case(name)["par"], 1.5, 2)


@pytest.mark.parametrize("seed", range(60))
def test_consequences_on_random_small_fleets(seed):
    case = ft.random_fleet(seed)
    par = case["par"]
    goals, mask, rec, sums, need, counts, cls, grp, lower = ft.model(case)
    B, g = int(par["block"]), int(par["gain_blocks"])
    origin, res, dims = case["grid"]
    C = fa.blocks_of(dims, B)[0]
    s2 = np.float64(par["r_spread"]) * np.float64(par["r_spread"])
    # (a) without peers, (b) without a gain, (c) with both: against far_model on the far chooser's part of the params
    lone = unshared(case)
    check_a(lone, par)
    check_c(lone, ft.far_part(par), float(par["r_spread"]), int(par["claim_blocks"]), 1 + seed % 3)
    check_b(case, ft.from_spread_params(ft.spread_part(par), claim_blocks=int(par["claim_blocks"])))
    # (d) the gain of a chosen block is at most K23's gain of that block
    views = {v: fg.unknown_counts(case["views"][v], B) for v in counts}
    for i in np.nonzero(mask)[0]:
        b = int(rec["block_cell"][i])
        bxyz = (b % C[0], (b // C[0]) % C[1], b // (C[0] * C[1]))
        full = fg.gain_of(views[int(rec["view"][i])], bxyz, g)
        assert 0 <= int(rec["gain"][i]) <= full and int(rec["best_gain"][i]) >= int(rec["gain"][i])
        assert int(rec["removed"][i]) >= full - int(rec["gain"][i])
    # (e) K22's separation: passes (16) > every lower
    assert not (rec["flags"] & ft.UNSETTLED).any()
    for i in np.nonzero(mask)[0]:
        for j in range(len(mask)):
            if j == i or cls[j] == ft.NONE or grp[j] != grp[i]:
                continue
            other = goals[j] if cls[j] == ft.SEARCHER and mask[j] == 1 else (case["vehicles"]["g_term"][j] if cls[j] == ft.STANDING else None)
            if other is None:
                continue
            d = goals[i] - other
            assert (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] >= s2, (seed, i, j)
