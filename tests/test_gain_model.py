"""The Python model of include/fasterhip_gain.h (tests/gain_model.py) on its named cases, without a device: every case has the property
its name claims, every wrong variant of the model changes the outputs of at least one named case — so the byte-for-byte comparison of
tests/test_gpu_gain.py would catch a kernel that made that mistake — and with gain_radius 0, hop_cost 1 and min_gain 0 the model is
the model of include/fasterhip_reach.h on that model's own cases."""
import numpy as np
import pytest

from faster_amd import abi

import gain_model as gm
import reach_model as rm

WANTED, FOUND, CUT, ALL_POOR = abi.FH_FRONTIER_WANTED, abi.FH_FRONTIER_FOUND, abi.FH_REACH_CUT, abi.FH_GAIN_ALL_POOR
HOLE_NEAR, WALL_NEAR = rm.cell_index(gm.HOLE_NEAR, gm.HOLE_DIMS), rm.cell_index(gm.WALL_NEAR, gm.HOLE_DIMS)


def rec_of(name):
    return gm.expected(name)[2]


def details_of(name):
    d = {}
    got = gm.model(gm.case(name), details=d)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, gm.expected(name)))
    return d


def chosen(name, i=0):
    r = rec_of(name)[i]
    return int(r["cell"]), int(r["hops"]), int(r["gain"]), int(r["utility"])


def test_the_hole_is_the_reach_models_choice_and_the_wall_this_models():
    case = gm.case("hole_and_wall")
    _, k_mask, k_rec = gm.reach_model_of(case)
    assert int(k_mask[0]) == 1 and (int(k_rec["cell"][0]), int(k_rec["hops"][0])) == (HOLE_NEAR, 2)
    assert chosen("hole_and_wall") == (WALL_NEAR, 8, 10, 2)
    rec = rec_of("hole_and_wall")
    assert int(rec["flags"][0]) == WANTED | FOUND and int(rec["poor"][0]) == 0 and int(rec["best_gain"][0]) == 10
    d = details_of("hole_and_wall")[0]
    assert d[HOLE_NEAR][:3] == (2, 1, -1) and len(d) == int(rec["reachable"][0]) == 20
    # the hole is one voxel, known on all six sides
    view = case["views"][0]
    assert view[gm.HOLE[2], gm.HOLE[1], gm.HOLE[0]] == 1 and int((view[:, :, :gm.WALL_X] != 0).sum()) == 1
    # hops at their dearest: the hole; the utility is far below zero
    assert chosen("hole_and_wall_dear_hops") == (HOLE_NEAR, 2, 1, 1 - 2 * abi.FH_GAIN_MAX_HOP_COST)
    # hops for nothing: the wall, utility = gain
    assert chosen("hole_and_wall_free_hops") == (WALL_NEAR, 8, 10, 10)
    # min_gain = 2: the five neighbours of the hole are poor and counted; min_gain = 1: none of them is
    poor = rec_of("hole_and_wall_min_gain")
    assert chosen("hole_and_wall_min_gain")[0] == WALL_NEAR and int(poor["poor"][0]) == 5 and int(poor["flags"][0]) == WANTED | FOUND
    assert sorted(c for c, v in d.items() if v[1] < 2) == sorted(rm.cell_index(c, gm.HOLE_DIMS) for c in ((1, 2, 1), (0, 1, 1), (0, 3, 1), (0, 2, 0), (0, 2, 2)))
    assert chosen("hole_and_wall_min_gain_met") == (HOLE_NEAR, 2, 1, 1 - 2 * abi.FH_GAIN_MAX_HOP_COST) and int(rec_of("hole_and_wall_min_gain_met")["poor"][0]) == 0


def test_an_unknown_voxel_counts_whatever_the_map_says_of_it():
    case = gm.case("hole_and_wall_occupied")
    assert (case["occ"][:, :, gm.WALL_X:] != 0).all() and (case["views"][0][:, :, gm.WALL_X:] != 0).all()
    assert chosen("hole_and_wall_occupied") == chosen("hole_and_wall")
    wrong = gm.model(case, "map_known")[2]
    assert int(wrong["cell"][0]) == HOLE_NEAR and int(wrong["best_gain"][0]) == 1


def test_all_poor_is_a_flag_and_no_reachable_candidate_is_not():
    case = gm.case("all_poor")
    goals, mask, rec = gm.expected("all_poor")
    assert int(rec["flags"][0]) == WANTED | ALL_POOR and int(mask[0]) == 0 and int(rec["poor"][0]) == int(rec["reachable"][0]) == 20
    assert (int(rec["cell"][0]), int(rec["hops"][0]), int(rec["gain"][0]), int(rec["utility"][0]), int(rec["best_gain"][0])) == (-1, -1, -1, 0, 10)
    assert np.isinf(rec["d2"][0]) and goals.tobytes() == case["vehicles"]["g_term"].tobytes()
    goals, mask, rec = gm.expected("none_reachable")
    assert rec["flags"].tolist() == [WANTED, WANTED] and rec["candidates"].tolist() == [2, 2] and rec["reachable"].tolist() == [0, 0]
    assert rec["best_gain"].tolist() == [-1, -1] and rec["gain"].tolist() == [-1, -1] and rec["poor"].tolist() == [0, 0] and mask.tolist() == [0, 0]


def test_max_hops_before_at_and_after_the_level_of_the_richest_candidate():
    before, at, after = (rec_of("max_hops_" + k)[0] for k in ("before", "at", "after"))
    assert (int(before["flags"]), int(before["levels"]), int(before["cell"]), int(before["best_gain"])) == (WANTED | FOUND | CUT, 7, HOLE_NEAR, 1)
    assert (int(at["flags"]), int(at["levels"]), int(at["cell"]), int(at["hops"]), int(at["best_gain"])) == (WANTED | FOUND | CUT, 8, WALL_NEAR, 8, 10)
    assert (int(after["flags"]), int(after["levels"]), int(after["cell"]), int(after["hops"])) == (WANTED | FOUND | CUT, 9, WALL_NEAR, 8)
    assert int(before["reachable"]) < int(at["reachable"]) < int(after["reachable"]) < int(rec_of("hole_and_wall")["reachable"][0])


def test_the_start_may_be_a_candidate_unknown_or_occupied():
    assert chosen("start_is_candidate") == (HOLE_NEAR, 0, 1, 1)
    assert 0 in [v[0] for v in details_of("start_is_candidate")[0].values()]
    case = gm.case("start_blocked")
    assert case["views"][0][0, 2, 2] != 0 and case["occ"][1, 3, 3] != 0
    rec = rec_of("start_blocked")
    assert (rec["flags"] == WANTED | FOUND).all() and (rec["reached"] > 10).all() and (rec["gain"] > 0).all()


def test_word_edges_has_candidates_on_both_sides_of_both_word_boundaries_and_rows_across_them():
    case = gm.case("word_edges")
    assert case["grid"][2][0] >= 130 and case["grid"][2][1:] == (3, 3)
    view = case["views"][0]
    d = details_of("word_edges")
    dims = case["grid"][2]
    for i, x in enumerate(gm.WORD_XS):
        assert rm.cell_index((x, 1, 1), dims) in d[i] and d[i][rm.cell_index((x, 1, 1), dims)][0] == 0   # the start: a candidate, at bit x & 63
    for edge in (64, 128):   # unknown voxels on both sides of the boundary, within the ball of a candidate on either side
        assert view[:, :, edge - 3:edge].any() and view[:, :, edge:edge + 3].any()
    wrong = {}
    gm.model(case, "first_word", details=wrong)
    differ = {c % dims[0] for i in d for c in d[i] if d[i][c][1] != wrong[i][c][1]}   # the columns of the candidates whose gain needs the second word
    for edge in (64, 128):   # on both sides of both boundaries
        assert differ & {edge - 3, edge - 2, edge - 1} and differ & {edge, edge + 1, edge + 2}, (edge, sorted(differ))


def test_row_ends_do_not_count_the_start_of_the_next_row():
    case = gm.case("row_ends")
    assert case["grid"][2][0] % 64 != 0
    rec = rec_of("row_ends")
    assert rec["gain"].tolist() == [2, 2] and rec["best_gain"].tolist() == [2, 2]    # the end of the row and the end of the row beside it
    wrong = gm.model(case, "x_wrap")[2]
    assert wrong["best_gain"].tolist() == [3, 3]   # with the voxel at the start of the next row, in y and in z, that a row 66 .. 70 runs into


def test_box_faces_cut_the_ball_on_every_side():
    case = gm.case("box_faces")
    origin, res, dims = case["grid"]
    r_max, g = float(case["par"]["r_max"]), int(case["par"]["gain_radius"])
    boxes = [[rm.box_axis(p[k], r_max, origin[k], res, dims[k]) for k in range(3)] for p in case["vehicles"]["state"]["pos"]]
    assert all(0 < b[0] and b[1] < dims[k] - 1 for k, b in enumerate(boxes[0]))        # vehicle 0: a box inside the lattice
    assert [b[0] for b in boxes[1]] == [0, 0, 0] and [b[1] for b in boxes[2]] == [dims[k] - 1 for k in range(3)]   # the corners
    d = details_of("box_faces")
    nx, ny = dims[0], dims[1]
    for i, box in enumerate(boxes):   # a reachable candidate nearer than g to a face of its box, for every face that vehicle's box has
        xyz = [(c % nx, (c // nx) % ny, c // (nx * ny)) for c in d[i]]
        near = {(k, side) for c in xyz for k in range(3) for side in (0, 1) if abs(c[k] - box[k][side]) < g}
        assert len(near) == 6, (i, near)
    assert (rec_of("box_faces")["flags"] == WANTED | FOUND).all()
    # unknown voxels beyond the box are not counted: with the whole lattice as the box vehicle 0 sees more
    wide = dict(case, par=gm.gain_params(100.0, g))
    assert int(gm.model(wide)[2]["best_gain"][0]) > int(rec_of("box_faces")["best_gain"][0])
    one, layer = rec_of("one_voxel"), rec_of("one_layer")
    assert (int(one["flags"][0]), int(one["reached"][0]), int(one["best_gain"][0]), int(one["gain"][0])) == (WANTED, 1, -1, -1)
    assert gm.case("one_layer")["grid"][2][2] == 1 and int(layer["flags"][0]) == WANTED | FOUND and int(layer["gain"][0]) > 0


def test_radii_0_1_and_31():
    zero, one, wide = rec_of("radius_0")[0], rec_of("radius_1")[0], rec_of("radius_31")[0]
    assert gm.case("radius_31")["grid"][2][0] == 63 and int(gm.case("radius_31")["par"]["gain_radius"]) == abi.FH_GAIN_MAX_RADIUS == 31
    assert (int(zero["gain"]), int(zero["best_gain"]), int(zero["utility"])) == (0, 0, -3 * int(zero["hops"]))
    assert 1 <= int(one["best_gain"]) <= 6     # at most the six face neighbours
    assert int(wide["best_gain"]) > 500
    d = details_of("radius_31")[0]
    assert any(c % 63 == 31 for c in d)        # a candidate in the middle column: its row of the ball is columns 0 .. 62
    # the plain triple loop and the numpy count agree
    case = gm.case("radius_31")
    unknown = case["views"][0] != 0
    for c in list(d)[:3]:
        xyz = (c % 63, (c // 63) % 9, c // (63 * 9))
        assert gm.gain_of(xyz, (0, 0, 0), (62, 8, 2), unknown, 31) == d[c][1] == gm._fast_gain(xyz, (0, 0, 0), (62, 8, 2), unknown, 31)


def test_squared_distance_g2_counts_and_g2_plus_1_does_not():
    g2 = gm.EXACT_G ** 2
    assert sorted(sum(x * x for x in d) for d in gm.EXACT_IN) == [1] + [g2] * 7 and min(sum(x * x for x in d) for d in gm.EXACT_OUT) == g2 + 1
    c = rm.cell_index(gm.EXACT_C, (9, 9, 9))
    assert chosen("exact_radius") == (c, 0, len(gm.EXACT_IN), len(gm.EXACT_IN))
    assert int(gm.model(gm.case("exact_radius"), "lt")[2]["gain"][0]) < len(gm.EXACT_IN)


def test_ties():
    a, b, c = rec_of("ties_hops")[0], rec_of("ties_d2")[0], rec_of("ties_cell")[0]
    d = details_of("ties_hops")[0]
    tied = {k: v for k, v in d.items() if v[2] == int(a["utility"])}
    assert sorted(v[0] for v in tied.values()) == [3, 5, 5, 6] and int(a["utility"]) == max(v[2] for v in d.values()) == -2
    assert (int(a["cell"]), int(a["hops"]), float(a["d2"])) == (rm.cell_index((6, 1, 0), (8, 5, 2)), 3, 2.25)
    assert min(tied, key=lambda k: tied[k][3]) == rm.cell_index((3, 3, 0), (8, 5, 2))   # the nearest of them is not the choice
    d = details_of("ties_d2")[0]
    assert sorted(v[:3] for v in d.values()) == [(2, 2, 0), (2, 2, 0)]
    assert (int(b["cell"]), float(b["d2"])) == (rm.cell_index((4, 2, 0), (7, 4, 2)), 0.5) and int(b["cell"]) == max(d)
    d = details_of("ties_cell")[0]
    assert sorted(v for v in d.values()) == [(2, 1, -1, 1.0), (2, 1, -1, 1.0)]
    assert int(c["cell"]) == rm.cell_index((1, 1, 0), (7, 3, 2)) == min(d)


def test_the_dearest_hops_on_the_serpentine_do_not_wrap():
    rec = rec_of("serpentine_dear_hops")[0]
    assert (int(rec["hops"]), int(rec["levels"]), int(rec["gain"])) == (240, 240, 1)
    assert int(rec["utility"]) == 1 - 240 * 16384 < -(1 << 21) and abi.FH_GAIN_MAX_HOP_COST == 16384


def test_many_levels_hold_candidates_in_every_wavefronts_share():
    d = details_of("many_levels")[0]
    assert len({v[0] for v in d.values()}) >= 20
    case = gm.case("many_levels")
    nx, ny, _ = case["grid"][2]
    # the box is the lattice and a row of it is one word: word u = row, which wavefront u & 3 looks at
    by_wave = {w: [v for c, v in d.items() if ((c // nx) % ny + ny * (c // (nx * ny))) % 4 == w] for w in range(4)}
    assert all(len(v) > 10 for v in by_wave.values())
    rec = rec_of("many_levels")[0]
    assert int(rec["utility"]) == int(rec["gain"]) == int(rec["best_gain"]) == 9 and int(rec["hops"]) > 1


def test_the_inherited_exits():
    rec = rec_of("shared_view")
    assert rec["view"].tolist() == [0, 0, 0, 7, 0]
    assert rec["flags"][3] == WANTED | abi.FH_FRONTIER_NO_VIEW and rec["flags"][4] == WANTED | abi.FH_FRONTIER_BAD_POS and (rec["flags"][:3] & FOUND).all()
    rec = rec_of("start_outside")
    assert rec["flags"].tolist() == [WANTED | abi.FH_REACH_START_OUTSIDE] * 2 + [WANTED | FOUND]
    big, cap = rec_of("box_too_large")[0], rec_of("box_at_cap")[0]
    assert int(big["flags"]) == WANTED | abi.FH_REACH_BOX_TOO_LARGE and int(cap["flags"]) == WANTED | FOUND and int(cap["reached"]) == 7 * 32 * 32
    for r in list(rec_of("shared_view")[3:]) + list(rec[:2]) + [big]:   # not searched
        assert (int(r["cell"]), int(r["hops"]), int(r["gain"]), int(r["utility"]), int(r["poor"]), int(r["best_gain"])) == (-1, -1, -1, 0, 0, -1)
        assert (int(r["candidates"]), int(r["reachable"]), int(r["reached"]), int(r["levels"])) == (0, 0, 0, 0) and np.isinf(r["d2"])
    rec = rec_of("other_lattice")
    assert (rec["flags"] == WANTED | FOUND).all() and (rec["gain"] > 0).all()


@pytest.mark.parametrize("name", gm.ALL_CASES)
def test_the_first_40_bytes_count_what_the_reach_model_counts(name):
    """Whatever the gain parameters are, the flood and the candidates are those of the reach model: every field but the choice."""
    rec = rec_of(name)
    _, _, k_rec = gm.reach_model_of(gm.case(name))
    for k in ("view", "candidates", "reachable", "reached", "levels"):
        assert np.array_equal(rec[k], k_rec[k]), k
    assert np.array_equal(rec["flags"] & ~(FOUND | ALL_POOR), k_rec["flags"] & ~FOUND)
    for k in ("flags", "view", "cell", "hops", "candidates", "reachable", "reached", "levels", "d2"):
        assert abi.gain_record_dtype.fields[k] == abi.reach_record_dtype.fields[k], k
    assert not rec["reserved"].any() and (rec["poor"] <= rec["reachable"]).all()


@pytest.mark.parametrize("name", gm.REDUCTIONS)
def test_with_radius_0_cost_1_and_no_minimum_it_is_the_reach_model(name):
    case = gm.case(name)
    par = case["par"]
    assert (int(par["gain_radius"]), int(par["hop_cost"]), int(par["min_gain"])) == (0, 1, 0)
    goals, mask, rec = gm.expected(name)
    k_goals, k_mask, k_rec = rm.expected(name.split(":", 1)[1])
    assert goals.tobytes() == k_goals.tobytes() and mask.tobytes() == k_mask.tobytes()
    assert all(bytes(rec[i].tobytes()[:40]) == bytes(k_rec[i].tobytes()[:40]) for i in range(len(rec)))
    found = mask == 1
    assert (rec["gain"][found] == 0).all() and np.array_equal(rec["utility"][found], -rec["hops"][found]) and not rec["poor"].any()


def test_every_wrong_variant_changes_a_named_case():
    assert gm.wrong_variants() == gm.VARIANTS and len(gm.VARIANTS) >= 10
    by_voxel = ("cube", "lt", "x_wrap", "first_word")   # (these count voxel by voxel in Python: not on the cases with thousands of candidates)
    told = {}
    for variant in gm.VARIANTS:
        names = [n for n in gm.CASES if not (variant in by_voxel and n in gm.LARGE)]
        told[variant] = [name for name in names
                         if any(a.tobytes() != b.tobytes() for a, b in zip(gm.model(gm.case(name), variant), gm.expected(name)))]
    assert all(told.values()), told
    # the case built for the mistake tells it
    for variant, name in (("cube", "exact_radius"), ("lt", "exact_radius"), ("x_wrap", "row_ends"), ("first_word", "word_edges"),
                          ("no_hops", "hole_and_wall_dear_hops"), ("poor_le", "hole_and_wall_min_gain_met"), ("d2_first", "ties_hops"),
                          ("cell_largest", "ties_cell"), ("map_known", "hole_and_wall_occupied"), ("first_level", "hole_and_wall")):
        assert name in told[variant], (variant, told[variant])


def test_the_gap_bytes_are_never_read():
    case = gm.case("shared_view")
    assert case["stride"] > case["cells"]
    got = gm.model(rm.with_gap(case, 1))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, gm.expected("shared_view")))
