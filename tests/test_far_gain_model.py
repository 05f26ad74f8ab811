"""What the named cases of tests/far_gain_model.py are for (CPU only): each case has the property it is named for; each case named for the
gain differs from far_model's choice on the same inputs; every deliberately wrong variant changes the case named for it; and with
gain_blocks 0, hop_cost 1 and min_gain 0 the model is far_model's on all of far_model.CASES and on 60 random small fleets."""
import numpy as np
import pytest

from faster_amd import abi

import far_gain_model as fg
import far_model as fa

FOUND, ALL_POOR, CUT = abi.FH_FRONTIER_FOUND, abi.FH_PROSPECT_ALL_POOR, abi.FH_REACH_CUT


def rec_of(name):
    return fg.expected(name)[2]


def far_rec(name):
    return fg.far_outputs(fg.case(name))[2]


def counts_of(name, view=0):
    c = fg.case(name)
    return fg.unknown_counts(c["views"][view], int(c["par"]["block"]))


def same_outputs(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3])) and set(a[5]) == set(b[5]) and \
        all(a[5][v].tobytes() == b[5][v].tobytes() for v in a[5])


def test_the_constants_and_the_records_of_the_model():
    assert (abi.FH_PROSPECT_SKIPPED, abi.FH_PROSPECT_MAX_WORDS, abi.FH_PROSPECT_ALL_POOR, abi.FH_PROSPECT_MAX_BLOCKS,
            abi.FH_PROSPECT_MAX_HOP_COST) == (128, 512, 1024, 5, 16384)
    assert abi.far_gain_params_dtype.itemsize == 64 and abi.far_gain_record_dtype.itemsize == 80
    p = abi.default_far_gain_params(8, 2)
    assert (int(p["block"]), int(p["gain_blocks"]), int(p["hop_cost"]), int(p["min_gain"])) == (8, 2, 64, 0)   # hop_cost: a face of a block
    assert fg.work_bytes((64, 64, 8), 1, 1) == 4 * 512 * 8 + 64 + 64 * 512 * 2 and fg.work_bytes(fa.OVER_CAP, 1, 1) == 0
    assert len(fg.VARIANTS) >= 10 and len(fg.CASES) >= 30


def test_a_hole_next_door_loses_to_the_edge_of_a_hall_four_steps_on():
    r, f = rec_of("hole_vs_hall"), far_rec("hole_vs_hall")
    U = counts_of("hole_vs_hall")
    assert U[0, 0].tolist() == [0, 1, 0, 0, 0] + [8] * 7                      # one unknown voxel in block 1, the hall from block 5 on
    assert (int(f["block_cell"][0]), int(f["hops"][0])) == (1, 1)             # without a gain: the hole
    assert (int(r["block_cell"][0]), int(r["hops"][0]), int(r["gain"][0]), int(r["utility"][0])) == (4, 4, 16, 12)
    assert int(r["best_gain"][0]) == 16 and int(r["poor"][0]) == 0 and int(r["reachable"][0]) == 3


def test_at_the_break_even_hop_cost_the_fewer_hops_win_and_one_more_gives_the_hole():
    below, even, above = rec_of("break_even_below"), rec_of("break_even"), rec_of("break_even_above")
    assert (int(below["block_cell"][0]), int(below["utility"][0])) == (4, 16 - 4 * 4)          # 0 against 1 - 4
    assert (int(even["block_cell"][0]), int(even["hops"][0]), int(even["utility"][0])) == (1, 1, 1 - 5) and 16 - 4 * 5 == 1 - 5
    assert (int(above["block_cell"][0]), int(above["utility"][0])) == (1, 1 - 6) and 16 - 4 * 6 < 1 - 6


def test_the_best_block_need_not_be_in_the_first_level_with_a_target():
    r, f = rec_of("later_level"), far_rec("later_level")
    assert int(f["hops"][0]) == 1 and int(r["hops"][0]) == 4 and int(r["levels"][0]) == 4
    assert int(fg.model(fg.case("later_level"), "first_level")[2]["hops"][0]) == 1


def test_ties_hops_then_d2_then_b():
    r = rec_of("ties_hops")
    wrong = fg.model(fg.case("ties_hops"), "d2_first")[2]
    assert (int(r["hops"][0]), int(r["gain"][0]), int(r["utility"][0]), float(r["block_d2"][0])) == (3, 1, -2, 2.25)
    assert (int(wrong["hops"][0]), int(wrong["gain"][0]), int(wrong["utility"][0]), float(wrong["block_d2"][0])) == (6, 4, -2, 1.0)
    r = rec_of("ties_d2")
    assert (int(r["block_cell"][0]), int(r["hops"][0]), int(r["utility"][0])) == (7, 2, 0)      # block 3 has the same utility and hops
    c = fg.case("ties_d2")
    d3, d7 = (fa.block_d2((b, 0, 0), 2, c["grid"], c["vehicles"]["state"]["pos"][0]) for b in (3, 7))
    assert d7 < d3 and float(r["block_d2"][0]) == d7
    r = rec_of("ties_block")
    c = fg.case("ties_block")
    d3, d7 = (fa.block_d2((b, 0, 0), 2, c["grid"], c["vehicles"]["state"]["pos"][0]) for b in (3, 7))
    assert d3 == d7 and (int(r["block_cell"][0]), int(r["hops"][0]), int(r["utility"][0])) == (3, 2, 0)


def test_min_gain_edges_all_poor_and_best_gain():
    eq, up = rec_of("min_gain_equal"), rec_of("all_poor")
    assert (int(eq["block_cell"][0]), int(eq["gain"][0]), int(eq["poor"][0]), int(eq["flags"][0]) & ALL_POOR) == (4, 8, 2, 0)   # gain == min_gain
    g, m, _, _, _, _ = fg.expected("all_poor")
    assert int(up["flags"][0]) & ALL_POOR and not int(up["flags"][0]) & FOUND and int(m[0]) == 0                # one less: poor, all of them
    assert g[0].tobytes() == fg.case("all_poor")["vehicles"]["g_term"][0].tobytes()
    assert (int(up["poor"][0]), int(up["reachable"][0]), int(up["best_gain"][0]), int(up["gain"][0]), int(up["utility"][0]),
            int(up["block_cell"][0])) == (3, 3, 8, -1, 0, -1)                                                     # best_gain counts a poor block
    assert int(fg.model(fg.case("all_poor"), "best_gain_rich")[2]["best_gain"][0]) == -1
    assert int(fg.model(fg.case("min_gain_equal"), "poor_le")[2]["flags"][0]) & ALL_POOR


def test_gain_blocks_0_1_and_5():
    assert fg.expected("no_gain")[2].view(np.uint8).reshape(-1, 80)[:, :64].tobytes() == far_rec("no_gain").tobytes()
    assert int(rec_of("no_gain")["gain"][0]) == 0 and int(rec_of("no_gain")["best_gain"][0]) == 0
    U = counts_of("block_alone")
    assert fg.gain_of(U, (4, 0, 0), 1) == 0 and U[0, 0, 5] == 8 and fg.expected("block_alone")[3][0][0][0] >> 4 & 1   # a target block, gain 0
    assert (int(rec_of("block_alone")["block_cell"][0]), int(rec_of("block_alone")["gain"][0])) == (1, 1)
    assert (int(rec_of("widest")["block_cell"][0]), int(rec_of("widest")["gain"][0])) == (4, 1 + 4 * 8)
    assert fg.gain_of(U, (1, 0, 0), 5) == 1 + 8


def test_the_cube_is_clipped_at_all_six_faces_and_at_a_partial_block():
    c, r = fg.case("faces"), rec_of("faces")
    U = counts_of("faces")
    ends = [(0, 2, 2), (4, 2, 2), (2, 0, 2), (2, 4, 2), (2, 2, 0), (2, 2, 4)]
    for b in ends:   # target blocks in the six faces of the lattice of blocks, each with a cube of 2 x 3 x 3 blocks
        assert fg.gain_of(U, b, 2) < fg.gain_of(U, b, 2, "delta_le") and fg.gain_of(U, b, 2) > 0
        inside = sum(1 for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)
                     if all(0 <= b[k] + d < 5 for k, d in enumerate((dx, dy, dz))))
        assert inside == 18
    assert (r["flags"] & FOUND).all() and (r["gain"] > 0).all() and len(c["vehicles"]) == 6
    U = counts_of("partial_block")
    assert U.shape == (1, 2, 4) and U[0, 1, 3] == 1 * 2 * 3 and U[0, 1, 2] == 1 * 2 * 3 and U.sum() == 12
    assert fg.unknown_counts(fg.case("partial_block")["views"][0], 4, variant="full_block")[0, 1, 3] > 6
    assert rec_of("partial_block")["gain"].tolist() == [12, 12]


def test_word_and_row_edges():
    c, r = fg.case("word_edge"), rec_of("word_edge")
    assert fa.blocks_of(c["grid"][2], 2) == ((65, 1, 1), 2, 2)
    U = counts_of("word_edge")
    assert (int(r["block_cell"][0]), int(r["gain"][0])) == (61, 6) and U[0, 0, 62:65].tolist() == [2, 2, 2]     # 58 .. 64: astride 63 | 64
    table = fg.expected("word_edge")[5][0]
    assert table.shape == (128,) and table[62:66].tolist() == [2, 2, 2, 0] and not table[65:].any()             # entries beyond Cx are 0
    r = rec_of("row_edge")
    U = counts_of("row_edge")
    assert U[0].tolist() == [[0, 0, 0, 1], [4, 0, 0, 0]]
    assert fg.gain_of(U, (3, 0, 0), 2) == 1 and fg.gain_of(U, (3, 0, 0), 2, "row_wrap") == 5                    # (3, 0) must not see (0, 1)
    assert int(r["reachable"][0]) == 2 and (int(r["block_cell"][0]), int(r["gain"][0])) == (0, 4) and int(r["best_gain"][0]) == 4


def test_block_sizes_3_1_16_and_the_cap():
    c = fg.case("block_3")
    assert fa.blocks_of(c["grid"][2], 3) == ((44, 1, 1), 1, 1)
    U = counts_of("block_3")
    assert U[0, 0, 20:23].tolist() == [1, 3, 1] and U[0, 0, 42:].tolist() == [4, 2]        # blocks 21 and 42 straddle the runs of 64 voxels
    assert rec_of("block_3")["gain"].tolist() == [4, 6]
    assert counts_of("block_1").tolist() == (fg.case("block_1")["views"][0] != 0).astype(int).tolist()
    assert int(counts_of("block_16")[0, 0, 1]) == 4096 and int(rec_of("block_16")["gain"][0]) == 4096
    c = fg.case("cap")
    assert fa.blocks_of(c["grid"][2], 1)[2] == 512 == abi.FH_PROSPECT_MAX_WORDS
    assert int(rec_of("cap")["hops"][0]) > int(far_rec("cap")["hops"][0]) and int(rec_of("cap")["gain"][0]) == 3


def test_unknown_voxels_that_still_count():
    for name, variant in (("occupied_unknown", "free_only"), ("outside_z", "z_filter")):
        r, w = rec_of(name), fg.model(fg.case(name), variant)
        assert (int(r["block_cell"][0]), int(r["gain"][0])) == (4, 16), name
        assert int(w[2]["gain"][0]) < 16 and not same_outputs(fg.expected(name), w), name
    assert fg.case("occupied_unknown")["occ"][1, 1, 20] != 0
    assert fg.expected("outside_z")[5][0][1] == 2   # both voxels of the hole's column, the one inside z and the one outside


def test_a_block_that_r_avoid_removes_still_feeds_its_neighbours():
    c, r = fg.case("avoided_feeds"), rec_of("avoided_feeds")
    free_par = c["par"].copy()
    free_par["r_avoid"] = 0.0
    assert int(fg.model(c, par=free_par)[2]["targets"][0]) == int(r["targets"][0]) + 1        # block 3 is a target without r_avoid
    assert (int(r["block_cell"][0]), int(r["gain"][0])) == (4, 1 + 0 + 8)
    assert int(fg.model(c, "avoid_removed")[2]["gain"][0]) == 8


def test_max_hops_cuts_the_choice_and_the_counts():
    r = rec_of("max_hops_cut")
    assert int(r["flags"][0]) & CUT and (int(r["block_cell"][0]), int(r["hops"][0]), int(r["levels"][0])) == (1, 1, 3)
    assert (int(r["best_gain"][0]), int(r["reachable"][0]), int(r["targets"][0])) == (1, 2, 3)    # block 4 (gain 16) is beyond the cut
    r = rec_of("max_hops_poor")
    assert int(r["flags"][0]) & CUT and int(r["flags"][0]) & ALL_POOR
    assert (int(r["poor"][0]), int(r["reachable"][0]), int(r["best_gain"][0]), int(r["levels"][0])) == (1, 1, 1, 1)


def test_views_vehicles_that_are_not_searched_and_fleet_sizes():
    g, m, r, sums, need, counts = fg.expected("shared_view")
    assert set(sums) == set(counts) == {0, 2} and need[:3].tolist() == [1, 0, 1]
    assert r["hops"].tolist() == [4, 0, 10] and r["gain"].tolist() == [16, 16, 8]
    g, m, r, sums, need, counts = fg.expected("not_searched")
    c = fg.case("not_searched")
    assert r["flags"][:5].tolist() == [abi.FH_FRONTIER_WANTED | abi.FH_PROSPECT_SKIPPED, 0, abi.FH_FRONTIER_WANTED | abi.FH_FRONTIER_NO_VIEW,
                                       abi.FH_FRONTIER_WANTED | abi.FH_FRONTIER_BAD_POS, abi.FH_FRONTIER_WANTED | abi.FH_REACH_START_OUTSIDE]
    for i in range(5):
        assert (int(r["gain"][i]), int(r["best_gain"][i]), int(r["utility"][i]), int(r["poor"][i]), int(r["cell"][i]), int(m[i])) == (-1, -1, 0, 0, -1, 0)
        assert g[i].tobytes() == c["vehicles"]["g_term"][i].tobytes() and np.isinf(r["d2"][i])
    assert int(m[5]) == 1 and int(r["gain"][5]) == 16
    assert len(fg.expected("fleet_1")[1]) == 1 and len(fg.expected("fleet_257")[1]) == 257 and fg.expected("fleet_257")[1].all()
    assert len(set(fg.expected("fleet_257")[2]["hops"].tolist())) >= 4


NAMED_FOR = {"delta_le": "hole_vs_hall", "ball": "faces", "row_wrap": "row_edge", "full_block": "partial_block", "free_only": "occupied_unknown",
             "z_filter": "outside_z", "poor_le": "min_gain_equal", "d2_first": "ties_hops", "first_level": "later_level",
             "avoid_removed": "avoided_feeds", "best_gain_rich": "all_poor"}


@pytest.mark.parametrize("variant", fg.VARIANTS)
def test_every_wrong_variant_changes_the_case_named_for_it(variant):
    name = NAMED_FOR[variant]
    assert not same_outputs(fg.expected(name), fg.model(fg.case(name), variant)), (variant, name)


def test_the_cases_named_for_the_gain_differ_from_the_choice_without_one():
    for name in ("hole_vs_hall", "break_even_below", "later_level", "min_gain_equal", "all_poor", "widest", "faces", "cap", "occupied_unknown",
                 "outside_z", "avoided_feeds", "max_hops_poor", "fleet_1", "fleet_257"):
        r, f = rec_of(name), far_rec(name)
        assert r["cell"].tolist() != f["cell"].tolist(), name


def test_without_a_gain_the_model_is_far_models_on_all_its_cases_and_on_random_fleets():
    """gain_blocks 0, hop_cost 1 (and 7), min_gain 0: goals, mask, the first 64 bytes of every record, the summary words and the need
    bytes.  All cases of far_model.CASES, and 60 random small fleets."""
    def check(case, what):
        want = fa.model(case)
        for hop_cost in (1, 7):
            got = fg.model(case, par=fg.reduction_params(case["par"], hop_cost))
            assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), what
            assert got[2].view(np.uint8).reshape(-1, 80)[:, :64].tobytes() == want[2].tobytes(), what
            assert set(got[3]) == set(want[3]) and all(got[3][v].tobytes() == want[3][v].tobytes() for v in want[3]), what
            assert got[4].tobytes() == want[4].tobytes(), what
            found = got[1] == 1
            assert np.array_equal(got[2]["gain"], np.where(found, 0, -1)) and np.array_equal(got[2]["utility"], np.where(found, -hop_cost * got[2]["hops"], 0))

    for name in fa.CASES:
        check(fa.case(name), name)
    assert len(fa.CASES) == 29
    rng = np.random.default_rng(23)
    fleets = 0
    for k in range(60):
        dims = tuple(int(d) for d in rng.integers(3, 12, size=3))
        n_views, n = int(rng.integers(1, 4)), int(rng.integers(1, 6))
        unknown = [rng.random((dims[2], dims[1], dims[0])) < 0.25 for _ in range(n_views)]
        occupied = [tuple(int(c) for c in q) for q in zip(*[rng.integers(0, d, size=6) for d in dims])]
        pos = [tuple(float(x) for x in rng.random(3) * np.array(dims) * 0.5) for _ in range(n)]
        par = fa.far_params(int(rng.integers(1, 5)), r_avoid=float(rng.choice([0.0, 0.7])), max_hops=int(rng.choice([0, 0, 2])))
        case = fg.scene(dims, unknown, pos, par, occupied=occupied, view_of=[int(v) for v in rng.integers(0, n_views, size=n)],
                        skip=[int(s) for s in (rng.random(n) < 0.2)], g_term=np.array(pos) + rng.random((n, 3)))
        check(case, k)
        fleets += 1
    assert fleets == 60
