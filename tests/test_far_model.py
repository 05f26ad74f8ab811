"""The model of include/fasterhip_far.h (tests/far_model.py) on the CPU: every named case has the property it is named for, every wrong
variant changes a named case, the consequence of the block rule for r_avoid holds voxel by voxel, and with blocks of one voxel the model
is the model of include/fasterhip_reach.h (tests/reach_model.py) with a box that holds the whole lattice."""
import numpy as np
import pytest

from faster_amd import abi

import far_model as fa
import frontier_model as fm
import reach_model as rm

WANTED, FOUND, CUT = abi.FH_FRONTIER_WANTED, abi.FH_FRONTIER_FOUND, abi.FH_REACH_CUT
OUTSIDE, SKIPPED = abi.FH_REACH_START_OUTSIDE, abi.FH_FAR_SKIPPED


def out(name):
    goals, mask, rec, sums, need = fa.expected(name)
    return fa.case(name), goals, mask, rec, sums, need


def cell(case, voxel):
    return rm.cell_index(voxel, case["grid"][2])


def bits(word_row):
    return int(sum(bin(int(w)).count("1") for w in word_row))


def test_stranded_is_left_without_a_goal_by_the_voxel_flood_and_found_here():
    case, goals, mask, rec, _, _ = out("stranded")
    par = rm.reach_params(fa.REACH_R)
    _, r_mask, r_rec = rm.reach_goals(par, case["grid"], case["flags"], case["stride"], case["view_of"], case["n_views"], case["vehicles"], case["occ"],
                                      case["m_origin"], case["m_res"])
    assert r_mask.tolist() == [0] and int(r_rec["candidates"][0]) == 0 and int(r_rec["flags"][0]) == WANTED   # searched, nothing in the box
    assert mask.tolist() == [1] and int(rec["cell"][0]) == cell(case, (19, 1, 0)) and int(rec["hops"][0]) == 4
    assert np.array_equal(goals[0], rm.centre((19, 1, 0))) and float(rec["d2"][0]) == 81.0 > fa.REACH_R ** 2


def test_detour_diagonal_gap_and_sealed_links_are_pairs_of_free_voxels():
    case, _, mask, rec, sums, _ = out("detour")
    assert mask.tolist() == [1] and int(rec["block_cell"][0]) == 0 and int(rec["hops"][0]) == 2
    assert int(rec["targets"][0]) == 2 and int(rec["reachable"][0]) == 1                      # block 3 is a target block, and nearer
    assert fa.block_d2((3, 0, 0), 2, case["grid"], case["vehicles"]["state"]["pos"][0]) < float(rec["block_d2"][0])
    assert int(sums[0][1][0]) == 0b01011   # LX: 0 | 1, 1 | 2 and 3 | 4, not 2 | 3 (the wall is the first column of block 3)
    for name in ("diagonal_gap", "sealed"):
        case, goals, mask, rec, sums, _ = out(name)
        assert mask.tolist() == [0] and int(rec["targets"][0]) == 1 and int(rec["reachable"][0]) == 0 and int(rec["reached"][0]) == 1
        assert int(rec["flags"][0]) == WANTED and goals.tobytes() == case["vehicles"]["g_term"].tobytes()
        assert bits(sums[0][1]) == 0
    wrong = fa.model(fa.case("diagonal_gap"), "links_any_free")
    assert wrong[1].tolist() == [1]   # both blocks hold free voxels


def test_corner_link_and_partial_blocks():
    case, _, mask, rec, sums, _ = out("corner_link")
    assert mask.tolist() == [1] and int(rec["hops"][0]) == 1 and int(rec["cell"][0]) == cell(case, (3, 2, 2))
    assert bits(sums[0][1]) == 1 and bits(sums[0][2]) == 0 and bits(sums[0][3]) == 0        # one link in the whole lattice
    (cx, cy, cz), wx, W = fa.blocks_of(case["grid"][2], 2)
    assert (cx, cy, cz, W) == (3, 2, 2, 4) and int(sums[0][1][(1 * cy + 1) * wx]) == 1    # at block (0, 1, 1): one row of one layer
    case, _, mask, rec, sums, _ = out("partial_blocks")
    assert fa.blocks_of(case["grid"][2], 4)[0] == (4, 2, 1)
    assert mask.tolist() == [1, 1] and rec["block_cell"].tolist() == [7, 6] and rec["hops"].tolist() == [0, 3] and rec["members"].tolist() == [3, 1]
    # vehicle 0 stands beyond the centre of the last voxel of its (partial) block along x and y: the distance to the block is not 0
    assert abs(float(rec["block_d2"][0]) - (0.2 ** 2 + 0.2 ** 2)) < 1e-12
    assert float(fa.model(case, "full_hi")[2]["block_d2"][0]) == 0.0
    assert int(sums[0][0][0]) == 0 and int(sums[0][0][1]) == 0b1100   # T: the blocks (2, 1, 0) and (3, 1, 0)
    assert int(sums[0][1][0]) == int(sums[0][1][1]) == 0b0111           # no LX bit in the last block of a row


def test_word_carry_row_end_and_z_links():
    case, _, mask, rec, sums, _ = out("word_carry")
    assert fa.blocks_of(case["grid"][2], 1)[:2] == ((65, 1, 2), 2)
    assert mask.tolist() == [1, 1] and rec["cell"].tolist() == [64, 0] and rec["hops"].tolist() == [64, 64]   # bit 63 -> word 1, and back
    assert fa.model(case, "no_carry")[1].tolist() == [0, 0]
    case, _, mask, rec, sums, _ = out("row_end")
    assert fa.blocks_of(case["grid"][2], 1)[:2] == ((64, 2, 2), 1)
    assert mask.tolist() == [0, 0] and rec["targets"].tolist() == [1, 1] and rec["reached"].tolist() == [1, 1]
    assert fa.model(case, "row_wrap")[1].tolist() == [1, 1]
    case, _, mask, rec, sums, _ = out("z_links")
    assert mask.tolist() == [1] and int(rec["hops"][0]) == 2 and int(rec["members"][0]) == 3
    assert bits(sums[0][1]) == 0 and bits(sums[0][2]) == 0 and sums[0][3].tolist() == [1, 1, 0]


def test_own_block_and_start_blocked():
    case, _, mask, rec, _, _ = out("own_block")
    assert mask.tolist() == [1] and int(rec["hops"][0]) == 0 and float(rec["block_d2"][0]) == 0.0 and int(rec["levels"][0]) == 0
    case, _, mask, rec, _, _ = out("start_blocked")
    assert case["occ"][0, 0, 0] != 0
    assert mask.tolist() == [1] and int(rec["hops"][0]) == 2 and int(rec["reached"][0]) == 3
    assert fa.model(case, "start_passable")[1].tolist() == [0]


def test_the_vehicles_that_are_not_searched():
    for name, flags, masks in (("start_outside", [WANTED | OUTSIDE, WANTED | OUTSIDE, WANTED | FOUND], [0, 0, 1]),
                               ("no_view", [WANTED | FOUND, WANTED | abi.FH_FRONTIER_NO_VIEW, WANTED | abi.FH_FRONTIER_NO_VIEW], [1, 0, 0]),
                               ("bad_pos", [WANTED | FOUND, WANTED | abi.FH_FRONTIER_BAD_POS, WANTED | abi.FH_FRONTIER_BAD_POS], [1, 0, 0]),
                               ("not_wanted", [WANTED | FOUND, 0, 0], [1, 0, 0]),
                               ("skipped", [WANTED | FOUND, WANTED | SKIPPED, WANTED | SKIPPED | abi.FH_FRONTIER_BAD_POS, WANTED | OUTSIDE], [1, 0, 0, 0])):
        case, goals, mask, rec, _, need = out(name)
        assert rec["flags"].tolist() == flags and mask.tolist() == masks, name
        idle = np.nonzero(mask == 0)[0]
        assert goals[idle].tobytes() == case["vehicles"]["g_term"][idle].tobytes(), name   # the bits of g_term, NaN and infinity included
        for k in ("cell", "block_cell", "hops"):
            assert (rec[k][idle] == -1).all(), (name, k)
        for k in ("targets", "reachable", "reached", "levels", "members"):
            assert (rec[k][idle] == 0).all(), (name, k)
        assert np.isinf(rec["d2"][idle]).all() and np.isinf(rec["block_d2"][idle]).all() and not rec["reserved"].any()
        assert int(need.sum()) == 1, name   # the one searched vehicle's view
    assert out("no_view")[3]["view"].tolist() == [0, 2, -1]
    # a skipped vehicle would have been searched, and found something
    case = dict(fa.case("skipped"))
    case["skip"] = None
    assert fa.model(case)[1].tolist() == [1, 1, 0, 0]


def test_avoid_edge_equality_is_kept_and_one_step_nearer_moves_the_choice():
    case, _, mask, rec, _, _ = out("avoid_edge")
    g = case["vehicles"]["g_term"]
    assert fa.block_d2((4, 0, 0), 2, case["grid"], g[0]) == 1.0 == float(case["par"]["r_avoid"]) ** 2
    assert fa.block_d2((4, 0, 0), 2, case["grid"], g[1]) < 1.0 and g[1][0] == np.nextafter(g[0][0], 0.0)
    assert mask.tolist() == [1, 1] and rec["block_cell"].tolist() == [4, 0] and rec["targets"].tolist() == [2, 1] and rec["hops"].tolist() == [2, 2]


def test_no_target_voxel_of_a_target_block_is_within_r_avoid():
    """The consequence the header states: the voxel rule of fasterhip_frontier.h need not be tested again."""
    seen = 0
    for name in fa.CASES:
        case = fa.case(name)
        if float(case["par"]["r_avoid"]) == 0.0:
            continue
        _, _, rec, _, _ = fa.expected(name)
        origin, res, dims = case["grid"]
        B = int(case["par"]["block"])
        views = fm.views_of(case["flags"], case["n_views"], case["stride"], dims)
        free, qz = rm.map_free(case["grid"], case["occ"], case["m_origin"], case["m_res"])
        a2 = np.float64(case["par"]["r_avoid"]) ** 2
        for i in np.nonzero(rec["flags"] & FOUND)[0]:
            v = int(i if case["view_of"] is None else case["view_of"][i])
            _, _, target = fa.summary(views[v], free, qz, case["par"], B)
            g = case["vehicles"]["g_term"][i]
            C = fa.blocks_of(dims, B)[0]
            for iz, iy, ix in zip(*np.nonzero(target)):
                b = (ix // B, iy // B, iz // B)
                if fa.block_d2(b, B, case["grid"], g) < a2:
                    continue   # not a target block of this vehicle
                e = [(np.float64(c) + 0.5) * res + origin[k] - g[k] for k, c in enumerate((ix, iy, iz))]
                assert (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2] >= a2, (name, i, (ix, iy, iz))
                seen += 1
            assert C[0] * C[1] * C[2] >= 1
    assert seen > 0


def test_z_edges_other_lattice_and_shared_view():
    case, _, mask, rec, sums, _ = out("z_edges")
    q = lambda iz: (iz + 0.5) * case["grid"][1] + case["grid"][0][2]   # noqa: E731
    assert q(1) == float(case["par"]["z_lo"]) and q(3) == float(case["par"]["z_hi"])
    assert sums[0][0].tolist() == [1, 1, 0] and rec["targets"].tolist() == [2, 2]   # the frontier voxels of block 2 all fail z: T clear
    assert rec["cell"].tolist() == [cell(case, (0, 0, 1)), cell(case, (0, 0, 3))] and rec["members"].tolist() == [1, 1]
    assert fa.model(case, "z_ignored")[2]["targets"].tolist() == [3, 3] and fa.model(case, "z_exclusive")[2]["targets"].tolist() == [0, 0]
    case, _, mask, rec, sums, need = out("other_lattice")
    free, _ = rm.map_free(case["grid"], case["occ"], case["m_origin"], case["m_res"])
    assert not free[:, 0, :].any() and not free[:, :, -1].any()                      # centres outside the map: not passable
    assert (case["views"][:, :, 0, :] == 0).any() and mask.tolist() == [1, 1, 1]
    assert case["m_res"] != case["grid"][1]
    case, _, mask, rec, sums, need = out("shared_view")
    assert need[:3].tolist() == [1, 0, 1] and sorted(sums) == [0, 2] and rec["view"].tolist() == [0, 0, 2]
    assert mask.tolist() == [1, 1, 1] and int(rec["cell"][0]) == int(rec["cell"][1])


def test_ties():
    case, _, _, rec, _, _ = out("ties_hops")
    p = case["vehicles"]["state"]["pos"][0]
    assert int(rec["cell"][0]) == cell(case, (6, 1, 0)) and int(rec["hops"][0]) == 3 and float(rec["block_d2"][0]) == 2.25
    assert fa.block_d2((3, 3, 0), 1, case["grid"], p) == 1.0                         # nearer, but six links away
    assert int(fa.model(case, "d2_first")[2]["cell"][0]) == cell(case, (3, 3, 0))
    case, _, _, rec, _, _ = out("ties_block_d2")
    assert int(rec["cell"][0]) == cell(case, (4, 2, 0)) > cell(case, (5, 1, 0)) and float(rec["block_d2"][0]) == 0.5 and int(rec["reachable"][0]) == 2
    case, _, _, rec, _, _ = out("ties_block")
    p = case["vehicles"]["state"]["pos"][0]
    assert fa.block_d2((1, 0, 0), 2, case["grid"], p) == fa.block_d2((3, 0, 0), 2, case["grid"], p) == 0.5625
    assert int(rec["block_cell"][0]) == 1 and int(rec["hops"][0]) == 1
    case, _, _, rec, _, _ = out("ties_voxel")
    assert int(rec["cell"][0]) == cell(case, (5, 1, 0)) and int(rec["members"][0]) == 3 and float(rec["d2"][0]) == 4.25
    assert int(fa.model(case, "voxel_c")[2]["cell"][0]) == cell(case, (7, 0, 0))


def test_max_hops_block_sizes_and_the_cap():
    _, _, mask, rec, _, _ = out("max_hops")
    assert mask.tolist() == [1] and int(rec["hops"][0]) == 3 == int(rec["levels"][0]) and int(rec["flags"][0]) == WANTED | FOUND | CUT
    _, _, mask, rec, _, _ = out("max_hops_short")
    assert mask.tolist() == [0] and int(rec["levels"][0]) == 2 and int(rec["flags"][0]) == WANTED | CUT and int(rec["targets"][0]) == 1
    case, _, mask, rec, _, _ = out("block_1")
    assert int(case["par"]["block"]) == 1 and mask.tolist() == [1] and int(rec["targets"][0]) > int(rec["reachable"][0])
    case, _, mask, rec, _, _ = out("block_16")
    assert int(case["par"]["block"]) == 16 and fa.blocks_of(case["grid"][2], 16)[0] == (2, 2, 1) and mask.tolist() == [1] and int(rec["hops"][0]) == 2
    case, _, mask, rec, sums, _ = out("cap")
    assert fa.blocks_of(case["grid"][2], 1)[2] == 512 == abi.FH_FAR_MAX_WORDS and sums[0].shape == (4, 512)
    assert mask.tolist() == [1] and int(rec["reached"][0]) == 64 * 64 * 8 - 1 and int(rec["hops"][0]) == 63 + 63 + 6
    assert fa.blocks_of(fa.OVER_CAP, 1)[2] == 513 and fa.work_bytes(fa.OVER_CAP, 1, 1) == 0 and fa.work_bytes(fa.OVER_CAP, 2, 1) > 0


@pytest.mark.parametrize("variant", fa.VARIANTS)
def test_every_wrong_variant_changes_a_named_case(variant):
    changed = []
    for name in fa.CASES:
        if name == "cap":
            continue   # (the largest case: the others tell every variant apart)
        want, got = fa.expected(name), fa.model(fa.case(name), variant)
        if any(a.tobytes() != b.tobytes() for a, b in zip(want[:3], got[:3])):
            changed.append(name)
    assert changed, variant
    named_for = {"links_any_free": "diagonal_gap", "one_way": "word_carry", "row_wrap": "row_end", "no_carry": "word_carry", "full_hi": "partial_blocks",
                 "centre": "stranded", "d2_first": "ties_hops", "avoid_le": "avoid_edge", "avoid_first_voxel": "avoid_edge", "z_ignored": "z_edges",
                 "z_exclusive": "z_edges", "start_passable": "start_blocked", "voxel_c": "ties_voxel"}
    assert named_for[variant] in changed, (variant, changed)
    assert len(fa.VARIANTS) >= 10


def test_with_blocks_of_one_voxel_it_is_the_voxel_flood_over_the_whole_lattice():
    """B = 1, the start passable, r_max = 1e6: reach_model gives the same goals, mask, cell, hops, d2, reached, reachable and levels, and
    its candidates are the targets.  At least two thirds of the named cases qualify."""
    qualified = 0
    for name in fa.CASES:
        red = fa.reduced(fa.case(name))
        if red is None:
            continue
        qualified += 1
        one, rpar = red
        goals, mask, rec, _, _ = fa.model(one)
        r_goals, r_mask, r_rec = rm.reach_goals(rpar, one["grid"], one["flags"], one["stride"], one["view_of"], one["n_views"], one["vehicles"],
                                                one["occ"], one["m_origin"], one["m_res"])
        assert goals.tobytes() == r_goals.tobytes() and mask.tobytes() == r_mask.tobytes(), name
        assert not (r_rec["flags"] & abi.FH_REACH_BOX_TOO_LARGE).any(), name
        assert np.array_equal(rec["flags"], r_rec["flags"]), name
        for k in ("view", "cell", "hops", "reachable", "reached", "levels", "d2"):
            assert rec[k].tobytes() == r_rec[k].tobytes(), (name, k)
        assert np.array_equal(rec["targets"], r_rec["candidates"]) and np.array_equal(rec["block_cell"], rec["cell"]), name
    assert 3 * qualified >= 2 * len(fa.CASES), (qualified, len(fa.CASES))
