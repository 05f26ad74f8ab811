"""The numpy / Python model of include/fasterhip_reach.h (tests/reach_model.py) on its named cases, without a device: every case has
the property its name claims, the candidates are those of the frontier model on every case, and every wrong variant of the model
changes the outputs of at least one named case — so the byte-for-byte comparison of tests/test_gpu_reach.py would catch a kernel that
made that mistake."""
import numpy as np
import pytest

from faster_amd import abi

import frontier_model as fm
import reach_model as rm

WANTED, FOUND = abi.FH_FRONTIER_WANTED, abi.FH_FRONTIER_FOUND


def rec_of(name):
    return rm.expected(name)[2]


def test_sealed_pocket_is_the_frontier_models_choice_and_not_the_reach_models():
    case = rm.case("sealed_pocket")
    dims = case["grid"][2]
    pocket = rm.cell_index((2, 5, 1), dims)
    _, k_mask, k_rec = rm.frontier_model_of(case)
    assert int(k_mask[0]) == 1 and int(k_rec["cell"][0]) == pocket and float(k_rec["d2"][0]) == 2.25
    goals, mask, rec = rm.expected("sealed_pocket")
    assert int(mask[0]) == 1 and int(rec["flags"][0]) == WANTED | FOUND
    assert int(rec["cell"][0]) != pocket and int(rec["cell"][0]) >= 0
    assert int(rec["candidates"][0]) - int(rec["reachable"][0]) >= 1
    # the pocket is enclosed: all six face neighbours are occupied or unknown
    for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
        x, y, z = 2 + d[0], 5 + d[1], 1 + d[2]
        assert case["occ"][z, y, x] != 0 or case["views"][0][z, y, x] != 0, d


def test_word_carry_runs_across_two_word_boundaries_in_both_directions():
    case = rm.case("word_carry")
    rec = rec_of("word_carry")
    assert case["grid"][2][0] > 128
    assert rec["hops"].tolist() == [149, 149] and rec["levels"].tolist() == [149, 149] and rec["reached"].tolist() == [150, 150]
    assert rec["cell"].tolist() == [rm.cell_index((149, 1, 0), (150, 3, 1)), rm.cell_index((0, 1, 0), (150, 3, 1))]
    assert rec["candidates"].tolist() == [1, 1] and rec["reachable"].tolist() == [1, 1]


def test_row_ends_reach_nothing_across_the_end_of_a_row_or_of_a_slab():
    case = rm.case("row_ends")
    assert case["grid"][2][0] % 64 != 0
    goals, mask, rec = rm.expected("row_ends")
    assert rec["reached"].tolist() == [1, 1] and rec["levels"].tolist() == [0, 0]
    assert rec["candidates"].tolist() == [2, 2] and rec["reachable"].tolist() == [0, 0] and mask.tolist() == [0, 0]
    assert rec["flags"].tolist() == [WANTED, WANTED] and rec["cell"].tolist() == [-1, -1] and rec["hops"].tolist() == [-1, -1]
    assert goals.tobytes() == case["vehicles"]["g_term"].tobytes()


def test_serpentine_has_many_more_levels_than_the_box_has_sides():
    rec = rec_of("serpentine")
    assert int(rec["levels"][0]) == 240 >= 200 and int(rec["hops"][0]) == 240
    assert int(rec["cell"][0]) == rm.cell_index((20, 20, 0), (21, 22, 1)) and int(rec["reached"][0]) == 11 * 21 + 10


def test_clipped_boxes_and_a_lattice_of_one_voxel():
    case = rm.case("clipped_box")
    origin, res, dims = case["grid"]
    for i, p in enumerate(case["vehicles"]["state"]["pos"]):
        box = [rm.box_axis(p[k], 1.0, origin[k], res, dims[k]) for k in range(3)]
        clipped = [(b[0] == 0, b[1] == dims[k] - 1) for k, b in enumerate(box)]
        assert clipped == ([(True, False)] * 3 if i == 0 else [(False, True)] * 3), (i, box)
    rec = rec_of("clipped_box")
    assert (rec["flags"] == WANTED | FOUND).all() and (rec["reached"] > 1).all()
    one = rec_of("one_voxel")
    assert (int(one["flags"][0]), int(one["reached"][0]), int(one["levels"][0]), int(one["candidates"][0]), int(one["cell"][0])) == (WANTED, 1, 0, 0, -1)


def test_a_start_that_is_unknown_or_occupied_still_floods():
    case = rm.case("start_blocked")
    assert case["views"][0][0, 2, 2] != 0 and case["occ"][1, 3, 3] != 0
    rec = rec_of("start_blocked")
    assert (rec["flags"] == WANTED | FOUND).all() and (rec["reached"] > 10).all() and (rec["hops"] > 0).all()


def test_start_outside_and_box_too_large_are_flags():
    rec = rec_of("start_outside")
    assert rec["flags"].tolist() == [WANTED | abi.FH_REACH_START_OUTSIDE] * 2 + [WANTED | FOUND]
    _, _, k_rec = rm.frontier_model_of(rm.case("start_outside"))
    assert (k_rec["candidates"][:2] > 0).all()   # the frontier model searches them: they are within r_max of frontier voxels
    for k in ("candidates", "reachable", "reached", "levels"):
        assert rec[k][:2].tolist() == [0, 0], k
    assert rec["cell"][:2].tolist() == [-1, -1] and rec["hops"][:2].tolist() == [-1, -1] and np.isinf(rec["d2"][:2]).all()
    big, cap = rec_of("box_too_large"), rec_of("box_at_cap")
    for name, words in (("box_too_large", 1025), ("box_at_cap", 1024)):
        dims = rm.case(name)["grid"][2]
        assert -(-dims[0] // 64) * dims[1] * dims[2] == words
    assert abi.FH_REACH_MAX_WORDS == 1024
    assert int(big["flags"][0]) == WANTED | abi.FH_REACH_BOX_TOO_LARGE and int(big["reached"][0]) == 0 and int(big["candidates"][0]) == 0
    assert int(cap["flags"][0]) == WANTED | FOUND and int(cap["reached"][0]) == 7 * 32 * 32


def test_max_hops_cuts_exactly_when_the_last_level_is_not_empty():
    before, at, after = (rec_of("max_hops_" + k) for k in ("before", "at", "after"))
    assert (int(before["flags"][0]), int(before["levels"][0]), int(before["hops"][0]), int(before["reached"][0])) == (WANTED | abi.FH_REACH_CUT, 4, -1, 5)
    assert (int(before["candidates"][0]), int(before["reachable"][0])) == (1, 0)
    assert (int(at["flags"][0]), int(at["levels"][0]), int(at["hops"][0]), int(at["reached"][0])) == (WANTED | FOUND | abi.FH_REACH_CUT, 5, 5, 6)
    assert (int(after["flags"][0]), int(after["levels"][0]), int(after["hops"][0]), int(after["reached"][0])) == (WANTED | FOUND, 5, 5, 6)


def test_ties():
    a, b, c = rec_of("ties_cell"), rec_of("ties_d2"), rec_of("ties_hops")
    assert (int(a["cell"][0]), int(a["hops"][0]), float(a["d2"][0]), int(a["reachable"][0])) == (rm.cell_index((1, 1, 0), (7, 3, 2)), 2, 1.0, 2)
    assert (int(b["cell"][0]), int(b["hops"][0]), float(b["d2"][0]), int(b["reachable"][0])) == (rm.cell_index((4, 2, 0), (7, 4, 2)), 2, 0.5, 2)
    assert (int(c["cell"][0]), int(c["hops"][0]), float(c["d2"][0]), int(c["reachable"][0])) == (rm.cell_index((6, 1, 0), (8, 5, 2)), 3, 2.25, 2)
    _, _, k_rec = rm.frontier_model_of(rm.case("ties_hops"))
    assert int(k_rec["cell"][0]) == rm.cell_index((3, 3, 0), (8, 5, 2))   # the nearer one, six steps away


def test_other_lattice_and_shared_view():
    case = rm.case("other_lattice")
    free, _ = rm.map_free(case["grid"], case["occ"], case["m_origin"], case["m_res"])
    assert not free[:, 0, :].any() and not free[:, :, -1].any() and free.any()   # voxel centres outside the map
    assert (case["m_res"] / case["grid"][1]) % 1.0 != 0.0 and (case["grid"][1] / case["m_res"]) % 1.0 != 0.0
    rec = rec_of("other_lattice")
    assert (rec["flags"] & WANTED).all() and (rec["reached"] > 1).all() and (rec["candidates"] > 0).all()
    rec = rec_of("shared_view")
    assert rec["view"].tolist() == [0, 0, 0, 7, 0]
    assert rec["flags"][3] == WANTED | abi.FH_FRONTIER_NO_VIEW and rec["flags"][4] == WANTED | abi.FH_FRONTIER_BAD_POS
    assert (rec["flags"][:3] & FOUND).all()


@pytest.mark.parametrize("name", rm.ALL_CASES)
def test_candidates_are_those_of_the_frontier_model(name):
    """candidates wherever the vehicle is searched, and the three flags the two models share on every vehicle; a vehicle the reach model
    does not search beyond that (its start outside the lattice, its box too large) has zero counts."""
    rec = rec_of(name)
    _, _, k_rec = rm.frontier_model_of(rm.case(name))
    shared = WANTED | abi.FH_FRONTIER_NO_VIEW | abi.FH_FRONTIER_BAD_POS
    assert np.array_equal(rec["flags"] & shared, k_rec["flags"] & shared) and np.array_equal(rec["view"], k_rec["view"])
    searched = (rec["flags"] & ~(FOUND | abi.FH_REACH_CUT)) == WANTED
    assert np.array_equal(rec["candidates"][searched], k_rec["candidates"][searched])
    assert not rec["candidates"][~searched].any() and not rec["reached"][~searched].any()
    assert (rec["reachable"] <= rec["candidates"]).all() and (rec["reached"][searched] >= 1).all()
    if name.startswith("equality:"):
        assert searched.any() or name == "equality:reached"


def test_every_wrong_variant_changes_a_named_case():
    told = {}
    for variant in rm.VARIANTS:
        told[variant] = [name for name in rm.CASES
                         if any(a.tobytes() != b.tobytes() for a, b in zip(rm.model(rm.case(name), variant), rm.expected(name)))]
    assert all(told.values()), told
    # the case built for the mistake tells it
    for variant, name in (("row_wrap", "row_ends"), ("no_carry", "word_carry"), ("cap64", "serpentine"), ("cap64", "word_carry"),
                          ("start_passable", "start_blocked"), ("diag_xy", "ties_d2"), ("n26", "ties_d2"), ("d2_first", "ties_hops"),
                          ("z_pass", "other_lattice")):
        assert name in told[variant], (variant, told[variant])


def test_the_gap_bytes_are_never_read():
    case = rm.case("shared_view")
    assert case["stride"] > case["cells"]
    want = rm.expected("shared_view")
    got = rm.model(rm.with_gap(case, 1))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
