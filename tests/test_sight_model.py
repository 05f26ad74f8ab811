"""The Python model of include/fasterhip_sight.h (tests/sight_model.py) on its named cases, without a device: every case has the
property its name claims, every wrong variant of the model changes the outputs of at least one named case — so the byte-for-byte
comparison of tests/test_gpu_sight.py would catch a kernel that made that mistake — and the two reductions hold: (A) where no searched
box holds a wall the model is tests/gain_model.py in bytes 0 .. 55, goals and mask, (B) with gain_radius 0, hop_cost 1 and min_gain 0
it is tests/reach_model.py on that model's own cases."""
import numpy as np
import pytest

from faster_amd import abi

import gain_model as gm
import reach_model as rm
import sight_model as sm

WANTED, FOUND, ALL_POOR = abi.FH_FRONTIER_WANTED, abi.FH_FRONTIER_FOUND, abi.FH_SIGHT_ALL_POOR
DEAR = abi.FH_SIGHT_MAX_HOP_COST


def rec_of(name):
    return sm.expected(name)[2]


def details_of(name, variant=None):
    d = {}
    got = sm.model(sm.case(name), variant, details=d)
    if variant is None:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, sm.expected(name)))
    return d


def line(d):
    """The line voxels of the header for the offset d, one integer division each: plain Python, no numpy."""
    m = max(abs(a) for a in d)
    sgn = lambda a: (a > 0) - (a < 0)   # noqa: E731
    return [tuple(sgn(a) * ((2 * abs(a) * k + m) // (2 * m)) for a in d) for k in range(1, m)]


def probe_gain(name, i=0):
    """(gain, ball_gain, walls) of the choice of a case whose vehicle stands on the probed candidate."""
    r = rec_of(name)[i]
    assert int(r["flags"]) == WANTED | FOUND and int(r["hops"]) == 0
    return int(r["gain"]), int(r["ball_gain"]), int(r["walls"])


def test_the_line_of_the_header():
    assert line((2, 1, 0)) == [(1, 1, 0)] and line((2, -1, 0)) == [(1, -1, 0)] and line((-1, 2, 0)) == [(-1, 1, 0)]     # a half: away from c
    assert line((6, 3, 0)) == [(1, 1, 0), (2, 1, 0), (3, 2, 0), (4, 2, 0), (5, 3, 0)]
    assert line((1, 4, 0)) == [(0, 1, 0), (1, 2, 0), (1, 3, 0)] and line((0, 1, 4)) == [(0, 0, 1), (0, 1, 2), (0, 1, 3)]
    assert line((1, 1, 1)) == [] and line((0, 0, 0)) == [] and line(sm.PARENTS_U) == [(1, 0, 0), (2, 1, 0)]
    for d in ((7, -3, 2), (-5, 5, 1), (0, -31, 17), (31, 30, -31)):
        pts = line(d)
        assert len(pts) == max(abs(a) for a in d) - 1 and all(abs(p[k]) <= abs(d[k]) for p in pts for k in range(3))
        assert line(tuple(-a for a in d)) == [tuple(-a for a in p) for p in pts]                                          # sign and magnitude
        assert all(max(abs(p[k] - q[k]) for k in range(3)) == 1 for p, q in zip([(0, 0, 0)] + pts, pts + [d]))            # 26-connected
    # the model's vectorised formula is this one
    d = np.array([(7, -3, 2), (-5, 5, 1), (2, 1, 0)])
    m = np.abs(d).max(axis=1)
    for k in range(1, 7):
        got = sm.line_offsets(d, m, k)
        for row, dd in zip(got, d):
            if k < max(abs(int(a)) for a in dd):
                assert tuple(int(v) for v in row) == line(tuple(int(a) for a in dd))[k - 1]


def test_a_hole_before_a_wall_is_the_gain_models_choice_and_the_open_edge_this_models():
    case = sm.case("hole_before_wall")
    near, edge = rm.cell_index(sm.HB_NEAR, sm.HB_DIMS), rm.cell_index(sm.HB_EDGE, sm.HB_DIMS)
    _, k_mask, k_rec = sm.gain_model_of(case)
    assert int(k_mask[0]) == 1 and (int(k_rec["cell"][0]), int(k_rec["hops"][0]), int(k_rec["gain"][0])) == (near, 6, 17)
    r = rec_of("hole_before_wall")[0]
    assert (int(r["cell"]), int(r["hops"]), int(r["gain"]), int(r["ball_gain"]), int(r["utility"])) == (edge, 6, 15, 15, 9)
    assert int(r["walls"]) == 27 and int(r["poor"]) == 0 and int(r["best_gain"]) == 15
    d = details_of("hole_before_wall")[0]
    assert d[near] == (6, 1, 17, -5)                      # the slab is in its ball, and the hole is all it sees
    hole_side = [rm.cell_index(c, sm.HB_DIMS) for c in ((3, 4, 1), (5, 4, 1), (4, 3, 1), (4, 5, 1), (4, 4, 0), (4, 4, 2))]
    assert all(d[c][1] == 1 for c in hole_side)
    # the plane is known and occupied, one voxel thick, between HB_NEAR and the slab
    view, occ = case["views"][0], case["occ"]
    assert (occ[:, :, 2] != 0).all() and not occ[:, :, 3:].any() and not occ[:, :, :2].any() and not view[:, :, 2].any() and view[:, :, :2].all()
    # min_gain 2: the six neighbours of the hole are poor by what they see, not by their balls
    p = rec_of("hole_before_wall_min_gain")[0]
    assert int(p["cell"]) == edge and int(p["poor"]) == 6 and int(p["flags"]) == WANTED | FOUND
    assert int(sm.model(sm.case("hole_before_wall_min_gain"), "poor_on_ball")[2]["poor"][0]) < 6


def test_a_closed_plane_a_window_and_a_pillar():
    near = rm.cell_index(sm.PL_NEAR, sm.PL_DIMS)
    # closed: 16 voxels behind the plane are in the ball and none is seen; what is left is the hole the candidate touches (m = 1)
    assert probe_gain("closed_plane") == (1, 17, 21) and int(rec_of("closed_plane")["cell"][0]) == near
    # a window of one voxel straight ahead: the voxels seen through it are those whose line goes over the window
    c, w = sm.PL_NEAR, sm.PL_WINDOW
    through = [(x, y, z) for x in range(5, 9) for y in range(7) for z in range(3)
               if (x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2 <= 9
               and all(p[0] + c[0] != 4 or (p[0] + c[0], p[1] + c[1], p[2] + c[2]) == w for p in line((x - c[0], y - c[1], z - c[2])))]
    assert through == [(5, 3, 1), (6, 3, 1)] and probe_gain("window") == (1 + len(through), 17, 20)
    # a pillar: its shadow is what lies behind it
    gain, ball, walls = probe_gain("pillar")
    assert (gain, ball, walls) == (13, 17, 3)
    shadow = [(x, y, z) for x in range(5, 9) for y in range(7) for z in range(3)
              if (x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2 <= 9
              and any((p[0] + c[0], p[1] + c[1]) == (4, 3) for p in line((x - c[0], y - c[1], z - c[2])))]
    assert len(shadow) == ball - gain and (5, 3, 1) in shadow and (5, 2, 1) not in shadow


def test_rounding_a_half_goes_away_from_the_candidate_in_sign_and_magnitude():
    for name, told in (("round_plus", ("floor", "half_toward")), ("round_minus", ("floor", "half_toward", "floor_signed")),
                       ("round_3_of_6", ("floor", "half_toward")), ("round_negative_x", ("floor", "half_toward", "floor_signed"))):
        assert probe_gain(name) == (1, 2, 1), name       # the wall stands on the half-way voxel: the target is hidden
        for v in told:
            assert int(sm.model(sm.case(name), v)[2]["gain"][0]) == 2, (name, v)
    assert int(sm.model(sm.case("round_plus"), "floor_signed")[2]["gain"][0]) == 1   # (positive offsets do not tell it)


def test_the_largest_component_drives_the_walk_whichever_axis_it_is():
    for name in ("drive_y", "drive_z", "drive_z_oblique"):
        assert probe_gain(name) == (1, 2, 1), name
        assert int(sm.model(sm.case(name), "x_drives")[2]["gain"][0]) == 2, name
    assert (0, 1, 0) in line((1, 4, 0)) and (0, 0, 1) in line((0, 1, 4)) and (3, 1, 4) in line((4, 1, 6))


def test_unknown_space_is_transparent_whatever_the_map_says_of_it():
    case = sm.case("transparent_unknown")
    c = sm.PROBE_C
    assert case["occ"][c[2], c[1] + 2, c[0]] != 0 and case["views"][0][c[2], c[1] + 2, c[0]] != 0 and int(case["occ"].astype(bool).sum()) == 1
    assert probe_gain("transparent_unknown") == (5, 5, 0)      # both targets and both voxels on their lines, and no wall in the box
    assert int(sm.model(case, "unknown_blocks")[2]["gain"][0]) == 3 and int(sm.model(case, "occupied_unknown")[2]["gain"][0]) == 4


def test_a_known_voxel_outside_the_map_is_a_wall():
    case = sm.case("outside_map")
    assert case["occ"].shape == (3, 3, 4) and not case["occ"].any()
    assert probe_gain("outside_map") == (1, 2, 8 * 9 - 4 * 9 - 1)   # every known voxel with x >= 4
    assert int(sm.model(case, "outside_free")[2]["gain"][0]) == 2 and int(sm.model(case, "outside_free")[2]["walls"][0]) == 0


def test_a_neighbour_between_two_walls_is_seen_and_a_diagonal_wall_leaks():
    assert probe_gain("between_two_walls") == (2, 2, 2)
    gain, ball, walls = probe_gain("diagonal_leak")
    assert (gain, ball, walls) == (2, 2, 18)
    # the stated limit: no face-connected path of free voxels leads through that wall
    case = sm.case("diagonal_leak")
    free = case["occ"] == 0
    assert int(rm.flood((1, 1, 1), (0, 0, 0), (5, 5, 2), free, 0)[1, 4, 4]) == -1


def test_the_closed_line_is_not_a_chain_of_parents():
    assert probe_gain("parents_differ") == (1, 2, 1) and int(sm.model(sm.case("parents_differ"), "parents")[2]["gain"][0]) == 2


def test_lines_across_word_boundaries_and_walls_at_row_ends():
    rec = rec_of("word_lines")
    assert rec["gain"].tolist() == [2, 2, 2, 2, 2] and rec["ball_gain"].tolist() == [3, 3, 3, 3, 2] and rec["hops"].tolist() == [0] * 5
    case = sm.case("word_lines")
    assert case["grid"][2] == (132, 5, 3) and sorted(int(x) for x in np.nonzero(case["occ"])[2]) == [64, 64, 128, 128]
    # walls at the ends of rows, the starts of the next rows in memory unknown: walls in balls, on no line, nothing hidden
    rec, d = rec_of("row_ends"), details_of("row_ends")
    assert rec["walls"].tolist() == [2, 2] and all(v[1] == v[2] for i in d for v in d[i].values()) and (rec["gain"] == rec["ball_gain"]).all()
    view = sm.case("row_ends")["views"][0]
    assert view[1, 2, 0] and view[2, 0, 0] and sm.case("row_ends")["occ"][1, 1, 69] and sm.case("row_ends")["occ"][1, 2, 69]


def test_the_shortcut_a_wall_in_no_ball_changes_nothing_but_walls():
    goals, mask, rec = sm.expected("far_wall")
    k_goals, k_mask, k_rec = sm.gain_model_of(sm.case("far_wall"))
    assert int(rec["walls"][0]) == 1 and goals.tobytes() == k_goals.tobytes() and mask.tobytes() == k_mask.tobytes()
    assert rec[0].tobytes()[:56] == k_rec[0].tobytes()[:56] and int(rec["ball_gain"][0]) == int(rec["gain"][0]) == 15


def test_all_poor_only_because_of_walls():
    goals, mask, rec = sm.expected("closed_plane_all_poor")
    assert int(rec["flags"][0]) == WANTED | ALL_POOR and int(mask[0]) == 0 and int(rec["poor"][0]) == int(rec["reachable"][0]) == 6
    assert (int(rec["cell"][0]), int(rec["gain"][0]), int(rec["ball_gain"][0]), int(rec["utility"][0]), int(rec["best_gain"][0])) == (-1, -1, -1, 0, 1)
    _, k_mask, k_rec = sm.gain_model_of(sm.case("closed_plane_all_poor"))
    assert int(k_mask[0]) == 1 and int(k_rec["poor"][0]) < 6 and int(k_rec["best_gain"][0]) == 17    # counted through the plane they are not all poor


def test_balls_cut_by_the_box_and_the_three_radii():
    rec = rec_of("box_faces")
    assert rec["flags"].tolist() == [WANTED | FOUND] * 6 and (rec["walls"] > 0).all() and (rec["gain"] <= rec["ball_gain"]).all()
    assert (rec["gain"] < rec["ball_gain"]).sum() >= 4
    d = details_of("box_faces")
    assert all(v[1] <= v[2] for i in d for v in d[i].values()) and sum(v[1] < v[2] for i in d for v in d[i].values()) > 50
    r0, r1, r31 = (rec_of("radius_%d" % g)[0] for g in (0, 1, 31))
    assert (int(r0["gain"]), int(r0["ball_gain"])) == (0, 0) and int(r1["gain"]) == int(r1["ball_gain"]) > 0    # m <= 1: nothing can hide
    assert 0 < int(r31["gain"]) < int(r31["ball_gain"]) and int(r31["walls"]) == int(r0["walls"]) > 100


def test_an_unsearched_vehicle_has_the_fields_of_the_header():
    rec = sm.expected("gain:start_outside")[2]
    out = rec[(rec["flags"] & abi.FH_REACH_START_OUTSIDE) != 0]
    assert len(out) and (out["gain"] == -1).all() and (out["best_gain"] == -1).all() and (out["ball_gain"] == -1).all()
    assert not out["utility"].any() and not out["poor"].any() and not out["walls"].any()


@pytest.mark.parametrize("variant", sm.VARIANTS)
def test_every_wrong_variant_changes_a_named_case(variant):
    told = []
    for name in sm.CASES:
        if variant == "parents" and name in sm.LARGE:
            continue
        got = sm.model(sm.case(name), variant)
        if any(a.tobytes() != b.tobytes() for a, b in zip(got, sm.expected(name))):
            told.append(name)
    assert told, variant
    assert len(sm.VARIANTS) >= 10


def test_reduction_a_without_a_wall_the_model_of_the_gain_chooser():
    free = [k for k in sm.GAIN_CASES if sm.wall_free(k)]
    assert len(sm.GAIN_CASES) == 32 and len(free) == 22
    rest = [k.split(":", 1)[1] for k in sm.GAIN_CASES if k not in free]
    assert all(k in rest for k in ("word_edges", "serpentine_dear_hops", "other_lattice"))
    for name in free:
        goals, mask, rec = sm.expected(name)
        k_goals, k_mask, k_rec = gm.expected(name.split(":", 1)[1])
        assert goals.tobytes() == k_goals.tobytes() and mask.tobytes() == k_mask.tobytes(), name
        assert all(rec[i].tobytes()[:56] == k_rec[i].tobytes()[:56] for i in range(len(rec))), name
        assert np.array_equal(rec["ball_gain"], rec["gain"]) and not rec["walls"].any(), name
    # the other ten run against this model alone; with walls the ties and the levels of the gain chooser's cases still decide
    for name in ("gain:ties_hops", "gain:ties_d2", "gain:ties_cell", "gain:many_levels"):
        rec = sm.expected(name)[2]
        assert rec["walls"].all() and (rec["flags"] & FOUND).all(), name
    assert int(sm.expected("gain:many_levels")[2]["levels"][0]) >= 26


@pytest.mark.parametrize("name", sm.REDUCTIONS)
def test_reduction_b_with_radius_0_cost_1_and_no_minimum_the_model_of_reach(name):
    case = sm.case(name)
    assert (int(case["par"]["gain_radius"]), int(case["par"]["hop_cost"]), int(case["par"]["min_gain"])) == (0, 1, 0)
    goals, mask, rec = sm.expected(name)
    k_goals, k_mask, k_rec = rm.expected(name.split(":", 1)[1])
    assert goals.tobytes() == k_goals.tobytes() and mask.tobytes() == k_mask.tobytes()
    assert all(rec[i].tobytes()[:40] == k_rec[i].tobytes()[:40] for i in range(len(rec)))
    found = mask == 1
    assert (rec["gain"][found] == 0).all() and (rec["ball_gain"][found] == 0).all() and np.array_equal(rec["utility"][found], -rec["hops"][found])
    assert (rec["gain"][~found] == -1).all() and (rec["ball_gain"][~found] == -1).all() and not rec["poor"].any()
