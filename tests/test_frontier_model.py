"""The numpy model of include/fasterhip_frontier.h (tests/frontier_model.py) on the CPU: its own invariants, the worked example of the
header's tie rule, and that the inputs of the GPU equality tests tell every deliberately wrong variant from the model — each variant
changes at least one output byte, so a kernel that made that mistake would fail tests/test_gpu_frontier.py."""
import numpy as np
import pytest

import frontier_model as fm
from faster_amd import abi


@pytest.fixture(scope="module")
def case():
    return fm.equality_case(0)


@pytest.fixture(scope="module")
def outputs(case):
    return {name: fm.equality_model(case, par) for name, par in fm.PARAM_SETS.items()}


def _brute_candidates(case, par, i):
    """The candidates of vehicle i, cell by cell in plain Python: (d2, c) of each."""
    (origin, res, dims), veh = case["grid"], case["vehicles"]
    nx, ny, nz = dims
    view = case["views"][case["view_of"][i]]
    p, g = veh["state"]["pos"][i], veh["g_term"][i]
    occ, mo = case["occ"], case["m_origin"]
    out = []
    for iz in range(nz):
        for iy in range(ny):
            for ix in range(nx):
                if view[iz, iy, ix] != 0:
                    continue
                near = [(ix + 1, iy, iz), (ix - 1, iy, iz), (ix, iy + 1, iz), (ix, iy - 1, iz), (ix, iy, iz + 1), (ix, iy, iz - 1)]
                if not any(0 <= a < nx and 0 <= b < ny and 0 <= c < nz and view[c, b, a] != 0 for a, b, c in near):
                    continue
                q = [(k + 0.5) * res + o for k, o in zip((ix, iy, iz), origin)]
                if not float(par["z_lo"]) <= q[2] <= float(par["z_hi"]):
                    continue
                d = [q[k] - float(p[k]) for k in range(3)]
                d2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
                if not d2 < float(par["r_max"]) * float(par["r_max"]):
                    continue
                e = [q[k] - float(g[k]) for k in range(3)]
                if e[0] * e[0] + e[1] * e[1] + e[2] * e[2] < float(par["r_avoid"]) * float(par["r_avoid"]):
                    continue
                f = [int(np.floor((q[k] - mo[k]) / fm.MAP_RES)) for k in range(3)]
                if not all(0 <= f[k] < occ.shape[2 - k] for k in range(3)) or occ[f[2], f[1], f[0]] != 0:
                    continue
                out.append((d2, (iz * ny + iy) * nx + ix))
    return out


@pytest.mark.parametrize("name", ["exact", "wide", "mid"])
def test_the_choice_is_the_smallest_key_among_the_candidates_and_the_count_is_direct(case, outputs, name):
    par = fm.PARAM_SETS[name]
    goals, mask, rec = outputs[name]
    cov = fm.view_coverage(case["flags"], fm.N_VIEWS, fm.STRIDE, fm.DIMS)
    searched = 0
    for i in range(len(rec)):
        if rec["flags"][i] & ~abi.FH_FRONTIER_FOUND != abi.FH_FRONTIER_WANTED:
            assert (mask[i], rec["cell"][i], rec["candidates"][i], rec["d2"][i]) == (0, -1, 0, np.inf)
            assert goals[i].tobytes() == case["vehicles"]["g_term"][i].tobytes()
            continue
        searched += 1
        cand = _brute_candidates(case, par, i)
        assert rec["candidates"][i] == len(cand)                                  # a direct count
        assert cov["frontier"][case["view_of"][i]] >= len(cand)                   # candidates are frontier voxels of that view
        if not cand:
            assert mask[i] == 0 and rec["cell"][i] == -1 and goals[i].tobytes() == case["vehicles"]["g_term"][i].tobytes()
            continue
        key = (float(rec["d2"][i]), int(rec["cell"][i]))
        assert key in cand and key == min(cand)                                   # a candidate, and none has a smaller key
        assert mask[i] == 1 and rec["flags"][i] == abi.FH_FRONTIER_WANTED | abi.FH_FRONTIER_FOUND
        c = key[1]
        ix, iy, iz = c % fm.DIMS[0], (c // fm.DIMS[0]) % fm.DIMS[1], c // (fm.DIMS[0] * fm.DIMS[1])
        assert goals[i].tolist() == [(k + 0.5) * fm.RES + o for k, o in zip((ix, iy, iz), fm.ORIGIN)]
    assert searched == 12   # (all but the two that are not finite and the two without a view)


def test_what_the_case_is_built_to_hold(case, outputs):
    """The exact equalities, the ties, the edges and the flags the issue asks for are really in the tables."""
    _, mask, rec = outputs["exact"]
    par = fm.PARAM_SETS["exact"]
    veh = case["vehicles"]
    # vehicle 1: voxel 23 of its row at exactly d2 == r_max^2, voxels 19 and 23 at exactly e2 == r_avoid^2, the row at q.z == z_lo
    q19, q23 = fm._q(19, 3, 1), fm._q(23, 3, 1)
    p, g = veh["state"]["pos"][1], veh["g_term"][1]
    assert float(((q23 - p) ** 2).sum()) == float(par["r_max"]) ** 2 and float(((q19 - g) ** 2).sum()) == float(par["r_avoid"]) ** 2
    assert q19[2] == float(par["z_lo"]) and rec["cell"][1] == (1 * 7 + 3) * 70 + 19 and rec["candidates"][1] == 1
    # vehicle 0 stands on a voxel corner: several candidates tie exactly at the minimum
    ties = [k for k in _brute_candidates(case, fm.PARAM_SETS["wide"], 0) if k[0] == 0.6875]
    assert len(ties) >= 8 and outputs["wide"][2]["cell"][0] == min(ties)[1] == 213 and outputs["wide"][2]["d2"][0] == 0.6875
    # frontier voxels at ix = 0, ix = nx - 1 and the last cell; K is known, at ix = nx - 1, and no frontier voxel
    front = fm.frontier_mask(case["views"][1])
    assert front[1, 1, 0] and front[2, 1, 69] and front[4, 6, 69] and case["views"][1][2, 2, 69] == 0 and not front[2, 2, 69]
    assert case["views"][1][2, 3, 0] != 0                                        # the byte after the end of K's row is unknown
    assert fm.frontier_mask(case["views"][1], "flat_x")[2, 2, 69] and fm.frontier_mask(case["views"][1], "boundary_unknown")[2, 2, 69]
    # flags: a position and a goal that are not finite, a view of -1 and of n_views, and vehicles that are not wanted
    W, F, NV, BP = abi.FH_FRONTIER_WANTED, abi.FH_FRONTIER_FOUND, abi.FH_FRONTIER_NO_VIEW, abi.FH_FRONTIER_BAD_POS
    assert rec["flags"][10:14].tolist() == [W | BP, W | BP, W | NV, W | NV] and rec["view"][12:14].tolist() == [-1, fm.N_VIEWS]
    assert rec["flags"][14:].tolist() == [W, W] and rec["candidates"][14:].tolist() == [0, 0]   # all known, all unknown
    reached = outputs["reached"][2]
    assert [bool(f & W) for f in reached["flags"]] == [s == fm.GOAL_REACHED for s in veh["status"]]
    no_path = outputs["no_path"][2]
    assert [bool(f & W) for f in no_path["flags"]] == [s == fm.NO_PATH for s in veh["stage"]]
    both = outputs["reached_or_no_path"][2]
    assert [bool(f & W) for f in both["flags"]] == [s == fm.GOAL_REACHED or t == fm.NO_PATH for s, t in zip(veh["status"], veh["stage"])]
    assert {(int(s), int(t) == fm.NO_PATH) for s, t in zip(veh["status"], veh["stage"])} >= {(s, b) for s in range(4) for b in (False, True)}
    # the map: a candidate's centre in an occupied cell, a voxel outside the map, an occupied cell next to a free candidate
    wide = fm.PARAM_SETS["wide"]
    ok, _, _ = fm.candidates_of(fm.frontier_mask(case["views"][0]), veh["state"]["pos"][5], veh["g_term"][5], wide, case["grid"], case["occ"],
                                case["m_origin"], fm.MAP_RES)
    free, _, _ = fm.candidates_of(fm.frontier_mask(case["views"][0]), veh["state"]["pos"][5], veh["g_term"][5], wide, case["grid"], case["occ"],
                                  case["m_origin"], fm.MAP_RES, "no_map")
    ox, oy, oz = case["occupied"]
    assert free[oz, oy, ox] and not ok[oz, oy, ox]                               # its centre lies in an occupied cell
    assert free[:, 0, :].any() and not ok[:, 0, :].any()                         # the row iy = 0 is outside the map
    bx, by, bz = case["beside"]
    ok7, _, _ = fm.candidates_of(fm.frontier_mask(case["views"][0]), veh["state"]["pos"][7], veh["g_term"][7], wide, case["grid"], case["occ"],
                                 case["m_origin"], fm.MAP_RES)
    fb = np.floor((fm._q(bx, by, bz) - case["m_origin"]) / fm.MAP_RES).astype(int)
    assert ok7[bz, by, bx] and case["occ"][fb[2], fb[1], fb[0]] == 0 and case["occ"][fb[2], fb[1], fb[0] + 1] != 0   # free, beside an occupied cell


def test_an_all_known_and_an_all_unknown_view_have_no_frontier(case):
    cov = fm.view_coverage(case["flags"], fm.N_VIEWS, fm.STRIDE, fm.DIMS)
    assert (int(cov["known"][2]), int(cov["frontier"][2])) == (fm.CELLS, 0) and (int(cov["known"][3]), int(cov["frontier"][3])) == (0, 0)
    assert cov["frontier"][0] > 0 and cov["frontier"][1] == 14 and cov["known"][1] == 15
    one = fm.view_coverage(np.array([0, 1], dtype=np.uint8), 2, 1, (1, 1, 1))
    assert one.tolist() == [(1, 0), (0, 0)]


def test_the_gap_bytes_are_not_read(case):
    other = fm.equality_case(1)
    assert other["flags"].tobytes() != case["flags"].tobytes()
    for par in fm.PARAM_SETS.values():
        a, b = fm.equality_model(case, par), fm.equality_model(other, par)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert fm.view_coverage(other["flags"], fm.N_VIEWS, fm.STRIDE, fm.DIMS).tobytes() == \
        fm.view_coverage(case["flags"], fm.N_VIEWS, fm.STRIDE, fm.DIMS).tobytes()


@pytest.mark.parametrize("variant", fm.VARIANTS)
def test_the_gpu_inputs_separate_every_wrong_variant_from_the_model(case, outputs, variant):
    changed = []
    for name, par in fm.PARAM_SETS.items():
        got = fm.equality_model(case, par, variant)
        if any(x.tobytes() != y.tobytes() for x, y in zip(got, outputs[name])):
            changed.append(name)
    if variant in ("boundary_unknown", "flat_x"):   # these two change the coverage as well
        assert fm.view_coverage(case["flags"], fm.N_VIEWS, fm.STRIDE, fm.DIMS, variant).tobytes() != \
            fm.view_coverage(case["flags"], fm.N_VIEWS, fm.STRIDE, fm.DIMS).tobytes()
    assert changed, variant


def test_the_header_example_of_the_tie_rule():
    """dims (9, 7, 5), res 0.5, origin (-2, -1.5, 0), a vehicle on the voxel corner (0, 0.5, 1) inside a known ball of radius 1: 24
    candidates, all at d2 = 0.6875 or farther, the choice is cell 30."""
    view = np.ones((5, 7, 9), dtype=np.uint8)
    p = np.array([0.0, 0.5, 1.0])
    for iz in range(5):
        for iy in range(7):
            for ix in range(9):
                d = np.array([(ix + 0.5) * 0.5 - 2.0, (iy + 0.5) * 0.5 - 1.5, (iz + 0.5) * 0.5]) - p
                if d[0] * d[0] + d[1] * d[1] + d[2] * d[2] < 1.0:
                    view[iz, iy, ix] = 0
    veh = np.zeros(1, dtype=abi.vehicle_dtype)
    veh["state"]["pos"][0] = veh["g_term"][0] = p
    par = fm._params(10.0, 0.0, -1.0, 9.0, abi.FH_FRONTIER_WANT_ALL)
    grid = ((-2.0, -1.5, 0.0), 0.5, (9, 7, 5))
    occ = np.zeros((10, 12, 14), dtype=np.uint8)
    goals, mask, rec = fm.frontier_goals(par, grid, view.ravel(), 315, None, 1, veh, occ, np.array([-2.1, -1.7, -0.2]), 0.3)
    assert (int(rec["candidates"][0]), int(rec["cell"][0]), float(rec["d2"][0]), int(mask[0])) == (24, 30, 0.6875, 1)
    assert goals[0].tolist() == [-0.25, 0.25, 0.25]
    larger = fm.frontier_goals(par, grid, view.ravel(), 315, None, 1, veh, occ, np.array([-2.1, -1.7, -0.2]), 0.3, "tie_larger")[2]
    assert int(larger["cell"][0]) > 30 and float(larger["d2"][0]) == 0.6875
