"""fh_sight_goals_device on the device (include/fasterhip_sight.h): every byte of d_goals, d_mask and d_records equal to the Python model
(tests/sight_model.py: the flood of tests/reach_model.py, the ball of tests/gain_model.py and a line per voxel by the closed formula) on
every named case and on every case of the gain chooser — tests/test_sight_model.py shows what each case is for and which wrong
variants they separate — with and without gap bytes in view_stride, into poisoned buffers with guards; reduction A against what
fh_gain_goals_device itself writes, reduction B against fh_reach_goals_device itself; and a fleet beside a hole before a wall, which
explore_gain() sends to the hole and explore_sight() to the open edge."""
import numpy as np
import pytest

from faster_amd import abi, capi

import frontier_model as fm
import gain_model as gm
import heading_model as hm
import reach_model as rm
import sight_model as sm
from test_gpu_fleet import P, fleet_params
from test_gpu_gain import device_gain
from test_gpu_reach import GUARD, POISON, dev, device_reach, grid_record, map_bits

pytestmark = pytest.mark.gpu

WANTED, FOUND = abi.FH_FRONTIER_WANTED, abi.FH_FRONTIER_FOUND


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch  # noqa: F401  (torch before the HIP library: one HIP runtime in the process)


def device_sight(case, par=None):
    """fh_sight_goals_device on device copies of the case's tables, the map's bits packed from its occupancy, into poisoned outputs
    with guard bytes on both sides.  A measurement: the inputs and the guards must have the bytes they had."""
    import torch

    veh, view_of = case["vehicles"], case["view_of"]
    n = len(veh)
    par = np.ascontiguousarray(case["par"] if par is None else par).reshape(1)
    assert par.dtype == abi.sight_params_dtype
    bits = map_bits(case["occ"])
    d_f, d_v, d_b = dev(case["flags"]), dev(veh), dev(bits)
    d_vo = None if view_of is None else dev(view_of)
    mz, my, mx = case["occ"].shape
    mg, g = grid_record(case["m_origin"], case["m_res"], (mx, my, mz)), grid_record(*case["grid"])
    sizes = (24 * n, 4 * n, 64 * n)
    outs = [torch.full((s + 2 * GUARD,), POISON, dtype=torch.uint8, device="cuda:0") for s in sizes]
    torch.cuda.synchronize()
    rc = capi.lib().fh_sight_goals_device(None, abi.ptr(par), abi.ptr(mg), d_b.data_ptr(), abi.ptr(g), d_f.data_ptr(), case["stride"],
                                          None if d_vo is None else d_vo.data_ptr(), case["n_views"], d_v.data_ptr(), n,
                                          *(o.data_ptr() + GUARD for o in outs))
    assert rc == 0
    torch.cuda.synchronize()
    host = [o.cpu().numpy() for o in outs]
    for h, s in zip(host, sizes):
        assert (h[:GUARD] == POISON).all() and (h[GUARD + s:] == POISON).all()
    assert d_f.cpu().numpy().tobytes() == case["flags"].tobytes() and d_v.cpu().numpy().tobytes() == veh.tobytes()
    assert d_b.cpu().numpy().tobytes() == bits.tobytes()
    goals = host[0][GUARD:GUARD + sizes[0]].view(np.float64).reshape(n, 3).copy()
    mask = host[1][GUARD:GUARD + sizes[1]].view(np.int32).copy()
    rec = host[2][GUARD:GUARD + sizes[2]].view(abi.sight_record_dtype).copy()
    return goals, mask, rec


def same(got, want, what):
    for name, g, w in zip(("goals", "mask", "records"), got, want):
        assert g.tobytes() == w.tobytes(), (what, name, np.nonzero(got[2] != want[2])[0].tolist(), got[2], want[2])


# ---- 1. every byte equal to the model ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gap", ("packed", "gap"))
@pytest.mark.parametrize("name", list(sm.CASES) + sm.GAIN_CASES)
def test_goals_mask_and_records_equal_the_model(name, gap):
    case = sm.case(name)
    case = gm.packed(case) if gap == "packed" else rm.with_gap(case, 1)   # (the model of the case as built: the gap bytes are never read)
    assert (case["stride"] == case["cells"]) == (gap == "packed")
    got = device_sight(case)
    same(got, sm.expected(name), name)
    idle = np.nonzero(got[1] == 0)[0]
    assert got[0][idle].tobytes() == case["vehicles"]["g_term"][idle].tobytes()   # not chosen: the bits of g_term, NaN and infinity included


def test_two_runs_give_the_same_bytes():
    for name in ("box_faces", "radius_31", "gain:many_levels"):
        same(device_sight(sm.case(name)), device_sight(sm.case(name)), name)


# ---- 2. reduction A: without a wall, what fh_gain_goals_device itself writes -------------------------------------------------------------------
@pytest.mark.parametrize("name", list(gm.CASES))
def test_without_a_wall_in_the_box_the_bytes_of_the_gain_chooser(name):
    """On the same tables: for every searched vehicle without a wall in its box the goal, the mask and bytes 0 .. 55 of the record are
    those fh_gain_goals_device writes, and ball_gain == gain.  22 of the 32 cases have no wall at all (tests/test_sight_model.py counts
    them); in the others the vehicles without one are compared, and those that are not searched."""
    case = gm.case(name)
    goals, mask, rec = device_sight(sm.case("gain:" + name))
    k_goals, k_mask, k_rec = device_gain(case)
    free = rec["walls"] == 0
    assert free.all() == sm.wall_free("gain:" + name)
    assert goals[free].tobytes() == k_goals[free].tobytes() and mask[free].tobytes() == k_mask[free].tobytes()
    assert all(rec[i].tobytes()[:56] == k_rec[i].tobytes()[:56] for i in np.nonzero(free)[0])
    assert np.array_equal(rec["ball_gain"][free], rec["gain"][free])


# ---- 3. reduction B: g = 0, hop_cost = 1, min_gain = 0 against fh_reach_goals_device itself ------------------------------------------------------
@pytest.mark.parametrize("name", sm.REDUCTIONS)
def test_the_reduction_equals_what_fh_reach_goals_device_returns(name):
    reach_case = rm.case(name.split(":", 1)[1])
    case = sm.case(name)
    assert case["flags"] is reach_case["flags"] and case["vehicles"] is reach_case["vehicles"]
    par = case["par"]
    assert (int(par["gain_radius"]), int(par["hop_cost"]), int(par["min_gain"])) == (0, 1, 0)
    assert par.tobytes()[:40] == reach_case["par"].tobytes()[:40]
    goals, mask, rec = device_sight(case)
    same((goals, mask, rec), sm.expected(name), name)
    k_goals, k_mask, k_rec = device_reach(reach_case)
    assert goals.tobytes() == k_goals.tobytes() and mask.tobytes() == k_mask.tobytes()
    assert all(rec[i].tobytes()[:40] == k_rec[i].tobytes()[:40] for i in range(len(rec)))
    found = mask == 1
    assert (rec["gain"][found] == 0).all() and (rec["ball_gain"][found] == 0).all() and np.array_equal(rec["utility"][found], -rec["hops"][found])
    assert (rec["gain"][~found] == -1).all() and (rec["ball_gain"][~found] == -1).all() and not rec["utility"][~found].any() and not rec["poor"].any()


# ---- 4. a fleet beside a hole before a wall ----------------------------------------------------------------------------------------------------
CELLS, CENTER, R_MAX, Z = (40, 40, 15), (4.0, 4.0, 1.5), 6.0, (0.6, 1.4)
HERE, HOLE, PLANE_X, EDGE_X = (14, 10, 5), (10, 10, 5), 8, 25   # vehicle 0; the unknown voxel; the known, occupied plane; the unknown plane
G = 5                                                            # a sensor of 1 m on a lattice of 0.2 m


def wall_scene():
    """8 m x 8 m x 2.8 m, res 0.2, no inflation.  The cloud: a point in every cell of the plane x == PLANE_X, and two far points.  Vehicle 0
    knows everything but HOLE, the slab behind the plane (x < PLANE_X) and the plane x == EDGE_X, the open edge; vehicle 1 knows a ball
    of 1.5 m around itself."""
    res = P["res"]
    _, origin, dims = fm.map_read(np.zeros((0, 3)), CELLS, res, CENTER, 0.0, P["z_max"])
    q = lambda c: np.array([(c[k] + 0.5) * res + origin[k] for k in range(3)])   # noqa: E731
    cloud = np.array([q((PLANE_X, y, z)) for z in range(dims[2]) for y in range(dims[1])] + [q((38, 1, 12)), q((38, 2, 12))])
    starts = np.array([q(HERE), q((30, 30, 5))])
    goals = starts + np.array([0.0, 2.0, 0.0])
    iz, iy, ix = np.meshgrid(np.arange(dims[2]), np.arange(dims[1]), np.arange(dims[0]), indexing="ij")
    centres = np.stack([(ix + 0.5) * res + origin[0], (iy + 0.5) * res + origin[1], (iz + 0.5) * res + origin[2]], axis=-1)
    views = np.ones((2, dims[2], dims[1], dims[0]), dtype=np.uint8)
    views[0][:, :, PLANE_X:] = 0
    views[0][:, :, EDGE_X] = 1
    views[0][HOLE[2], HOLE[1], HOLE[0]] = 1
    views[1][np.linalg.norm(centres - starts[1], axis=-1) < 1.5] = 0
    return {"cloud": cloud, "starts": starts, "goals": goals, "dims": [int(d) for d in dims], "origin": np.array(origin, dtype=np.float64),
            "views": views.reshape(2, -1)}


def wall_fleet(sc):
    from faster_amd.fleet import Fleet

    fl = Fleet(2, fleet_params(), n_seg=P["N"], max_poly=P["max_poly"], dc=P["dc"], v_max=P["v_max"], a_max=P["a_max"], j_max=P["j_max"],
               decomp_radius=P["decomp_radius"], dist_max_vertexes=P["dist_max_vertexes"])
    fl.set_map(sc["cloud"], CELLS, P["res"], CENTER, P["z_max"], 0.0)
    fl.init(sc["starts"], sc["goals"])
    fl.set_unknown_views(sc["views"].copy(), origin=sc["origin"], res=P["res"], dims=sc["dims"])
    return fl


def test_a_vehicle_beside_a_hole_before_a_wall_is_sent_there_by_explore_gain_and_to_the_open_edge_by_explore_sight():
    sc = wall_scene()
    dims = sc["dims"]
    near = rm.cell_index((HOLE[0] - 1, HOLE[1], HOLE[2]), dims)     # between the plane and the hole
    K, R = wall_fleet(sc), wall_fleet(sc)
    try:
        m_dims, m_origin = R.map.dims()
        assert [int(d) for d in m_dims] == dims and np.array_equal(m_origin, sc["origin"])
        occ = R.map.occupancy()
        assert (occ[:, :, PLANE_X] != 0).all() and not occ[:, :, PLANE_X + 1:EDGE_X + 2].any() and not occ[:, :, :PLANE_X].any()
        with pytest.raises(capi.FasterHipError):
            R.sight_records()                                      # nothing to read before the first explore_sight
        with pytest.raises(capi.FasterHipError):
            R.explore_sight(R_MAX, G)                              # "reached" needs enable_heading
        assert [name for name, _ in R.explore_sight_stages(R_MAX, G, want="all")] == ["sight_goals", "set_goals"]
        before = R.vehicles()
        assert before.tobytes() == K.vehicles().tobytes()
        views = R.views().reshape(2, -1)
        grid = (tuple(float(o) for o in sc["origin"]), P["res"], tuple(dims))
        # explore_gain: the slab behind the plane is in the ball of the voxel by the hole, and that voxel is the choice
        K.explore_gain(R_MAX, G, z=Z, want="all")
        k_rec, k_goals, k_mask = K.gain_records()
        assert int(k_rec["cell"][0]) == near and int(k_mask[0]) == 1 and int(k_rec["gain"][0]) > 100
        # explore_sight with the same parameters: the model's record and goal, a voxel at the open edge, which sees all of its ball
        R.explore_sight(R_MAX, G, z=Z, want="all")
        rec, goals, mask = R.sight_records()
        par = sm.sight_params(R_MAX, G, 1, 0, float(R.params["goal_radius"]), Z[0], Z[1], abi.FH_FRONTIER_WANT_ALL)
        det = {}
        want = sm.sight_goals(par, grid, views.reshape(-1), views.shape[1], None, 2, before, occ, sc["origin"], P["res"], details=det)
        same((goals, mask, rec), want, "Fleet.explore_sight")
        assert np.array_equal(R.views().reshape(2, -1), views)    # the views are only read
        assert mask.tolist() == [1, 1] and int(rec["cell"][0]) == rm.cell_index((EDGE_X - 1, HERE[1], HERE[2]), dims)
        assert int(rec["gain"][0]) == int(rec["ball_gain"][0]) == int(rec["best_gain"][0]) and int(rec["walls"][0]) >= dims[1] * dims[2] - 40
        assert det[0][near][1] == 1 and det[0][near][2] == int(k_rec["gain"][0])      # the voxel by the hole sees the hole, whatever its ball holds
        assert np.array_equal(rec["candidates"], k_rec["candidates"]) and np.array_equal(rec["reachable"], k_rec["reachable"])
        assert R.vehicles().tobytes() == hm.set_goals(before, goals, mask, P["wd"]).tobytes()
        R.replan()
        after = R.vehicles()
        assert (after["stage"] != abi.FH_FLEET_STAGE_NO_PATH).all() and (after["active"] == 1).all()
        # min_gain reaches the kernel and is judged on what is seen: above every gain nothing is chosen
        R.explore_sight(R_MAX, G, min_gain=60000, z=Z, want="all")
        rec3, _, mask3 = R.sight_records()
        assert mask3.tolist() == [0, 0] and (rec3["flags"] == WANTED | abi.FH_SIGHT_ALL_POOR).all() and np.array_equal(rec3["poor"], rec3["reachable"])
    finally:
        K.close()
        R.close()
