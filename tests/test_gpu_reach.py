"""fh_reach_goals_device on the device (include/fasterhip_reach.h): every byte of d_goals, d_mask and d_records equal to the Python
model (tests/reach_model.py, a queue over voxels) on every named case — tests/test_reach_model.py shows what each case is for and which
wrong variants they separate — and on the tables of the frontier tests; the candidates against the kernel of
fh_map_frontier_goals_device; the composition with fh_fleet_set_goals_device; and a fleet beside a sealed pocket, which explore() sends
into NO_PATH and explore_reachable() does not."""
import numpy as np
import pytest

from faster_amd import abi, capi

import frontier_model as fm
import heading_model as hm
import reach_model as rm
from test_gpu_fleet import P, fleet_params

pytestmark = pytest.mark.gpu

GUARD, POISON = 64, 0xA5
WANTED, FOUND = abi.FH_FRONTIER_WANTED, abi.FH_FRONTIER_FOUND


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch  # noqa: F401  (torch before the HIP library: one HIP runtime in the process)


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


def map_bits(occ):
    """[mz][my][mx] -> the words of fh_map_occupancy_bits_device: cell (x, y, z) = bit ((z my + y) mx + x) & 31 of word ... >> 5."""
    bits = np.packbits(np.asarray(occ).ravel() != 0, bitorder="little")
    return np.concatenate([bits, np.zeros(-len(bits) % 4, dtype=np.uint8)]).view(np.uint32)


def grid_record(origin, res, dims):
    g = np.zeros(1, dtype=abi.voxel_grid_dtype)
    g["origin"], g["res"], g["dims"] = origin, res, dims
    return g


def device_reach(case, par=None, n=None):
    """fh_reach_goals_device on device copies of the case's tables, the map's bits packed from its occupancy, into poisoned outputs
    with guard bytes on both sides.  A measurement: the inputs and the guards must have the bytes they had."""
    import torch

    veh = case["vehicles"] if n is None else case["vehicles"][:n]
    view_of = case["view_of"] if n is None or case["view_of"] is None else case["view_of"][:n]
    n = len(veh)
    par = np.ascontiguousarray(case["par"] if par is None else par).reshape(1)
    bits = map_bits(case["occ"])
    d_f, d_v, d_b = dev(case["flags"]), dev(veh), dev(bits)
    d_vo = None if view_of is None else dev(view_of)
    mz, my, mx = case["occ"].shape
    mg, g = grid_record(case["m_origin"], case["m_res"], (mx, my, mz)), grid_record(*case["grid"])
    sizes = (24 * n, 4 * n, 48 * n)
    outs = [torch.full((s + 2 * GUARD,), POISON, dtype=torch.uint8, device="cuda:0") for s in sizes]
    torch.cuda.synchronize()
    rc = capi.lib().fh_reach_goals_device(None, abi.ptr(par), abi.ptr(mg), d_b.data_ptr(), abi.ptr(g), d_f.data_ptr(), case["stride"],
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
    rec = host[2][GUARD:GUARD + sizes[2]].view(abi.reach_record_dtype).copy()
    return goals, mask, rec


def same(got, want, what):
    for name, g, w in zip(("goals", "mask", "records"), got, want):
        assert g.tobytes() == w.tobytes(), (what, name, np.nonzero(got[2] != want[2])[0].tolist(), got[2], want[2])


# ---- 1. every byte equal to the model ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gap", (0, 1))
@pytest.mark.parametrize("name", rm.ALL_CASES)
def test_goals_mask_and_records_equal_the_model(name, gap):
    case = rm.case(name)
    if gap:
        case = rm.equality_as_case(name.split(":", 1)[1], gap) if name.startswith("equality:") else rm.with_gap(case, gap)
    got = device_reach(case)
    same(got, rm.expected(name), name)   # (the model of the tables with gap 0: the gap bytes are never read)
    idle = np.nonzero(got[1] == 0)[0]
    assert got[0][idle].tobytes() == case["vehicles"]["g_term"][idle].tobytes()   # not chosen: the bits of g_term, NaN and infinity included


def test_two_runs_give_the_same_bytes_and_a_sub_fleet_has_the_records_of_the_fleet():
    case = rm.case("equality:wide")
    a, b = device_reach(case), device_reach(case)
    same(a, b, "second run")
    for n in (1, 7):
        same(device_reach(case, n=n), tuple(x[:n] for x in a), "sub-fleet of %d" % n)
    case = rm.case("shared_view")
    a = device_reach(case)
    same(device_reach(case, n=3), tuple(x[:3] for x in a), "sub-fleet of shared_view")


def test_max_hops_far_above_the_last_level_changes_nothing():
    case = rm.case("serpentine")
    par = case["par"].copy()
    par["max_hops"] = (1 << 31) - 1
    same(device_reach(case, par=par), rm.expected("serpentine"), "max_hops 2^31 - 1")


# ---- 2. against the kernel of fh_map_frontier_goals_device -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vmap():
    """The map of the frontier equality tests, read once."""
    eq = fm.equality_case(0)
    m = capi.Map(0)
    m.read(eq["cloud"], fm.MAP_CELLS, fm.MAP_RES, fm.MAP_CENTER, fm.MAP_Z[0], fm.MAP_Z[1], 0.0)
    dims, origin = m.dims()
    assert tuple(int(d) for d in dims) == eq["m_dims"] and np.array_equal(origin, eq["m_origin"])
    yield m
    m.close()


@pytest.mark.parametrize("name", list(fm.PARAM_SETS))
def test_candidates_and_flags_are_those_of_the_frontier_kernel(vmap, name):
    """Map.reach_goals_device (the map's own lattice and bits) beside Map.frontier_goals_device on the same device tables: the flags the
    two share on every vehicle, the candidates of every vehicle that the flood searches, and the whole of it equal to the model."""
    import torch

    case = rm.case("equality:" + name)
    n = len(case["vehicles"])
    d_f, d_v, d_vo = dev(case["flags"]), dev(case["vehicles"]), dev(case["view_of"])
    d_g, d_m = torch.zeros((n, 3), dtype=torch.float64, device="cuda:0"), torch.zeros(n, dtype=torch.int32, device="cuda:0")
    d_r, d_k = torch.zeros(n * 48, dtype=torch.uint8, device="cuda:0"), torch.zeros(n * 32, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    vmap.frontier_goals_device(fm.PARAM_SETS[name], case["grid"], d_f.data_ptr(), fm.STRIDE, d_vo.data_ptr(), fm.N_VIEWS, d_v.data_ptr(), n,
                               d_g.data_ptr(), d_m.data_ptr(), d_k.data_ptr())
    vmap.sync()
    k_rec = d_k.cpu().numpy().view(abi.frontier_record_dtype).copy()
    vmap.reach_goals_device(case["par"], case["grid"], d_f.data_ptr(), fm.STRIDE, d_vo.data_ptr(), fm.N_VIEWS, d_v.data_ptr(), n, d_g.data_ptr(),
                            d_m.data_ptr(), d_r.data_ptr(), None)
    torch.cuda.synchronize()
    rec = d_r.cpu().numpy().view(abi.reach_record_dtype).copy()
    same((d_g.cpu().numpy(), d_m.cpu().numpy(), rec), rm.expected("equality:" + name), name)
    shared = WANTED | abi.FH_FRONTIER_NO_VIEW | abi.FH_FRONTIER_BAD_POS
    assert np.array_equal(rec["flags"] & shared, k_rec["flags"] & shared) and np.array_equal(rec["view"], k_rec["view"])
    searched = (rec["flags"] & ~(FOUND | abi.FH_REACH_CUT)) == WANTED
    assert np.array_equal(rec["candidates"][searched], k_rec["candidates"][searched])
    # a vehicle the frontier kernel does not search is not searched here either; the others that are not have their start outside
    assert not searched[(k_rec["flags"] & ~FOUND) != WANTED].any()
    extra = ~searched & ((k_rec["flags"] & ~FOUND) == WANTED)
    assert ((rec["flags"][extra] & abi.FH_REACH_START_OUTSIDE) != 0).all()
    with pytest.raises(capi.FasterHipError):
        vmap.reach_goals_device(fm.PARAM_SETS[name], case["grid"], d_f.data_ptr(), fm.STRIDE, d_vo.data_ptr(), fm.N_VIEWS, d_v.data_ptr(), n,
                                d_g.data_ptr(), d_m.data_ptr(), d_r.data_ptr(), None)   # a frontier record is not a reach record


# ---- 3. composition ----------------------------------------------------------------------------------------------------------------------------
def test_reach_goals_then_set_goals_is_the_model_then_set_terminal_goal():
    import torch

    fpar = fleet_params()
    ctx = capi.Context(0)
    try:
        for name in ("wide", "reached", "mid"):
            case = dict(rm.case("equality:" + name))
            veh = case["vehicles"].copy()
            veh["plan_size"], veh["active"] = 1, 1
            veh["state"]["pos"][10] = (4.0, 0.5, 1.0)   # (set_goals projects from the state: no NaN in this one; g_term of 11 stays infinite)
            case["vehicles"] = veh
            n = len(veh)
            goals, mask, _ = rm.model(case)
            got = device_reach(case)
            same(got[:2], (goals, mask), name)
            d_v, d_g, d_m = dev(veh), dev(got[0]), dev(got[1])
            torch.cuda.synchronize()
            ctx.fleet_set_goals_device(fpar, d_v.data_ptr(), d_g.data_ptr(), d_m.data_ptr(), n)
            ctx.sync()
            after = d_v.cpu().numpy().view(abi.vehicle_dtype)
            want = hm.set_goals(veh, goals, mask, P["wd"])
            assert after.tobytes() == want.tobytes(), (name, np.nonzero(after["status"] != want["status"])[0])
            assert mask.any() and not mask.all()
            moved = mask.astype(bool)
            assert np.array_equal(after["g_term"][moved], goals[moved]) and after[~moved].tobytes() == veh[~moved].tobytes()
    finally:
        ctx.close()


# ---- 4. a fleet beside a sealed pocket ---------------------------------------------------------------------------------------------------------
POCKET_CELLS, POCKET_CENTER, POCKET_R, POCKET_Z = (40, 40, 15), (4.0, 4.0, 1.5), 6.0, (0.6, 1.4)
HERE, POCKET = (10, 10, 5), (14, 10, 5)   # the voxel vehicle 0 stands in; the middle of the pocket, four voxels (0.8 m) away


def pocket_scene():
    """8 m x 8 m x 2.8 m, res 0.2, no inflation.  A shell of occupied cells, one cell thick, at Chebyshev distance 2 from POCKET encloses
    3 x 3 x 3 free voxels.  Vehicle 0 knows a ball of 1.5 m around itself, which holds the pocket, but not the voxel beyond POCKET: that
    makes POCKET a frontier voxel at 0.8 m, nearer than the surface of the ball.  Vehicle 1 stands in the open, with a ball of its own."""
    res = P["res"]
    _, origin, dims = fm.map_read(np.zeros((0, 3)), POCKET_CELLS, res, POCKET_CENTER, 0.0, P["z_max"])
    q = lambda c: np.array([(c[k] + 0.5) * res + origin[k] for k in range(3)])   # noqa: E731
    shell = [(POCKET[0] + a, POCKET[1] + b, POCKET[2] + c) for a in range(-2, 3) for b in range(-2, 3) for c in range(-2, 3)
             if max(abs(a), abs(b), abs(c)) == 2]
    cloud = np.array([q(c) for c in shell])
    starts = np.array([q(HERE), q((30, 30, 5))])
    goals = starts + np.array([0.0, 2.0, 0.0])
    iz, iy, ix = np.meshgrid(np.arange(dims[2]), np.arange(dims[1]), np.arange(dims[0]), indexing="ij")
    centres = np.stack([(ix + 0.5) * res + origin[0], (iy + 0.5) * res + origin[1], (iz + 0.5) * res + origin[2]], axis=-1)
    views = np.ones((2, dims[2], dims[1], dims[0]), dtype=np.uint8)
    for i, s in enumerate(starts):
        views[i][np.linalg.norm(centres - s, axis=-1) < 1.5] = 0
    views[0][POCKET[2], POCKET[1], POCKET[0] + 1] = 1
    return {"cloud": cloud, "starts": starts, "goals": goals, "dims": [int(d) for d in dims], "origin": np.array(origin, dtype=np.float64),
            "views": views.reshape(2, -1), "shell": shell}


def pocket_fleet(sc):
    from faster_amd.fleet import Fleet

    fl = Fleet(2, fleet_params(), n_seg=P["N"], max_poly=P["max_poly"], dc=P["dc"], v_max=P["v_max"], a_max=P["a_max"], j_max=P["j_max"],
               decomp_radius=P["decomp_radius"], dist_max_vertexes=P["dist_max_vertexes"])
    fl.set_map(sc["cloud"], POCKET_CELLS, P["res"], POCKET_CENTER, P["z_max"], 0.0)
    fl.init(sc["starts"], sc["goals"])
    fl.set_unknown_views(sc["views"].copy(), origin=sc["origin"], res=P["res"], dims=sc["dims"])
    return fl


def test_a_vehicle_beside_a_sealed_pocket_is_sent_into_no_path_by_explore_and_not_by_explore_reachable():
    sc = pocket_scene()
    dims = sc["dims"]
    pocket = rm.cell_index(POCKET, dims)
    K, R = pocket_fleet(sc), pocket_fleet(sc)
    try:
        m_dims, m_origin = R.map.dims()
        assert [int(d) for d in m_dims] == dims and np.array_equal(m_origin, sc["origin"])
        occ = R.map.occupancy()
        assert int((occ != 0).sum()) == len(sc["shell"]) == 98 and occ[POCKET[2], POCKET[1], POCKET[0]] == 0
        with pytest.raises(capi.FasterHipError):
            R.reach_records()                                      # nothing to read before the first explore_reachable
        with pytest.raises(capi.FasterHipError):
            R.explore_reachable(POCKET_R)                          # "reached" needs enable_heading
        assert [name for name, _ in R.explore_reachable_stages(POCKET_R, want="all")] == ["reach_goals", "set_goals"]
        before = R.vehicles()
        assert before.tobytes() == K.vehicles().tobytes()
        views = R.views().reshape(2, -1)
        # explore: the nearest frontier voxel is the middle of the pocket, and the replan finds no path to it
        K.explore(POCKET_R, z=POCKET_Z, want="all")
        k_rec, _, k_mask = K.explore_records()
        assert int(k_rec["cell"][0]) == pocket and int(k_mask[0]) == 1 and abs(float(k_rec["d2"][0]) - 0.64) < 1e-9
        K.replan()
        k_after = K.vehicles()
        assert int(k_after["stage"][0]) == abi.FH_FLEET_STAGE_NO_PATH and int(k_after["stage"][1]) != abi.FH_FLEET_STAGE_NO_PATH
        # explore_reachable: the model's record and goal, another voxel, and the replan does not end in NO_PATH
        R.explore_reachable(POCKET_R, z=POCKET_Z, want="all")
        rec, goals, mask = R.reach_records()
        par = rm.reach_params(POCKET_R, float(R.params["goal_radius"]), POCKET_Z[0], POCKET_Z[1], abi.FH_FRONTIER_WANT_ALL)
        grid = (tuple(float(o) for o in sc["origin"]), P["res"], tuple(dims))
        want = rm.reach_goals(par, grid, views.reshape(-1), views.shape[1], None, 2, before, occ, sc["origin"], P["res"])
        same((goals, mask, rec), want, "Fleet.explore_reachable")
        assert np.array_equal(R.views().reshape(2, -1), views)    # the views are only read
        assert mask.tolist() == [1, 1] and int(rec["cell"][0]) != pocket and int(rec["hops"][0]) > 4
        assert int(rec["candidates"][0]) == int(k_rec["candidates"][0]) and int(rec["candidates"][0]) - int(rec["reachable"][0]) >= 1
        assert R.vehicles().tobytes() == hm.set_goals(before, goals, mask, P["wd"]).tobytes()
        R.replan()
        after = R.vehicles()
        assert (after["stage"] != abi.FH_FLEET_STAGE_NO_PATH).all() and (after["active"] == 1).all()
        # max_hops reaches the kernel: a flood of two levels finds nothing for vehicle 0 and says that it was cut
        R.explore_reachable(POCKET_R, z=POCKET_Z, want="all", max_hops=2)
        rec2, _, mask2 = R.reach_records()
        assert int(rec2["levels"][0]) == 2 and int(rec2["flags"][0]) == WANTED | abi.FH_REACH_CUT and int(mask2[0]) == 0
    finally:
        K.close()
        R.close()
