"""The frontier entry points on the device (include/fasterhip_frontier.h): every clause of both prologues on a real map; every byte of
d_goals, d_mask and d_records equal to the numpy model (tests/frontier_model.py) on tables built to hold every edge the model names
(tests/test_frontier_model.py shows which wrong variants they separate); coverage against the model; the composition with
fh_fleet_set_goals_device; Fleet.explore against the two calls made by hand; a fleet that never explores; and a closed loop of eight
vehicles that explore an open scene, checked against the model in every period."""
import numpy as np
import pytest

from faster_amd import abi, capi

import frontier_model as fm
import heading_model as hm
from test_gpu_fleet import P, fleet_params

pytestmark = pytest.mark.gpu

OK, ARG = 0, -1
GUARD, POISON = 64, 0xA5
TODAY = ["begin", "path_search", "corridors", "corridor_problems", "whole_solve", "safe_corridor", "safe_solve", "commit"]


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch  # noqa: F401  (torch before the HIP library: one HIP runtime in the process)


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


@pytest.fixture(scope="module")
def case():
    return fm.equality_case(0)


@pytest.fixture(scope="module")
def vmap(case):
    """The map of the equality tests, read once; its lattice and occupancy are what the CPU restatement says."""
    m = capi.Map(0)
    m.read(case["cloud"], fm.MAP_CELLS, fm.MAP_RES, fm.MAP_CENTER, fm.MAP_Z[0], fm.MAP_Z[1], 0.0)
    dims, origin = m.dims()
    assert tuple(int(d) for d in dims) == case["m_dims"] and np.array_equal(origin, case["m_origin"])
    assert np.array_equal(m.occupancy() != 0, case["occ"] != 0) and int((case["occ"] != 0).sum()) == 3
    yield m
    m.close()


def device_goals(m, par, grid, flags, stride, view_of, n_views, veh):
    """fh_map_frontier_goals_device on device copies, into poisoned outputs with guard bytes on both sides.  A measurement: the inputs
    and the guards must have the bytes they had.  -> (goals, mask, records, the device tensors of goals and mask)."""
    import torch

    n = len(veh)
    d_f, d_v = dev(flags), dev(veh)
    d_vo = None if view_of is None else dev(view_of)
    sizes = (24 * n, 4 * n, 32 * n)
    outs = [torch.full((s + 2 * GUARD,), POISON, dtype=torch.uint8, device="cuda:0") for s in sizes]
    torch.cuda.synchronize()
    m.frontier_goals_device(par, grid, d_f.data_ptr(), stride, None if d_vo is None else d_vo.data_ptr(), n_views, d_v.data_ptr(), n,
                            *(o.data_ptr() + GUARD for o in outs))
    m.sync()
    host = [o.cpu().numpy() for o in outs]
    for h, s in zip(host, sizes):
        assert (h[:GUARD] == POISON).all() and (h[GUARD + s:] == POISON).all()
    assert d_f.cpu().numpy().tobytes() == np.ascontiguousarray(flags).tobytes() and d_v.cpu().numpy().tobytes() == veh.tobytes()
    goals = host[0][GUARD:GUARD + sizes[0]].view(np.float64).reshape(n, 3).copy()
    mask = host[1][GUARD:GUARD + sizes[1]].view(np.int32).copy()
    rec = host[2][GUARD:GUARD + sizes[2]].view(abi.frontier_record_dtype).copy()
    return goals, mask, rec


def device_coverage(m, grid, flags, stride, n_views, skew=0):
    """fh_map_view_coverage_device on a device copy that begins `skew` bytes into its allocation (the kernel loads words aligned in
    memory), into a poisoned output with guard bytes on both sides."""
    import torch

    d_f = dev(np.concatenate([np.zeros(skew, dtype=np.uint8), np.asarray(flags, dtype=np.uint8).reshape(-1)]))
    out = torch.full((16 * n_views + 2 * GUARD,), POISON, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    m.view_coverage_device(grid, d_f.data_ptr() + skew, stride, n_views, out.data_ptr() + GUARD)
    m.sync()
    h = out.cpu().numpy()
    assert (h[:GUARD] == POISON).all() and (h[GUARD + 16 * n_views:] == POISON).all()
    return h[GUARD:GUARD + 16 * n_views].view(abi.view_coverage_dtype).copy()


def same(got, want, what):
    for name, g, w in zip(("goals", "mask", "records"), got, want):
        assert g.tobytes() == w.tobytes(), (what, name, np.nonzero(got[2] != want[2])[0].tolist(), got[2], want[2])


# ---- 1. the prologues ------------------------------------------------------------------------------------------------------------------------
def test_every_argument_rule_of_both_prologues_in_order(vmap, case):
    import torch

    L = capi.lib()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    d = buf.data_ptr()
    nan, inf = float("nan"), float("inf")

    def grid(res=0.5, dims=(8, 8, 4)):
        g = np.zeros(1, dtype=abi.voxel_grid_dtype)
        g["origin"], g["res"], g["dims"] = (0.1, 0.2, 0.3), res, dims
        return g

    def par(**kw):
        p = np.ascontiguousarray(abi.default_frontier_params(1.5)).reshape(1).copy()
        for k, v in kw.items():
            p[k] = v
        return p

    def call(m=vmap._h, p=par(), g=grid(), flags=d, stride=256, view_of=None, n_views=2, veh=d, n=1, goals=d + 4096, mask=d + 8192, rec=d + 12288):
        return L.fh_map_frontier_goals_device(m, None if p is None else abi.ptr(p), None if g is None else abi.ptr(g), flags, stride, view_of,
                                              n_views, veh, n, goals, mask, rec)

    fresh = capi.Map(0)   # never read
    try:
        # every later rule broken as well: the earlier one answers, and n == 0 with null pointers does not turn it into FH_OK
        nothing = dict(flags=None, veh=None, goals=None, mask=None, rec=None)
        assert call(m=None) == ARG and call(m=None, n=0, **nothing) == ARG                                       # 1. a null map
        assert call(m=fresh._h) == ARG and call(m=fresh._h, n=0, **nothing) == ARG                               # 2. never read
        assert call(p=None) == ARG and call(p=None, n=0, **nothing) == ARG                                       # 3. no params
        for v in (nan, inf, -inf, 0.0, -0.0, -1.0):                                                              # 4. r_max
            assert call(p=par(r_max=v)) == ARG and call(p=par(r_max=v), n=0, **nothing) == ARG, v
        for v in (nan, inf, -inf, -1e-300, -1.0):                                                                # 5. r_avoid
            assert call(p=par(r_avoid=v)) == ARG and call(p=par(r_avoid=v), n=0, **nothing) == ARG, v
        for lo, hi in ((nan, 1.0), (0.0, nan), (nan, nan), (1.0, 0.5), (inf, -inf)):                             # 6. z
            assert call(p=par(z_lo=lo, z_hi=hi)) == ARG and call(p=par(z_lo=lo, z_hi=hi), n=0, **nothing) == ARG, (lo, hi)
        for v in (0, 8, 9, 16, -1, 1 << 30):                                                                     # 7. want
            assert call(p=par(want=v)) == ARG and call(p=par(want=v), n=0, **nothing) == ARG, v
        assert call(g=None) == ARG and call(g=None, n=0, **nothing) == ARG                                       # 8. the grid
        for res in (0.0, -0.5, nan):
            assert call(g=grid(res=res)) == ARG, res
        for dims in ((0, 8, 4), (8, 0, 4), (8, 8, -1)):
            assert call(g=grid(dims=dims)) == ARG and call(g=grid(dims=dims), n=0, **nothing) == ARG, dims
        for dims in ((1 << 16, 1 << 15, 1), (1 << 16, 1 << 16, 1 << 16), (2, 1 << 30, 1), ((1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1)):
            assert call(g=grid(dims=dims), stride=1 << 62) == ARG, dims                                          # 9. more than 2^31 - 1 cells
        assert call(stride=255) == ARG and call(stride=0) == ARG and call(stride=255, n=0, **nothing) == ARG     # 10. the stride
        assert call(n_views=0) == ARG and call(n_views=-3) == ARG and call(n_views=0, n=0, **nothing) == ARG     # 11. n_views
        assert call(n=-1) == ARG and call(n=-1, **nothing) == ARG                                                # 12. n
        # every rule passes: n == 0 is fine without any pointer, then the pointers
        assert call(n=0, **nothing) == OK and call(n=0) == OK
        for k in nothing:
            assert call(**{k: None}) == ARG, k
        # the edges of the rules that pass (one vehicle, zeroed tables: status TRAVELING, not wanted by the default params)
        assert call() == OK and call(view_of=d + 16384) == OK
        assert call(p=par(r_max=1e-300)) == OK and call(p=par(r_max=1e300)) == OK and call(p=par(r_avoid=0.0)) == OK
        assert call(p=par(z_lo=-inf, z_hi=inf)) == OK and call(p=par(z_lo=1.0, z_hi=1.0)) == OK and call(p=par(z_lo=inf, z_hi=inf)) == OK
        for v in (1, 2, 3, 4, 5, 6, 7):
            assert call(p=par(want=v)) == OK, v
        assert call(stride=256) == OK and call(g=grid(dims=(1, 1, 1)), stride=1) == OK
        vmap.sync()

        def cover(m=vmap._h, g=grid(), flags=d, stride=256, n_views=2, out=d + 4096):
            return L.fh_map_view_coverage_device(m, None if g is None else abi.ptr(g), flags, stride, n_views, out)

        assert cover(m=None) == ARG and cover(m=None, g=None, flags=None, out=None) == ARG
        assert cover(g=None) == ARG and cover(g=None, flags=None, out=None) == ARG
        for dims in ((0, 8, 4), (8, 0, 4), (8, 8, -1)):
            assert cover(g=grid(dims=dims)) == ARG and cover(g=grid(dims=dims), flags=None) == ARG, dims
        assert cover(g=grid(dims=(1 << 16, 1 << 15, 1)), stride=1 << 62) == ARG and cover(g=grid(dims=(1 << 16, 1 << 16, 1 << 16)), stride=1 << 62) == ARG
        assert cover(stride=255) == ARG and cover(stride=255, out=None) == ARG
        assert cover(n_views=0) == ARG and cover(n_views=-1) == ARG and cover(n_views=0, flags=None) == ARG
        assert cover(flags=None) == ARG and cover(out=None) == ARG
        assert cover() == OK and cover(g=grid(res=-1.0)) == OK        # only the dims are read
        assert cover(m=fresh._h) == OK                                 # the map need not have been read
        fresh.sync()
        vmap.sync()
    finally:
        fresh.close()
    assert L.fh_abi_version() == 9


# ---- 2. every byte equal to the model ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gap", (0, 1))
@pytest.mark.parametrize("name", list(fm.PARAM_SETS))
def test_goals_mask_and_records_equal_the_model(vmap, case, name, gap):
    tables = case if gap == 0 else fm.equality_case(gap)
    par = fm.PARAM_SETS[name]
    want = fm.equality_model(case, par)   # (the model of the tables with gap 0: the gap bytes are never read)
    got = device_goals(vmap, par, case["grid"], tables["flags"], fm.STRIDE, case["view_of"], fm.N_VIEWS, case["vehicles"])
    same(got, want, name)
    # not wanted: the goal bytes are those of g_term, NaN and infinity included
    idle = np.nonzero(got[1] == 0)[0]
    assert len(idle) and got[0][idle].tobytes() == case["vehicles"]["g_term"][idle].tobytes()


def test_the_header_example_without_view_of(vmap):
    """dims (9, 7, 5), view_of NULL (view i), two vehicles of which the second stands on the voxel corner of the header's example."""
    view = np.ones((2, 5, 7, 9), dtype=np.uint8)
    p = np.array([0.0, 0.5, 1.0])
    for iz in range(5):
        for iy in range(7):
            for ix in range(9):
                dd = np.array([(ix + 0.5) * 0.5 - 2.0, (iy + 0.5) * 0.5 - 1.5, (iz + 0.5) * 0.5]) - p
                if dd[0] * dd[0] + dd[1] * dd[1] + dd[2] * dd[2] < 1.0:
                    view[1, iz, iy, ix] = 0
    veh = np.zeros(2, dtype=abi.vehicle_dtype)
    veh["state"]["pos"][:] = p
    veh["g_term"][:] = p
    par = fm._params(10.0, 0.0, -1.0, 9.0, abi.FH_FRONTIER_WANT_ALL)
    grid = ((-2.0, -1.5, 0.0), 0.5, (9, 7, 5))
    dims, origin = vmap.dims()
    occ = vmap.occupancy()
    got = device_goals(vmap, par, grid, view.ravel(), 315, None, 2, veh)
    same(got, fm.frontier_goals(par, grid, view.ravel(), 315, None, 2, veh, occ, origin, fm.MAP_RES), "header example")
    assert (int(got[2]["candidates"][0]), int(got[2]["cell"][0])) == (0, -1) and float(got[2]["d2"][1]) == 0.6875 and int(got[1][1]) == 1


def test_two_runs_give_the_same_bytes_and_a_sub_fleet_has_the_records_of_the_fleet(vmap, case):
    par = fm.PARAM_SETS["wide"]
    args = (vmap, par, case["grid"], case["flags"], fm.STRIDE)
    a = device_goals(*args, case["view_of"], fm.N_VIEWS, case["vehicles"])
    b = device_goals(*args, case["view_of"], fm.N_VIEWS, case["vehicles"])
    same(a, b, "second run")
    for n in (1, 7):
        sub = device_goals(*args, case["view_of"][:n], fm.N_VIEWS, case["vehicles"][:n])
        same(sub, tuple(x[:n] for x in a), "sub-fleet of %d" % n)


@pytest.mark.parametrize("gap", (0, 1))
def test_coverage_equals_the_model(vmap, case, gap):
    tables = case if gap == 0 else fm.equality_case(gap)
    want = fm.view_coverage(case["flags"], fm.N_VIEWS, fm.STRIDE, fm.DIMS)
    got = device_coverage(vmap, case["grid"], tables["flags"], fm.STRIDE, fm.N_VIEWS)
    assert got.tobytes() == want.tobytes(), (got, want)
    for skew in (0, 1, 7, 15, 16):   # two runs; and wherever the table begins (the leading bytes are zeros: they would count as known)
        assert got.tobytes() == device_coverage(vmap, case["grid"], tables["flags"], fm.STRIDE, fm.N_VIEWS, skew).tobytes(), skew


def test_coverage_of_a_lattice_of_one_voxel_and_of_more_cells_than_one_launch_of_threads(vmap):
    one = np.array([0, 1, 0], dtype=np.uint8)
    for skew in (0, 14):
        got = device_coverage(vmap, ((0.0, 0.0, 0.0), 1.0, (1, 1, 1)), one, 1, 3, skew)
        assert got.tolist() == [(1, 0), (0, 0), (1, 0)], skew
    # rows shorter than a chunk, a chunk exactly, and one byte more, known and unknown alternating along x: every known voxel is a
    # frontier voxel except where the row has one cell
    for nx in (1, 2, 15, 16, 17, 33):
        row = (np.arange(nx) % 2).astype(np.uint8)
        want = fm.view_coverage(np.concatenate([row, row]), 2, nx, (nx, 1, 1))
        for skew in (0, 3):
            assert device_coverage(vmap, ((0.0, 0.0, 0.0), 1.0, (nx, 1, 1)), np.concatenate([row, row]), nx, 2, skew).tobytes() == want.tobytes(), (nx, skew)
    # 300 x 33 x 9 = 89 100 cells: more than 256 workgroups of 256 threads, so threads take a second cell; random flags, two views
    dims = (300, 33, 9)
    cells = dims[0] * dims[1] * dims[2]
    flags = (np.random.default_rng(8).random(2 * (cells + 5)) < 0.4).astype(np.uint8)
    got = device_coverage(vmap, ((0.0, 0.0, 0.0), 0.2, dims), flags, cells + 5, 2)
    assert got.tobytes() == fm.view_coverage(flags, 2, cells + 5, dims).tobytes()


# ---- 3. composition ----------------------------------------------------------------------------------------------------------------------------
def test_frontier_goals_then_set_goals_is_the_model_then_set_terminal_goal(vmap, case):
    """fh_map_frontier_goals_device followed by fh_fleet_set_goals_device leaves the vehicle array equal to heading_model.set_goals
    applied to the model's goals and mask."""
    import torch

    fpar = fleet_params()
    veh = case["vehicles"].copy()
    veh["plan_size"], veh["active"] = 1, 1
    veh["state"]["pos"][10] = (4.0, 0.5, 1.0)   # (set_goals projects from the state: no NaN in this one; g_term of 11 stays infinite)
    n = len(veh)
    ctx = capi.Context(0)
    try:
        for name in ("wide", "reached", "mid"):
            par = fm.PARAM_SETS[name]
            goals, mask, rec = fm.frontier_goals(par, case["grid"], case["flags"], fm.STRIDE, case["view_of"], fm.N_VIEWS, veh, case["occ"],
                                                 case["m_origin"], fm.MAP_RES)
            d_f, d_v, d_vo = dev(case["flags"]), dev(veh), dev(case["view_of"])
            d_g, d_m, d_r = dev(np.full((n, 3), 7.0)), dev(np.full(n, 7, dtype=np.int32)), dev(np.zeros(n, dtype=abi.frontier_record_dtype))
            torch.cuda.synchronize()
            vmap.frontier_goals_device(par, case["grid"], d_f.data_ptr(), fm.STRIDE, d_vo.data_ptr(), fm.N_VIEWS, d_v.data_ptr(), n, d_g.data_ptr(),
                                       d_m.data_ptr(), d_r.data_ptr())
            vmap.sync()
            assert d_v.cpu().numpy().tobytes() == veh.tobytes()                                  # a pure measurement
            ctx.fleet_set_goals_device(fpar, d_v.data_ptr(), d_g.data_ptr(), d_m.data_ptr(), n)
            ctx.sync()
            got = d_v.cpu().numpy().view(abi.vehicle_dtype)
            want = hm.set_goals(veh, goals, mask, P["wd"])
            assert got.tobytes() == want.tobytes(), (name, np.nonzero(got["status"] != want["status"])[0], got["goal"] - want["goal"])
            assert mask.any() and not mask.all()
            moved = mask.astype(bool)
            assert np.array_equal(got["g_term"][moved], goals[moved]) and got[~moved].tobytes() == veh[~moved].tobytes()
            assert (got["status"][moved & (veh["status"] == hm.GOAL_REACHED)] == hm.YAWING).all()
    finally:
        ctx.close()


# ---- 4. Fleet.explore --------------------------------------------------------------------------------------------------------------------------
SCENE_CELLS, SCENE_CENTER = (80, 80, 15), (8.0, 8.0, 1.5)
R_SENSE, R_EXPLORE, Z_EXPLORE = 2.5, 6.0, (0.6, 1.4)
LOOP_PERIODS, LOOP_TICKS = 12, 60


def open_scene():
    """16 m x 16 m x 3 m with four pillars; eight vehicles in two rows, 5 m apart, whose first goals lie 2 m ahead towards the middle."""
    zs = np.arange(0.05, 3.0, 0.1)
    ring = [(0.15 * np.cos(a), 0.15 * np.sin(a)) for a in np.linspace(0, 2 * np.pi, 8, endpoint=False)]
    cloud = np.array([(cx + dx, cy + dy, z) for cx, cy in ((5.0, 8.0), (11.0, 8.0), (8.0, 3.0), (8.0, 13.0)) for dx, dy in ring for z in zs])
    xs = (3.5, 6.5, 9.5, 12.5)
    starts = np.array([(x, 5.5, 1.0) for x in xs] + [(x, 10.5, 1.0) for x in xs])
    goals = np.array([(x, 7.5, 1.0) for x in xs] + [(x, 8.5, 1.0) for x in xs])
    probe = capi.Map(0)
    probe.read(cloud, SCENE_CELLS, P["res"], SCENE_CENTER, 0.0, P["z_max"], 0.1)
    dims, origin = probe.dims()
    occ = probe.occupancy()
    probe.close()
    dims, origin = [int(d) for d in dims], np.array(origin, dtype=np.float64)
    iz, iy, ix = np.meshgrid(np.arange(dims[2]), np.arange(dims[1]), np.arange(dims[0]), indexing="ij")
    centres = np.stack([(ix + 0.5) * P["res"] + origin[0], (iy + 0.5) * P["res"] + origin[1], (iz + 0.5) * P["res"] + origin[2]], axis=-1)
    views = np.ones((len(starts), dims[2], dims[1], dims[0]), dtype=np.uint8)
    for i, s in enumerate(starts):
        views[i][np.linalg.norm(centres - s, axis=-1) < 1.5] = 0
    return {"cloud": cloud, "starts": starts, "goals": goals, "dims": dims, "origin": origin, "occ": occ, "views": views.reshape(len(starts), -1)}


@pytest.fixture(scope="module")
def scene():
    return open_scene()


def scene_fleet(sc, heading=True):
    from faster_amd.fleet import Fleet

    B = len(sc["starts"])
    fl = Fleet(B, fleet_params(), n_seg=P["N"], max_poly=P["max_poly"], dc=P["dc"], v_max=P["v_max"], a_max=P["a_max"], j_max=P["j_max"],
               decomp_radius=P["decomp_radius"], dist_max_vertexes=P["dist_max_vertexes"])
    fl.set_map(sc["cloud"], SCENE_CELLS, P["res"], SCENE_CENTER, P["z_max"], 0.1)
    fl.init(sc["starts"], sc["goals"])
    fl.set_unknown_views(sc["views"].copy(), origin=sc["origin"], res=P["res"], dims=sc["dims"])
    fl.set_point_views()
    if heading:
        fl.enable_heading()
    return fl


def scene_model(fl, sc, par, veh, views):
    grid = (tuple(float(o) for o in sc["origin"]), P["res"], tuple(sc["dims"]))
    return fm.frontier_goals(par, grid, views.reshape(-1), views.shape[1], None, len(veh), veh, sc["occ"], sc["origin"], P["res"])


def explore_params(fl, want):
    par = abi.default_frontier_params(R_EXPLORE)
    par["r_avoid"], par["z_lo"], par["z_hi"], par["want"] = float(fl.params["goal_radius"]), Z_EXPLORE[0], Z_EXPLORE[1], want
    return par


def test_fleet_explore_equals_the_two_calls_made_by_hand_and_the_model(scene):
    import torch

    sc = scene
    fl = scene_fleet(sc, heading=False)
    B = fl.n
    try:
        with pytest.raises(capi.FasterHipError):
            fl.explore(R_EXPLORE)                                  # "reached" needs enable_heading
        assert [name for name, _ in fl.explore_stages(R_EXPLORE, want="all")] == ["frontier_goals", "set_goals"]
        fl.sense(R_SENSE)
        fl.observe()
        before = fl.vehicles()                                     # (synchronises)
        views = fl.views().reshape(B, -1)
        d_copy = fl.d_vehicles.clone()
        fl.explore(R_EXPLORE, z=Z_EXPLORE, want="all")
        rec, goals, mask = fl.explore_records()
        after = fl.vehicles()
        assert np.array_equal(fl.views().reshape(B, -1), views)    # the views are only read
        par = explore_params(fl, abi.FH_FRONTIER_WANT_ALL)
        want = scene_model(fl, sc, par, before, views)
        same((goals, mask, rec), want, "Fleet.explore")
        assert mask.all() and (rec["candidates"] > 0).all()
        assert after.tobytes() == hm.set_goals(before, goals, mask, P["wd"]).tobytes()
        # by hand, on a copy of the vehicles, into buffers of the test
        d_g, d_m = torch.zeros((B, 3), dtype=torch.float64, device="cuda:0"), torch.zeros(B, dtype=torch.int32, device="cuda:0")
        d_r = torch.zeros(B * 32, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        grid = (tuple(float(o) for o in sc["origin"]), P["res"], tuple(sc["dims"]))
        fl.map.frontier_goals_device(par, grid, fl.view_flags.data_ptr(), views.shape[1], None, B, d_copy.data_ptr(), B, d_g.data_ptr(), d_m.data_ptr(),
                                     d_r.data_ptr())
        fl.ctx.fleet_set_goals_device(fl.params, d_copy.data_ptr(), d_g.data_ptr(), d_m.data_ptr(), B)
        fl.sync()
        assert d_copy.cpu().numpy().tobytes() == after.tobytes()
        assert d_g.cpu().numpy().tobytes() == goals.tobytes() and d_m.cpu().numpy().tobytes() == mask.tobytes()
        assert d_r.cpu().numpy().tobytes() == rec.tobytes()
        # the defaults: r_avoid = goal_radius, z = (z_ground, z_max of set_map)
        fl.explore(R_EXPLORE, want=("no_path", "all"))
        par = abi.default_frontier_params(R_EXPLORE)
        par["r_avoid"], par["z_lo"], par["z_hi"], par["want"] = P["goal_radius"], 0.0, P["z_max"], 6
        rec2, goals2, mask2 = fl.explore_records()
        same((goals2, mask2, rec2), scene_model(fl, sc, par, after, views), "defaults")
        # coverage: the model's, and every vehicle's candidates are frontier voxels of its view
        cov = fl.coverage()
        assert cov.tobytes() == fm.view_coverage(views.reshape(-1), B, views.shape[1], sc["dims"]).tobytes()
        assert (cov["frontier"] >= rec["candidates"]).all() and (cov["known"] > 0).all()
    finally:
        fl.close()


def test_set_unknowns_single_grid_is_one_view_of_all_vehicles(scene):
    sc = scene
    fl = scene_fleet(sc, heading=False)
    B = fl.n
    try:
        shared = sc["views"].min(axis=0)
        fl.set_point_views(False)
        fl.set_unknown(shared, sc["origin"], P["res"], sc["dims"])
        before = fl.vehicles()
        fl.explore(R_EXPLORE, z=Z_EXPLORE, want="all")
        rec, goals, mask = fl.explore_records()
        par = explore_params(fl, abi.FH_FRONTIER_WANT_ALL)
        grid = (tuple(float(o) for o in sc["origin"]), P["res"], tuple(sc["dims"]))
        want = fm.frontier_goals(par, grid, shared, len(shared), np.zeros(B, dtype=np.int32), 1, before, sc["occ"], sc["origin"], P["res"])
        same((goals, mask, rec), want, "one grid")
        assert (rec["view"] == 0).all() and mask.all()
        cov = fl.coverage()
        assert cov.tobytes() == fm.view_coverage(shared, 1, len(shared), sc["dims"]).tobytes()
    finally:
        fl.close()


def test_a_fleet_that_never_explores_makes_todays_calls_and_flies_todays_plans(scene):
    """Two fleets, three periods of sense -> observe -> replan -> next goals.  One of them also measures in every period — coverage, and
    frontier_goals into buffers of the test — and never applies a goal: vehicles, goals and plans are equal byte for byte."""
    import torch

    sc = scene
    A, M = scene_fleet(sc), scene_fleet(sc)
    B = A.n
    try:
        names = [name for name, _ in A.stages()]
        assert names[0] == TODAY[0] and names[-6:] == TODAY[-6:] and not any("frontier" in n or "explore" in n or n == "set_goals" for n in names)
        with pytest.raises(capi.FasterHipError):
            A.explore_records()
        d_g, d_m = torch.zeros((B, 3), dtype=torch.float64, device="cuda:0"), torch.zeros(B, dtype=torch.int32, device="cuda:0")
        d_r = torch.zeros(B * 32, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        par = explore_params(M, abi.FH_FRONTIER_WANT_ALL)
        grid = (tuple(float(o) for o in sc["origin"]), P["res"], tuple(sc["dims"]))
        for c in range(3):
            for fl in (A, M):
                fl.sense(R_SENSE)
                fl.observe()
            M.coverage()
            M.map.frontier_goals_device(par, grid, M.view_flags.data_ptr(), M.view_flags.shape[1], None, B, M.d_vehicles.data_ptr(), B, d_g.data_ptr(),
                                        d_m.data_ptr(), d_r.data_ptr())
            for fl in (A, M):
                fl.replan()
            assert A.vehicles().tobytes() == M.vehicles().tobytes(), ("after replan", c)
            for fl in (A, M):
                fl.next_goals(LOOP_TICKS, follow=True)
            assert A.vehicles().tobytes() == M.vehicles().tobytes() and A.goals().tobytes() == M.goals().tobytes(), ("after next_goals", c)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(A.plans(), M.plans())), ("plans", c)
        assert [name for name, _ in M.stages()] == names and d_m.cpu().numpy().any()
        assert (A.vehicles()["stage"] == abi.FH_FLEET_STAGE_COMMITTED).any()
    finally:
        A.close()
        M.close()


# ---- 5. the closed loop ------------------------------------------------------------------------------------------------------------------------
def test_eight_vehicles_explore_an_open_scene(scene):
    """Eight vehicles with a view each, heading enabled, first goals 2 m away.  Twelve periods of sense -> observe -> explore -> replan ->
    next goals (60 ticks).  In every period the outputs of explore are the model's, computed from the views, the vehicles and the
    occupancy read back just before; what explore did to the vehicles is set_goals of those outputs.  At the end the fleet knows more
    voxels than a control fleet on the same scene that never explores and stops at its first goals, and some vehicle whose record said
    FOUND has, in a later period, committed a replan."""
    sc = scene
    X, Y = scene_fleet(sc), scene_fleet(sc)
    B = X.n
    par = explore_params(X, abi.FH_FRONTIER_WANT_REACHED)
    found_at, committed_after, log = {}, [], []
    try:
        for c in range(LOOP_PERIODS):
            for fl in (X, Y):
                fl.sense(R_SENSE)
                fl.observe()
            before = X.vehicles()
            views = X.views().reshape(B, -1)
            X.explore(R_EXPLORE, z=Z_EXPLORE)
            rec, goals, mask = X.explore_records()
            same((goals, mask, rec), scene_model(X, sc, par, before, views), "period %d" % c)
            assert X.vehicles().tobytes() == hm.set_goals(before, goals, mask, P["wd"]).tobytes(), c
            assert np.array_equal((rec["flags"] & abi.FH_FRONTIER_WANTED) != 0, before["status"] == abi.FH_VEHICLE_GOAL_REACHED)
            for i in np.nonzero(rec["flags"] & abi.FH_FRONTIER_FOUND)[0]:
                found_at.setdefault(int(i), c)
            for fl in (X, Y):
                fl.replan()
            after = X.vehicles()
            for i, c0 in found_at.items():
                if c > c0 and after["active"][i] and after["stage"][i] == abi.FH_FLEET_STAGE_COMMITTED:
                    committed_after.append((i, c0, c))
            log.append((int((rec["flags"] & abi.FH_FRONTIER_WANTED != 0).sum()), int(mask.sum()), np.bincount(after["status"], minlength=4).tolist()))
            for fl in (X, Y):
                fl.next_goals(LOOP_TICKS, follow=True)
        known_x, known_y = int(X.coverage()["known"].sum()), int(Y.coverage()["known"].sum())
        print("explore: (wanted, found, statuses) per period %s; known %d against %d without; found at %s, committed after %s"
              % (log, known_x, known_y, found_at, committed_after[:4]))
        assert (Y.vehicles()["status"] == abi.FH_VEHICLE_GOAL_REACHED).any()     # the control fleet stops at its first goals
        assert known_x > known_y
        assert found_at and committed_after
    finally:
        X.close()
        Y.close()
