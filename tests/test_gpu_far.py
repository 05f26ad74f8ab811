"""fh_far_goals_device on the device (include/fasterhip_far.h): every byte of d_goals, d_mask and d_records, the summary words of the
needed views and the need bytes equal to the Python model (tests/far_model.py, a queue over blocks) on every named case —
tests/test_far_model.py shows what each case is for and which wrong variants they separate; with blocks of one voxel against what
fh_reach_goals_device itself writes; and a vehicle in a known room whose only frontier lies round a wall, beyond r_max, which
explore_reachable() leaves where it is and explore_far() sends on its way."""
import numpy as np
import pytest

from faster_amd import abi, capi

import far_model as fa
import heading_model as hm
from test_gpu_fleet import P, fleet_params
from test_gpu_reach import dev, device_reach, grid_record, map_bits

pytestmark = pytest.mark.gpu

GUARD, POISON = 64, 0xA5
WANTED, FOUND = abi.FH_FRONTIER_WANTED, abi.FH_FRONTIER_FOUND


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch  # noqa: F401  (torch before the HIP library: one HIP runtime in the process)


def device_far(case, par=None):
    """fh_far_goals_device on device copies of the case's tables, the map's bits packed from its occupancy, into poisoned outputs and a
    poisoned workspace with guard bytes on both sides.  A measurement: the inputs and the guards must have the bytes they had.
    -> (goals, mask, records, the workspace's bytes)."""
    import torch

    veh, view_of, skip = case["vehicles"], case["view_of"], case["skip"]
    n, n_views = len(veh), case["n_views"]
    par = np.ascontiguousarray(case["par"] if par is None else par).reshape(1)
    bits = map_bits(case["occ"])
    d_f, d_v, d_b = dev(case["flags"]), dev(veh), dev(bits)
    d_vo = None if view_of is None else dev(view_of)
    d_s = None if skip is None else dev(skip)
    mz, my, mx = case["occ"].shape
    mg, g = grid_record(case["m_origin"], case["m_res"], (mx, my, mz)), grid_record(*case["grid"])
    work = int(capi.lib().fh_far_work_bytes(abi.ptr(g), int(par["block"][0]), n_views))
    assert work == fa.work_bytes(case["grid"][2], int(par["block"][0]), n_views) > 0
    sizes = (24 * n, 4 * n, 64 * n, work)
    outs = [torch.full((s + 2 * GUARD,), POISON, dtype=torch.uint8, device="cuda:0") for s in sizes]
    torch.cuda.synchronize()
    rc = capi.lib().fh_far_goals_device(None, abi.ptr(par), abi.ptr(mg), d_b.data_ptr(), abi.ptr(g), d_f.data_ptr(), case["stride"],
                                        None if d_vo is None else d_vo.data_ptr(), n_views, None if d_s is None else d_s.data_ptr(), d_v.data_ptr(), n,
                                        outs[3].data_ptr() + GUARD, work, *(o.data_ptr() + GUARD for o in outs[:3]))
    assert rc == 0
    torch.cuda.synchronize()
    host = [o.cpu().numpy() for o in outs]
    for h, s in zip(host, sizes):
        assert (h[:GUARD] == POISON).all() and (h[GUARD + s:] == POISON).all()
    assert d_f.cpu().numpy().tobytes() == case["flags"].tobytes() and d_v.cpu().numpy().tobytes() == veh.tobytes()
    assert d_b.cpu().numpy().tobytes() == bits.tobytes()
    assert d_vo is None or d_vo.cpu().numpy().tobytes() == view_of.tobytes()
    assert d_s is None or d_s.cpu().numpy().tobytes() == skip.tobytes()
    goals = host[0][GUARD:GUARD + sizes[0]].view(np.float64).reshape(n, 3).copy()
    mask = host[1][GUARD:GUARD + sizes[1]].view(np.int32).copy()
    rec = host[2][GUARD:GUARD + sizes[2]].view(abi.far_record_dtype).copy()
    return goals, mask, rec, host[3][GUARD:GUARD + work].copy()


def same(got, want, what):
    for name, g, w in zip(("goals", "mask", "records"), got, want):
        assert g.tobytes() == w.tobytes(), (what, name, np.nonzero(got[2] != want[2])[0].tolist(), got[2], want[2])


def same_work(case, work, sums, need, what):
    """The workspace against the model: the four bitmaps of every needed view, poison in those of the others, and the need bytes."""
    n_views = case["n_views"]
    W = fa.blocks_of(case["grid"][2], int(case["par"]["block"]))[2]
    words = work[:n_views * 4 * W * 8].view(np.uint64).reshape(n_views, 4, W)
    for v in range(n_views):
        if v in sums:
            assert words[v].tobytes() == sums[v].tobytes(), (what, "summary of view", v, words[v], sums[v])
        else:
            assert (words[v].view(np.uint8) == POISON).all(), (what, "view nobody needs", v)
    assert work[n_views * 4 * W * 8:].tobytes() == need.tobytes(), (what, "need bytes")


# ---- 1. every byte equal to the model ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ("gap", "packed"))
@pytest.mark.parametrize("name", list(fa.CASES))
def test_goals_mask_records_and_workspace_equal_the_model(name, layout):
    case = fa.case(name)
    if layout == "packed":
        packed = dict(case)   # view_stride = cells
        cells, stride = case["cells"], case["stride"]
        packed["flags"] = np.concatenate([case["flags"][v * stride: v * stride + cells] for v in range(case["n_views"])])
        packed["stride"] = cells
        case = packed
    else:
        case = fa.with_gap(case, 1)   # gap bytes that say "unknown": they are never read
    goals, mask, rec, work = device_far(case)
    want = fa.expected(name)
    same((goals, mask, rec), want[:3], name)
    same_work(case, work, want[3], want[4], name)
    idle = np.nonzero(mask == 0)[0]
    assert goals[idle].tobytes() == case["vehicles"]["g_term"][idle].tobytes()   # not chosen: the bits of g_term, NaN and infinity included


def test_two_runs_give_the_same_bytes_and_the_unneeded_view_keeps_its_poison():
    case = fa.case("shared_view")
    a, b = device_far(case), device_far(case)
    same(a[:3], b[:3], "second run")
    assert a[3].tobytes() == b[3].tobytes()
    W = fa.blocks_of(case["grid"][2], int(case["par"]["block"]))[2]
    assert (a[3][4 * W * 8: 2 * 4 * W * 8] == POISON).all() and a[3][3 * 4 * W * 8:][:3].tolist() == [1, 0, 1]
    case = fa.case("other_lattice")
    a, b = device_far(case), device_far(case)
    same(a[:3], b[:3], "second run of other_lattice")
    assert a[3].tobytes() == b[3].tobytes()


def test_max_hops_far_above_the_last_level_changes_nothing():
    case = fa.case("block_1")
    par = case["par"].copy()
    par["max_hops"] = (1 << 31) - 1
    same(device_far(case, par=par)[:3], fa.expected("block_1")[:3], "max_hops 2^31 - 1")


# ---- 2. blocks of one voxel: the voxel flood over the whole lattice ------------------------------------------------------------------------------
def test_with_blocks_of_one_voxel_it_writes_what_the_voxel_flood_writes():
    qualified = 0
    for name in fa.CASES:
        red = fa.reduced(fa.case(name))
        if red is None:
            continue
        qualified += 1
        one, rpar = red
        goals, mask, rec, _ = device_far(one)
        r_case = dict(one)
        r_case["par"] = rpar
        r_goals, r_mask, r_rec = device_reach(r_case)
        assert goals.tobytes() == r_goals.tobytes() and mask.tobytes() == r_mask.tobytes(), name
        assert np.array_equal(rec["flags"], r_rec["flags"]), name
        for k in ("view", "cell", "hops", "reachable", "reached", "levels", "d2"):
            assert rec[k].tobytes() == r_rec[k].tobytes(), (name, k)
        assert np.array_equal(rec["targets"], r_rec["candidates"]) and np.array_equal(rec["block_cell"], rec["cell"]), name
    assert 3 * qualified >= 2 * len(fa.CASES)


# ---- 3. a vehicle in a known room whose only frontier lies round a wall, beyond r_max --------------------------------------------------------------
ROOM_CELLS, ROOM_CENTER, ROOM_Z = (60, 40, 15), (6.0, 4.0, 1.5), (0.6, 1.4)
R_SENSE, R_REACH, FAR_BLOCK = 2.5, 3.0, 8
WALL_X, WALL_Y, KNOWN_X = 5.1, 5.6, 8.0
PERIODS, TICKS = 10, 100


def room_scene():
    """12 m x 8 m x 2.8 m, res 0.2.  A wall at x = 5.1 from y = 0 to y = 5.6 leaves a gap of 2.4 m.  Vehicle 0 stands at (2.5, 2, 1) and
    knows every voxel with x < 8: the room it is in, the gap and three metres behind the wall.  Its frontier is the plane x = 8, 5.4 m
    away and more: outside the sphere of R_REACH.  Vehicle 1 is a bystander whose view knows everything."""
    res = P["res"]
    cloud = np.array([(WALL_X, y, z) for y in np.arange(0.1, WALL_Y, res) for z in np.arange(0.1, P["z_max"], res)])
    probe = capi.Map(0)   # (the lattice of the inflated map is the lattice of the views)
    probe.read(cloud, ROOM_CELLS, res, ROOM_CENTER, 0.0, P["z_max"], P["inflation"])
    dims, origin = probe.dims()
    probe.close()
    starts = np.array([(2.5, 2.0, 1.0), (1.0, 6.0, 1.0)])
    goals = starts + np.array([0.0, 1.0, 0.0])
    iz, iy, ix = np.meshgrid(np.arange(dims[2]), np.arange(dims[1]), np.arange(dims[0]), indexing="ij")
    views = np.zeros((2, dims[2], dims[1], dims[0]), dtype=np.uint8)
    views[0][(ix + 0.5) * res + origin[0] > KNOWN_X] = 1
    return {"cloud": cloud, "starts": starts, "goals": goals, "dims": [int(d) for d in dims], "origin": np.array(origin, dtype=np.float64),
            "views": views.reshape(2, -1)}


def room_fleet(sc):
    from faster_amd.fleet import Fleet

    fl = Fleet(2, fleet_params(), n_seg=P["N"], max_poly=P["max_poly"], dc=P["dc"], v_max=P["v_max"], a_max=P["a_max"], j_max=P["j_max"],
               decomp_radius=P["decomp_radius"], dist_max_vertexes=P["dist_max_vertexes"])
    fl.set_map(sc["cloud"], ROOM_CELLS, P["res"], ROOM_CENTER, P["z_max"], P["inflation"])
    fl.init(sc["starts"], sc["goals"])
    fl.set_unknown_views(sc["views"].copy(), origin=sc["origin"], res=P["res"], dims=sc["dims"])
    fl.set_point_views()
    fl.enable_heading()
    return fl


def test_a_stranded_vehicle_stays_under_explore_reachable_and_flies_on_under_explore_far():
    """Two fleets, PERIODS periods of sense -> observe -> explore_reachable [-> explore_far(after="reachable")] -> replan -> next goals.
    Once vehicle 0 has reached its first goal explore_reachable finds no candidate in its box, in either fleet, and in the fleet without
    explore_far it stays GOAL_REACHED to the end and its view learns nothing.  In the other fleet explore_far gives it the model's
    voxel, beyond the wall; the replan that follows does not end in NO_PATH (the vehicle is YAWING and sits that one out), the first
    replan it takes part in commits, and at the end its view knows more voxels than it did."""
    sc = room_scene()
    R, F = room_fleet(sc), room_fleet(sc)
    grid = (tuple(float(o) for o in sc["origin"]), P["res"], tuple(sc["dims"]))
    try:
        m_dims, m_origin = F.map.dims()
        assert [int(d) for d in m_dims] == sc["dims"] and np.array_equal(m_origin, sc["origin"])
        occ = F.map.occupancy()
        with pytest.raises(capi.FasterHipError):
            F.far_records()                                             # nothing to read before the first explore_far
        with pytest.raises(capi.FasterHipError, match="has not run"):
            F.explore_far(FAR_BLOCK, after="gain")                      # that chooser has not run
        F.explore_reachable(R_REACH, z=ROOM_Z)
        assert [name for name, _ in F.explore_far_stages(FAR_BLOCK, z=ROOM_Z, after="reachable")] == ["far_goals", "set_goals"]
        work = F.d_far_work
        known0 = [int(k) for k in F.coverage()["known"]]
        assert [int(k) for k in R.coverage()["known"]] == known0
        stranded_r, found_at, first_active, log = [], None, None, []
        for c in range(PERIODS):
            for fl in (R, F):
                fl.sense(R_SENSE)
                fl.observe()
                fl.explore_reachable(R_REACH, z=ROOM_Z)
            r_rec, _, r_mask = R.reach_records()
            if int(R.vehicles()["status"][0]) == abi.FH_VEHICLE_GOAL_REACHED:
                assert int(r_rec["flags"][0]) == WANTED and int(r_rec["candidates"][0]) == 0 and int(r_mask[0]) == 0, c
                stranded_r.append(c)
            before = F.vehicles()
            views = F.views().reshape(2, -1)
            k_rec, _, k_mask = F.reach_records()
            F.explore_far(FAR_BLOCK, z=ROOM_Z, after="reachable")
            rec, goals, mask = F.far_records()
            par = fa.far_params(FAR_BLOCK, float(F.params["goal_radius"]), ROOM_Z[0], ROOM_Z[1], abi.FH_FRONTIER_WANT_REACHED)
            want = fa.far_goals(par, grid, views.reshape(-1), views.shape[1], None, 2, k_mask, before, occ, sc["origin"], P["res"])
            same((goals, mask, rec), want[:3], "Fleet.explore_far, period %d" % c)
            assert F.vehicles().tobytes() == hm.set_goals(before, goals, mask, P["wd"]).tobytes(), c
            assert np.array_equal(F.views().reshape(2, -1), views)       # the views are only read
            if found_at is None and int(mask[0]) == 1:
                found_at = c
                assert int(before["status"][0]) == abi.FH_VEHICLE_GOAL_REACHED and int(k_rec["candidates"][0]) == 0 and int(k_mask[0]) == 0
                # beyond the wall, which the straight line to it crosses, and beyond the box
                assert int(rec["hops"][0]) >= 1 and goals[0][0] > WALL_X and goals[0][1] < WALL_Y and float(rec["d2"][0]) > R_REACH ** 2
            for fl in (R, F):
                fl.replan()
            after = F.vehicles()
            assert int(after["stage"][0]) != abi.FH_FLEET_STAGE_NO_PATH, c
            if found_at is not None and first_active is None and int(after["active"][0]) == 1:
                first_active = c
                assert int(after["stage"][0]) == abi.FH_FLEET_STAGE_COMMITTED, (c, int(after["stage"][0]))
            log.append((int(before["status"][0]), int(mask[0]), int(rec["hops"][0]), int(after["stage"][0]), int(after["active"][0])))
            for fl in (R, F):
                fl.next_goals(TICKS, follow=True)
        known_r, known_f = [int(k) for k in R.coverage()["known"]], [int(k) for k in F.coverage()["known"]]
        print("far: (status, mask, hops, stage, active) of vehicle 0 per period %s; found at %s, first active replan %s; stranded without it in "
              "periods %s; known %s -> %s with it, %s without" % (log, found_at, first_active, stranded_r, known0, known_f, known_r))
        assert F.d_far_work is work                                     # one workspace per lattice, block and number of views
        assert found_at is not None and first_active is not None and first_active > found_at
        assert len(stranded_r) >= 3 and stranded_r[-1] == PERIODS - 1 and known_r == known0
        assert int(R.vehicles()["status"][0]) == abi.FH_VEHICLE_GOAL_REACHED
        assert known_f[0] > known0[0] and known_f[1] == known0[1]
    finally:
        R.close()
        F.close()
