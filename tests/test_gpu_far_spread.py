"""fh_apart_goals_device on the device (include/fasterhip_apart.h): every byte of d_goals, d_mask and d_records, the summary
words of the needed views and the need bytes equal to the Python model (tests/far_spread_model.py) on every named case —
tests/test_far_spread_model.py shows what each case is for and which wrong variants they separate; 64 passes against the smallest
sufficient number; with a view per vehicle and no labels against what fh_far_goals_device itself writes on every case of
tests/test_gpu_far.py; and two stranded vehicles of one view, which explore_far() sends to one voxel and explore_far_spread() to two."""
import numpy as np
import pytest

from faster_amd import abi, capi

import far_model as fa
import far_spread_model as fs
import heading_model as hm
from test_gpu_far import GUARD, POISON, R_REACH, R_SENSE, ROOM_CELLS, ROOM_CENTER, ROOM_Z, FAR_BLOCK, KNOWN_X, TICKS, WALL_X, device_far, room_scene, \
    same_work
from test_gpu_fleet import P, fleet_params
from test_gpu_reach import dev, grid_record, map_bits

pytestmark = pytest.mark.gpu

REC = abi.far_spread_record_dtype.itemsize


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch  # noqa: F401  (torch before the HIP library: one HIP runtime in the process)


def device_far_spread(case, par=None):
    """fh_apart_goals_device on device copies of the case's tables into poisoned outputs and a poisoned workspace of exactly the
    stated size, with guard bytes on both sides.  A measurement: the inputs and the guards must have the bytes they had.
    -> (goals, mask, records, the workspace's bytes)."""
    import torch

    veh, view_of, skip, group = case["vehicles"], case["view_of"], case["skip"], case["group"]
    n, n_views = len(veh), case["n_views"]
    par = np.ascontiguousarray(case["par"] if par is None else par).reshape(1)
    bits = map_bits(case["occ"])
    d_f, d_v, d_b = dev(case["flags"]), dev(veh), dev(bits)
    d_vo = None if view_of is None else dev(view_of)
    d_s = None if skip is None else dev(skip)
    d_g = None if group is None else dev(group)
    mz, my, mx = case["occ"].shape
    mg, g = grid_record(case["m_origin"], case["m_res"], (mx, my, mz)), grid_record(*case["grid"])
    work = int(capi.lib().fh_apart_work_bytes(abi.ptr(g), int(par["block"][0]), n_views, n))
    assert work == fs.work_bytes(case["grid"][2], int(par["block"][0]), n_views, n) > 0
    sizes = (24 * n, 4 * n, REC * n, work)
    outs = [torch.full((s + 2 * GUARD,), POISON, dtype=torch.uint8, device="cuda:0") for s in sizes]
    torch.cuda.synchronize()
    ptr = lambda d: None if d is None else d.data_ptr()   # noqa: E731
    rc = capi.lib().fh_apart_goals_device(None, abi.ptr(par), abi.ptr(mg), d_b.data_ptr(), abi.ptr(g), d_f.data_ptr(), case["stride"], ptr(d_vo),
                                               n_views, ptr(d_s), ptr(d_g), d_v.data_ptr(), n, outs[3].data_ptr() + GUARD, work,
                                               *(o.data_ptr() + GUARD for o in outs[:3]))
    assert rc == 0
    torch.cuda.synchronize()
    host = [o.cpu().numpy() for o in outs]
    for h, s in zip(host, sizes):
        assert (h[:GUARD] == POISON).all() and (h[GUARD + s:] == POISON).all()
    assert d_f.cpu().numpy().tobytes() == case["flags"].tobytes() and d_v.cpu().numpy().tobytes() == veh.tobytes()
    assert d_b.cpu().numpy().tobytes() == bits.tobytes()
    for d, h in ((d_vo, view_of), (d_s, skip), (d_g, group)):
        assert d is None or d.cpu().numpy().tobytes() == h.tobytes()
    goals = host[0][GUARD:GUARD + sizes[0]].view(np.float64).reshape(n, 3).copy()
    mask = host[1][GUARD:GUARD + sizes[1]].view(np.int32).copy()
    rec = host[2][GUARD:GUARD + sizes[2]].view(abi.far_spread_record_dtype).copy()
    return goals, mask, rec, host[3][GUARD:GUARD + work].copy()


def same(got, want, what):
    for name, g, w in zip(("goals", "mask", "records"), got, want):
        assert g.tobytes() == w.tobytes(), (what, name, np.nonzero(got[2] != want[2])[0].tolist(), got[2][got[2] != want[2]], want[2][got[2] != want[2]])


def far_bytes(case):
    return fa.work_bytes(case["grid"][2], int(case["par"]["block"]), case["n_views"])


# ---- 1. every byte equal to the model ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ("gap", "packed"))
@pytest.mark.parametrize("name", list(fs.CASES))
def test_goals_mask_records_and_workspace_equal_the_model(name, layout):
    case = fs.case(name)
    if layout == "packed":
        packed = dict(case)   # view_stride = cells
        cells, stride = case["cells"], case["stride"]
        packed["flags"] = np.concatenate([case["flags"][v * stride: v * stride + cells] for v in range(case["n_views"])])
        packed["stride"] = cells
        case = packed
    else:
        case = fs.with_gap(case, 1)   # gap bytes that say "unknown": they are never read
    goals, mask, rec, work = device_far_spread(case)
    want = fs.expected(name)
    same((goals, mask, rec), want[:3], name)
    same_work(case, work[:far_bytes(case)], want[3], want[4], name)
    idle = np.nonzero(mask == 0)[0]
    assert goals[idle].tobytes() == case["vehicles"]["g_term"][idle].tobytes()   # not chosen: the bits of g_term, NaN and infinity included


def test_two_runs_give_the_same_bytes():
    for name in ("fleet_513", "chain_two_passes", "shared_and_invalid_view"):
        a, b = device_far_spread(fs.case(name)), device_far_spread(fs.case(name))
        same(a[:3], b[:3], "second run of " + name)
        assert a[3][:far_bytes(fs.case(name))].tobytes() == b[3][:far_bytes(fs.case(name))].tobytes()


@pytest.mark.parametrize("name", ("chain_of_three", "fleet_513", "standing_300", "labels"))
def test_64_passes_give_the_bytes_of_the_smallest_sufficient_number(name):
    case = fs.case(name)
    most = int(fs.expected(name)[2]["lower"].max())
    outs = []
    for passes in (most + 1, abi.FH_APART_MAX_PASSES):
        par = case["par"].copy()
        par["passes"] = passes
        outs.append(device_far_spread(case, par=par))
        assert (outs[-1][2]["decided_pass"] >= 0).all()
    same(outs[0][:3], outs[1][:3], name)
    same(outs[0][:3], fs.expected(name)[:3], name)
    if most > 0:   # one pass fewer leaves the last of the chain unsettled
        par = case["par"].copy()
        par["passes"] = most
        rec = device_far_spread(case, par=par)[2]
        assert int((rec["decided_pass"] == -1).sum()) >= 1 and (rec["flags"][rec["decided_pass"] == -1] & fs.UNSETTLED).all()


# ---- 2. a view per vehicle and no labels: the chooser without claims -------------------------------------------------------------------------------
def own_views(case):
    """The case with a copy of its view for every vehicle (an invalid view stays invalid) and a spread record for its params."""
    n, cells, stride = len(case["vehicles"]), case["cells"], case["stride"]
    out = dict(case)
    flags = np.ones(n * stride, dtype=np.uint8)
    view_of = np.zeros(n, dtype=np.int32)
    for i in range(n):
        v = int(i if case["view_of"] is None else case["view_of"][i])
        if 0 <= v < case["n_views"]:
            flags[i * stride: i * stride + cells] = case["flags"][v * stride: v * stride + cells]
            view_of[i] = i
        else:
            view_of[i] = -1
    out["flags"], out["view_of"], out["n_views"], out["group"] = flags, view_of, n, None
    return out


@pytest.mark.parametrize("name", list(fa.CASES))
def test_with_a_view_per_vehicle_it_writes_what_the_chooser_without_claims_writes(name):
    case = own_views(fa.case(name))
    f_goals, f_mask, f_rec, f_work = device_far(case)
    par = abi.default_far_spread_params(int(case["par"]["block"]), 2.0)
    for k in abi.far_params_dtype.names:
        par[k] = case["par"][k]
    s_case = dict(case)
    s_case["par"] = par
    goals, mask, rec, work = device_far_spread(s_case)
    assert goals.tobytes() == f_goals.tobytes() and mask.tobytes() == f_mask.tobytes(), name
    assert rec.view(np.uint8).reshape(len(rec), REC)[:, :64].tobytes() == f_rec.tobytes(), (name, rec, f_rec)
    assert work[:len(f_work)].tobytes() == f_work.tobytes(), name
    searched = (f_rec["flags"] & ~(abi.FH_FRONTIER_FOUND | abi.FH_REACH_CUT)) == abi.FH_FRONTIER_WANTED
    assert np.array_equal(rec["decided_pass"], searched.astype(np.int32)) and not rec["lower"].any() and not rec["claims"].any() and not rec["claimed"].any()


# ---- 3. two stranded vehicles of one view ------------------------------------------------------------------------------------------------------------
PERIODS, R_SPREAD, PATCH_LO, PATCH_HI = 10, 2.0, 2.4, 5.6


def pair_scene():
    """The room of tests/test_gpu_far.py with two vehicles in one place that share ONE view.  The view knows everything but two regions
    behind the wall, x > 8 with y < 2.4 and x > 8 with y > 5.6: their frontiers are 3.2 m apart, and both beyond R_REACH."""
    sc = room_scene()
    res, dims, origin = P["res"], sc["dims"], sc["origin"]
    iz, iy, ix = np.meshgrid(np.arange(dims[2]), np.arange(dims[1]), np.arange(dims[0]), indexing="ij")
    x, y = (ix + 0.5) * res + origin[0], (iy + 0.5) * res + origin[1]
    view = np.zeros((1, dims[2], dims[1], dims[0]), dtype=np.uint8)
    view[0][(x > KNOWN_X) & ((y < PATCH_LO) | (y > PATCH_HI))] = 1
    sc["views"] = view.reshape(1, -1)
    sc["starts"] = np.array([(2.5, 2.0, 1.0), (2.5, 2.0, 1.0)])
    sc["goals"] = sc["starts"] + np.array([0.0, 1.0, 0.0])
    return sc


def pair_fleet(sc):
    from faster_amd.fleet import Fleet

    fl = Fleet(2, fleet_params(), n_seg=P["N"], max_poly=P["max_poly"], dc=P["dc"], v_max=P["v_max"], a_max=P["a_max"], j_max=P["j_max"],
               decomp_radius=P["decomp_radius"], dist_max_vertexes=P["dist_max_vertexes"])
    fl.set_map(sc["cloud"], ROOM_CELLS, P["res"], ROOM_CENTER, P["z_max"], P["inflation"])
    fl.init(sc["starts"], sc["goals"])
    fl.set_unknown_views(sc["views"].copy(), view_of=[0, 0], n_views=1, origin=sc["origin"], res=P["res"], dims=sc["dims"])
    fl.set_point_views()
    fl.enable_heading()
    return fl


def test_two_stranded_teammates_fly_to_one_voxel_under_explore_far_and_to_two_under_explore_far_spread():
    """Two fleets, PERIODS periods of sense -> observe -> explore_reachable -> explore_far | explore_far_spread (after="reachable") ->
    replan -> next goals.  Once both vehicles have reached their first goal explore_reachable finds nothing in their boxes.  explore_far
    then gives both the same voxel; explore_far_spread gives the model's two voxels, at least R_SPREAD apart, the replan that follows
    does not end in NO_PATH, and the first replan each takes part in commits.  The known voxels of the view after PERIODS periods are
    reported under each chooser."""
    sc = pair_scene()
    A, S = pair_fleet(sc), pair_fleet(sc)
    grid = (tuple(float(o) for o in sc["origin"]), P["res"], tuple(sc["dims"]))
    view_of = np.zeros(2, dtype=np.int32)
    try:
        occ = S.map.occupancy()
        with pytest.raises(capi.FasterHipError, match="explore_far_spread first"):
            S.far_spread_records()
        with pytest.raises(capi.FasterHipError, match="has not run"):
            S.explore_far_spread(FAR_BLOCK, R_SPREAD, after="gain")
        S.explore_reachable(R_REACH, z=ROOM_Z)
        assert [name for name, _ in S.explore_far_spread_stages(FAR_BLOCK, R_SPREAD, z=ROOM_Z, after="reachable")] == ["far_spread_goals", "set_goals"]
        work = S.d_far_spread_work
        known0 = int(S.coverage()["known"][0])
        assert int(A.coverage()["known"][0]) == known0
        same_at, split_at, first_active, log = None, None, [None, None], []
        for c in range(PERIODS):
            for fl in (A, S):
                fl.sense(R_SENSE)
                fl.observe()
                fl.explore_reachable(R_REACH, z=ROOM_Z)
            A.explore_far(FAR_BLOCK, z=ROOM_Z, after="reachable")
            _, a_goals, a_mask = A.far_records()
            if same_at is None and a_mask.tolist() == [1, 1]:
                same_at = c
                assert a_goals[0].tobytes() == a_goals[1].tobytes()                  # one voxel for both
            before = S.vehicles()
            views = S.views().reshape(1, -1)
            _, _, k_mask = S.reach_records()
            S.explore_far_spread(FAR_BLOCK, R_SPREAD, z=ROOM_Z, after="reachable")
            rec, goals, mask = S.far_spread_records()
            par = fs.fsp(FAR_BLOCK, R_SPREAD, r_avoid=float(S.params["goal_radius"]), z_lo=ROOM_Z[0], z_hi=ROOM_Z[1], want=abi.FH_FRONTIER_WANT_REACHED)
            want = fs.far_spread_goals(par, grid, views.reshape(-1), views.shape[1], view_of, 1, k_mask, None, before, occ, sc["origin"], P["res"])
            same((goals, mask, rec), want[:3], "Fleet.explore_far_spread, period %d" % c)
            assert S.vehicles().tobytes() == hm.set_goals(before, goals, mask, P["wd"]).tobytes(), c
            assert np.array_equal(S.views().reshape(1, -1), views)                   # the views are only read
            if split_at is None and mask.tolist() == [1, 1]:
                split_at = c
                assert [int(s) for s in before["status"]] == [abi.FH_VEHICLE_GOAL_REACHED] * 2 and k_mask.tolist() == [0, 0]
                e = goals[1] - goals[0]
                assert (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2] >= R_SPREAD ** 2 and int(rec["claimed"][1]) >= 1 and int(rec["decided_pass"][1]) == 2
                assert goals[0][0] > WALL_X and goals[1][0] > WALL_X                 # both behind the wall
            for fl in (A, S):
                fl.replan()
            after = S.vehicles()
            for i in range(2):
                assert int(after["stage"][i]) != abi.FH_FLEET_STAGE_NO_PATH, (c, i)
                if split_at is not None and first_active[i] is None and int(after["active"][i]) == 1:
                    first_active[i] = c
                    assert int(after["stage"][i]) == abi.FH_FLEET_STAGE_COMMITTED, (c, i, int(after["stage"][i]))
            log.append(([int(s) for s in before["status"]], mask.tolist(), a_mask.tolist(), [int(s) for s in after["stage"]]))
            for fl in (A, S):
                fl.next_goals(TICKS, follow=True)
        known_a, known_s = int(A.coverage()["known"][0]), int(S.coverage()["known"][0])
        print("far_spread: (status, mask, mask under explore_far, stage) per period %s; one voxel for both at %s, two voxels at %s, first active "
              "replans %s; known voxels of the view %d -> %d under explore_far, %d under explore_far_spread"
              % (log, same_at, split_at, first_active, known0, known_a, known_s))
        assert S.d_far_spread_work is work                                           # one workspace per lattice, block, views and vehicles
        assert same_at is not None and split_at is not None
        assert all(f is not None and f > split_at for f in first_active)
        assert known_a >= known0 and known_s >= known0
    finally:
        A.close()
        S.close()
