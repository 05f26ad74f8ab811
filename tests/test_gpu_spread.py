"""fh_spread_goals_device on the device (include/fasterhip_spread.h): every byte of d_goals, d_mask and d_records equal to the Python
model (tests/spread_model.py, vehicle by vehicle in index order) on every named case — tests/test_spread_model.py shows what each case
is for and which wrong variants they separate; equal to fh_reach_goals_device itself where nobody has a peer; the same bytes from two
runs and from more passes than are needed; and through Fleet: a team of two that explore_reachable() sends to one voxel and
explore_spread() to two, and two teams of four in a closed loop."""
import numpy as np
import pytest

from faster_amd import abi, capi

import frontier_model as fm
import heading_model as hm
import reach_model as rm
import spread_model as sm
from test_gpu_fleet import P, fleet_params
from test_gpu_reach import dev, device_reach, grid_record, map_bits

pytestmark = pytest.mark.gpu

GUARD, POISON = 64, 0xA5
WANTED, FOUND = abi.FH_FRONTIER_WANTED, abi.FH_FRONTIER_FOUND
REC = abi.spread_record_dtype.itemsize


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch  # noqa: F401  (torch before the HIP library: one HIP runtime in the process)


def device_spread(case, par=None, group="case"):
    """fh_spread_goals_device on device copies of the case's tables into poisoned outputs, and a poisoned workspace of exactly
    fh_spread_work_bytes(n), with guard bytes on both sides.  A measurement: the inputs and the guards must have the bytes they had."""
    import torch

    veh, view_of = case["vehicles"], case["view_of"]
    group = case.get("group") if isinstance(group, str) else group
    n = len(veh)
    par = np.ascontiguousarray(case["par"] if par is None else par).reshape(1)
    bits = map_bits(case["occ"])
    d_f, d_v, d_b = dev(case["flags"]), dev(veh), dev(bits)
    d_vo = None if view_of is None else dev(view_of)
    d_gr = None if group is None else dev(group)
    mz, my, mx = case["occ"].shape
    mg, g = grid_record(case["m_origin"], case["m_res"], (mx, my, mz)), grid_record(*case["grid"])
    work = int(capi.lib().fh_spread_work_bytes(n))
    sizes = (24 * n, 4 * n, REC * n, work)
    outs = [torch.full((s + 2 * GUARD,), POISON, dtype=torch.uint8, device="cuda:0") for s in sizes]
    torch.cuda.synchronize()
    rc = capi.lib().fh_spread_goals_device(None, abi.ptr(par), abi.ptr(mg), d_b.data_ptr(), abi.ptr(g), d_f.data_ptr(), case["stride"],
                                           None if d_vo is None else d_vo.data_ptr(), case["n_views"], None if d_gr is None else d_gr.data_ptr(),
                                           d_v.data_ptr(), n, outs[3].data_ptr() + GUARD, work, *(o.data_ptr() + GUARD for o in outs[:3]))
    assert rc == 0
    torch.cuda.synchronize()
    host = [o.cpu().numpy() for o in outs]
    for h, s in zip(host, sizes):
        assert (h[:GUARD] == POISON).all() and (h[GUARD + s:] == POISON).all()
    assert d_f.cpu().numpy().tobytes() == case["flags"].tobytes() and d_v.cpu().numpy().tobytes() == veh.tobytes()
    assert d_b.cpu().numpy().tobytes() == bits.tobytes()
    assert d_vo is None or d_vo.cpu().numpy().tobytes() == np.ascontiguousarray(view_of).tobytes()
    assert d_gr is None or d_gr.cpu().numpy().tobytes() == np.ascontiguousarray(group).tobytes()
    goals = host[0][GUARD:GUARD + sizes[0]].view(np.float64).reshape(n, 3).copy()
    mask = host[1][GUARD:GUARD + sizes[1]].view(np.int32).copy()
    rec = host[2][GUARD:GUARD + sizes[2]].view(abi.spread_record_dtype).copy()
    return goals, mask, rec


def same(got, want, what):
    for name, g, w in zip(("goals", "mask", "records"), got, want):
        assert g.tobytes() == w.tobytes(), (what, name, np.nonzero(got[2] != want[2])[0].tolist()[:8], got[2][got[2] != want[2]][:4], want[2][got[2] != want[2]][:4])


# ---- 1. every byte equal to the model ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gap", (0, 1))
@pytest.mark.parametrize("name", list(sm.CASES))
def test_goals_mask_and_records_equal_the_model(name, gap):
    case = sm.case(name)
    if gap:
        case = rm.with_gap(case, 1)
    got = device_spread(case)
    same(got, sm.expected(name), name)   # (the model of the tables as they are: the gap bytes are never read)
    idle = np.nonzero(got[1] == 0)[0]
    assert got[0][idle].tobytes() == case["vehicles"]["g_term"][idle].tobytes()   # not chosen: the bits of g_term, NaN and infinity included


def test_d_group_null_is_the_view_and_labels_are_only_compared():
    """The labelled case without its labels: four groups of one.  And labels that are no index of anything."""
    case = sm.case("labels")
    got = device_spread(case, group=None)
    same(got, sm.model(case, group=None), "labels without d_group")
    assert got[2]["group"].tolist() == [0, 1, 2, 3] and got[2]["decided_pass"].tolist() == [1, 1, 1, 1]
    for name in ("labels_negative", "labels_large"):
        assert device_spread(sm.case(name))[2]["group"].tolist() == sm.case(name)["group"].tolist()


# ---- 2. nobody has a peer: fh_reach_goals_device -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rm.ALL_CASES)
def test_without_peers_the_outputs_are_those_of_reach_goals_device(name):
    case = sm.own_groups(rm.case(name))
    goals, mask, rec = device_reach(case)
    got = device_spread(case, par=sm.spread_par_of(case["par"], r_spread=1.0))
    assert got[0].tobytes() == goals.tobytes() and got[1].tobytes() == mask.tobytes(), name
    assert got[2].view(np.uint8).reshape(-1, REC)[:, :40].tobytes() == rec.view(np.uint8).reshape(-1, 48)[:, :40].tobytes(), name
    searched = (rec["flags"] & ~(FOUND | abi.FH_REACH_CUT)) == WANTED
    assert np.array_equal(got[2]["decided_pass"], searched.astype(np.int32)) and not got[2]["lower"].any() and not got[2]["claimed"].any()


# ---- 3. determinism ----------------------------------------------------------------------------------------------------------------------------
def test_two_runs_and_more_passes_than_needed_give_the_same_bytes():
    for name, enough in (("chain_passes_3", 3), ("shared_and_invalid", 3), ("fleet_129_at_64", 2)):
        case = sm.case(name)
        par = case["par"].copy()
        par["passes"] = enough
        a, b = device_spread(case, par=par), device_spread(case, par=par)
        same(a, b, name + ": second run")
        assert int(a[2]["decided_pass"].max()) == enough and not (a[2]["flags"] & abi.FH_SPREAD_UNSETTLED).any()
        par["passes"] = abi.FH_SPREAD_MAX_PASSES
        same(device_spread(case, par=par), a, name + ": 64 passes")


# ---- 4. through Fleet: a team of two -----------------------------------------------------------------------------------------------------------
TEAM_CELLS, TEAM_CENTER, TEAM_R, TEAM_SPREAD, TEAM_Z = (40, 40, 15), (4.0, 4.0, 1.5), 6.0, 2.0, (0.6, 1.4)


def team_scene():
    """8 m x 8 m x 2.8 m at res 0.2, a pillar in a corner.  Two vehicles of one view, 0.4 m apart along x; the view knows every voxel
    with x < 26 and nothing beyond, so the nearest frontier voxel of both, in steps, is the one straight ahead."""
    res = P["res"]
    _, origin, dims = fm.map_read(np.zeros((0, 3)), TEAM_CELLS, res, TEAM_CENTER, 0.0, P["z_max"])
    q = lambda c: np.array([(c[k] + 0.5) * res + origin[k] for k in range(3)])   # noqa: E731
    cloud = np.array([q((2, 2, z)) for z in range(dims[2])])
    starts = np.array([q((18, 20, 5)), q((20, 20, 5))])
    view = np.zeros((dims[2], dims[1], dims[0]), dtype=np.uint8)
    view[:, :, 26:] = 1
    return {"cloud": cloud, "starts": starts, "goals": starts + np.array([0.0, 2.0, 0.0]), "dims": [int(d) for d in dims],
            "origin": np.array(origin, dtype=np.float64), "views": view.reshape(1, -1), "ahead": (25, 20, 5)}


def team_fleet(sc, own_views=False):
    """The two vehicles with the one view of the scene, or with a copy of it each."""
    from faster_amd.fleet import Fleet

    fl = Fleet(2, fleet_params(), n_seg=P["N"], max_poly=P["max_poly"], dc=P["dc"], v_max=P["v_max"], a_max=P["a_max"], j_max=P["j_max"],
               decomp_radius=P["decomp_radius"], dist_max_vertexes=P["dist_max_vertexes"])
    fl.set_map(sc["cloud"], TEAM_CELLS, P["res"], TEAM_CENTER, P["z_max"], 0.0)
    fl.init(sc["starts"], sc["goals"])
    if own_views:
        fl.set_unknown_views(np.repeat(sc["views"], 2, axis=0), origin=sc["origin"], res=P["res"], dims=sc["dims"])
    else:
        fl.set_unknown_views(sc["views"].copy(), view_of=np.zeros(2, dtype=np.int32), n_views=1, origin=sc["origin"], res=P["res"], dims=sc["dims"])
    return fl


def test_groups_are_the_labels_of_the_last_link_or_the_views():
    """The two vehicles with a view each.  Before any link(), and with groups="view" after it, each is a group of its own and both take
    the voxel straight ahead; after link() with a range that joins them the labels make them peers and the second yields."""
    sc = team_scene()
    ahead = rm.cell_index(sc["ahead"], sc["dims"])
    S = team_fleet(sc, own_views=True)
    try:
        before = S.vehicles()
        S.explore_spread(TEAM_R, TEAM_SPREAD, z=TEAM_Z, want="all")
        rec = S.spread_records()[0]
        assert rec["cell"].tolist() == [ahead, ahead] and rec["group"].tolist() == [0, 1] and rec["decided_pass"].tolist() == [1, 1]
        S.link(1.0)
        labels, _ = S.link_records()
        assert labels.tolist() == [0, 0]
        S.set_goals(before["g_term"])   # (the goals they held: r_avoid is around g_term)
        S.explore_spread(TEAM_R, TEAM_SPREAD, z=TEAM_Z, want="all", groups="view")
        rec = S.spread_records()[0]
        assert rec["cell"].tolist() == [ahead, ahead] and rec["group"].tolist() == [0, 1]
        S.set_goals(before["g_term"])
        S.explore_spread(TEAM_R, TEAM_SPREAD, z=TEAM_Z, want="all")
        rec, goals, mask = S.spread_records()
        assert rec["group"].tolist() == [0, 0] and rec["decided_pass"].tolist() == [1, 2] and rec["lower"].tolist() == [0, 1]
        assert mask.tolist() == [1, 1] and int(rec["cell"][0]) == ahead and int(rec["cell"][1]) != ahead
        assert sm.d2_of(goals[0], goals[1]) >= TEAM_SPREAD * TEAM_SPREAD
    finally:
        S.close()


def test_a_team_of_two_is_sent_to_one_voxel_by_explore_reachable_and_to_two_by_explore_spread():
    sc = team_scene()
    dims = sc["dims"]
    ahead = rm.cell_index(sc["ahead"], dims)
    K, S = team_fleet(sc), team_fleet(sc)
    try:
        with pytest.raises(capi.FasterHipError):
            S.spread_records()                                               # nothing to read before the first explore_spread
        with pytest.raises(capi.FasterHipError):
            S.explore_spread(TEAM_R, TEAM_SPREAD)                            # "reached" needs enable_heading
        assert [name for name, _ in S.explore_spread_stages(TEAM_R, TEAM_SPREAD, want="all")] == ["spread_goals", "set_goals"]
        before = S.vehicles()
        occ = S.map.occupancy()
        views = S.views().reshape(1, -1)
        # the limit as it stands: both take the voxel straight ahead
        K.explore_reachable(TEAM_R, z=TEAM_Z, want="all")
        k_rec, _, k_mask = K.reach_records()
        assert k_mask.tolist() == [1, 1] and k_rec["cell"].tolist() == [ahead, ahead]
        # explore_spread: the model's two voxels
        S.explore_spread(TEAM_R, TEAM_SPREAD, z=TEAM_Z, want="all")
        rec, goals, mask = S.spread_records()
        par = sm.spread_params(TEAM_R, TEAM_SPREAD, r_avoid=float(S.params["goal_radius"]), z_lo=TEAM_Z[0], z_hi=TEAM_Z[1], want=abi.FH_FRONTIER_WANT_ALL)
        grid = (tuple(float(o) for o in sc["origin"]), P["res"], tuple(dims))
        want = sm.spread_goals(par, grid, views.reshape(-1), views.shape[1], np.zeros(2, dtype=np.int32), 1, None, before, occ, sc["origin"], P["res"])
        same((goals, mask, rec), want, "Fleet.explore_spread")
        assert np.array_equal(S.views().reshape(1, -1), views)              # the views are only read
        assert mask.tolist() == [1, 1] and int(rec["cell"][0]) == ahead and int(rec["cell"][1]) != ahead
        assert rec["decided_pass"].tolist() == [1, 2] and rec["lower"].tolist() == [0, 1] and rec["claims"].tolist() == [0, 1] and rec["claimed"][1] > 0
        assert sm.d2_of(goals[0], goals[1]) >= TEAM_SPREAD * TEAM_SPREAD
        assert S.vehicles().tobytes() == hm.set_goals(before, goals, mask, P["wd"]).tobytes()
        S.replan()
        after = S.vehicles()
        assert (after["stage"] == abi.FH_FLEET_STAGE_COMMITTED).all() and (after["active"] == 1).all(), after["stage"]
    finally:
        K.close()
        S.close()


# ---- 5. through Fleet: two teams of four in a closed loop --------------------------------------------------------------------------------------
LOOP_R, LOOP_SPREAD = 3.0, 2.0


def test_two_teams_of_four_explore_an_open_scene():
    """The scene, the periods and the ticks of the closed loop of tests/test_gpu_frontier.py; the eight vehicles read two views, four
    each, and the view is the team.  In every period the outputs of explore_spread are the model's, computed from the views, the
    vehicles and the occupancy read back just before, and whenever a vehicle is given a goal no teammate that is on its way (its
    g_term after set_goals: the goal it held, or the one it has just been given) holds one within r_spread of it."""
    import test_gpu_frontier as tf

    sc = tf.open_scene()
    B = len(sc["starts"])
    team = np.array([0, 0, 0, 0, 1, 1, 1, 1], dtype=np.int32)
    views = np.stack([sc["views"][team == v].min(axis=0) for v in (0, 1)])   # a team knows what one of its four knows
    from faster_amd.fleet import Fleet

    X = Fleet(B, fleet_params(), n_seg=P["N"], max_poly=P["max_poly"], dc=P["dc"], v_max=P["v_max"], a_max=P["a_max"], j_max=P["j_max"],
              decomp_radius=P["decomp_radius"], dist_max_vertexes=P["dist_max_vertexes"])
    grid = (tuple(float(o) for o in sc["origin"]), P["res"], tuple(sc["dims"]))
    log, given = [], 0
    try:
        X.set_map(sc["cloud"], tf.SCENE_CELLS, P["res"], tf.SCENE_CENTER, P["z_max"], 0.1)
        X.init(sc["starts"], sc["goals"])
        X.set_unknown_views(views.copy(), view_of=team, n_views=2, origin=sc["origin"], res=P["res"], dims=sc["dims"])
        X.set_point_views()
        X.enable_heading()
        par = sm.spread_params(LOOP_R, LOOP_SPREAD, r_avoid=float(X.params["goal_radius"]), z_lo=tf.Z_EXPLORE[0], z_hi=tf.Z_EXPLORE[1])
        for c in range(tf.LOOP_PERIODS):
            X.sense(tf.R_SENSE)
            X.observe()
            before = X.vehicles()
            now = X.views().reshape(2, -1)
            X.explore_spread(LOOP_R, LOOP_SPREAD, z=tf.Z_EXPLORE)
            rec, goals, mask = X.spread_records()
            same((goals, mask, rec), sm.spread_goals(par, grid, now.reshape(-1), now.shape[1], team, 2, None, before, sc["occ"], sc["origin"], P["res"]),
                 "period %d" % c)
            after = X.vehicles()
            assert after.tobytes() == hm.set_goals(before, goals, mask, P["wd"]).tobytes(), c
            assert not (rec["flags"] & (abi.FH_SPREAD_OVERFLOW | abi.FH_SPREAD_UNSETTLED)).any()
            for i in np.nonzero(mask)[0]:
                given += 1
                for k in np.nonzero(team == team[i])[0]:
                    if k != i and after["status"][k] != abi.FH_VEHICLE_GOAL_REACHED:
                        assert sm.d2_of(after["g_term"][k], goals[i]) >= LOOP_SPREAD * LOOP_SPREAD, (c, int(i), int(k))
            X.replan()
            log.append((int((rec["flags"] & WANTED != 0).sum()), int(mask.sum()), int(rec["decided_pass"].max()), int(rec["claimed"].sum())))
            X.next_goals(tf.LOOP_TICKS, follow=True)
        print("explore_spread: (wanted, given, last pass, claimed) per period %s; known voxels per team %s" % (log, X.coverage()["known"].tolist()))
        assert given >= 4
    finally:
        X.close()
