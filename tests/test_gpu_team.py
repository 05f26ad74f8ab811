"""fh_team_goals_device on the device (include/fasterhip_team.h): every byte of d_goals, d_mask and d_records equal to the Python model
(tests/team_model.py) on every named case — tests/test_team_model.py shows what each case is for and which wrong variants they
separate — with and without gap bytes in view_stride, into poisoned buffers with guards; the two reductions against what
fh_spread_goals_device and fh_gain_goals_device themselves return on the same device tables; and a team of two with one view before a
hall, which explore_gain() sends to one voxel and explore_team() to two whose balls share no counted voxel."""
import numpy as np
import pytest

from faster_amd import abi, capi

import gain_model as gm
import heading_model as hm
import reach_model as rm
import spread_model as sm
import team_model as tm
from test_gpu_fleet import P
from test_gpu_gain import device_gain
from test_gpu_reach import dev, grid_record, map_bits
from test_gpu_spread import GUARD, POISON, TEAM_R, TEAM_SPREAD, TEAM_Z, device_spread, team_fleet, team_scene

pytestmark = pytest.mark.gpu

REC = abi.team_record_dtype.itemsize
G = 5   # a sensor of 1 m on a lattice of 0.2 m


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch  # noqa: F401  (torch before the HIP library: one HIP runtime in the process)


def device_team(case, par=None):
    """fh_team_goals_device on device copies of the case's tables into poisoned outputs, and a poisoned workspace of exactly
    fh_spread_work_bytes(n), with guard bytes on both sides.  A measurement: the inputs and the guards must have the bytes they had."""
    import torch

    veh, view_of, group = case["vehicles"], case["view_of"], case.get("group")
    n = len(veh)
    par = np.ascontiguousarray(case["par"] if par is None else par).reshape(1)
    assert par.dtype == abi.team_params_dtype
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
    rc = capi.lib().fh_team_goals_device(None, abi.ptr(par), abi.ptr(mg), d_b.data_ptr(), abi.ptr(g), d_f.data_ptr(), case["stride"],
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
    rec = host[2][GUARD:GUARD + sizes[2]].view(abi.team_record_dtype).copy()
    return goals, mask, rec


def same(got, want, what):
    for name, g, w in zip(("goals", "mask", "records"), got, want):
        assert g.tobytes() == w.tobytes(), (what, name, np.nonzero(got[2] != want[2])[0].tolist()[:8], got[2][got[2] != want[2]][:4], want[2][got[2] != want[2]][:4])


# ---- 1. every byte equal to the model ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gap", ("packed", "gap"))
@pytest.mark.parametrize("name", list(tm.CASES))
def test_goals_mask_and_records_equal_the_model(name, gap):
    case = tm.case(name)
    case = gm.packed(case) if gap == "packed" else rm.with_gap(case, 1)   # (the model of the case as built: the gap bytes are never read)
    assert (case["stride"] == case["cells"]) == (gap == "packed")
    got = device_team(case)
    same(got, tm.expected(name), name)
    idle = np.nonzero(got[1] == 0)[0]
    assert got[0][idle].tobytes() == case["vehicles"]["g_term"][idle].tobytes()   # not chosen: the bits of g_term
    assert not got[2]["reserved"].any() and not got[2]["reserved0"].any()


def test_two_runs_and_more_passes_than_needed_give_the_same_bytes():
    for name in ("chain_passes_3", "word_edge_claim", "two_claims"):
        first = device_team(tm.case(name))
        same(device_team(tm.case(name)), first, name)
        same(device_team(tm.with_par(tm.case(name), passes=abi.FH_TEAM_MAX_PASSES)), first, name)
    assert int(tm.case("chain_passes_3")["par"]["passes"]) == 3 == int(tm.expected("chain_passes_3")[2]["decided_pass"].max())


# ---- 2. the reductions, against the two entry points themselves --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sm.CASES))
def test_reduction_a_equals_what_fh_spread_goals_device_returns(name):
    """claim_radius -1, gain_radius 0, hop_cost 1, min_gain 0 on the tables of the spread cases: d_goals, d_mask and the first 64 bytes of
    every record are those the other entry point writes on the same tables."""
    case = tm.case("A:" + name)
    assert case["flags"] is sm.case(name)["flags"] and case["vehicles"] is sm.case(name)["vehicles"]
    goals, mask, rec = device_team(case)
    k_goals, k_mask, k_rec = device_spread(sm.case(name))
    assert goals.tobytes() == k_goals.tobytes() and mask.tobytes() == k_mask.tobytes()
    assert all(rec[i].tobytes()[:64] == k_rec[i].tobytes() for i in range(len(rec)))
    same((goals, mask, rec), tm.expected("A:" + name), name)
    found = mask == 1
    assert (rec["gain"][found] == 0).all() and (rec["gain"][~found] == -1).all() and not rec["covered"].any() and not rec["poor"].any()


@pytest.mark.parametrize("name", list(gm.CASES))
def test_reduction_b_equals_what_fh_gain_goals_device_returns(name):
    """Every vehicle a group of its own, so no searcher has a peer: d_goals and d_mask are those fh_gain_goals_device writes on the
    tables of the gain cases, bytes 0 .. 39 of every record its record's with bit 128 read as bit 1024, bytes 64 .. 79 its 40 .. 55."""
    case = tm.case("B:" + name)
    goals, mask, rec = device_team(case)
    k_goals, k_mask, k_rec = device_gain(gm.case(name))
    assert goals.tobytes() == k_goals.tobytes() and mask.tobytes() == k_mask.tobytes()
    as_team = k_rec.copy()
    as_team["flags"] = tm.as_team_flags(k_rec["flags"])
    as_team["view"] = rec["view"]   # (a copy of its view under an index of its own: the one word that differs, see spread_model.own_groups)
    for i in range(len(rec)):
        assert rec[i].tobytes()[:40] == as_team[i].tobytes()[:40], (name, i)
        assert rec[i].tobytes()[64:80] == k_rec[i].tobytes()[40:56], (name, i)
    same((goals, mask, rec), tm.expected("B:" + name), name)


# ---- 3. through Fleet: a team of two before a hall ---------------------------------------------------------------------------------------------
def test_a_team_of_two_is_sent_to_one_voxel_by_explore_gain_and_to_two_by_explore_team():
    sc = team_scene()
    dims = sc["dims"]
    ahead = rm.cell_index(sc["ahead"], dims)
    K, S = team_fleet(sc), team_fleet(sc)
    try:
        with pytest.raises(capi.FasterHipError):
            S.team_records()                                                 # nothing to read before the first explore_team
        with pytest.raises(capi.FasterHipError):
            S.explore_team(TEAM_R, TEAM_SPREAD, G)                           # "reached" needs enable_heading
        assert [name for name, _ in S.explore_team_stages(TEAM_R, TEAM_SPREAD, G, want="all")] == ["team_goals", "set_goals"]
        before = S.vehicles()
        occ = S.map.occupancy()
        views = S.views().reshape(1, -1)
        # the limit as it stands: both take the voxel straight ahead
        K.explore_gain(TEAM_R, G, z=TEAM_Z, want="all")
        k_rec, _, k_mask = K.gain_records()
        assert k_mask.tolist() == [1, 1] and k_rec["cell"].tolist() == [ahead, ahead]
        # explore_team: the model's two voxels
        S.explore_team(TEAM_R, TEAM_SPREAD, G, z=TEAM_Z, want="all")
        rec, goals, mask = S.team_records()
        par = tm.team_params(TEAM_R, TEAM_SPREAD, G, None, r_avoid=float(S.params["goal_radius"]), z_lo=TEAM_Z[0], z_hi=TEAM_Z[1],
                             want=abi.FH_FRONTIER_WANT_ALL)
        assert int(par["claim_radius"]) == G
        grid = (tuple(float(o) for o in sc["origin"]), P["res"], tuple(dims))
        details = {}
        want = tm.team_goals(par, grid, views.reshape(-1), views.shape[1], np.zeros(2, dtype=np.int32), 1, None, before, occ, sc["origin"], P["res"],
                             details=details)
        same((goals, mask, rec), want, "Fleet.explore_team")
        assert np.array_equal(S.views().reshape(1, -1), views)              # the views are only read
        assert mask.tolist() == [1, 1] and int(rec["cell"][0]) == ahead and int(rec["cell"][1]) != ahead
        assert rec["decided_pass"].tolist() == [1, 2] and rec["lower"].tolist() == [0, 1] and rec["claims"].tolist() == [0, 1]
        assert sm.d2_of(goals[0], goals[1]) >= TEAM_SPREAD * TEAM_SPREAD
        # no covered voxel is counted in the second's gain: its ball, counted voxel by voxel without the covered ones, is its gain
        info = details[1]
        nx, ny = dims[0], dims[1]
        c1 = int(rec["cell"][1])
        second = (c1 % nx, (c1 // nx) % ny, c1 // (nx * ny))
        assert int(rec["covered"][1]) == int(info["cov"].sum()) == int(k_rec["gain"][0]) > 0   # the ball of the first vehicle's goal, all of it in the box
        assert int(rec["gain"][1]) == gm._fast_gain(second, info["lo"], info["hi"], info["unknown"] & ~info["cov"], G)
        assert int(rec["gain"][1]) <= gm._fast_gain(second, info["lo"], info["hi"], info["unknown"], G)
        assert S.vehicles().tobytes() == hm.set_goals(before, goals, mask, P["wd"]).tobytes()
        S.replan()
        after = S.vehicles()
        assert (after["stage"] == abi.FH_FLEET_STAGE_COMMITTED).all() and (after["active"] == 1).all(), after["stage"]
        # the other parameters reach the kernels: claims that cover nothing, and a minimum above every gain
        S.explore_team(TEAM_R, TEAM_SPREAD, G, claim_radius=-1, z=TEAM_Z, want="all")
        rec2 = S.team_records()[0]
        assert not rec2["covered"].any() and int(rec2["claimed"][1]) > 0
        S.explore_team(TEAM_R, TEAM_SPREAD, G, min_gain=60000, z=TEAM_Z, want="all", passes=1)
        rec3, _, mask3 = S.team_records()
        assert mask3.tolist() == [0, 0] and int(rec3["flags"][0]) == abi.FH_FRONTIER_WANTED | abi.FH_TEAM_ALL_POOR
        assert int(rec3["flags"][1]) == abi.FH_FRONTIER_WANTED | abi.FH_TEAM_UNSETTLED
    finally:
        K.close()
        S.close()
