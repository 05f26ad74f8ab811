"""fh_bid_goals_device on the device (include/fasterhip_bid.h): every byte of d_goals, d_mask and d_records equal to the Python model
(tests/bid_model.py) on every named case — tests/test_bid_model.py shows what each case is for and which wrong variants they separate —
with and without gap bytes in view_stride, into poisoned buffers with guards; two runs and more rounds than needed give the same bytes;
Reduction A against what fh_team_goals_device itself writes on the same device tables; and a team of two with one view before a hall,
the higher index beside it: explore_team() gives the voxel straight ahead to index 0, explore_bid() to the vehicle that stands nearer."""
import numpy as np
import pytest

from faster_amd import abi, capi

import bid_model as bm
import gain_model as gm
import heading_model as hm
import reach_model as rm
from test_gpu_fleet import P
from test_gpu_reach import dev, grid_record, map_bits
from test_gpu_spread import GUARD, POISON, TEAM_R, TEAM_SPREAD, TEAM_Z, team_fleet, team_scene
from test_gpu_team import device_team

pytestmark = pytest.mark.gpu

REC = abi.bid_record_dtype.itemsize
G = 5   # a sensor of 1 m on a lattice of 0.2 m


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch  # noqa: F401  (torch before the HIP library: one HIP runtime in the process)


def device_bid(case, par=None):
    """fh_bid_goals_device on device copies of the case's tables into poisoned outputs, and a poisoned workspace of exactly
    fh_bid_work_bytes(n), with guard bytes on both sides.  A measurement: the inputs and the guards must have the bytes they had."""
    import torch

    veh, view_of, group = case["vehicles"], case["view_of"], case.get("group")
    n = len(veh)
    par = np.ascontiguousarray(case["par"] if par is None else par).reshape(1)
    assert par.dtype == abi.bid_params_dtype
    bits = map_bits(case["occ"])
    d_f, d_v, d_b = dev(case["flags"]), dev(veh), dev(bits)
    d_vo = None if view_of is None else dev(view_of)
    d_gr = None if group is None else dev(group)
    mz, my, mx = case["occ"].shape
    mg, g = grid_record(case["m_origin"], case["m_res"], (mx, my, mz)), grid_record(*case["grid"])
    work = int(capi.lib().fh_bid_work_bytes(n))
    sizes = (24 * n, 4 * n, REC * n, work)
    outs = [torch.full((s + 2 * GUARD,), POISON, dtype=torch.uint8, device="cuda:0") for s in sizes]
    torch.cuda.synchronize()
    rc = capi.lib().fh_bid_goals_device(None, abi.ptr(par), abi.ptr(mg), d_b.data_ptr(), abi.ptr(g), d_f.data_ptr(), case["stride"],
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
    rec = host[2][GUARD:GUARD + sizes[2]].view(abi.bid_record_dtype).copy()
    return goals, mask, rec


def same(got, want, what):
    for name, g, w in zip(("goals", "mask", "records"), got, want):
        assert g.tobytes() == w.tobytes(), (what, name, np.nonzero(got[2] != want[2])[0].tolist()[:8], got[2][got[2] != want[2]][:4], want[2][got[2] != want[2]][:4])


# ---- 1. every byte equal to the model ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gap", ("packed", "gap"))
@pytest.mark.parametrize("name", list(bm.CASES))
def test_goals_mask_and_records_equal_the_model(name, gap):
    case = bm.case(name)
    case = gm.packed(case) if gap == "packed" else rm.with_gap(case, 1)   # (the model of the case as built: the gap bytes are never read)
    assert (case["stride"] == case["cells"]) == (gap == "packed")
    got = device_bid(case)
    same(got, bm.expected(name), name)
    idle = np.nonzero(got[1] == 0)[0]
    assert got[0][idle].tobytes() == case["vehicles"]["g_term"][idle].tobytes()   # not chosen: the bits of g_term
    assert not got[2]["reserved"].any()


def test_two_runs_and_more_rounds_than_needed_give_the_same_bytes():
    for name in ("chain", "flip", "word_edge_winner", "listed_64"):
        first = device_bid(bm.case(name))
        same(device_bid(bm.case(name)), first, name)
        fewest = int(first[2]["decided_pass"].max())
        assert not (first[2]["flags"] & abi.FH_BID_UNSETTLED).any() and fewest >= 3
        same(device_bid(bm.with_par(bm.case(name), passes=fewest)), first, name)              # the fewest rounds that leave nobody unsettled
        same(device_bid(bm.with_par(bm.case(name), passes=abi.FH_BID_MAX_PASSES)), first, name)   # 64 rounds: nothing further is decided
        short = device_bid(bm.with_par(bm.case(name), passes=fewest - 1))
        assert (short[2]["flags"] & abi.FH_BID_UNSETTLED).any()
        same(short, bm.model(bm.with_par(bm.case(name), passes=fewest - 1)), name)


# ---- 2. Reduction A, against the other entry point itself -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bm.REDUCTIONS_A)
def test_reduction_a_equals_what_fh_team_goals_device_returns(name):
    """No searcher has a rival and no list exceeds 32: d_goals, d_mask and every record word except `searches` are those the other
    entry point writes on the same tables."""
    case = bm.case(name)
    goals, mask, rec = device_bid(case)
    k_goals, k_mask, k_rec = device_team(bm.as_team(case))
    assert goals.tobytes() == k_goals.tobytes() and mask.tobytes() == k_mask.tobytes()
    assert bm.as_team_records(rec).tobytes() == k_rec.tobytes()
    assert np.array_equal(rec["searches"], (rec["decided_pass"] == 1).astype(np.int32)) and not rec["rivals"].any()
    same((goals, mask, rec), bm.expected(name), name)


# ---- 3. through Fleet: a team of two before a hall, the higher index beside it ------------------------------------------------------------------
def test_a_team_of_two_before_a_hall_the_nearer_vehicle_gets_the_voxel_straight_ahead():
    sc = team_scene()
    dims = sc["dims"]
    ahead = rm.cell_index(sc["ahead"], dims)
    K, S = team_fleet(sc), team_fleet(sc)
    try:
        with pytest.raises(capi.FasterHipError):
            S.bid_records()                                                  # nothing to read before the first explore_bid
        with pytest.raises(capi.FasterHipError):
            S.explore_bid(TEAM_R, TEAM_SPREAD, G)                            # "reached" needs enable_heading
        assert [name for name, _ in S.explore_bid_stages(TEAM_R, TEAM_SPREAD, G, want="all")] == ["bid_goals", "set_goals"]
        before = S.vehicles()
        assert before["state"]["pos"][1][0] > before["state"]["pos"][0][0]   # vehicle 1 stands two voxels nearer to the hall
        occ = S.map.occupancy()
        views = S.views().reshape(1, -1)
        # the limit as it stands: the index decides, vehicle 0 takes the voxel straight ahead
        K.explore_team(TEAM_R, TEAM_SPREAD, G, z=TEAM_Z, want="all")
        k_rec, _, k_mask = K.team_records()
        assert k_mask.tolist() == [1, 1] and int(k_rec["cell"][0]) == ahead != int(k_rec["cell"][1]) and k_rec["decided_pass"].tolist() == [1, 2]
        # explore_bid: the model's assignment
        S.explore_bid(TEAM_R, TEAM_SPREAD, G, z=TEAM_Z, want="all")
        rec, goals, mask = S.bid_records()
        par = bm.bid_params(TEAM_R, TEAM_SPREAD, G, None, r_avoid=float(S.params["goal_radius"]), z_lo=TEAM_Z[0], z_hi=TEAM_Z[1],
                            want=abi.FH_FRONTIER_WANT_ALL)
        assert int(par["claim_radius"]) == G
        grid = (tuple(float(o) for o in sc["origin"]), P["res"], tuple(dims))
        want = bm.bid_goals(par, grid, views.reshape(-1), views.shape[1], np.zeros(2, dtype=np.int32), 1, None, before, occ, sc["origin"], P["res"])
        same((goals, mask, rec), want, "Fleet.explore_bid")
        assert np.array_equal(S.views().reshape(1, -1), views)              # the views are only read
        assert mask.tolist() == [1, 1] and int(rec["cell"][1]) == ahead != int(rec["cell"][0])
        assert rec["decided_pass"].tolist() == [2, 1] and rec["rivals"].tolist() == [1, 1] and rec["claims"].tolist() == [1, 0]
        assert rec["searches"].tolist() == [2, 1] and int(rec["hops"][1]) < int(k_rec["hops"][0])
        assert bm.sm.d2_of(goals[0], goals[1]) >= TEAM_SPREAD * TEAM_SPREAD
        assert S.vehicles().tobytes() == hm.set_goals(before, goals, mask, P["wd"]).tobytes()
        S.replan()
        after = S.vehicles()
        assert (after["stage"] == abi.FH_FLEET_STAGE_COMMITTED).all() and (after["active"] == 1).all(), after["stage"]
        # the other parameters reach the kernels: one round leaves the loser unsettled
        S.explore_bid(TEAM_R, TEAM_SPREAD, G, z=TEAM_Z, want="all", passes=1)
        rec1, _, mask1 = S.bid_records()
        assert sorted(mask1.tolist()) == [0, 1] and sorted(rec1["decided_pass"].tolist()) == [-1, 1]
        loser = int(np.argmin(mask1))
        assert int(rec1["flags"][loser]) == abi.FH_FRONTIER_WANTED | abi.FH_BID_UNSETTLED and int(rec1["searches"][loser]) == 1
    finally:
        K.close()
        S.close()
