"""fh_stake_goals_device on the device (include/fasterhip_stake.h): every byte of d_goals, d_mask and d_records and the whole workspace —
the summary words, the need bytes, every count of every needed view, the class bytes, the groups and `lower` — equal to the Python model
(tests/far_team_model.py) on every named case; tests/test_far_team_model.py shows what each case is for and which wrong variants they
separate.  Where no searcher has a peer, against what fh_prospect_goals_device itself writes on the same device tables; without a gain,
against what fh_apart_goals_device itself writes; and through Fleet two stranded teammates on one view with two unknown regions:
explore_far_gain() gives both the same block, explore_far_team() the model's two different blocks."""
import numpy as np
import pytest

from faster_amd import abi, capi

import far_gain_model as fg
import far_model as fa
import far_spread_model as fs
import far_team_model as ft
from test_far_team_model import unshared
from test_gpu_far import GUARD, POISON, ROOM_Z, FAR_BLOCK, WALL_X, same
from test_gpu_far_gain import device_far_gain, same_work as same_gain_work
from test_gpu_far_spread import R_SPREAD, device_far_spread, pair_fleet, pair_scene
from test_gpu_fleet import P
from test_gpu_reach import dev, grid_record, map_bits

pytestmark = pytest.mark.gpu

REC = abi.far_team_record_dtype.itemsize


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch  # noqa: F401  (torch before the HIP library: one HIP runtime in the process)


def device_far_team(case, par=None):
    """fh_stake_goals_device on device copies of the case's tables into poisoned outputs and a poisoned workspace of exactly the stated
    sizes, with guard bytes on both sides.  A measurement: the inputs and the guards must have the bytes they had.
    -> (goals, mask, records, the workspace's bytes)."""
    import torch

    veh, view_of, skip, group = case["vehicles"], case["view_of"], case["skip"], case.get("group")
    n, n_views = len(veh), case["n_views"]
    par = np.ascontiguousarray(case["par"] if par is None else par).reshape(1)
    bits = map_bits(case["occ"])
    d_f, d_v, d_b = dev(case["flags"]), dev(veh), dev(bits)
    d_vo = None if view_of is None else dev(view_of)
    d_s = None if skip is None else dev(skip)
    d_g = None if group is None else dev(group)
    mz, my, mx = case["occ"].shape
    mg, g = grid_record(case["m_origin"], case["m_res"], (mx, my, mz)), grid_record(*case["grid"])
    work = int(capi.lib().fh_stake_work_bytes(abi.ptr(g), int(par["block"][0]), n_views, n))
    assert work == ft.work_bytes(case["grid"][2], int(par["block"][0]), n_views, n) > 0
    sizes = (24 * n, 4 * n, REC * n, work)
    outs = [torch.full((s + 2 * GUARD,), POISON, dtype=torch.uint8, device="cuda:0") for s in sizes]
    torch.cuda.synchronize()
    ptr = lambda d: None if d is None else d.data_ptr()   # noqa: E731
    rc = capi.lib().fh_stake_goals_device(None, abi.ptr(par), abi.ptr(mg), d_b.data_ptr(), abi.ptr(g), d_f.data_ptr(), case["stride"], ptr(d_vo),
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
    rec = host[2][GUARD:GUARD + sizes[2]].view(abi.far_team_record_dtype).copy()
    return goals, mask, rec, host[3][GUARD:GUARD + work].copy()


def split(case, work, block=None):
    """(the far chooser by gain's part of the workspace, class bytes [n], the padding behind them, groups [n], lower [n])."""
    n, B = len(case["vehicles"]), int(case["par"]["block"] if block is None else block)
    pro = fg.work_bytes(case["grid"][2], B, case["n_views"])
    rows = (n + 63) & ~63
    tail = work[pro:]
    assert len(tail) == rows + 8 * n
    return work[:pro], tail[:n], tail[n:rows], tail[rows:rows + 4 * n].view(np.int32), tail[rows + 4 * n:].view(np.int32)


def same_whole_work(case, work, want, what):
    head, cls, pad, grp, lower = split(case, work)
    same_gain_work(case, head, want[3], want[4], want[5], what)
    assert cls.tobytes() == want[6].tobytes(), (what, "class bytes", cls, want[6])
    assert (pad == POISON).all(), (what, "the bytes behind the class bytes")
    assert grp.tobytes() == want[7].tobytes(), (what, "groups", grp, want[7])
    assert lower.tobytes() == want[8].tobytes(), (what, "lower", lower, want[8])


# ---- 1. every byte equal to the model ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ("gap", "packed"))
@pytest.mark.parametrize("name", list(ft.CASES))
def test_goals_mask_records_and_workspace_equal_the_model(name, layout):
    case = ft.case(name)
    if layout == "packed":
        packed = dict(case)   # view_stride = cells
        cells, stride = case["cells"], case["stride"]
        packed["flags"] = np.concatenate([case["flags"][v * stride: v * stride + cells] for v in range(case["n_views"])])
        packed["stride"] = cells
        case = packed
    else:
        case = ft.with_gap(case, 1)   # gap bytes that say "unknown": they are never read, and never counted
    goals, mask, rec, work = device_far_team(case)
    want = ft.expected(name)
    for k in rec.dtype.names:
        assert rec[k].tobytes() == want[2][k].tobytes(), (name, k, rec[k], want[2][k])
    same((goals, mask, rec), want[:3], name)
    same_whole_work(case, work, want, name)
    idle = np.nonzero(mask == 0)[0]
    assert goals[idle].tobytes() == case["vehicles"]["g_term"][idle].tobytes()   # not chosen: the bits of g_term, NaN and infinity included


def test_two_runs_give_the_same_bytes_and_the_unneeded_view_keeps_its_poison():
    case = ft.case("unneeded_view")
    a, b = device_far_team(case), device_far_team(case)
    same(a[:3], b[:3], "second run")
    assert a[3].tobytes() == b[3].tobytes()
    n_views, W = 3, fa.blocks_of(case["grid"][2], 2)[2]
    words = a[3][:n_views * 4 * W * 8].reshape(n_views, -1)
    counts = a[3][n_views * 4 * W * 8 + 64:n_views * 4 * W * 8 + 64 + n_views * 128 * W].reshape(n_views, -1)
    assert (words[1] == POISON).all() and (counts[1] == POISON).all() and a[3][n_views * 4 * W * 8:][:3].tolist() == [1, 0, 1]
    assert not (counts[0] == POISON).all() and not (counts[2] == POISON).all()
    for name in ("six_faces", "many_claims"):
        case = ft.case(name)
        a, b = device_far_team(case), device_far_team(case)
        same(a[:3], b[:3], "second run of " + name)
        assert a[3].tobytes() == b[3].tobytes()


# ---- 2. (a) where no searcher has a peer: what the far chooser by gain writes ---------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fg.CASES))
def test_without_peers_it_writes_what_the_far_chooser_by_gain_writes(name):
    """Every case of far_gain_model with a copy of its view for every vehicle: goals, mask, the first 64 bytes of every record, gain,
    utility, poor, best_gain and that chooser's part of the workspace are fh_prospect_goals_device's own, on the same tables."""
    case = unshared(dict(fg.case(name), group=None))
    par = ft.from_gain_params(case["par"], r_spread=1.0, claim_blocks=3)
    assert not ft.has_peers(dict(case, par=par))
    g_goals, g_mask, g_rec, g_work = device_far_gain(case)
    goals, mask, rec, work = device_far_team(case, par=par)
    assert goals.tobytes() == g_goals.tobytes() and mask.tobytes() == g_mask.tobytes(), name
    assert rec.view(np.uint8).reshape(len(rec), REC)[:, :64].tobytes() == g_rec.view(np.uint8).reshape(len(rec), 80)[:, :64].tobytes(), name
    for k in ("gain", "utility", "poor", "best_gain"):
        assert rec[k].tobytes() == g_rec[k].tobytes(), (name, k)
    for k in ("lower", "standing", "claims", "claimed", "covered", "removed"):
        assert not rec[k].any(), (name, k)
    assert work[:len(g_work)].tobytes() == g_work.tobytes(), name


# ---- 3. (b) without a gain: what the far chooser for a team writes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fs.CASES))
def test_with_gain_blocks_0_it_writes_what_the_far_chooser_for_a_team_writes(name):
    """gain_blocks 0, hop_cost 1, min_gain 0 and claim_blocks 3 on every case of far_spread_model: goals, mask, the first 96 bytes of
    every record, the summary words, the need bytes and the class / group / lower tail are fh_apart_goals_device's own."""
    case = fs.case(name)
    s_goals, s_mask, s_rec, s_work = device_far_spread(case)
    goals, mask, rec, work = device_far_team(case, par=ft.from_spread_params(case["par"], claim_blocks=3))
    assert goals.tobytes() == s_goals.tobytes() and mask.tobytes() == s_mask.tobytes(), name
    assert rec.view(np.uint8).reshape(len(rec), REC)[:, :96].tobytes() == s_rec.tobytes(), (name, rec, s_rec)
    far = fa.work_bytes(case["grid"][2], int(case["par"]["block"]), case["n_views"])
    pro = fg.work_bytes(case["grid"][2], int(case["par"]["block"]), case["n_views"])
    assert work[:far].tobytes() == s_work[:far].tobytes() and work[pro:].tobytes() == s_work[far:].tobytes(), name
    found = mask == 1
    assert np.array_equal(rec["gain"], np.where(found, 0, -1)) and np.array_equal(rec["utility"], np.where(found, -rec["hops"], 0)), name
    assert not rec["poor"].any(), name


# ---- 4. through Fleet: two stranded teammates on one view, two unknown regions ----------------------------------------------------------------------
def test_explore_far_gain_gives_both_teammates_one_block_and_explore_far_team_two():
    """K21's room with K22's pair: two vehicles in one place that share one view, which knows everything but two regions behind the wall.
    Every vehicle is wanted, so no period has to pass.  explore_far_gain gives both the same block; explore_far_team gives the model's two
    different blocks, the second vehicle's record says what the first one's goal took out of its gains, and set_goals applies both."""
    import heading_model as hm

    sc = pair_scene()
    G, T = pair_fleet(sc), pair_fleet(sc)
    grid = (tuple(float(o) for o in sc["origin"]), P["res"], tuple(sc["dims"]))
    view_of = np.zeros(2, dtype=np.int32)
    try:
        with pytest.raises(capi.FasterHipError, match="explore_far_team first"):
            T.far_team_records()
        with pytest.raises(capi.FasterHipError, match="has not run"):
            T.explore_far_team(FAR_BLOCK, R_SPREAD, 2, after="gain")
        assert [name for name, _ in T.explore_far_team_stages(FAR_BLOCK, R_SPREAD, 2, z=ROOM_Z, want="all")] == ["far_team_goals", "set_goals"]
        work = T.d_far_team_work
        G.explore_far_gain(FAR_BLOCK, 2, z=ROOM_Z, want="all")
        g_rec, g_goals, g_mask = G.far_gain_records()
        assert g_mask.tolist() == [1, 1] and int(g_rec["block_cell"][0]) == int(g_rec["block_cell"][1]) and g_goals[0].tobytes() == g_goals[1].tobytes()
        occ = T.map.occupancy()
        before, views = T.vehicles(), T.views().reshape(1, -1)
        T.explore_far_team(FAR_BLOCK, R_SPREAD, 2, z=ROOM_Z, want="all")
        rec, goals, mask = T.far_team_records()
        par = ft.ftp(FAR_BLOCK, R_SPREAD, 2, FAR_BLOCK * FAR_BLOCK, 0, 2, None, float(T.params["goal_radius"]), ROOM_Z[0], ROOM_Z[1],
                     abi.FH_FRONTIER_WANT_ALL)
        want = ft.far_team_goals(par, grid, views.reshape(-1), views.shape[1], view_of, 1, None, None, before, occ, sc["origin"], P["res"])
        same((goals, mask, rec), want[:3], "Fleet.explore_far_team")
        assert T.vehicles().tobytes() == hm.set_goals(before, goals, mask, P["wd"]).tobytes()
        assert np.array_equal(T.views().reshape(1, -1), views)               # the views are only read
        assert T.d_far_team_work is work                                     # one workspace per lattice, block, views and vehicles
        assert mask.tolist() == [1, 1] and int(rec["block_cell"][0]) != int(rec["block_cell"][1])
        assert int(rec["block_cell"][0]) == int(g_rec["block_cell"][0]) and goals[0].tobytes() == g_goals[0].tobytes()   # the first chooses alone
        assert rec["decided_pass"].tolist() == [1, 2] and int(rec["claims"][1]) == 1 and int(rec["claimed"][1]) >= 1
        assert int(rec["covered"][0]) == 0 and int(rec["removed"][0]) == 0 and int(rec["covered"][1]) > 0 and int(rec["removed"][1]) > 0
        assert int(rec["gain"][1]) > 0 and goals[0][0] > WALL_X and goals[1][0] > WALL_X   # both behind the wall
        e = goals[1] - goals[0]
        assert (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2] >= R_SPREAD ** 2
        print("far_team: blocks %s under explore_far_gain, %s under explore_far_team; gain %s, covered %s, removed %s"
              % (g_rec["block_cell"].tolist(), rec["block_cell"].tolist(), rec["gain"].tolist(), rec["covered"].tolist(), rec["removed"].tolist()))
    finally:
        G.close()
        T.close()
