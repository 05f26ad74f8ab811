"""fh_prospect_goals_device on the device (include/fasterhip_prospect.h): every byte of d_goals, d_mask and d_records, the summary words,
the need bytes and EVERY count of every needed view equal to the Python model (tests/far_gain_model.py) on every named case —
tests/test_far_gain_model.py shows what each case is for and which wrong variants they separate; with gain_blocks 0 against what
fh_far_goals_device itself writes on the same device tables; and a vehicle in a known room with a one-voxel hole of unknown space in the
block next to it and an unexplored region round a wall: explore_far() sends it to the hole, explore_far_gain() round the wall."""
import numpy as np
import pytest

from faster_amd import abi, capi

import far_gain_model as fg
import far_model as fa
import heading_model as hm
from test_gpu_far import GUARD, POISON, ROOM_CELLS, ROOM_CENTER, ROOM_Z, WALL_X, FAR_BLOCK, device_far, room_scene, same
from test_gpu_fleet import P, fleet_params
from test_gpu_reach import dev, grid_record, map_bits

pytestmark = pytest.mark.gpu

WANTED, FOUND = abi.FH_FRONTIER_WANTED, abi.FH_FRONTIER_FOUND


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch  # noqa: F401  (torch before the HIP library: one HIP runtime in the process)


def device_far_gain(case, par=None):
    """fh_prospect_goals_device on device copies of the case's tables, the map's bits packed from its occupancy, into poisoned outputs
    and a poisoned workspace of exactly the stated sizes with guard bytes on both sides.  A measurement: the inputs and the guards must
    have the bytes they had.  -> (goals, mask, records, the workspace's bytes)."""
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
    work = int(capi.lib().fh_prospect_work_bytes(abi.ptr(g), int(par["block"][0]), n_views))
    assert work == fg.work_bytes(case["grid"][2], int(par["block"][0]), n_views) > 0
    sizes = (24 * n, 4 * n, 80 * n, work)
    outs = [torch.full((s + 2 * GUARD,), POISON, dtype=torch.uint8, device="cuda:0") for s in sizes]
    torch.cuda.synchronize()
    rc = capi.lib().fh_prospect_goals_device(None, abi.ptr(par), abi.ptr(mg), d_b.data_ptr(), abi.ptr(g), d_f.data_ptr(), case["stride"],
                                             None if d_vo is None else d_vo.data_ptr(), n_views, None if d_s is None else d_s.data_ptr(),
                                             d_v.data_ptr(), n, outs[3].data_ptr() + GUARD, work, *(o.data_ptr() + GUARD for o in outs[:3]))
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
    rec = host[2][GUARD:GUARD + sizes[2]].view(abi.far_gain_record_dtype).copy()
    return goals, mask, rec, host[3][GUARD:GUARD + work].copy()


def split_work(case, work, block=None):
    """(words [n_views][4][W] uint64, need bytes, counts [n_views][64 W] uint16) of a workspace."""
    n_views = case["n_views"]
    W = fa.blocks_of(case["grid"][2], int(case["par"]["block"] if block is None else block))[2]
    a, b = n_views * 4 * W * 8, n_views * 4 * W * 8 + ((n_views + 63) & ~63)
    return work[:a].view(np.uint64).reshape(n_views, 4, W), work[a:b], work[b:].view(np.uint16).reshape(n_views, 64 * W)


def same_work(case, work, sums, need, counts, what):
    """The workspace against the model: the four bitmaps and every count of every needed view, poison in those of the others, and the
    need bytes."""
    words, need_bytes, table = split_work(case, work)
    assert set(sums) == set(counts)
    for v in range(case["n_views"]):
        if v in sums:
            assert words[v].tobytes() == sums[v].tobytes(), (what, "summary of view", v, words[v], sums[v])
            assert table[v].tobytes() == counts[v].tobytes(), (what, "counts of view", v, np.nonzero(table[v] != counts[v])[0].tolist())
        else:
            assert (words[v].view(np.uint8) == POISON).all() and (table[v].view(np.uint8) == POISON).all(), (what, "view nobody needs", v)
    assert need_bytes.tobytes() == need.tobytes(), (what, "need bytes")


# ---- 1. every byte equal to the model ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ("gap", "packed"))
@pytest.mark.parametrize("name", list(fg.CASES))
def test_goals_mask_records_and_workspace_equal_the_model(name, layout):
    case = fg.case(name)
    if layout == "packed":
        packed = dict(case)   # view_stride = cells
        cells, stride = case["cells"], case["stride"]
        packed["flags"] = np.concatenate([case["flags"][v * stride: v * stride + cells] for v in range(case["n_views"])])
        packed["stride"] = cells
        case = packed
    else:
        case = fg.with_gap(case, 1)   # gap bytes that say "unknown": they are never read, and never counted
    goals, mask, rec, work = device_far_gain(case)
    want = fg.expected(name)
    for k in rec.dtype.names:
        assert rec[k].tobytes() == want[2][k].tobytes(), (name, k, rec[k], want[2][k])
    same((goals, mask, rec), want[:3], name)
    same_work(case, work, want[3], want[4], want[5], name)
    idle = np.nonzero(mask == 0)[0]
    assert goals[idle].tobytes() == case["vehicles"]["g_term"][idle].tobytes()   # not chosen: the bits of g_term, NaN and infinity included


def test_two_runs_give_the_same_bytes_and_the_unneeded_view_keeps_its_poison():
    case = fg.case("shared_view")
    a, b = device_far_gain(case), device_far_gain(case)
    same(a[:3], b[:3], "second run")
    assert a[3].tobytes() == b[3].tobytes()
    words, need, table = split_work(case, a[3])
    assert (words[1].view(np.uint8) == POISON).all() and (table[1].view(np.uint8) == POISON).all() and need[:3].tolist() == [1, 0, 1]
    assert not (table[0].view(np.uint8) == POISON).all() and not (table[2].view(np.uint8) == POISON).all()
    case = fg.case("faces")
    a, b = device_far_gain(case), device_far_gain(case)
    same(a[:3], b[:3], "second run of faces")
    assert a[3].tobytes() == b[3].tobytes()


# ---- 2. without a gain: what the chooser without one writes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fa.CASES))
def test_with_gain_blocks_0_it_writes_what_the_chooser_without_a_gain_writes(name):
    """gain_blocks 0, hop_cost 1, min_gain 0 on every case of far_model: goals, mask, the first 64 bytes of every record, the summary
    words and the need bytes are fh_far_goals_device's own, on the same tables."""
    case = fa.case(name)
    f_goals, f_mask, f_rec, f_work = device_far(case)
    goals, mask, rec, work = device_far_gain(case, par=fg.reduction_params(case["par"]))
    assert goals.tobytes() == f_goals.tobytes() and mask.tobytes() == f_mask.tobytes(), name
    head = rec.view(np.uint8).reshape(len(rec), 80)
    assert head[:, :64].tobytes() == f_rec.tobytes(), (name, rec, f_rec)
    found = mask == 1
    assert np.array_equal(rec["gain"], np.where(found, 0, -1)) and np.array_equal(rec["utility"], np.where(found, -rec["hops"], 0)), name
    assert not rec["poor"].any() and np.array_equal(rec["best_gain"], np.where(rec["reachable"] > 0, 0, -1)), name
    assert work[:len(f_work)].tobytes() == f_work.tobytes(), name   # the first two parts of the workspace


# ---- 3. through Fleet: a hole next door, an unexplored region round the wall ---------------------------------------------------------------------
R_NEAR = 1.2   # the sensor's range and explore_reachable's r_max in this scene: the hole, 1.5 m in x from the vehicle's path, lies beyond both
HOLE = (1.0, 2.6, 1.0)   # the centre of a voxel: the lattice has res 0.2 and its voxel centres at multiples of 0.2
PERIODS, TICKS = 10, 100


def hole_scene():
    """K21's room scene (tests/test_gpu_far.py): 12 m x 8 m x 2.8 m, a wall at x = 5.1 with a gap of 2.4 m, vehicle 0 at (2.5, 2, 1) on
    its way to (2.5, 3, 1), everything with x < 8 known to it.  Added: the voxel around HOLE is unknown in its view, 1.5 m to the side of
    the vehicle's path: a block step or two away at FAR_BLOCK = 8 (blocks of 1.6 m), while the region x > 8 lies 5.5 m away, beyond the
    wall's block."""
    sc = room_scene()
    res, dims, origin = P["res"], sc["dims"], sc["origin"]
    cell = [int(np.floor((HOLE[k] - origin[k]) / res)) for k in range(3)]
    views = sc["views"].reshape(2, dims[2], dims[1], dims[0])
    assert views[0][cell[2], cell[1], cell[0]] == 0
    assert all(abs((cell[k] + 0.5) * res + origin[k] - HOLE[k]) < 1e-9 for k in range(3))   # (no voxel boundary near the point)
    views[0][cell[2], cell[1], cell[0]] = 1
    sc["hole_cell"] = (cell[2] * dims[1] + cell[1]) * dims[0] + cell[0]
    return sc


def hole_fleet(sc):
    from faster_amd.fleet import Fleet

    fl = Fleet(2, fleet_params(), n_seg=P["N"], max_poly=P["max_poly"], dc=P["dc"], v_max=P["v_max"], a_max=P["a_max"], j_max=P["j_max"],
               decomp_radius=P["decomp_radius"], dist_max_vertexes=P["dist_max_vertexes"])
    fl.set_map(sc["cloud"], ROOM_CELLS, P["res"], ROOM_CENTER, P["z_max"], P["inflation"])
    fl.init(sc["starts"], sc["goals"])
    fl.set_unknown_views(sc["views"].copy(), origin=sc["origin"], res=P["res"], dims=sc["dims"])
    fl.set_point_views()
    fl.enable_heading()
    return fl


def test_explore_far_takes_the_hole_next_door_and_explore_far_gain_the_region_round_the_wall():
    """Two fleets, PERIODS periods of sense -> observe -> explore_reachable -> the far chooser (after="reachable") -> replan -> next
    goals; fleet K uses explore_far(8), fleet G explore_far_gain(8, 2).  Every call of either chooser is compared with its model on the
    tables it read.  When vehicle 0 has arrived, K's first far goal is a voxel beside the hole, a block step or two away, and G's is the
    model's voxel at the edge of the unknown region, beyond the wall; G's vehicle commits a plan to it, and after PERIODS periods its
    view knows more voxels than K's."""
    sc = hole_scene()
    K, G = hole_fleet(sc), hole_fleet(sc)
    grid = (tuple(float(o) for o in sc["origin"]), P["res"], tuple(sc["dims"]))
    nx, ny = sc["dims"][0], sc["dims"][1]
    try:
        occ = G.map.occupancy()
        with pytest.raises(capi.FasterHipError):
            G.far_gain_records()                                        # nothing to read before the first explore_far_gain
        with pytest.raises(capi.FasterHipError, match="has not run"):
            G.explore_far_gain(FAR_BLOCK, 2, after="gain")              # that chooser has not run
        G.explore_reachable(R_NEAR, z=ROOM_Z)
        assert [name for name, _ in G.explore_far_gain_stages(FAR_BLOCK, 2, z=ROOM_Z, after="reachable")] == ["far_gain_goals", "set_goals"]
        work = G.d_far_gain_work
        known0 = [int(k) for k in G.coverage()["known"]]
        assert [int(k) for k in K.coverage()["known"]] == known0
        first_k = first_g = first_active = None
        log = []
        for c in range(PERIODS):
            for fl in (K, G):
                fl.sense(R_NEAR)
                fl.observe()
                fl.explore_reachable(R_NEAR, z=ROOM_Z)
            # K: the chooser without a gain
            before, views, k_mask = K.vehicles(), K.views().reshape(2, -1), K.reach_records()[2]
            K.explore_far(FAR_BLOCK, z=ROOM_Z, after="reachable")
            rec, goals, mask = K.far_records()
            par = fa.far_params(FAR_BLOCK, float(K.params["goal_radius"]), ROOM_Z[0], ROOM_Z[1], abi.FH_FRONTIER_WANT_REACHED)
            want = fa.far_goals(par, grid, views.reshape(-1), views.shape[1], None, 2, k_mask, before, occ, sc["origin"], P["res"])
            same((goals, mask, rec), want[:3], "Fleet.explore_far, period %d" % c)
            if first_k is None and int(mask[0]) == 1:
                first_k = (c, int(rec["cell"][0]), int(rec["hops"][0]), goals[0].copy())
            # G: with the gain
            before, views, g_mask = G.vehicles(), G.views().reshape(2, -1), G.reach_records()[2]
            G.explore_far_gain(FAR_BLOCK, 2, z=ROOM_Z, after="reachable")
            rec, goals, mask = G.far_gain_records()
            par = fg.fgp(FAR_BLOCK, 2, FAR_BLOCK * FAR_BLOCK, 0, float(G.params["goal_radius"]), ROOM_Z[0], ROOM_Z[1], abi.FH_FRONTIER_WANT_REACHED)
            want = fg.far_gain_goals(par, grid, views.reshape(-1), views.shape[1], None, 2, g_mask, before, occ, sc["origin"], P["res"])
            same((goals, mask, rec), want[:3], "Fleet.explore_far_gain, period %d" % c)
            assert G.vehicles().tobytes() == hm.set_goals(before, goals, mask, P["wd"]).tobytes(), c
            assert np.array_equal(G.views().reshape(2, -1), views)       # the views are only read
            if first_g is None and int(mask[0]) == 1:
                first_g = (c, int(rec["cell"][0]), int(rec["hops"][0]), goals[0].copy(), int(rec["gain"][0]), int(rec["utility"][0]))
                assert int(before["status"][0]) == abi.FH_VEHICLE_GOAL_REACHED and int(g_mask[0]) == 0
            for fl in (K, G):
                fl.replan()
            after = G.vehicles()
            assert int(after["stage"][0]) != abi.FH_FLEET_STAGE_NO_PATH, c
            if first_g is not None and first_active is None and int(after["active"][0]) == 1:
                first_active = c
                assert int(after["stage"][0]) == abi.FH_FLEET_STAGE_COMMITTED, (c, int(after["stage"][0]))
            log.append((int(before["status"][0]), int(mask[0]), int(rec["hops"][0]), int(rec["gain"][0]), int(after["stage"][0]), int(after["active"][0])))
            for fl in (K, G):
                fl.next_goals(TICKS, follow=True)
        known_k, known_g = [int(k) for k in K.coverage()["known"]], [int(k) for k in G.coverage()["known"]]
        print("far gain: (status, mask, hops, gain, stage, active) of vehicle 0 per period %s; first goal without gain %s, with gain %s, "
              "first active replan %s; known %s -> %s with gain, %s without" % (log, first_k, first_g, first_active, known0, known_g, known_k))
        assert G.d_far_gain_work is work                                # one workspace per lattice, block and number of views
        assert first_k is not None and first_g is not None and first_active is not None and first_active > first_g[0]
        # without a gain: a voxel that touches the hole, the fewest block steps away
        hole = sc["hole_cell"]
        assert 0 <= first_k[2] <= 2 and first_k[1] - hole in (1, -1, nx, -nx, nx * ny, -nx * ny), (first_k, hole)
        # with it: beyond the wall, more steps away, with a gain of hundreds of voxels that outweighs them
        assert first_g[2] > first_k[2] and first_g[3][0] > WALL_X and first_g[4] > 500 and first_g[5] > 0, first_g
        assert known_g[0] > known_k[0] >= known0[0] and known_g[1] == known_k[1] == known0[1]
    finally:
        K.close()
        G.close()
