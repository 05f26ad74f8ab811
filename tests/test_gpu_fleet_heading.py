"""GPU tests of the fleet's heading (fh_heading: fh_fleet_next_goals_yaw_device, fh_fleet_set_goals_device, fh_fleet_sense_fov_device,
the look_at write of fh_safe_corridor_batch_device; faster_amd/fleet.py): the yaw kernel is the model of tests/heading_model.py
exactly, new goals are setTerminalGoal, the forward sensor is the numpy model byte for byte, and a fleet that never enables heading
computes what it computed before; and in closed loop — forward sense, replan, next goals with yaw, new goals after arrival — every
vehicle stays where the host Planner is (tests/cpp/test_replan_fleet_heading.cpp)."""
import math
import os
import subprocess

import numpy as np
import pytest

from faster_amd import abi, capi

import heading_model as hm
from test_gpu_fleet import P, fleet_params, make_fleet, scenario
from test_gpu_fleet_views import forest_map

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_STATES = 48


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch  # noqa: F401  (torch before the HIP library: one HIP runtime in the process)


def to_dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def yaw_inputs():
    """heading_model.yaw_case as the device's records: plans stored from a head that is not always 0; vehicle 7 has an empty plan."""
    case = hm.yaw_case()
    n = len(case["status"])
    veh = np.zeros(n, dtype=abi.vehicle_dtype)
    veh["status"], veh["g_term"], veh["plan_size"], veh["plan_head"] = case["status"], case["g_term"], case["size"], np.arange(n) % 5
    veh["plan_size"][7] = 0
    plans = np.zeros((n, MAX_STATES), dtype=abi.state_dtype)
    rng = np.random.default_rng(1)
    for i in range(n):
        h, s = veh["plan_head"][i], case["size"][i]
        plans["pos"][i, h:h + s] = case["plans"][i, :s]
        plans["vel"][i, h:h + s] = rng.uniform(-1, 1, size=(s, 3))
    veh["state"] = plans[np.arange(n), veh["plan_head"]]
    head = np.zeros(n, dtype=abi.heading_dtype)
    head["yaw"], head["previous_yaw"], head["dyaw_filtered"], head["look_at"] = case["yaw0"], case["prev0"], case["dyaw0"], case["look_at"]
    head["dir"] = 7.0   # (must be overwritten)
    return case, veh, plans, head


@pytest.fixture(scope="module")
def yaw_data():
    return yaw_inputs()


@pytest.mark.parametrize("alpha", [0.0, 0.92])
@pytest.mark.parametrize("follow", [0, 1])
def test_yaw_kernel_equals_the_model(yaw_data, follow, alpha):
    """257 vehicles (one past a block), plans of 1 .. 40 states, all four statuses, targets ahead, behind and across the +-pi cut, ticks
    before, at and past the end of the plan: status, yaw, previous_yaw, dyaw_filtered, goal_yaw, goal_dyaw equal the model EXACTLY (the
    inputs keep clear of the thresholds where atan2's last bit could decide: asserted on the CPU in test_fleet_heading_abi.py); dir is
    (cos, sin) of previous_yaw within 1e-15; goals, plan cursor and state equal fh_fleet_next_goals_device bit for bit."""
    case, veh, plans, head = yaw_data
    n = len(veh)
    yp = abi.default_yaw_params(0.01)
    yp["alpha_filter_dyaw"] = alpha
    ctx = capi.Context(0)
    try:
        d_plans = to_dev(plans)
        for ticks in hm.YAW_TICKS:
            d_v, d_v2, d_h = to_dev(veh), to_dev(veh), to_dev(head)
            d_g, d_g2 = to_dev(np.ones(n, dtype=abi.state_dtype)), to_dev(np.ones(n, dtype=abi.state_dtype))
            d_gy = to_dev(np.full((n, 2), 9.0))
            ctx.fleet_next_goals_yaw_device(yp, d_v.data_ptr(), d_plans.data_ptr(), d_h.data_ptr(), n, MAX_STATES, ticks, follow, d_g.data_ptr(),
                                            d_gy.data_ptr())
            ctx.fleet_next_goals_device(d_v2.data_ptr(), d_plans.data_ptr(), n, MAX_STATES, ticks, follow, d_g2.data_ptr())
            ctx.sync()
            v, v2 = d_v.cpu().numpy().view(abi.vehicle_dtype), d_v2.cpu().numpy().view(abi.vehicle_dtype)
            h = d_h.cpu().numpy().view(abi.heading_dtype)
            gy = d_gy.cpu().numpy().view(np.float64).reshape(n, 2)
            where = "ticks %d follow %d alpha %g" % (ticks, follow, alpha)
            assert d_g.cpu().numpy().tobytes() == d_g2.cpu().numpy().tobytes(), where
            plain = v.copy()
            plain["status"] = v2["status"]
            assert plain.tobytes() == v2.tobytes(), where                      # everything but the status is the plain entry's
            st, hs, near = hm.yaw_case_model(case, ticks, follow, alpha)
            assert near == 0
            for i in range(n):
                if i == 7:   # empty plan: untouched
                    assert v[i].tobytes() == veh[i].tobytes() and h[i].tobytes() == head[i].tobytes() and tuple(gy[i]) == (0.0, 0.0), where
                    continue
                m = hs[i]
                got = (int(v["status"][i]), h["yaw"][i], h["previous_yaw"][i], h["dyaw_filtered"][i], h["goal_yaw"][i], h["goal_dyaw"][i])
                want = (int(st[i]), m["yaw"], m["previous_yaw"], m["dyaw_filtered"], m["goal_yaw"], m["goal_dyaw"])
                assert got == want, (where, i, int(case["status"][i]), got, want)
                assert tuple(gy[i]) == (m["goal_yaw"], m["goal_dyaw"]), (where, i)
                assert abs(h["dir"][i][0] - math.cos(m["previous_yaw"])) <= 1e-15 and abs(h["dir"][i][1] - math.sin(m["previous_yaw"])) <= 1e-15, (where, i)
                assert np.array_equal(h["look_at"][i], head["look_at"][i])
            if follow == 0:
                assert np.array_equal(h["yaw"], head["yaw"]), where
    finally:
        ctx.close()


def test_yaw_ticks_out_of_range_are_refused(yaw_data):
    _, veh, plans, head = yaw_data
    n = len(veh)
    ctx = capi.Context(0)
    try:
        d_v, d_p, d_h, d_g, d_gy = to_dev(veh), to_dev(plans), to_dev(head), to_dev(np.zeros(n, dtype=abi.state_dtype)), to_dev(np.zeros((n, 2)))
        for ticks in (0, 65537):
            with pytest.raises(capi.FasterHipError) as e:
                ctx.fleet_next_goals_yaw_device(abi.default_yaw_params(), d_v.data_ptr(), d_p.data_ptr(), d_h.data_ptr(), n, MAX_STATES, ticks, 1,
                                                d_g.data_ptr(), d_gy.data_ptr())
            assert "rc=-1" in str(e.value)
        ctx.sync()
        assert d_v.cpu().numpy().tobytes() == veh.tobytes() and d_h.cpu().numpy().tobytes() == head.tobytes()
    finally:
        ctx.close()


def test_heading_init_writes_the_records():
    yaw0 = np.array([0.0, math.pi / 2, -math.pi / 2, math.pi, 1.234, -2.5])
    ctx = capi.Context(0)
    try:
        for src in (yaw0, None):
            d_h = to_dev(np.full(6 * abi.heading_dtype.itemsize, 0xff, dtype=np.uint8))
            d_y = None if src is None else to_dev(src)
            ctx.fleet_heading_init_device(None if d_y is None else d_y.data_ptr(), 6, d_h.data_ptr())
            ctx.sync()
            h = d_h.cpu().numpy().view(abi.heading_dtype)
            want = np.zeros(6) if src is None else src
            assert np.array_equal(h["yaw"], want) and np.array_equal(h["previous_yaw"], want)
            for f in ("dyaw_filtered", "goal_yaw", "goal_dyaw", "look_at", "reserved"):
                assert not h[f].any(), f
            assert np.abs(h["dir"][:, 0] - np.cos(want)).max() <= 1e-15 and np.abs(h["dir"][:, 1] - np.sin(want)).max() <= 1e-15
            assert tuple(h["dir"][0]) == (1.0, 0.0)
    finally:
        ctx.close()


def test_set_goals_is_set_terminal_goal():
    """One vehicle per status (twice: the second four behind a mask of zeros): status, g_term and the projected goal equal the model
    exactly; the projected goal is what fh_fleet_begin_device writes for the same state; a YAWING vehicle goes through begin inactive
    with stage NONE, and one inside goal_radius of its new goal becomes GOAL_REACHED there."""
    par = fleet_params()
    n = 10
    veh = np.zeros(n, dtype=abi.vehicle_dtype)
    veh["status"] = [0, 1, 2, 3, 0, 1, 2, 3, 2, 3]
    veh["state"]["pos"] = np.random.default_rng(4).uniform([2, 2, 0.5], [18, 18, 2.5], size=(n, 3))
    veh["plan_size"], veh["stage"], veh["active"] = 1, 5, 1
    veh["whole_init"], veh["whole_final"], veh["whole_inc"], veh["safe_init"], veh["safe_final"], veh["safe_inc"] = 1, 10, 1, 1, 10, 1
    veh["g_term"] = veh["state"]["pos"] + 100.0
    goals = veh["state"]["pos"] + np.array([[1.0, 0.5, 0.2], [30.0, 2.0, 0.1], [2.0, -20.0, 0.5], [0.5, 0.0, 9.0], [-11.0, 12.0, 3.0], [3.0, 3.0, 0.0],
                                             [-7.77, 0.3, 0.3], [0.0, 4.0, 0.0], [0.1, 0.1, 0.0], [0.05, -0.1, 0.1]])   # (the last two: inside goal_radius)
    plans = np.zeros((n, 4), dtype=abi.state_dtype)
    plans[:, 0] = veh["state"]
    ctx = capi.Context(0)
    try:
        for mask in (None, np.array([1, 1, 1, 1, 0, 0, 0, 0, 1, 1], dtype=np.int32)):
            d_v, d_goals, d_p = to_dev(veh), to_dev(goals), to_dev(plans)
            d_m = None if mask is None else to_dev(mask)
            ctx.fleet_set_goals_device(par, d_v.data_ptr(), d_goals.data_ptr(), None if d_m is None else d_m.data_ptr(), n)
            ctx.sync()
            got = d_v.cpu().numpy().view(abi.vehicle_dtype).copy()
            want = hm.set_goals(veh, goals, mask, P["wd"])
            assert got.tobytes() == want.tobytes(), (mask, got["status"], want["status"], got["goal"] - want["goal"])
            assert list(want["status"][:4]) == [0, 1, 3, 3]
            if mask is not None:
                assert got[4:8].tobytes() == veh[4:8].tobytes()
            # begin on the result: the same G, YAWING inactive with stage NONE, inside goal_radius GOAL_REACHED
            whole, safe = to_dev(abi.make_problems(n)), to_dev(abi.make_problems(n))
            d_s, d_g, d_r, d_a = to_dev(np.zeros((n, 3))), to_dev(np.zeros((n, 3))), to_dev(np.zeros(n)), to_dev(np.full(n, 7, dtype=np.int32))
            ctx.fleet_begin_device(par, d_v.data_ptr(), d_p.data_ptr(), n, 4, whole.data_ptr(), safe.data_ptr(), d_s.data_ptr(), d_g.data_ptr(),
                                   d_r.data_ptr(), d_a.data_ptr())
            ctx.sync()
            after = d_v.cpu().numpy().view(abi.vehicle_dtype)
            active = d_a.cpu().numpy().view(np.int32)
            sel = np.ones(n, dtype=bool) if mask is None else mask.astype(bool)
            assert np.array_equal(after["goal"][sel], got["goal"][sel])
            assert np.array_equal(d_g.cpu().numpy().view(np.float64).reshape(n, 3)[sel], got["goal"][sel])
            for i in np.nonzero(sel)[0]:
                if i >= 8:
                    assert after["status"][i] == abi.FH_VEHICLE_GOAL_REACHED and not active[i] and after["stage"][i] == 0, i
                elif got["status"][i] == abi.FH_VEHICLE_YAWING:
                    assert after["status"][i] == abi.FH_VEHICLE_YAWING and not active[i] and not after["active"][i] and after["stage"][i] == 0, i
                else:
                    assert after["status"][i] == got["status"][i] and active[i] == 1, i
    finally:
        ctx.close()


# ---- the forward sensor ----
R_SENSE = 3.0
LATTICE_DIMS = [48, 48, 12]
SENSE_B = 96


@pytest.fixture(scope="module")
def sense_scene():
    cloud, cells, center, _, _, _, m_origin, occ = forest_map(41, SENSE_B)
    origin = m_origin + np.array([5.03, 4.97, 0.11])    # 48 x 48 x 12 cells of 0.2 m inside the map, not on its lattice
    rng = np.random.default_rng(12)
    span = np.array(LATTICE_DIMS) * 0.2
    pos = origin + rng.uniform([0.3, 0.3, 0.4], span - [0.3, 0.3, 0.4], size=(SENSE_B, 3))
    pos[0] = origin + [0.0, 4.0, 1.0]                   # on the border
    pos[1] = origin + [span[0], span[1], 1.2]           # on a corner
    pos[2] = origin + [-1.5, 5.0, 1.0]                  # outside, looking in (yaw 0)
    pos[3] = origin + [4.0, span[1] + 1.0, 1.0]         # outside, looking in (yaw -pi/2)
    pos[4] = origin + [-30.0, 4.0, 1.0]                 # far outside
    pos[5] = origin + [4.8, 4.8, -0.6]                  # below
    yaw = rng.uniform(-math.pi, math.pi, size=SENSE_B)
    yaw[:4] = [0.0, math.pi / 2, 0.0, -math.pi / 2]
    pos[11], yaw[11] = origin + [5.0, 0.2, 1.0], -math.pi / 2          # just inside, looking out
    pos[12], pos[13] = origin + [3.0, 6.0, 0.1], origin + [6.0, 3.0, span[2] - 0.1]   # at the floor and at the ceiling of the lattice
    yaw[6:10] = [0.0, math.pi / 2, -math.pi / 2, math.pi]
    yaw[10] = float("nan")                              # dir not finite: senses nothing
    view_of = np.arange(SENSE_B, dtype=np.int32)
    view_of[64:] = 64 + (np.arange(32) // 2)            # pairs share a view
    pos[65::2] = pos[64::2] + rng.uniform(-0.8, 0.8, size=(16, 3)) * [1, 1, 0.2]
    return {"cloud": cloud, "cells": cells, "center": center, "m_origin": m_origin, "occ": occ, "origin": origin, "pos": pos, "yaw": yaw,
            "view_of": view_of, "n_views": 80, "yaw2": yaw + rng.uniform(-1.2, 1.2, size=SENSE_B)}


@pytest.mark.parametrize("th,tv", [(1.0, 0.5), (0.1, 0.1), (50.0, 50.0)])
def test_forward_sensing_equals_the_numpy_model(sense_scene, th, tv):
    """96 vehicles on a 48 x 48 x 12 lattice of 0.2 m that is not the map's, r_sense 3 m: yaws exactly 0, +-pi/2, pi and random, vehicles
    outside the lattice and on its border, pairs sharing a view, one vehicle whose dir is not finite, two looks (the second after 0.9 m
    and a turn), occupancy staged in LDS and not.  The device's flags are the model's, every byte; the model gets the dir the DEVICE
    wrote.  "Clipped on every side": no box of 6 m spans a lattice of 9.6 m, so the assertion is that each of the six sides of the
    lattice clips the box of some vehicle, and that one box is clipped on both sides in z."""
    from faster_amd.fleet import Fleet

    sc = sense_scene
    B, origin, dims = SENSE_B, sc["origin"], LATTICE_DIMS
    pos1 = sc["pos"]
    step = np.stack([np.cos(np.nan_to_num(sc["yaw"])), np.sin(np.nan_to_num(sc["yaw"])), np.zeros(B)], axis=1)
    pos2 = pos1 + 0.9 * step
    model = np.ones((sc["n_views"], dims[2], dims[1], dims[0]), dtype=np.uint8)
    looks, hidden, out_of_view = [], 0, 0
    got = {}
    for staging in (True, False):
        fl = Fleet(B, abi.default_fleet_params())
        try:
            fl.ctx.set_sense_staging(staging)
            fl.set_map(sc["cloud"], sc["cells"], P["res"], sc["center"], P["z_max"], P["inflation"])
            fl.set_unknown_views(view_of=sc["view_of"], n_views=sc["n_views"], origin=origin, res=0.2, dims=dims)
            with pytest.raises(capi.FasterHipError):
                fl.sense(R_SENSE, fov=(th, tv))            # no headings yet
            got[staging] = []
            for k, (pos, yaw) in enumerate(((pos1, sc["yaw"]), (pos2, sc["yaw2"]))):
                fl.init(pos, pos)
                fl.enable_heading(yaw0=yaw)
                dirs = fl.headings()["dir"].copy()
                for bad in ((0.0, tv), (th, -1.0), (float("nan"), tv), (th, float("inf"))):
                    with pytest.raises(capi.FasterHipError):
                        fl.sense(R_SENSE, fov=bad)
                fl.sense(R_SENSE, fov=(th, tv))
                got[staging].append((dirs, fl.views()))
        finally:
            fl.close()
    for k, pos in enumerate((pos1, pos2)):
        dirs = got[True][k][0]
        assert got[False][k][0].tobytes() == dirs.tobytes()
        assert np.isnan(dirs[10]).all() and np.isfinite(np.delete(dirs, 10, axis=0)).all()
        if k == 0:
            assert tuple(dirs[6]) == (1.0, 0.0) and dirs[9][0] == -1.0 and abs(dirs[7][0]) < 1e-15 and dirs[7][1] == 1.0 and dirs[8][1] == -1.0
        before = model.copy()
        h, o = hm.sense_fov(model, sc["view_of"], pos, dirs, th, tv, R_SENSE, origin, 0.2, sc["occ"], sc["m_origin"], P["res"])
        hidden, out_of_view = hidden + h, out_of_view + o
        assert not ((before == 0) & (model != 0)).any() and (model != before).any()
        for staging in (True, False):
            views = got[staging][k][1]
            diff = np.nonzero(views != model)
            assert len(diff[0]) == 0, "tangents (%g, %g), staging %s, look %d: %d bytes differ, first at view %d cell (%d, %d, %d)" % (
                th, tv, staging, k, len(diff[0]), diff[0][0], diff[3][0], diff[2][0], diff[1][0])
        looks.append(model.copy())
    flat = model.reshape(sc["n_views"], -1)
    assert hidden > 0, hidden                         # in range and in view, and still hidden
    assert out_of_view > 1000, out_of_view            # in range, out of view (for (50, 50): behind the vehicle): left unknown
    assert flat[10].all() and flat[4].all()           # dir not finite / far outside: nothing seen
    assert (flat[0] == 0).any()
    # the lattice clips the scanned boxes: every side that of some vehicle, and in z one box on both sides
    lo, hi = origin, origin + np.array(dims) * 0.2
    clipped = np.zeros((B, 3, 2), dtype=bool)
    dirs = got[True][0][0]
    for i in range(B):
        if i == 10:
            continue
        box = hm.scan_box(pos1[i], dirs[i], th, tv, R_SENSE)
        for ax in range(3):
            clipped[i, ax, 0] = pos1[i][ax] + box[ax][0] < lo[ax] < pos1[i][ax] + box[ax][1]
            clipped[i, ax, 1] = pos1[i][ax] + box[ax][0] < hi[ax] < pos1[i][ax] + box[ax][1]
    assert clipped.any(axis=0).all(), clipped.any(axis=0)
    if tv >= 0.5:
        assert (clipped[:, 2, 0] & clipped[:, 2, 1]).any()
    print("forward sense == model: tangents (%g, %g): %d flags cleared, %d hidden, %d out of view" % (th, tv, int((flat == 0).sum()), hidden, out_of_view))


def test_a_wide_forward_sensor_sees_what_its_half_space_holds(sense_scene):
    """Tangents (50, 50) against the omnidirectional sensor from the same places: a subset of it, and nothing behind the vehicle."""
    from faster_amd.fleet import Fleet

    sc = sense_scene
    B, origin, dims = SENSE_B, sc["origin"], LATTICE_DIMS
    out = []
    for fov in (None, (50.0, 50.0)):
        fl = Fleet(B, abi.default_fleet_params())
        try:
            fl.set_map(sc["cloud"], sc["cells"], P["res"], sc["center"], P["z_max"], P["inflation"])
            fl.set_unknown_views(origin=origin, res=0.2, dims=dims)
            fl.init(sc["pos"], sc["pos"])
            fl.enable_heading(yaw0=sc["yaw"])
            fl.sense(R_SENSE, fov=fov)
            out.append(fl.views())
        finally:
            fl.close()
    omni, fwd = out
    assert not ((fwd == 0) & (omni != 0)).any()
    seen_o, seen_f = int((omni == 0).sum()), int((fwd == 0).sum())
    assert 0.3 * seen_o < seen_f < 0.7 * seen_o, (seen_o, seen_f)


def test_a_fleet_without_heading_is_unchanged_and_look_at_follows_the_safe_problem():
    """Two fleets on the shared-grid scenario of test_gpu_fleet.py, 8 cycles, one with enable_heading: vehicles, goals and plans are
    bit for bit equal (the yaw machinery does not leak into planning).  In the fleet with heading, look_at is the safe problem's xf
    whenever a safe path was needed and a safe corridor exists, changes only in vehicles that had a whole trajectory, and is left alone
    by a vehicle that is inactive, has no path or has no whole trajectory."""
    B, C = 64, 8
    sc = scenario(B, C, 31)
    fleets = [make_fleet(sc, B), make_fleet(sc, B)]
    try:
        fleets[1].enable_heading(yaw0=np.linspace(-3, 3, B))
        prev = fleets[1].headings()["look_at"].copy()
        assert not prev.any()
        counts = {"xf": 0, "march_only": 0, "kept": 0}
        for c in range(C):
            after = []
            for fl in fleets:
                fl.set_unknown(sc["flags"][c], sc["origin"], P["res"], sc["dims"])
                fl.replan()
                after.append(fl.vehicles())
            assert after[0].tobytes() == after[1].tobytes(), ("vehicles after replan", c)
            v, res = after[1], fleets[1].results()
            look = fleets[1].headings()["look_at"].copy()
            for i in range(B):
                if v["stage"][i] >= 3:                                   # the whole trajectory exists
                    assert np.isfinite(look[i]).all()
                    if v["needed_safe"][i] and res["safe"]["n_seg"][i] > 0:
                        assert np.array_equal(look[i], res["safe"]["xf"][i][:3]), (c, i)     # (xf: position, velocity, acceleration)
                        counts["xf"] += 1
                    elif not v["needed_safe"][i]:
                        counts["march_only"] += 1
                else:                                                    # inactive, no path, no whole: as it was
                    assert np.array_equal(look[i], prev[i]), (c, i, int(v["stage"][i]))
                    counts["kept"] += 1
            prev = look
            for fl in fleets:
                fl.next_goals(int(sc["ticks"][c]), follow=True)
            assert fleets[0].vehicles().tobytes() == fleets[1].vehicles().tobytes(), ("vehicles after next_goals", c)
            assert fleets[0].goals().tobytes() == fleets[1].goals().tobytes(), ("goals", c)
            gy, h = fleets[1].goal_yaw(), fleets[1].headings()
            assert np.array_equal(gy[:, 0], h["goal_yaw"]) and np.array_equal(h["yaw"], h["previous_yaw"])
            moving = fleets[1].vehicles()["status"] != abi.FH_VEHICLE_GOAL_REACHED
            assert (np.abs(gy[moving, 1]) == 4.0).all()                  # alpha 0: dyaw = +-w_max
        for a, b in zip(fleets[0].plans(), fleets[1].plans()):
            assert a.tobytes() == b.tobytes()
        assert all(n > 0 for n in counts.values()), counts
    finally:
        for fl in fleets:
            fl.close()


# ---- the closed loop against the host Planner ----
LOOP_SEED, LOOP_B, LOOP_C, LOOP_TICKS, LOOP_FOV = 31, 64, 24, 5, (1.0, 0.5)
ARRIVERS = range(40, 56)     # vehicles whose first goal is at hand, so that they arrive, get a second goal, turn and travel again


def loop_scenario():
    """The forest scenario of test_gpu_fleet.py for 64 vehicles x 24 cycles of 5 ticks (1.2 s of flight: nobody crosses the forest), with
    16 vehicles whose first goal is 0.1 .. 0.55 m ahead (the first ten inside goal_radius: GOAL_REACHED at the first replan), and the
    committed list of second goals: 2 .. 3 m away at a bearing within 0.5 rad of the +x axis, the direction a fresh vehicle looks in
    (yaw 0), so that the turn takes a few cycles of 5 ticks x 0.04 rad and not the whole run; three of them above the map, so that
    replans fail after M_ has been written."""
    sc = scenario(LOOP_B, LOOP_C, LOOP_SEED)
    sc["ticks"] = np.full(LOOP_C, LOOP_TICKS, dtype=np.int32)
    rng = np.random.default_rng(LOOP_SEED + 1000)
    starts = sc["states"]["pos"]
    second = starts.copy()
    for k, i in enumerate(ARRIVERS):
        u = sc["goals"][i] - starts[i]
        u[2] = 0.0
        u /= max(np.linalg.norm(u), 1e-9)
        d = (0.1, 0.15, 0.2, 0.25, 0.12, 0.18, 0.22, 0.08, 0.05, 0.27, 0.36, 0.4, 0.45, 0.5, 0.55, 0.38)[k]
        sc["goals"][i] = starts[i] + d * u
        sc["states"]["vel"][i] = u * (0.0 if k < 10 else 1.2)
        a = rng.uniform(0.1, 0.5) * (1 if k % 2 else -1)
        second[i] = starts[i] + rng.uniform(2.0, 3.0) * np.array([math.cos(a), math.sin(a), 0.0])
        if k in (10, 12, 14):
            second[i][2] = 6.0   # above the map: once it has turned, no path, every cycle — after M_ was written on the way to the first goal
    return sc, second


def run_heading_stub(tmp_path, sc, reveals, second, new_goal, w_max, alpha):
    from faster_amd import build as fb

    fb.build_all()
    exe = os.path.join(ROOT, "tests", "cpp", "test_replan_fleet_heading")
    src, host = exe + ".cpp", os.path.join(ROOT, "faster_amd", "host")
    deps = [src, fb.HOST_SO] + [os.path.join(host, f) for f in ("replan_stub.hpp", "corridor_frontend.hpp", "corridor_frontend.cpp", "solver_hip.hpp")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++14", "-fopenmp", "-I", os.path.join(ROOT, "include"), "-I", host, src,
                               os.path.join(host, "corridor_frontend.cpp"), "-o", exe, "-L", os.path.join(ROOT, "faster_amd"), "-lsolverhip",
                               "-lfasterhip", "-ldl", "-Wl,-rpath," + os.path.join(ROOT, "faster_amd")])
    B, C = len(sc["states"]), len(sc["ticks"])
    hi = np.zeros(16, dtype=np.int32)
    hi[:12] = [P["N"], P["max_poly"], sc["cells"][0], sc["cells"][1], sc["cells"][2], B, len(sc["cloud"]), C, *sc["dims"], P["delta_t"]]
    hd = np.zeros(32, dtype=np.float64)
    hd[:31] = [P["dc"], P["v_max"], P["a_max"], P["j_max"], P["Ra"], P["drone_radius"], P["decomp_radius"], P["dist_max_vertexes"], P["delta_a"],
               P["delta_h"], P["res"], P["inflation"], P["z_max"], *sc["center"], P["goal_radius"], *P["wd"], *sc["origin"], 20, 20, 1, 20, 20, 1,
               w_max, alpha]
    st = sc["states"]
    veh = np.concatenate([st["pos"], st["vel"], st["accel"], sc["goals"]], axis=1)
    scen, outp = tmp_path / "fleet_heading.bin", tmp_path / "fleet_heading.out"
    with open(scen, "wb") as f:
        for a in (hi, hd, np.ascontiguousarray(sc["cloud"], dtype=np.float64), np.ascontiguousarray(veh, dtype=np.float64), sc["ticks"]):
            f.write(np.ascontiguousarray(a).tobytes())
        for i in range(B):
            for c in range(C):
                idx = np.ascontiguousarray(reveals[i][c], dtype=np.int32)
                f.write(np.array([len(idx)], dtype=np.int32).tobytes())
                f.write(idx.tobytes())
        f.write(np.ascontiguousarray(second, dtype=np.float64).tobytes())
        f.write(np.ascontiguousarray(new_goal, dtype=np.int32).tobytes())
    r = subprocess.run([exe, str(scen), str(outp)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    raw = open(outp, "rb").read()
    rec = np.dtype([("i", "<i4", (12,)), ("d", "<f8", (32,))])
    out, pos = [], 0
    for _ in range(B):
        cyc = np.frombuffer(raw, dtype=rec, count=C, offset=pos).copy()
        pos += rec.itemsize * C
        n = int(np.frombuffer(raw, dtype=np.int32, count=1, offset=pos)[0])
        pos += 4
        plan = np.frombuffer(raw, dtype=np.float64, count=12 * n, offset=pos).reshape(n, 12).copy()
        pos += 96 * n
        out.append((cyc, plan))
    assert pos == len(raw)
    return out


def test_closed_loop_with_heading_equals_the_host_planner(tmp_path):
    """64 vehicles x 24 cycles in the forest, a view per vehicle that starts all unknown except 1.5 m around the start, a fresh heading
    (yaw 0).  Every cycle: a vehicle that reported GOAL_REACHED in the cycle before gets its second goal (set_goals, from the committed
    list of loop_scenario); forward sense (tangents 1, 0.5); replan; 5 ticks of next goals with follow.  Every cycle the views are the
    numpy model's given the device's dir (every byte), and every vehicle equals replan_stub.hpp's Planner, which is given the unknown
    voxels of its view, its new goal in the same cycle, and getNextGoalYaw: every field tests/test_gpu_fleet_views.py compares, to its
    bars; status after the replan and after the ticks, yaw, dyaw and previous_yaw exactly; look_at to 1e-9 (the bar of that file for
    states), and bit for bit the safe problem's xf whenever a safe path was needed and a safe corridor exists.  The host's log must hold
    a GOAL_REACHED -> YAWING -> TRAVELING sequence followed by a commit of the same vehicle, M_ written from each of its three sources,
    and a failed cycle that leaves M_ alone."""
    from test_gpu_fleet import as12

    B, C = LOOP_B, LOOP_C
    sc, second = loop_scenario()
    dims, origin = sc["dims"], sc["origin"]
    cells = dims[0] * dims[1] * dims[2]
    iz, iy, ix = np.meshgrid(np.arange(dims[2]), np.arange(dims[1]), np.arange(dims[0]), indexing="ij")
    centres = np.stack([(ix + 0.5) * P["res"] + origin[0], (iy + 0.5) * P["res"] + origin[1], (iz + 0.5) * P["res"] + origin[2]], axis=-1)
    start_views = np.ones((B, dims[2], dims[1], dims[0]), dtype=np.uint8)
    for i in range(B):
        start_views[i][np.linalg.norm(centres - sc["states"]["pos"][i], axis=-1) < 1.5] = 0
    fl = make_fleet(sc, B)
    model = start_views.copy()
    prev = np.ones((B, cells), dtype=np.uint8)
    reveals = [[None] * C for _ in range(B)]
    new_goal = np.zeros((B, C), dtype=np.int32)
    per_cycle = []
    try:
        occ = fl.map.occupancy()
        fl.set_unknown_views(start_views.reshape(B, cells), origin=origin, res=P["res"], dims=dims)
        fl.enable_heading()
        reached = np.zeros(B, dtype=bool)
        for c in range(C):
            if reached.any():
                new_goal[:, c] = reached
                fl.set_goals(second, mask=reached)
            v0 = fl.vehicles()
            here, dirs = v0["state"]["pos"].copy(), fl.headings()["dir"].copy()
            fl.sense(R_SENSE, fov=LOOP_FOV)
            got = fl.views()
            hm.sense_fov(model, None, here, dirs, LOOP_FOV[0], LOOP_FOV[1], R_SENSE, origin, P["res"], occ, origin, P["res"])
            assert np.array_equal(got, model), ("views differ from the model", c, int((got != model).sum()))
            flat = got.reshape(B, cells)
            for i in range(B):
                reveals[i][c] = np.nonzero((prev[i] != 0) & (flat[i] == 0))[0]
            prev = flat.copy()
            fl.replan()
            after, look, res = fl.vehicles(), fl.headings()["look_at"].copy(), fl.results()
            fl.next_goals(LOOP_TICKS, follow=True)
            later = fl.vehicles()
            per_cycle.append((after, later, fl.goals(), look, fl.headings(), fl.goal_yaw(), res["safe"]["xf"][:, :3].copy(), res["safe"]["n_seg"].copy()))
            reached = (after["status"] == abi.FH_VEHICLE_GOAL_REACHED) & (v0["status"] != abi.FH_VEHICLE_GOAL_REACHED) & np.isin(np.arange(B), ARRIVERS)
        plans = fl.plans()
    finally:
        fl.close()
    yp = abi.default_yaw_params()
    st = run_heading_stub(tmp_path, sc, reveals, second, new_goal, float(yp["w_max"]), float(yp["alpha_filter_dyaw"]))
    worst = worst_look = 0.0
    for c in range(C):
        after, later, goals, look, heads, gy, xf, nseg = per_cycle[c]
        for i in range(B):
            ri, rd = st[i][0][c]["i"], st[i][0][c]["d"]
            v, w = after[i], later[i]
            where = "vehicle %d cycle %d" % (i, c)
            got = (v["stage"], v["needed_safe"], v["k_end_whole"], v["k_safe"], v["index_h"], v["n_whole"], v["n_safe"], v["status"], w["plan_size"],
                   w["status"])
            want = (ri[1], ri[2], ri[3], ri[4], ri[5], ri[6], ri[7], ri[8], ri[9], ri[11])
            assert tuple(int(x) for x in got) == tuple(int(x) for x in want), (where, got, want)
            assert (v["whole_factor"], v["safe_factor"]) == (rd[0], rd[1]), (where, v["whole_factor"], v["safe_factor"], rd[:2])
            win = (v["whole_init"], v["whole_final"], v["whole_inc"], v["safe_init"], v["safe_final"], v["safe_inc"])
            assert win == tuple(rd[2:8]), (where, win, rd[2:8])
            assert np.array_equal(v["goal"], rd[8:11]), (where, v["goal"], rd[8:11])
            if v["active"]:
                assert v["ra"] == rd[11], (where, v["ra"], rd[11])
            worst = max(worst, float(np.abs(as12(goals[i]) - rd[12:24]).max()))
            h = heads[i]
            assert (gy[i][0], gy[i][1], h["previous_yaw"], h["yaw"]) == (rd[27], rd[28], rd[29], rd[27]), (where, gy[i], h["previous_yaw"], rd[27:30])
            worst_look = max(worst_look, float(np.abs(look[i] - rd[24:27]).max()))
            if v["stage"] >= 3 and v["needed_safe"] and nseg[i] > 0:
                assert np.array_equal(look[i], xf[i]), where
    for i in range(B):
        assert len(plans[i]) == len(st[i][1]), (i, len(plans[i]), len(st[i][1]))
        worst = max(worst, float(np.abs(as12(plans[i]) - st[i][1]).max()))
    # what the HOST planner's log holds
    host = np.array([[st[i][0][c]["i"] for c in range(C)] for i in range(B)])        # [B][C][12]
    hostM = np.array([[st[i][0][c]["d"][24:27] for c in range(C)] for i in range(B)])
    h_stage, h_status, h_later, h_m = host[..., 1], host[..., 8], host[..., 11], host[..., 10]
    sequences = 0
    for i in range(B):
        r = np.nonzero(h_status[i] == 2)[0]
        if not len(r):
            continue
        y = np.nonzero((h_status[i] == 3) & (np.arange(C) > r[0]))[0]
        if not len(y):
            continue
        t = np.nonzero((h_later[i] == 0) & (np.arange(C) >= y[0]))[0]
        if len(t) and ((h_stage[i] == 5) & (np.arange(C) > t[0])).any():
            sequences += 1
    failed_kept = 0
    for i in range(B):
        for c in range(1, C):
            if h_stage[i, c] in (1, 2) and hostM[i, c - 1].any() and np.array_equal(hostM[i, c], hostM[i, c - 1]):
                failed_kept += 1
    cover = {"reached_yawing_traveling_commit": sequences, "m_from_march_only": int((h_m == 1).sum()), "m_from_safe_path": int((h_m == 3).sum()),
             "m_from_G": int((h_m == 7).sum()), "failed_cycle_keeps_m": failed_kept, "yawing_cycles": int((h_status == 3).sum()),
             "commits": int((h_stage == 5).sum()), "new_goals": int(new_goal.sum())}
    print("fleet with heading == host planner over %d vehicles x %d cycles: host coverage %s, worst state difference %.2e, worst look_at difference %.2e"
          % (B, C, cover, worst, worst_look))
    assert worst < 1e-9, worst
    assert worst_look < 1e-9, worst_look
    assert all(n > 0 for n in cover.values()), cover
