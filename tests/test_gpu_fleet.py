"""GPU tests of steady-state replanning on the device (fh_fleet_*, faster_amd/fleet.py): N vehicles keep their plan, status and factor
windows on the device across replan cycles, and after every cycle each of them is where the host restatement of Faster::replan
(faster_amd/host/replan_stub.hpp, Planner driving SolverHip: tests/cpp/test_replan_fleet.cpp) is."""
import os
import subprocess

import numpy as np
import pytest

from faster_amd import abi, capi, corridor, frontend

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

P = {"N": 6, "max_poly": 3, "dc": 0.01, "v_max": 5.0, "a_max": 5.0, "j_max": 8.0, "Ra": 4.0, "drone_radius": 0.3, "decomp_radius": 0.05,
     "dist_max_vertexes": 1.5, "delta_a": 0.5, "delta_h": 1.0, "res": 0.2, "inflation": 0.3, "z_max": 3.0, "goal_radius": 0.3,
     "wd": (8.0, 8.0, 4.0), "delta_t": 10}


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch  # noqa: F401  (torch before the HIP library: one HIP runtime in the process)


def fleet_params():
    p = abi.default_fleet_params()
    p["delta_t"], p["goal_radius"], p["ra"] = P["delta_t"], P["goal_radius"], P["Ra"]
    p["wdx"], p["wdy"], p["wdz"] = P["wd"]
    p["rule"]["mode"], p["rule"]["drone_radius"], p["rule"]["delta_h"], p["rule"]["delta_a"] = 2, P["drone_radius"], P["delta_h"], P["delta_a"]
    return p


def scenario(B, C, seed):
    """Vehicles in a random forest: starts, goals (some near the start, a few above the map), an unknown-voxel grid per cycle that follows
    a fixed reveal schedule, and the ticks flown between two cycles (mostly fewer than deltaT, some far beyond the end of every plan)."""
    cloud, cells, center, starts, goals, rng = frontend.forest_queries(B, seed, return_rng=True)
    pts = np.concatenate([starts, goals])
    near = rng.choice(B, B // 4, replace=False)
    for i in near:  # a free point 1.5 .. 4 m away: these vehicles see and reach their goals
        d = np.linalg.norm(pts - starts[i], axis=1)
        cand = np.nonzero((d > 1.5) & (d < 4.0))[0]
        if len(cand):
            goals[i] = pts[cand[np.argmin(d[cand])]]
    high = [i for i in range(B) if i not in set(near)][:3]
    goals[high, 2] = 6.0  # above the map: no path, every cycle
    u = goals - starts
    u /= np.maximum(np.linalg.norm(u, axis=1, keepdims=True), 1e-9)
    states = np.zeros(B, dtype=abi.state_dtype)
    states["pos"], states["vel"] = starts, u * rng.uniform(0, 1.5, size=(B, 1))
    away = [i for i in range(B) if i not in set(near) and i not in high][:6]
    states["vel"][away] = -4.5 * u[away]  # flying away from the goal near v_max: no whole trajectory within the first factor window
    probe = capi.Map(0)
    probe.read(cloud, cells, P["res"], center, 0.0, P["z_max"], P["inflation"])
    dims, origin = probe.dims()
    probe.close()
    dims, origin = [int(d) for d in dims], np.array(origin, dtype=np.float64)
    iz, iy, ix = np.meshgrid(np.arange(dims[2]), np.arange(dims[1]), np.arange(dims[0]), indexing="ij")
    centres = np.stack([(ix + 0.5) * P["res"] + origin[0], (iy + 0.5) * P["res"] + origin[1], (iz + 0.5) * P["res"] + origin[2]], axis=-1)
    seen = np.zeros(iz.shape, dtype=bool)
    for s in starts:
        seen |= np.linalg.norm(centres - s, axis=-1) < 1.5
    spheres = rng.uniform([1, 1, 1.5], [19, 19, 1.5], size=(12 + 2 * C, 3))
    radii = rng.uniform(2.0, 3.5, size=len(spheres))
    flags = np.zeros((C,) + iz.shape, dtype=np.uint8)
    for c in range(C):
        for k in (range(0, 12) if c == 0 else range(10 + 2 * c, 12 + 2 * c)):
            seen |= np.linalg.norm(centres - spheres[k], axis=-1) < radii[k]
        flags[c] = ~seen
    ticks = rng.integers(2, P["delta_t"], size=C).astype(np.int32)
    ticks[[C // 4, C // 2, (3 * C) // 4]] = 400
    return {"cloud": cloud, "cells": cells, "center": center, "states": states, "goals": goals, "flags": flags, "dims": dims, "origin": origin,
            "ticks": ticks, "high": high, "near": near}


def make_fleet(sc, B):
    from faster_amd.fleet import Fleet

    fl = Fleet(B, fleet_params(), n_seg=P["N"], max_poly=P["max_poly"], dc=P["dc"], v_max=P["v_max"], a_max=P["a_max"], j_max=P["j_max"],
               decomp_radius=P["decomp_radius"], dist_max_vertexes=P["dist_max_vertexes"])
    fl.set_map(sc["cloud"], sc["cells"], P["res"], sc["center"], P["z_max"], P["inflation"])
    fl.init(sc["states"], sc["goals"])
    return fl


def run_stub(tmp_path, sc):
    from faster_amd import build as fb

    fb.build_all()
    exe = os.path.join(ROOT, "tests", "cpp", "test_replan_fleet")
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
    hd[:29] = [P["dc"], P["v_max"], P["a_max"], P["j_max"], P["Ra"], P["drone_radius"], P["decomp_radius"], P["dist_max_vertexes"], P["delta_a"],
               P["delta_h"], P["res"], P["inflation"], P["z_max"], *sc["center"], P["goal_radius"], *P["wd"], *sc["origin"], 20, 20, 1, 20, 20, 1]
    st = sc["states"]
    veh = np.concatenate([st["pos"], st["vel"], st["accel"], sc["goals"]], axis=1)
    scen, outp = tmp_path / "fleet.bin", tmp_path / "fleet.out"
    with open(scen, "wb") as f:
        for a in (hi, hd, np.ascontiguousarray(sc["cloud"], dtype=np.float64), np.ascontiguousarray(veh, dtype=np.float64), sc["ticks"], sc["flags"]):
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, str(scen), str(outp)], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-2000:]
    raw = open(outp, "rb").read()
    rec = np.dtype([("i", "<i4", (12,)), ("d", "<f8", (24,))])
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


def as12(s):
    return np.concatenate([s["pos"], s["vel"], s["accel"], s["jerk"]], axis=-1)


def test_fleet_over_many_cycles_equals_the_host_planner(tmp_path):
    """128 vehicles x 32 cycles: every cycle, every vehicle — stage, needed_safe, k_end_whole, k_safe, indexH, sample counts, both factors,
    both windows, status, plan size, G and ra exactly equal to replan_stub.hpp's Planner; the goals popped and the final plans to 1e-9."""
    B, C = 128, 32
    sc = scenario(B, C, 31)
    fl = make_fleet(sc, B)
    per_cycle = []
    try:
        for c in range(C):
            fl.set_unknown(sc["flags"][c], sc["origin"], P["res"], sc["dims"])
            fl.replan()
            after = fl.vehicles()
            fl.next_goals(int(sc["ticks"][c]), follow=True)
            per_cycle.append((after, fl.vehicles(), fl.goals()))
        plans = fl.plans()
    finally:
        fl.close()
    st = run_stub(tmp_path, sc)
    cover = dict(kend=0, no_safe_needed=0, seen=0, reached=0, ra_small=0, projected=0)
    stages = {}
    worst = 0.0
    for c in range(C):
        after, later, goals = per_cycle[c]
        for i in range(B):
            ri, rd = st[i][0][c]["i"], st[i][0][c]["d"]
            v, w = after[i], later[i]
            where = "vehicle %d cycle %d" % (i, c)
            got = (v["stage"], v["needed_safe"], v["k_end_whole"], v["k_safe"], v["index_h"], v["n_whole"], v["n_safe"], v["status"], w["plan_size"])
            want = (ri[1], ri[2], ri[3], ri[4], ri[5], ri[6], ri[7], ri[8], ri[9])
            assert tuple(int(x) for x in got) == tuple(int(x) for x in want), (where, got, want)
            assert (v["whole_factor"], v["safe_factor"]) == (rd[0], rd[1]), (where, v["whole_factor"], v["safe_factor"], rd[:2])
            win = (v["whole_init"], v["whole_final"], v["whole_inc"], v["safe_init"], v["safe_final"], v["safe_inc"])
            assert win == tuple(rd[2:8]), (where, win, rd[2:8])
            assert np.array_equal(v["goal"], rd[8:11]), (where, v["goal"], rd[8:11])
            if v["active"]:
                assert v["ra"] == rd[11], (where, v["ra"], rd[11])
                cover["ra_small"] += int(v["ra"] < P["Ra"])
            cover["projected"] += int(not np.array_equal(v["goal"], sc["goals"][i]))
            worst = max(worst, float(np.abs(as12(goals[i]) - rd[12:24]).max()))
            stages[int(v["stage"])] = stages.get(int(v["stage"]), 0) + 1
            cover["kend"] += int(v["stage"] == 5 and v["k_end_whole"] > 0)
            cover["no_safe_needed"] += int(v["stage"] == 5 and not v["needed_safe"])
            cover["seen"] += int(v["status"] == abi.FH_VEHICLE_GOAL_SEEN)
            cover["reached"] += int(v["status"] == abi.FH_VEHICLE_GOAL_REACHED)
    for i in range(B):
        assert len(plans[i]) == len(st[i][1]), (i, len(plans[i]), len(st[i][1]))
        worst = max(worst, float(np.abs(as12(plans[i]) - st[i][1]).max()))
    print("fleet == host planner over %d vehicles x %d cycles: stages %s, coverage %s, worst state difference %.2e" % (B, C, stages, cover, worst))
    assert worst < 1e-9, worst
    assert all(stages.get(s, 0) > 0 for s in (1, 2, 3, 5)), stages
    assert all(v > 0 for v in cover.values()), cover


def test_first_cycle_commits_what_the_pair_chain_commits():
    """The first cycle of a fresh fleet (plan = the start state, k_end_whole = 0) commits, bit for bit, what fh_append_plans_device commits
    for the same problems and results: the new path is tied to the verified one."""
    import torch

    B, C = 256, 1
    sc = scenario(B, C, 37)
    fl = make_fleet(sc, B)
    try:
        fl.set_unknown(sc["flags"][0], sc["origin"], P["res"], sc["dims"])
        fl.replan()
        d_plans = torch.zeros(B * fl.max_states * abi.state_dtype.itemsize, dtype=torch.uint8, device=fl.dev)
        d_counts, d_k = torch.zeros(B, dtype=torch.int32, device=fl.dev), torch.zeros(B, dtype=torch.int32, device=fl.dev)
        fl.ctx.append_plans_device(fl.d_whole.data_ptr(), fl.d_wr.data_ptr(), fl.d_safe.data_ptr(), fl.d_sr.data_ptr(), B, 0.5, fl.max_states,
                                   d_plans.data_ptr(), d_counts.data_ptr(), d_k.data_ptr())
        fl.sync()
        v, plans = fl.vehicles(), fl.plans()
        ref = d_plans.cpu().numpy().view(abi.state_dtype).reshape(B, fl.max_states)
        counts, ks = d_counts.cpu().numpy(), d_k.cpu().numpy()
    finally:
        fl.close()
    committed = 0
    for i in range(B):
        if v["stage"][i] != abi.FH_FLEET_STAGE_COMMITTED:
            assert counts[i] == 0 and v["plan_size"][i] == 1, (i, v["stage"][i], counts[i])
            continue
        committed += 1
        assert v["k_safe"][i] == ks[i] and v["plan_size"][i] == counts[i], i
        assert plans[i].tobytes() == ref[i, :counts[i]].tobytes(), i
    assert committed > B // 3, committed


def test_plan_search_with_a_radius_per_query():
    """fh_map_plan_batch_radius_device: with every radius what the scalar clip computes and every query active, the paths of
    fh_map_plan_batch_device with fh_map_set_sphere; with radii of their own, the host clip at that radius; inactive queries: 0 vertices."""
    import torch

    cloud, cells, center, starts, goals = frontend.forest_queries(512, 12)   # |goal - start| >= 6: min(|g - s| - 0.001, Ra) = Ra for Ra <= 5.5
    B, mp, res, zmax, infl = len(starts), 48, P["res"], P["z_max"], P["inflation"]
    rng = np.random.default_rng(5)
    m = capi.Map(0)
    dev = torch.device("cuda", 0)
    t = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype=dt)  # noqa: E731
    try:
        m.read(cloud, cells, res, center, 0.0, zmax, infl)
        m.set_search("jps")
        d_s, d_g = t(starts), t(goals)
        d_p, d_n = torch.zeros((B, mp, 3), dtype=torch.float64, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        m.set_sphere(P["Ra"])
        m.plan_batch_device(d_s.data_ptr(), d_g.data_ptr(), B, mp, d_p.data_ptr(), d_n.data_ptr(), None, 1.5, 0)
        m.sync()
        want_p, want_n = d_p.cpu().numpy().copy(), d_n.cpu().numpy().copy()
        m.set_sphere(0.0)   # (the per-query entry point clips whatever fh_map_set_sphere holds)
        d_r = t(np.full(B, P["Ra"]))
        d_p.zero_(); d_n.zero_()
        m.plan_batch_radius_device(d_s.data_ptr(), d_g.data_ptr(), d_r.data_ptr(), None, B, mp, d_p.data_ptr(), d_n.data_ptr(), None, 1.5, 0)
        m.sync()
        assert np.array_equal(d_n.cpu().numpy(), want_n) and d_p.cpu().numpy().tobytes() == want_p.tobytes()
        assert (want_n > 1).mean() > 0.8
        # radii of their own, a quarter of the queries inactive
        R = np.array([1.0, 2.5, 4.0, 5.5])
        pick = rng.integers(0, len(R), B)
        active = (rng.uniform(size=B) > 0.25).astype(np.int32)
        d_r, d_a = t(R[pick]), t(active, torch.int32)
        d_p.zero_(); d_n.fill_(-7)
        m.plan_batch_radius_device(d_s.data_ptr(), d_g.data_ptr(), d_r.data_ptr(), d_a.data_ptr(), B, mp, d_p.data_ptr(), d_n.data_ptr(), None, 0.0, 0)
        m.sync()
        got_p, got_n = d_p.cpu().numpy(), d_n.cpu().numpy()
    finally:
        m.close()
    assert (got_n[active == 0] == 0).all()
    try:
        frontend.set_search("jps")
        for j, r in enumerate(R):
            sel = np.nonzero((pick == j) & (active == 1))[0]
            frontend.set_sphere(float(r))
            hp, hn, _ = frontend.plan_batch(cloud, cells, res, center, 0.0, zmax, infl, starts[sel], goals[sel], max_points=mp)
            assert np.array_equal(hn, got_n[sel]), r
            for a, i in enumerate(sel):
                assert hp[a, :hn[a]].tobytes() == got_p[i, :hn[a]].tobytes(), (r, i)
            ok = hn > 1
            ends = np.array([hp[a, hn[a] - 1] for a in np.nonzero(ok)[0]])
            assert (np.linalg.norm(ends - starts[sel][ok], axis=1) <= r + 1e-4).all()   # (the crossing is computed in single precision)
    finally:
        frontend.set_sphere(0.0)
        frontend.set_search("astar")


def test_commit_kernel_against_a_model_of_append_to_plan():
    """fh_fleet_commit_device alone, against a numpy model of appendToPlan / the window update written here, on solved pairs of the
    synthetic batch: plans with different head offsets and lengths (the kept prefix moves to the front), every failure stage leaves the
    vehicle untouched, the capacity overflow is its own stage, and the committed states are fh_sample_batch's bytes."""
    import torch

    ctx = capi.Context(0)
    dev = torch.device("cuda", 0)
    B, n_seg, deltaT = 384, 6, 10
    rng = np.random.default_rng(77)
    whole, faces, _ = corridor.whole_batch(B, seed=931, n_seg=n_seg, p_choices=(2, 3))
    tmpl = corridor.safe_templates(whole)
    gd = np.linalg.norm(whole["xf"][:, :3] - whole["x0"][:, :3], axis=1)
    rule = dict(mode=1, r_known=float(np.median(gd)) + 0.3, drone_radius=0.3, delta_h=1.0, delta_a=0.5)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    params = fleet_params()
    params["delta_t"] = deltaT
    params["rule"]["mode"], params["rule"]["r_known"] = 1, rule["r_known"]
    try:
        ctx.set_pair_rule(**rule)
        ctx.set_pair_margin(0.05)
        mf = int(whole["face_off"][np.arange(B), whole["n_poly"]].max())
        d_w, d_f, d_s = t(whole), t(faces), t(tmpl)
        d_sf = torch.zeros_like(d_f)
        d_wr = torch.zeros(B * abi.result_dtype.itemsize, dtype=torch.uint8, device=dev)
        d_sr = torch.zeros_like(d_wr)
        ctx.solve_pairs_device(d_w.data_ptr(), d_f.data_ptr(), B, n_seg, mf, 0.5, 0.2, 3, d_wr.data_ptr(), d_s.data_ptr(), d_sf.data_ptr(), d_sr.data_ptr())
        ctx.sync()
        wres, sres = d_wr.cpu().numpy().view(abi.result_dtype).copy(), d_sr.cpu().numpy().view(abi.result_dtype).copy()
        safe = d_s.cpu().numpy().view(abi.problem_dtype).copy()
        # failures on purpose: a few whole results and a few needed safe results marked unsolved
        need = (safe["n_seg"] > 0) & (wres["solved"] == 1)
        wres["solved"][rng.choice(np.nonzero(wres["solved"] == 1)[0], 12, replace=False)] = 0
        sres["solved"][rng.choice(np.nonzero(need & (sres["solved"] == 1))[0], 12, replace=False)] = 0
        d_wr, d_sr = t(wres), t(sres)
        big = 2048
        d_xw, d_xs = torch.zeros(B * big * 96, dtype=torch.uint8, device=dev), torch.zeros(B * big * 96, dtype=torch.uint8, device=dev)
        d_cw, d_cs, d_k = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(3))
        d_pl, d_cnt = torch.zeros(B * big * 96, dtype=torch.uint8, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        ctx.sample_batch_device(d_w.data_ptr(), d_wr.data_ptr(), B, big, d_xw.data_ptr(), d_cw.data_ptr())
        ctx.sample_batch_device(d_s.data_ptr(), d_sr.data_ptr(), B, big, d_xs.data_ptr(), d_cs.data_ptr())
        ctx.append_plans_device(d_w.data_ptr(), d_wr.data_ptr(), d_s.data_ptr(), d_sr.data_ptr(), B, 0.5, big, d_pl.data_ptr(), d_cnt.data_ptr(),
                                d_k.data_ptr())
        ctx.sync()
        xw = d_xw.cpu().numpy().view(abi.state_dtype).reshape(B, big)
        xs = d_xs.cpu().numpy().view(abi.state_dtype).reshape(B, big)
        cw, cs, counts, ks = d_cw.cpu().numpy(), d_cs.cpu().numpy(), d_cnt.cpu().numpy(), d_k.cpu().numpy()
        # the vehicles: plans at different head offsets and of different lengths, random windows and persisted safe factors
        max_states = int(np.percentile(counts[counts > 0], 75)) + 8
        assert max_states > 140
        veh = np.zeros(B, dtype=abi.vehicle_dtype)
        veh["plan_head"] = rng.choice([0, 1, 3, 17, 100], B)
        veh["plan_size"] = rng.integers(1, 30, B)
        veh["k_end_whole"] = np.maximum(veh["plan_size"] - deltaT, 0)
        veh["active"] = 1
        veh["status"] = rng.integers(0, 2, B)
        for k in ("whole_init", "whole_final", "whole_inc", "safe_init", "safe_final", "safe_inc"):
            veh[k] = rng.integers(1, 30, B).astype(np.float64)
        veh["safe_factor_worked"] = rng.choice([0.0, 3.0, 12.0], B)
        veh["g_term"] = rng.uniform(-50, 50, (B, 3))
        seen_i = np.nonzero(counts > 0)[0][::5]   # G_term at the end of the committed plan: GOAL_SEEN
        for i in seen_i:
            last = xs[i, cs[i] - 1] if counts[i] > ks[i] + 1 else xw[i, ks[i]]
            veh["g_term"][i] = last["pos"] + 0.1
        old_plans = np.zeros((B, max_states), dtype=abi.state_dtype)
        for f in ("pos", "vel", "accel", "jerk"):
            old_plans[f] = rng.normal(size=(B, max_states, 3))
        n_points = np.full(B, 5, dtype=np.int32)
        n_points[rng.choice(B, 10, replace=False)] = 0
        d_veh, d_plans, d_np = t(veh), t(old_plans), torch.from_numpy(n_points).to(dev)
        ctx.set_pair_margin(-1.0)
        ctx.fleet_commit_device(params, d_veh.data_ptr(), d_plans.data_ptr(), B, max_states, d_np.data_ptr(), d_w.data_ptr(), d_wr.data_ptr(),
                                d_s.data_ptr(), d_sr.data_ptr())
        ctx.sync()
        got = d_veh.cpu().numpy().view(abi.vehicle_dtype)
        got_plans = d_plans.cpu().numpy().view(abi.state_dtype).reshape(B, max_states)
    finally:
        ctx.set_pair_rule(mode=0)
        ctx.close()
    seen = {}
    for i in range(B):
        v, g = veh[i], got[i]
        whole_ok = wres["solved"][i] == 1 and whole["n_seg"][i] > 0
        need_i = safe["n_seg"][i] > 0
        safe_ok = need_i and sres["solved"][i] == 1
        kept = int(v["plan_size"] - v["k_end_whole"] - 1)
        if n_points[i] < 2:
            stage = 1
        elif not whole_ok:
            stage = 2
        elif need_i and not safe_ok:
            stage = 3
        else:
            stage = 6 if kept + counts[i] > max_states else 5
        seen[stage] = seen.get(stage, 0) + 1
        assert g["stage"] == stage, (i, g["stage"], stage)
        fs = sres["factor"][i] if (stage in (5, 6) and safe_ok) else v["safe_factor_worked"]
        assert g["safe_factor_worked"] == fs, i
        if stage != 5:   # nothing committed: plan, head, size, status and windows as they were
            for k in ("plan_head", "plan_size", "status", "whole_init", "whole_final", "whole_inc", "safe_init", "safe_final", "safe_inc"):
                assert g[k] == v[k], (i, k)
            assert got_plans[i].tobytes() == old_plans[i].tobytes(), i
            continue
        k = int(ks[i])
        ns = int(counts[i] - k - 1)
        assert g["k_safe"] == k and g["n_whole"] == cw[i] and g["n_safe"] == (cs[i] if need_i else 0) == ns, i
        assert g["plan_head"] == 0 and g["plan_size"] == kept + counts[i], i
        h = int(v["plan_head"])
        want = np.concatenate([old_plans[i, h:h + kept], xw[i, :k + 1], xs[i, :ns]])
        assert got_plans[i, :len(want)].tobytes() == want.tobytes(), i
        wf = wres["factor"][i]
        assert (g["whole_init"], g["whole_final"], g["whole_inc"]) == (max(wf - 20.0, 1.0), wf + 20.0, params["increment_whole"]), i
        assert (g["safe_init"], g["safe_final"], g["safe_inc"]) == (max(fs - 20.0, 1.0), fs + 20.0, params["increment_safe"]), i
        d = np.linalg.norm(v["g_term"] - want[-1]["pos"])
        assert g["status"] == (abi.FH_VEHICLE_GOAL_SEEN if d < P["goal_radius"] else v["status"]), i
    print("commit kernel == model: stages %s" % seen)
    assert all(seen.get(s, 0) > 0 for s in (1, 2, 3, 5, 6)), seen
    assert (got["status"][got["stage"] == 5] == abi.FH_VEHICLE_GOAL_SEEN).sum() >= len(seen_i) // 2
