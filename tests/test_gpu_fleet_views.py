"""GPU tests of unknown-voxel views per vehicle and of sensing on the device (fh_set_unknown_views_device, fh_fleet_sense_device,
faster_amd/fleet.py): one shared view is the shared grid, bit for bit; the device's sensing is the numpy model (tests/sense_model.py),
every byte; and a fleet that grows a view per vehicle by sensing stays, cycle by cycle, where the host restatement of Faster::replan is
when every Planner is given its own unknown voxels (tests/cpp/test_replan_fleet_views.cpp)."""
import os
import subprocess

import numpy as np
import pytest

from faster_amd import abi, capi, corridor, frontend

import sense_model
from test_gpu_fleet import P, as12, make_fleet, scenario

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R_SENSE = 3.0


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch  # noqa: F401  (torch before the HIP library: one HIP runtime in the process)


def run_cycles(sc, B, C, set_flags):
    """The fleet of test_gpu_fleet.py over C cycles; set_flags(fleet, c) gives it the unknown voxels of cycle c.  Returns per cycle the
    bytes of vehicles() after the replan and after next_goals, the popped goals and the stages, and the final plans."""
    fl = make_fleet(sc, B)
    out = []
    try:
        for c in range(C):
            set_flags(fl, c)
            fl.replan()
            after = fl.vehicles()
            fl.next_goals(int(sc["ticks"][c]), follow=True)
            out.append((after.tobytes(), fl.vehicles().tobytes(), fl.goals().tobytes(), after["stage"].copy()))
        plans = fl.plans()
    finally:
        fl.close()
    return out, plans


def test_one_shared_view_equals_the_shared_grid():
    """The scenario of test_gpu_fleet.py with set_unknown, with one view that every vehicle names, and (8 cycles) with a view per vehicle
    holding N copies of the same flags: vehicles(), popped goals and plans equal bit for bit."""
    import torch

    B, C = 128, 32
    sc = scenario(B, C, 31)
    grid = dict(origin=sc["origin"], res=P["res"], dims=sc["dims"])
    shared, shared_plans = run_cycles(sc, B, C, lambda fl, c: fl.set_unknown(sc["flags"][c], sc["origin"], P["res"], sc["dims"]))
    stages = np.concatenate([x[3] for x in shared])
    assert all((stages == s).any() for s in (1, 2, 3, 5)), np.bincount(stages)    # (not a trivial run)
    one, one_plans = run_cycles(sc, B, C, lambda fl, c: fl.set_unknown_views(sc["flags"][c].reshape(1, -1), view_of=np.zeros(B, dtype=np.int32),
                                                                           n_views=1, **grid))
    for c in range(C):
        assert one[c][0] == shared[c][0], ("one shared view: vehicles after replan", c)
        assert one[c][1] == shared[c][1], ("one shared view: vehicles after next_goals", c)
        assert one[c][2] == shared[c][2], ("one shared view: goals", c)
    for i in range(B):
        assert one_plans[i].tobytes() == shared_plans[i].tobytes(), ("one shared view: plan", i)

    def copies(fl, c):
        fl.set_unknown_views(torch.from_numpy(sc["flags"][c].reshape(1, -1)).to(fl.dev).repeat(B, 1), view_of=np.arange(B, dtype=np.int32), **grid)

    def copies_without_table(fl, c):   # view_of = None: view i
        fl.set_unknown_views(torch.from_numpy(sc["flags"][c].reshape(1, -1)).to(fl.dev).repeat(B, 1), **grid)

    for what, setter, cycles in (("view_of = arange(n)", copies, 8), ("view_of = None", copies_without_table, 2)):
        per, _ = run_cycles(sc, B, cycles, setter)
        for c in range(cycles):
            assert per[c][:3] == shared[c][:3], (what, c)


def forest_map(seed, n):
    cloud, cells, center, starts, goals, rng = frontend.forest_queries(n, seed, return_rng=True)
    probe = capi.Map(0)
    probe.read(cloud, cells, P["res"], center, 0.0, P["z_max"], P["inflation"])
    dims, origin = probe.dims()
    occ = probe.occupancy()
    probe.close()
    return cloud, cells, center, starts, goals, [int(d) for d in dims], np.array(origin, dtype=np.float64), occ


def test_sensing_equals_the_numpy_model():
    """320 vehicles in the forest at random free positions, some outside the lattice, the last 64 sharing 32 views in pairs: two sense
    calls with the vehicles moved in between, with and without the occupancy staged in LDS — the device's flags are the model's, every
    byte.  A lattice that is NOT the map's (other origin, coarser cells) is checked as well."""
    from faster_amd.fleet import Fleet

    B = 320
    cloud, cells, center, starts, goals, dims, origin, occ = forest_map(41, B)
    pos1 = starts.copy()
    pos1[:6] = [[-9.0, 4.0, 1.0], [-2.5, 10.0, 1.5], [10.0, 24.5, 1.0], [10.0, 10.0, 5.5], [40.0, 40.0, 1.0], [21.0, -3.0, 0.4]]   # outside the lattice
    step = goals - starts
    pos2 = pos1 + 0.9 * step / np.linalg.norm(step, axis=1, keepdims=True)   # (0.9 m on: a shell of new voxels)
    view_of = np.arange(B, dtype=np.int32)
    view_of[256:] = 256 + (np.arange(64) // 2)
    n_views = 288
    own = (origin, P["res"], dims)
    other = (origin + np.array([0.37, -0.21, 0.05]), 0.25, [70, 85, 11])
    for staging, (lo, lres, ldims) in ((True, own), (False, own), (True, other)):
        fl = Fleet(B, abi.default_fleet_params())
        try:
            fl.ctx.set_sense_staging(staging)
            fl.set_map(cloud, cells, P["res"], center, P["z_max"], P["inflation"])
            fl.set_unknown_views(view_of=view_of, n_views=n_views, origin=lo, res=lres, dims=ldims)
            model = np.ones((n_views, ldims[2], ldims[1], ldims[0]), dtype=np.uint8)
            assert fl.views().all()
            hidden = 0
            for k, pos in enumerate((pos1, pos2)):
                fl.init(pos, goals)       # (sensing reads fh_vehicle.state.pos)
                fl.sense(R_SENSE)
                got = fl.views()
                before = model.copy()
                hidden += sense_model.sense(model, view_of, pos, R_SENSE, lo, lres, occ, origin, P["res"])
                # what the MODEL must show for the comparison to mean something
                assert not ((before == 0) & (model != 0)).any()
                assert (model != before).any(), k
                diff = np.nonzero(got != model)
                assert len(diff[0]) == 0, "staging %s, lattice res %g, call %d: %d bytes differ, first at view %d cell (%d, %d, %d)" % (
                    staging, lres, k, len(diff[0]), diff[0][0], diff[3][0], diff[2][0], diff[1][0])
            assert hidden > 1000, hidden                                     # cells in range that stay unknown: occluded
            flat = model.reshape(n_views, -1)
            _, counts = np.unique(flat, axis=0, return_counts=True)
            assert (counts == 1).sum() >= n_views - 6                        # (all but those placed outside, which may see nothing: unlike every other view)
            assert (flat[0] == 1).all() and (flat[4] == 1).all()             # far outside: nothing seen
            assert (flat[1] == 0).any()                                      # just outside: the part of the sphere that reaches in
            print("sense == model: staging %s, lattice res %g: %d flags cleared, %d hidden" % (staging, lres, int((flat == 0).sum()), hidden))
        finally:
            fl.close()


def run_views_stub(tmp_path, sc, reveals):
    """tests/cpp/test_replan_fleet_views.cpp on the scenario: reveals[i][c] = the cell numbers vehicle i learned before the replan of
    cycle c (cycle 0: since everything was unknown)."""
    from faster_amd import build as fb

    fb.build_all()
    exe = os.path.join(ROOT, "tests", "cpp", "test_replan_fleet_views")
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
    scen, outp = tmp_path / "fleet_views.bin", tmp_path / "fleet_views.out"
    with open(scen, "wb") as f:
        for a in (hi, hd, np.ascontiguousarray(sc["cloud"], dtype=np.float64), np.ascontiguousarray(veh, dtype=np.float64), sc["ticks"]):
            f.write(np.ascontiguousarray(a).tobytes())
        for i in range(B):
            for c in range(C):
                idx = np.ascontiguousarray(reveals[i][c], dtype=np.int32)
                f.write(np.array([len(idx)], dtype=np.int32).tobytes())
                f.write(idx.tobytes())
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


CLOSED_LOOP_SEED = 31


def test_closed_loop_with_a_view_per_vehicle_equals_the_host_planner(tmp_path):
    """128 vehicles x 32 cycles, a view per vehicle that starts all unknown except a sphere of 1.5 m around the start; every cycle
    sense -> replan -> next_goals(ticks, follow=True).  Every cycle the device's views are the numpy model's applied to the vehicles'
    positions (every byte), and every vehicle — stage, needed_safe, k_end_whole, k_safe, indexH, sample counts, both factors, both
    windows, status, plan size, G and ra — is exactly where replan_stub.hpp's Planner is when it is given the unknown voxels of ITS
    view each cycle; the goals popped and the final plans to 1e-9.  Worst state difference found: 1.11e-16 (the shared-grid run of
    test_gpu_fleet.py: 8.7e-19); the host planner's coverage counts of that run are in DESIGN.md 7d'."""
    B, C = 128, 32
    sc = scenario(B, C, CLOSED_LOOP_SEED)
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
    per_cycle = []
    try:
        occ = fl.map.occupancy()
        fl.set_unknown_views(start_views.reshape(B, cells), origin=origin, res=P["res"], dims=dims)
        for c in range(C):
            here = fl.vehicles()["state"]["pos"].copy()
            fl.sense(R_SENSE)
            got = fl.views()
            sense_model.sense(model, None, here, R_SENSE, origin, P["res"], occ, origin, P["res"])
            assert np.array_equal(got, model), ("views differ from the model", c, int((got != model).sum()))
            flat = got.reshape(B, cells)
            for i in range(B):
                reveals[i][c] = np.nonzero((prev[i] != 0) & (flat[i] == 0))[0]
            prev = flat.copy()
            fl.replan()
            after = fl.vehicles()
            fl.next_goals(int(sc["ticks"][c]), follow=True)
            per_cycle.append((after, fl.vehicles(), fl.goals()))
        plans = fl.plans()
        final_views = fl.views().reshape(B, cells)
    finally:
        fl.close()
    st = run_views_stub(tmp_path, sc, reveals)
    # what the HOST planner's log covers
    host = np.array([[st[i][0][c]["i"] for c in range(C)] for i in range(B)])       # [B][C][12]
    h_stage, h_need, h_nsafe, h_status = host[..., 1], host[..., 2], host[..., 7], host[..., 8]
    cover = {"commit_with_safe": int(((h_stage == 5) & (h_nsafe > 0)).sum()), "commit_without_safe": int(((h_stage == 5) & (h_nsafe == 0)).sum()),
             "needed_safe": int((h_need == 1).sum()), "not_needed_safe": int(((h_stage >= 3) & (h_need == 0)).sum()),
             "no_path": int((h_stage == 1).sum()), "no_whole": int((h_stage == 2).sum()), "no_safe": int((h_stage == 3).sum()),
             "goal_reached": int((h_status == abi.FH_VEHICLE_GOAL_REACHED).sum()),
             "views_unlike_vehicle_0": int((final_views != final_views[0]).any(axis=1).sum())}
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
            worst = max(worst, float(np.abs(as12(goals[i]) - rd[12:24]).max()))
    for i in range(B):
        assert len(plans[i]) == len(st[i][1]), (i, len(plans[i]), len(st[i][1]))
        worst = max(worst, float(np.abs(as12(plans[i]) - st[i][1]).max()))
    print("fleet with a view per vehicle == host planner over %d vehicles x %d cycles: host coverage %s, worst state difference %.2e" % (B, C, cover, worst))
    assert worst < 1e-9, worst
    assert all(v > 0 for k, v in cover.items()), cover
    assert cover["views_unlike_vehicle_0"] >= B // 2, cover


def test_the_fused_pair_kernel_refuses_views():
    """With views set fh_solve_pairs_device returns FH_ERR_ARG and the context's error text names views; after
    fh_set_unknown_grid_device it runs again and gives what it gave before."""
    import torch

    rng = np.random.default_rng(77)
    B = 96
    whole, faces, _ = corridor.whole_batch(B, seed=21, n_seg=10, p_choices=(2, 3, 4))
    tmpl = corridor.safe_templates(whole)
    res, dims = 0.25, (96, 96, 16)
    origin = np.array([whole["x0"][:, 0].min() - 2.0, whole["x0"][:, 1].min() - 2.0, -0.5])
    flags = (rng.random(dims[::-1]) < 0.0008).astype(np.uint8)
    ctx = capi.Context(0)
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    try:
        d_flags = to_dev(flags)
        ctx.set_pair_rule(mode=2, drone_radius=0.3, delta_h=1.0, delta_a=0.5)
        ctx.set_pair_margin(0.0)
        mf = int(whole["face_off"][np.arange(B), whole["n_poly"]].max())
        d_w, d_f = to_dev(whole), to_dev(faces)

        def pairs():
            d_s, d_sf = to_dev(tmpl), torch.zeros_like(d_f)
            d_wr = torch.zeros(B * abi.result_dtype.itemsize, dtype=torch.uint8, device="cuda:0")
            d_sr = torch.zeros_like(d_wr)
            ctx.solve_pairs_device(d_w.data_ptr(), d_f.data_ptr(), B, 10, mf, 0.5, 0.0, 3, d_wr.data_ptr(), d_s.data_ptr(), d_sf.data_ptr(), d_sr.data_ptr())
            ctx.sync()
            return [t.cpu().numpy().copy() for t in (d_wr, d_sr, d_s)]

        ctx.set_unknown_grid_device(d_flags.data_ptr(), origin, res, dims)
        first = pairs()
        assert first[0].view(abi.result_dtype)["solved"].sum() > 0.9 * B and (first[2].view(abi.problem_dtype)["n_seg"] > 0).any()
        ctx.set_unknown_views_device(d_flags.data_ptr(), flags.size, None, 1, origin, res, dims)
        with pytest.raises(capi.FasterHipError) as e:
            pairs()
        assert "rc=-1" in str(e.value) and "views" in str(e.value), str(e.value)
        ctx.set_unknown_grid_device(d_flags.data_ptr(), origin, res, dims)
        again = pairs()
        fields = [n for n in abi.result_dtype.names if n not in ("nodes", "qp_iters", "kflops")]
        for a, b in ((first[0], again[0]), (first[1], again[1])):
            for f in fields:
                assert np.array_equal(a.view(abi.result_dtype)[f], b.view(abi.result_dtype)[f]), f
        assert first[2].tobytes() == again[2].tobytes()
    finally:
        ctx.set_pair_rule(mode=0)
        ctx.set_pair_margin(-1.0)
        ctx.close()
