"""GPU tests of occupied space per vehicle or team (fh_map_read_views_device, fh_map_plan_batch_radius_views_device,
fh_set_point_views_device, fh_fleet_observe_device, Fleet.set_point_views / observe): all-ones masks are the shared map, bit for bit;
masked vehicles are where the host Planner is when it is handed cloud[mask]; a masked decomposition is the decomposition of the
compacted sub-cloud, row for row; observing is the numpy model (tests/occupancy_model.py), every word; and the closed loop
sense -> observe -> replan -> next_goals stays on the host restatement (tests/cpp/test_replan_fleet_occupancy.cpp) cycle by cycle."""
import os
import subprocess

import numpy as np
import pytest

from faster_amd import abi, capi, corridor, frontend

import decomp_edge_cases as dec
import occupancy_model as om
import sense_model
from test_gpu_fleet import P, as12, fleet_params, make_fleet, scenario

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R_SENSE = 3.0
ONE_CELL = 0.1   # world inflation below one cell of 0.2 m: a point marks its own cell only, so its voxel can be seen from outside


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch  # noqa: F401  (torch before the HIP library: one HIP runtime in the process)


def new_fleet(sc, B, inflation):
    from faster_amd.fleet import Fleet

    fl = Fleet(B, fleet_params(), n_seg=P["N"], max_poly=P["max_poly"], dc=P["dc"], v_max=P["v_max"], a_max=P["a_max"], j_max=P["j_max"],
               decomp_radius=P["decomp_radius"], dist_max_vertexes=P["dist_max_vertexes"])
    fl.set_map(sc["cloud"], sc["cells"], P["res"], sc["center"], P["z_max"], inflation)
    fl.init(sc["states"], sc["goals"])
    return fl


def run_occ_stub(tmp_path, sc, reveals, learned, inflation, tag="occ"):
    """tests/cpp/test_replan_fleet_occupancy.cpp: reveals[i][c] = the cells, learned[i][c] = the cloud points vehicle i came to know before
    the replan of cycle c."""
    from faster_amd import build as fb

    fb.build_all()
    exe = os.path.join(ROOT, "tests", "cpp", "test_replan_fleet_occupancy")
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
               P["delta_h"], P["res"], inflation, P["z_max"], *sc["center"], P["goal_radius"], *P["wd"], *sc["origin"], 20, 20, 1, 20, 20, 1]
    st = sc["states"]
    veh = np.concatenate([st["pos"], st["vel"], st["accel"], sc["goals"]], axis=1)
    scen, outp = tmp_path / (tag + ".bin"), tmp_path / (tag + ".out")
    with open(scen, "wb") as f:
        for a in (hi, hd, np.ascontiguousarray(sc["cloud"], dtype=np.float64), np.ascontiguousarray(veh, dtype=np.float64), sc["ticks"]):
            f.write(np.ascontiguousarray(a).tobytes())
        for i in range(B):
            for c in range(C):
                for lst in (reveals[i][c], learned[i][c]):
                    idx = np.ascontiguousarray(lst, dtype=np.int32)
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


def assert_equals_host(per_cycle, plans, st, B, C):
    """every field tests/test_gpu_fleet_views.py compares, with its tolerances; -> the worst state difference"""
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
    assert worst < 1e-9, worst
    return worst


# ---- 1. all-ones masks change nothing ------------------------------------------------------------------------------------------------------
def test_all_ones_masks_change_nothing():
    """128 vehicles x 8 cycles: the shared-map fleet against all-ones masks with a row per vehicle (view_of = arange) and with one shared
    row: vehicles(), popped goals and plans bit for bit; every view's grid is the world map's."""
    import torch

    B, C = 128, 8
    sc = scenario(B, C, 31)
    grid = dict(origin=sc["origin"], res=P["res"], dims=sc["dims"])
    words = om.words_for(len(sc["cloud"]))

    def run(mode):
        fl = make_fleet(sc, B)
        out = []
        try:
            for c in range(C):
                flags = torch.from_numpy(sc["flags"][c].reshape(1, -1)).to(fl.dev)
                if mode == "shared":
                    fl.set_unknown_views(flags, view_of=np.zeros(B, dtype=np.int32), n_views=1, **grid)
                elif mode == "one row":
                    fl.set_unknown_views(flags, view_of=np.zeros(B, dtype=np.int32), n_views=1, **grid)
                else:
                    fl.set_unknown_views(flags.repeat(B, 1), view_of=np.arange(B, dtype=np.int32), **grid)
                if mode != "shared" and c == 0:
                    fl.set_point_views(np.full((fl.n_views, words), 0xFFFFFFFF, dtype=np.uint32))
                    assert [name for name, _ in fl.stages()][:3] == ["begin", "map_views", "path_search"]
                fl.replan()
                after = fl.vehicles()
                fl.next_goals(int(sc["ticks"][c]), follow=True)
                out.append((after.tobytes(), fl.vehicles().tobytes(), fl.goals().tobytes(), after["stage"].copy()))
            plans = fl.plans()
            if mode != "shared":
                world = fl.map.occupancy()
                assert world.any()
                for v in range(fl.n_views):
                    assert np.array_equal(fl.map.view_occupancy(v), world), (mode, "grid of view", v)
        finally:
            fl.close()
        return out, plans

    shared, shared_plans = run("shared")
    stages = np.concatenate([x[3] for x in shared])
    assert all((stages == s).any() for s in (1, 2, 5)), np.bincount(stages)    # (not a trivial run)
    for mode in ("arange", "one row"):
        got, plans = run(mode)
        for c in range(C):
            assert got[c][0] == shared[c][0], (mode, "vehicles after replan", c)
            assert got[c][1] == shared[c][1], (mode, "vehicles after next_goals", c)
            assert got[c][2] == shared[c][2], (mode, "goals", c)
        for i in range(B):
            assert plans[i].tobytes() == shared_plans[i].tobytes(), (mode, "plan", i)


def test_without_point_views_the_stages_are_todays():
    B = 4
    sc = scenario(B, 1, 31)
    fl = make_fleet(sc, B)
    try:
        fl.set_unknown_views(origin=sc["origin"], res=P["res"], dims=sc["dims"])
        names = ["begin", "path_search", "corridors", "corridor_problems", "whole_solve", "safe_corridor", "safe_solve", "commit"]
        assert [n for n, _ in fl.stages()] == names
        fl.set_point_views()
        assert [n for n, _ in fl.stages()] == names[:1] + ["map_views"] + names[1:]
        fl.set_point_views(False)
        assert [n for n, _ in fl.stages()] == names
    finally:
        fl.close()


# ---- 2. teams ------------------------------------------------------------------------------------------------------------------------------
def team_scene(pairs, seed):
    """`pairs` start/goal pairs, each flown by one vehicle of team A and one of team B; tree 2j stands 1.6 m and tree 2j + 1 3.2 m from
    start j on the straight line to its goal.  Trees as frontend.forest_cloud samples them; every start and goal is clear of every tree."""
    rng = np.random.default_rng(seed)
    size, radius, spacing = (20.0, 20.0, 3.0), 0.3, 0.15
    starts, goals, trees = [], [], []
    clear = radius + P["inflation"] + 0.45
    while len(starts) < pairs:
        s = rng.uniform([2.0, 2.0], [18.0, 18.0])
        a = rng.uniform(0, 2 * np.pi)
        u = np.array([np.cos(a), np.sin(a)])
        g = s + 9.0 * u
        if not (1.0 < g[0] < 19.0 and 1.0 < g[1] < 19.0):
            continue
        t = [s + 1.6 * u, s + 3.2 * u]
        pts = np.array(starts + goals).reshape(-1, 2)
        old = np.array(trees).reshape(-1, 2)
        if len(pts) and min(np.linalg.norm(pts - q, axis=1).min() for q in t) < clear:
            continue
        if len(old) and (min(np.linalg.norm(old - q, axis=1).min() for q in (s, g)) < clear or min(np.linalg.norm(old - q, axis=1).min() for q in t) < 2 * radius + 0.1):
            continue
        starts.append(s); goals.append(g); trees += t
    ang = np.arange(0, 2 * np.pi, spacing / radius)
    zs = np.arange(0.0, size[2] + 1e-9, spacing)
    ring = np.stack([radius * np.cos(ang), radius * np.sin(ang)], axis=1)
    per_tree = len(zs) * len(ang)
    cloud = np.concatenate([np.column_stack([np.tile(c + ring, (len(zs), 1)), np.repeat(zs, len(ang))]) for c in trees])
    tree_of = np.arange(len(cloud)) // per_tree
    z = rng.uniform(1.0, 2.0, size=pairs)
    s3, g3 = np.column_stack([starts, z]), np.column_stack([goals, z])
    return cloud, tree_of, np.concatenate([s3, s3]), np.concatenate([g3, g3])


def test_two_teams_equal_their_planners(tmp_path):
    """Two teams of 32 vehicles with the same 32 start/goal pairs: team A knows the even-numbered trees, team B the odd ones, and a tree of
    each parity stands on every straight line.  8 cycles; unknown space: everything farther than 3 m from the pair's start, one view
    per team member pair shared through view_of.  Every vehicle equals its Planner given cloud[mask_team]; on the CPU model alone at
    least a quarter of the vehicles differ from their twin in the other team."""
    pairs, C = 32, 8
    B = 2 * pairs
    cloud, tree_of, starts, goals = team_scene(pairs, 5)
    rng = np.random.default_rng(6)
    cells = (110, 110, 15)
    center = np.array([10.0, 10.0, 1.5])
    probe = capi.Map(0)
    probe.read(cloud, cells, P["res"], center, 0.0, P["z_max"], P["inflation"])
    dims, origin = probe.dims()
    probe.close()
    dims, origin = [int(d) for d in dims], np.array(origin, dtype=np.float64)
    states = np.zeros(B, dtype=abi.state_dtype)
    states["pos"] = starts
    ticks = rng.integers(2, P["delta_t"], size=C).astype(np.int32)
    ticks[C // 2] = 400
    sc = {"cloud": cloud, "cells": cells, "center": center, "states": states, "goals": goals, "dims": dims, "origin": origin, "ticks": ticks}
    iz, iy, ix = np.meshgrid(np.arange(dims[2]), np.arange(dims[1]), np.arange(dims[0]), indexing="ij")
    centres = np.stack([(ix + 0.5) * P["res"] + origin[0], (iy + 0.5) * P["res"] + origin[1], (iz + 0.5) * P["res"] + origin[2]], axis=-1)
    n_cells = dims[0] * dims[1] * dims[2]
    views = np.ones((pairs, n_cells), dtype=np.uint8)           # unknown views: one per PAIR (both teams know the same free space)
    for j in range(pairs):
        views[j][(np.linalg.norm(centres - starts[j], axis=-1) < 3.0).reshape(-1)] = 0
    known = np.stack([tree_of % 2 == 0, tree_of % 2 == 1])       # point views: one per TEAM ...
    # ... but both kinds of view share one numbering: view v = 2 * pair + team
    view_of = np.array([2 * (i % pairs) + i // pairs for i in range(B)], dtype=np.int32)
    flags = np.repeat(views, 2, axis=0)
    mask = om.pack(known)[np.arange(2 * pairs) % 2]
    fl = new_fleet(sc, B, P["inflation"])
    per_cycle = []
    try:
        fl.set_unknown_views(flags, view_of=view_of, n_views=2 * pairs, origin=origin, res=P["res"], dims=dims)
        fl.set_point_views(mask)
        for c in range(C):
            fl.replan()
            after = fl.vehicles()
            fl.next_goals(int(ticks[c]), follow=True)
            per_cycle.append((after, fl.vehicles(), fl.goals()))
        plans = fl.plans()
    finally:
        fl.close()
    none = np.zeros(0, dtype=np.int32)
    reveals = [[np.nonzero(views[i % pairs] == 0)[0] if c == 0 else none for c in range(C)] for i in range(B)]
    learned = [[np.nonzero(known[i // pairs])[0] if c == 0 else none for c in range(C)] for i in range(B)]
    st = run_occ_stub(tmp_path, sc, reveals, learned, P["inflation"], "teams")
    differ = sum(1 for j in range(pairs) if any(not np.array_equal(st[j][0][c]["d"][12:24], st[j + pairs][0][c]["d"][12:24]) for c in range(C)))
    print("teams: %d of %d pairs fly differently in the two teams (host model)" % (differ, pairs))
    assert 2 * differ >= B // 4, differ
    worst = assert_equals_host(per_cycle, plans, st, B, C)
    stages = np.concatenate([x[0]["stage"] for x in per_cycle])
    print("teams == host planners: worst state difference %.2e, stages %s" % (worst, np.bincount(stages)))
    assert (stages == 5).sum() > B


# ---- 3. mask edges in the decomposition ------------------------------------------------------------------------------------------------------
def masked_rows(ctx, cloud, keep, segment):
    """fh_corridor_batch_device for one path of one leg with the mask `keep` attached -> rows [r][4] (None: no corridor)"""
    import torch

    fpp = dec.MAX_FACES_POLY
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    d_cloud = to_dev(np.asarray(cloud, dtype=np.float64))
    d_mask = to_dev(om.pack(keep).view(np.int32))
    d_path, d_np = to_dev(np.asarray(segment, dtype=np.float64).reshape(1, 2, 3)), to_dev(np.array([2], dtype=np.int32))
    d_faces = torch.zeros(fpp * abi.face_dtype.itemsize, dtype=torch.uint8, device="cuda:0")
    d_off, d_npoly = torch.zeros(9, dtype=torch.int32, device="cuda:0"), torch.zeros(1, dtype=torch.int32, device="cuda:0")
    ctx.set_point_views_device(d_mask.data_ptr(), d_mask.shape[1], None, 1)
    try:
        ctx.corridor_batch_device(d_cloud.data_ptr(), len(cloud), d_path.data_ptr(), d_np.data_ptr(), 1, 2, 1, fpp, d_faces.data_ptr(), d_off.data_ptr(),
                                  d_npoly.data_ptr(), drone_radius=dec.DRONE_RADIUS, bbox=dec.BBOX)
        ctx.sync()
    finally:
        ctx.set_point_views_device(None)
    if int(d_npoly.cpu()[0]) != 1:
        return None
    count = int(d_off.cpu()[1])
    r = d_faces.cpu().numpy().view(abi.face_dtype)[:count]
    return np.column_stack([r["a"], r["b"]])


def host_rows(segment, cloud):
    (A, b), = frontend.decompose(np.asarray(segment).reshape(2, 3), cloud, drone_radius=dec.DRONE_RADIUS, bbox=dec.BBOX)[0]
    return np.column_stack([A, b])


def edge_cases():
    rng = np.random.default_rng(12)
    seg = dec.HORIZONTAL
    out = []
    for n in (31, 32, 33, 65):
        cloud = dec.exact_cloud(seg, n - n // 3, n // 3, 100 + n)
        keep = rng.random(n) < 0.5
        keep[n - 1] = True                                   # (the last point of the cloud: the last bit in use)
        out.append(("n_cloud %d" % n, cloud, keep))
    cloud = dec.exact_cloud(seg, 48, 16, 7)
    keep = np.zeros(64, dtype=bool)
    keep[63] = True
    inside = dec.plane_depth(seg, cloud) >= dec.MARGIN_IN
    if not inside[63]:                                        # the one known point must be a point of the box
        j = np.nonzero(inside)[0][-1]
        cloud[[j, 63]] = cloud[[63, j]]
    out.append(("only the last bit of the last word", cloud, keep))
    for extra in (0, 1):
        cloud = dec.exact_cloud(seg, 2 * dec.CAP, 192, 21 + extra)
        inside = np.nonzero(dec.plane_depth(seg, cloud) >= dec.MARGIN_IN)[0]
        keep = np.zeros(len(cloud), dtype=bool)
        keep[rng.choice(inside, dec.CAP + extra, replace=False)] = True
        keep[rng.choice(np.setdiff1d(np.arange(len(cloud)), inside), 64, replace=False)] = True   # (known points outside the box as well)
        out.append(("%d of %d box points known (cap %d)" % (dec.CAP + extra, 2 * dec.CAP, dec.CAP), cloud, keep))
    return out


@pytest.mark.parametrize("k", range(7))
def test_masked_decomposition_equals_the_sub_cloud(k):
    frontend_built()
    what, cloud, keep = edge_cases()[k]
    ctx = capi.Context(0)
    try:
        got = masked_rows(ctx, cloud, keep, dec.HORIZONTAL)
        ref = host_rows(dec.HORIZONTAL, cloud[keep])
        full = host_rows(dec.HORIZONTAL, cloud)
        print("%s: %d of %d points known, %d rows (all points: %d rows)" % (what, int(keep.sum()), len(cloud), len(ref), len(full)))
        assert len(ref) <= dec.MAX_FACES_POLY
        assert got is not None and got.shape == ref.shape and np.array_equal(got, ref), what
        assert ref.shape != full.shape or not np.array_equal(ref, full), "the mask makes no difference: the case checks nothing"
    finally:
        ctx.close()


def frontend_built():
    from faster_amd import build as fb

    fb.build_frontend()


# ---- 4. observing against the numpy restatement -----------------------------------------------------------------------------------------------
def test_observe_equals_the_numpy_model():
    """40 views, four of them shared by two vehicles; a cloud with points on voxel faces, outside the lattice and not finite; a lattice that
    is not the map's; two calls with the views grown in between: every word equals the model, and the second call only adds bits."""
    from faster_amd.fleet import Fleet

    B, n_views = 44, 40
    cloud, cells, center, starts, goals = frontend.forest_queries(B, 43)
    lo, lres, ldims = np.array([0.37, -0.21, 0.05]), 0.25, [70, 85, 11]
    rng = np.random.default_rng(9)
    k = rng.choice(len(cloud) - 64, 600, replace=False)       # (the cloud is cut short below: not its last points)
    cloud = cloud.copy()
    cloud[k[:200]] = lo + lres * rng.integers(0, 11, size=(200, 3))                       # on voxel corners: all three faces
    cloud[k[200:400], 0] = lo[0] + lres * rng.integers(0, 70, size=200)                   # on one face
    cloud[k[400:450]] = lo + lres * np.array(ldims) * rng.integers(0, 2, size=(50, 3))    # corners of the lattice: only (0, 0, 0) is inside
    cloud[k[450:500]] += 100.0                                                            # far outside
    cloud[k[500:520], 0] = np.nan
    cloud[k[520:540], 1] = np.inf
    cloud[k[540:560], 2] = -np.inf
    cloud = cloud[:len(cloud) - (len(cloud) % 32) - 7]                                    # (a last word that is not full)
    view_of = np.arange(B, dtype=np.int32)
    view_of[40:] = [3, 11, 17, 29]
    fl = Fleet(B, abi.default_fleet_params())
    try:
        fl.set_map(cloud, cells, P["res"], center, P["z_max"], ONE_CELL)
        occ, (mdims, morigin) = fl.map.occupancy(), fl.map.dims()
        fl.set_unknown_views(view_of=view_of, n_views=n_views, origin=lo, res=lres, dims=ldims)
        fl.set_point_views()
        words = om.words_for(len(cloud))
        assert fl.point_masks().shape == (n_views, words) and not fl.point_masks().any()
        views = np.ones((n_views, ldims[2], ldims[1], ldims[0]), dtype=np.uint8)
        model = np.zeros((n_views, words), dtype=np.uint32)
        step = goals - starts
        step /= np.linalg.norm(step, axis=1, keepdims=True)
        for call, pos in enumerate((starts, starts + 1.1 * step)):
            fl.init(pos, goals)
            fl.sense(R_SENSE)
            fl.observe()
            sense_model.sense(views, view_of, pos, R_SENSE, lo, lres, occ, np.array(morigin, dtype=np.float64), P["res"])
            assert np.array_equal(fl.views(), views)
            before = model.copy()
            om.observe(model, views, cloud, lo, lres)
            got = fl.point_masks()
            bad = np.nonzero(got != model)
            assert len(bad[0]) == 0, "call %d: %d words differ, first: view %d word %d got %08x model %08x" % (
                call, len(bad[0]), bad[0][0], bad[1][0], got[bad][0], model[bad][0])
            assert not (before & ~model).any() and (model != before).any(), call
            print("observe == model, call %d: %d bits set" % (call, int(om.unpack(model, len(cloud)).sum())))
        known = om.unpack(model, len(cloud))
        assert not known[:, k[400:560]][:, np.isnan(cloud[k[400:560]]).any(axis=1) | np.isinf(cloud[k[400:560]]).any(axis=1)].any()
        assert known[:, k[:400]].any() and known.any(axis=1).sum() > n_views // 2
        assert len(np.unique(model, axis=0)) > n_views // 2
        fl.observe()                                                                      # nothing new to see: nothing changes
        assert np.array_equal(fl.point_masks(), model)
    finally:
        fl.close()


# ---- 5. the closed loop -------------------------------------------------------------------------------------------------------------------------
def test_closed_loop_equals_the_host_planner(tmp_path):
    """64 vehicles x 16 cycles of sense -> observe -> replan -> next_goals; the masks start at zero, the views all unknown but 1.5 m around
    the start; world inflation below one cell.  Every cycle the masks equal the model; every vehicle equals its Planner.  On the model
    alone (two runs of the host planners, the second with masks that stay empty): some vehicle flies, in the very cycle whose replan
    follows its first observation of a tree, unlike the same vehicle that never learns a point, and like it in every cycle before.  The
    scene decides this on the CPU: the forest has 0.1 trees per square metre, so nearly every vehicle has a tree within r_sense of its
    start and first observes in cycle 0; vehicles that first observe later are counted as well."""
    B, C = 64, 16
    sc = scenario(B, C, 31)
    probe = capi.Map(0)
    probe.read(sc["cloud"], sc["cells"], P["res"], sc["center"], 0.0, P["z_max"], ONE_CELL)
    dims, origin = probe.dims()
    probe.close()
    dims, origin = [int(d) for d in dims], np.array(origin, dtype=np.float64)
    sc["dims"], sc["origin"] = dims, origin
    n_cells, n_cloud = dims[0] * dims[1] * dims[2], len(sc["cloud"])
    iz, iy, ix = np.meshgrid(np.arange(dims[2]), np.arange(dims[1]), np.arange(dims[0]), indexing="ij")
    centres = np.stack([(ix + 0.5) * P["res"] + origin[0], (iy + 0.5) * P["res"] + origin[1], (iz + 0.5) * P["res"] + origin[2]], axis=-1)
    start_views = np.ones((B, dims[2], dims[1], dims[0]), dtype=np.uint8)
    for i in range(B):
        start_views[i][np.linalg.norm(centres - sc["states"]["pos"][i], axis=-1) < 1.5] = 0
    fl = new_fleet(sc, B, ONE_CELL)
    views = start_views.copy()
    model = np.zeros((B, om.words_for(n_cloud)), dtype=np.uint32)
    prev, prev_known = np.ones((B, n_cells), dtype=np.uint8), np.zeros((B, n_cloud), dtype=bool)
    reveals, learned = [[None] * C for _ in range(B)], [[None] * C for _ in range(B)]
    per_cycle = []
    try:
        occ = fl.map.occupancy()
        fl.set_unknown_views(start_views.reshape(B, n_cells), origin=origin, res=P["res"], dims=dims)
        fl.set_point_views()
        for c in range(C):
            here = fl.vehicles()["state"]["pos"].copy()
            fl.sense(R_SENSE)
            fl.observe()
            sense_model.sense(views, None, here, R_SENSE, origin, P["res"], occ, origin, P["res"])
            om.observe(model, views, sc["cloud"], origin, P["res"])
            assert np.array_equal(fl.views(), views), ("views differ from the model", c)
            got = fl.point_masks()
            assert np.array_equal(got, model), ("masks differ from the model", c, int((got != model).sum()))
            flat, known = views.reshape(B, n_cells), om.unpack(model, n_cloud)
            for i in range(B):
                reveals[i][c] = np.nonzero((prev[i] != 0) & (flat[i] == 0))[0]
                learned[i][c] = np.nonzero(known[i] & ~prev_known[i])[0]
            prev, prev_known = flat.copy(), known
            fl.replan()
            after = fl.vehicles()
            fl.next_goals(int(sc["ticks"][c]), follow=True)
            per_cycle.append((after, fl.vehicles(), fl.goals()))
        plans = fl.plans()
    finally:
        fl.close()
    st = run_occ_stub(tmp_path, sc, reveals, learned, ONE_CELL, "loop")
    none = np.zeros(0, dtype=np.int32)
    blind = run_occ_stub(tmp_path, sc, reveals, [[none] * C for _ in range(B)], ONE_CELL, "blind")
    changed = []
    for i in range(B):
        first = next((c for c in range(C) if len(learned[i][c])), None)
        if first is None:
            continue
        same_before = all(np.array_equal(st[i][0][c]["d"][12:24], blind[i][0][c]["d"][12:24]) for c in range(first))
        differs = not np.array_equal(st[i][0][first]["d"][12:24], blind[i][0][first]["d"][12:24])   # (the goal popped after that replan)
        if same_before and differs:
            changed.append((i, first))
    frac = float(prev_known.mean())
    print("closed loop: %.1f %% of the points known at the end; %d vehicles fly differently in the cycle of their first observation (vehicle, cycle): %s"
          % (100 * frac, len(changed), changed[:8]))
    assert changed, "no vehicle's path depends on what it observed: the scene checks nothing"
    assert 0.0 < frac < 0.9
    worst = assert_equals_host(per_cycle, plans, st, B, C)
    stages = np.concatenate([x[0]["stage"] for x in per_cycle])
    print("closed loop == host planners over %d vehicles x %d cycles: worst state difference %.2e, stages %s" % (B, C, worst, np.bincount(stages)))
    assert (stages == 5).sum() > B


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_the_fused_pair_kernel_and_the_pool_refuse_masks():
    """With masks attached fh_solve_pairs_device returns FH_ERR_ARG and names them; detached it gives what it gave before.  The pool has
    contexts of its own and no call that attaches masks: its pair solve is what it was while another context holds masks."""
    import torch

    B = 64
    whole, faces, _ = corridor.whole_batch(B, seed=21, n_seg=P["N"], p_choices=(2, 3))
    tmpl = corridor.safe_templates(whole)
    ctx = capi.Context(0)
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    try:
        mf = int(whole["face_off"][np.arange(B), whole["n_poly"]].max())
        d_w, d_f = to_dev(whole), to_dev(faces)
        d_mask = torch.zeros(64, dtype=torch.int32, device="cuda:0")

        def pairs():
            d_s, d_sf = to_dev(tmpl), torch.zeros_like(d_f)
            d_wr = torch.zeros(B * abi.result_dtype.itemsize, dtype=torch.uint8, device="cuda:0")
            d_sr = torch.zeros_like(d_wr)
            ctx.solve_pairs_device(d_w.data_ptr(), d_f.data_ptr(), B, P["N"], mf, 0.5, 0.2, 3, d_wr.data_ptr(), d_s.data_ptr(), d_sf.data_ptr(), d_sr.data_ptr())
            ctx.sync()
            return [t.cpu().numpy().copy() for t in (d_wr, d_sr, d_s)]

        first = pairs()
        assert first[0].view(abi.result_dtype)["solved"].sum() > 0.8 * B
        ctx.set_point_views_device(d_mask.data_ptr(), 16, None, 4)
        with pytest.raises(capi.FasterHipError) as e:
            pairs()
        assert "rc=-1" in str(e.value) and "point masks" in str(e.value), str(e.value)
        assert not hasattr(capi.Pool, "set_point_views")
        ctx.set_point_views_device(None)
        again = pairs()
        fields = [n for n in abi.result_dtype.names if n not in ("nodes", "qp_iters", "kflops")]
        for a, b in ((first[0], again[0]), (first[1], again[1])):
            for f in fields:
                assert np.array_equal(a.view(abi.result_dtype)[f], b.view(abi.result_dtype)[f]), f
        assert first[2].tobytes() == again[2].tobytes()
    finally:
        ctx.close()
