"""The model of include/fasterhip_reach.h (fh_reach_goals_device) restated in Python, brute force: a queue over the voxels of the box,
one voxel at a time — no bitmaps and no words, so it shares no structure with the kernel.  The frontier mask, the candidate rule and
map_read are those of tests/frontier_model.py.  Not a test file.

`variant` names a deliberately WRONG model (VARIANTS): tests/test_reach_model.py shows that the named cases (CASES) tell every one of
them from the model, so a kernel that made one of these mistakes would not pass tests/test_gpu_reach.py."""
from collections import deque

import numpy as np

from faster_amd import abi

import frontier_model as fm

VARIANTS = ("row_wrap",        # the x neighbours are the voxels before and after in the box's memory order: rows wrap into the next
            "no_carry",        # no x step between box columns 63 | 64, 127 | 128, ...: no carry between the words of a row
            "cap64",           # the flood ends after level 64 whatever max_hops says
            "start_passable",  # a start that is not passable floods nothing
            "diag_xy",         # eight neighbours in the plane (and the two in z)
            "n26",             # 26 neighbours
            "d2_first",        # the smallest (d2, hops, c)
            "z_pass")          # z_lo <= q.z <= z_hi is asked of passable voxels too

INF, NAN = float("inf"), float("nan")
ALL = abi.FH_FRONTIER_WANT_ALL


def box_axis(p, r_max, origin, res, n):
    """(lo, hi) of the box along one axis, clipped to [0, n - 1] (lo > hi: empty), whatever the quotient is."""
    with np.errstate(all="ignore"):
        fl = np.floor((np.float64(p) - np.float64(r_max) - np.float64(origin)) / np.float64(res)) - 1.0
        fh = np.floor((np.float64(p) + np.float64(r_max) - np.float64(origin)) / np.float64(res)) + 1.0
    lo = (int(fl) if fl < n else n) if fl > 0.0 else 0
    hi = (int(fh) if fh >= 0.0 else -1) if fh < n - 1 else n - 1
    return lo, hi


def map_free(grid, occ, m_origin, m_res):
    """[nz][ny][nx] bool: the map cell of the voxel's centre lies inside the map and is clear (the expression of frontier_model)."""
    origin, res, dims = grid
    nx, ny, nz = (int(d) for d in dims)
    res = float(res)
    qx = ((np.arange(nx) + 0.5) * res + float(origin[0]))[None, None, :]
    qy = ((np.arange(ny) + 0.5) * res + float(origin[1]))[None, :, None]
    qz = ((np.arange(nz) + 0.5) * res + float(origin[2]))[:, None, None]
    mz, my, mx = occ.shape
    m_res = float(m_res)
    fx, fy, fz = np.floor((qx - m_origin[0]) / m_res), np.floor((qy - m_origin[1]) / m_res), np.floor((qz - m_origin[2]) / m_res)
    inside = np.broadcast_to((fx >= 0) & (fx < mx) & (fy >= 0) & (fy < my) & (fz >= 0) & (fz < mz), (nz, ny, nx))
    jx = np.broadcast_to(np.clip(fx, 0, mx - 1), (nz, ny, nx)).astype(np.int64)
    jy = np.broadcast_to(np.clip(fy, 0, my - 1), (nz, ny, nx)).astype(np.int64)
    jz = np.broadcast_to(np.clip(fz, 0, mz - 1), (nz, ny, nx)).astype(np.int64)
    return inside & (occ[jz, jy, jx] == 0), qz


_FACES = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
_DIAG_XY = _FACES + [(1, 1, 0), (1, -1, 0), (-1, 1, 0), (-1, -1, 0)]
_N26 = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)]


def flood(start, lo, hi, passable, max_hops, variant=None):
    """hops [nz][ny][nx] int, -1 where the flood does not come: a queue, voxel by voxel.  start, lo, hi: (x, y, z)."""
    hops = np.full(passable.shape, -1, dtype=np.int64)
    sx, sy, sz = start
    if variant == "start_passable" and not passable[sz, sy, sx]:
        return hops
    cap = max_hops
    if variant == "cap64":
        cap = 64 if max_hops == 0 else min(max_hops, 64)
    steps = {"diag_xy": _DIAG_XY, "n26": _N26}.get(variant, _FACES)
    bx, by, bz = hi[0] - lo[0] + 1, hi[1] - lo[1] + 1, hi[2] - lo[2] + 1
    hops[sz, sy, sx] = 0
    queue = deque([(sx, sy, sz)])
    while queue:
        x, y, z = queue.popleft()
        h = int(hops[z, y, x])
        if cap > 0 and h >= cap:
            continue
        near = []
        for dx, dy, dz in steps:
            if variant == "row_wrap" and dx != 0 and dy == 0 and dz == 0:
                f = ((z - lo[2]) * by + (y - lo[1])) * bx + (x - lo[0]) + dx
                if 0 <= f < bx * by * bz:
                    near.append((lo[0] + f % bx, lo[1] + (f // bx) % by, lo[2] + f // (bx * by)))
                continue
            u, v, w = x + dx, y + dy, z + dz
            if not (lo[0] <= u <= hi[0] and lo[1] <= v <= hi[1] and lo[2] <= w <= hi[2]):
                continue
            if variant == "no_carry" and dx != 0 and (u - lo[0]) // 64 != (x - lo[0]) // 64:
                continue
            near.append((u, v, w))
        for u, v, w in near:
            if hops[w, v, u] < 0 and passable[w, v, u]:
                hops[w, v, u] = h + 1
                queue.append((u, v, w))
    return hops


def reach_goals(par, grid, flags, view_stride, view_of, n_views, vehicles, occ, m_origin, m_res, variant=None):
    """-> (goals [n][3], mask [n] int32, records [n] abi.reach_record_dtype), the arguments of frontier_model.frontier_goals with an
    abi.reach_params_dtype record."""
    origin, res, dims = grid
    nx, ny, nz = (int(d) for d in dims)
    n = len(vehicles)
    views = fm.views_of(flags, n_views, view_stride, dims)
    free, qz_of = map_free(grid, occ, m_origin, m_res)
    fronts = {}
    goals = np.zeros((n, 3), dtype=np.float64)
    mask = np.zeros(n, dtype=np.int32)
    rec = np.zeros(n, dtype=abi.reach_record_dtype)
    r_max, max_hops = float(par["r_max"]), int(par["max_hops"])
    for i in range(n):
        v = int(i if view_of is None else view_of[i])
        p, g = vehicles["state"]["pos"][i], vehicles["g_term"][i]
        flag = abi.FH_FRONTIER_WANTED if fm.wanted(int(par["want"]), int(vehicles["status"][i]), int(vehicles["stage"][i])) else 0
        if not 0 <= v < n_views:
            flag |= abi.FH_FRONTIER_NO_VIEW
        if not (np.all(np.isfinite(p)) and np.all(np.isfinite(g))):
            flag |= abi.FH_FRONTIER_BAD_POS
        goals[i] = g   # (the bits: a copy)
        rec[i] = (flag, v, -1, -1, 0, 0, 0, 0, np.inf, 0.0)
        if flag != abi.FH_FRONTIER_WANTED:
            continue
        with np.errstate(all="ignore"):
            s = [np.floor((np.float64(p[k]) - np.float64(origin[k])) / np.float64(res)) for k in range(3)]
        if not all(0.0 <= s[k] < dims[k] for k in range(3)):
            rec["flags"][i] |= abi.FH_REACH_START_OUTSIDE
            continue
        start = tuple(int(x) for x in s)
        box = [box_axis(p[k], r_max, origin[k], res, int(dims[k])) for k in range(3)]
        lo, hi = [b[0] for b in box], [b[1] for b in box]
        assert all(lo[k] <= start[k] <= hi[k] for k in range(3))
        words = -(-(hi[0] - lo[0] + 1) // 64) * (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1)
        if words > abi.FH_REACH_MAX_WORDS:
            rec["flags"][i] |= abi.FH_REACH_BOX_TOO_LARGE
            continue
        if v not in fronts:
            fronts[v] = fm.frontier_mask(views[v])
        with np.errstate(over="ignore", invalid="ignore"):
            ok, d2, (qx, qy, qz) = fm.candidates_of(fronts[v], p, g, par, grid, occ, m_origin, m_res)
        passable = (views[v] == 0) & free
        if variant == "z_pass":
            passable = passable & (float(par["z_lo"]) <= qz_of) & (qz_of <= float(par["z_hi"]))
        hops = flood(start, lo, hi, passable, max_hops, variant)
        rec["candidates"][i] = int(ok.sum())
        rec["reachable"][i] = int((ok & (hops >= 0)).sum())
        rec["reached"][i] = int((hops >= 0).sum())
        rec["levels"][i] = max(int(hops.max()), 0)
        if max_hops > 0 and int(hops.max()) == max_hops:
            rec["flags"][i] |= abi.FH_REACH_CUT
        cells = np.nonzero((ok & (hops >= 0)).ravel())[0]
        if not len(cells):
            continue
        hh, dd = hops.ravel()[cells], d2.ravel()[cells]
        keys = [(dd[k], hh[k], cells[k]) if variant == "d2_first" else (hh[k], dd[k], cells[k]) for k in range(len(cells))]
        k = min(range(len(cells)), key=lambda j: keys[j])
        c = int(cells[k])
        iz, iy, ix = c // (nx * ny), (c // nx) % ny, c % nx
        goals[i] = (qx[0, 0, ix], qy[0, iy, 0], qz[iz, 0, 0])
        mask[i] = 1
        rec["flags"][i] |= abi.FH_FRONTIER_FOUND
        rec["cell"][i], rec["hops"][i], rec["d2"][i] = c, int(hh[k]), dd[k]
    return goals, mask, rec


# ---- the named cases: the smallest shapes at which the kernel can still go wrong ------------------------------------------------------
def reach_params(r_max, r_avoid=0.0, z_lo=-INF, z_hi=INF, want=ALL, max_hops=0):
    p = abi.default_reach_params(r_max)
    p["r_avoid"], p["z_lo"], p["z_hi"], p["want"], p["max_hops"] = r_avoid, z_lo, z_hi, want, max_hops
    return p


def centre(cell, res=0.5, origin=(0.0, 0.0, 0.0)):
    return tuple((cell[k] + 0.5) * res + origin[k] for k in range(3))


def cell_index(cell, dims):
    return (cell[2] * dims[1] + cell[1]) * dims[0] + cell[0]


def make_case(dims, views, positions, occ, par, res=0.5, origin=(0.0, 0.0, 0.0), view_of=None, g_term=None, m_origin=None, m_res=None, gap=2):
    """views: [n_views][nz][ny][nx] uint8; occ: [mz][my][mx], non-zero = occupied; the map's lattice is the views' unless stated.
    g_term: far away unless stated (r_avoid is 0 in most cases anyway)."""
    views = np.asarray(views, dtype=np.uint8)
    n_views, cells = len(views), int(dims[0]) * int(dims[1]) * int(dims[2])
    stride = cells + gap
    flags = np.zeros(n_views * stride, dtype=np.uint8)
    for v in range(n_views):
        flags[v * stride: v * stride + cells] = views[v].ravel()
    veh = np.zeros(len(positions), dtype=abi.vehicle_dtype)
    veh["state"]["pos"] = np.asarray(positions, dtype=np.float64)
    veh["g_term"] = np.asarray(positions, dtype=np.float64) + 1000.0 if g_term is None else g_term
    return {"grid": (tuple(float(o) for o in origin), float(res), tuple(int(d) for d in dims)), "flags": flags, "stride": stride, "cells": cells,
            "view_of": None if view_of is None else np.asarray(view_of, dtype=np.int32), "n_views": n_views, "vehicles": veh,
            "occ": np.asarray(occ, dtype=np.uint8), "m_origin": np.asarray(origin if m_origin is None else m_origin, dtype=np.float64),
            "m_res": float(res if m_res is None else m_res), "par": par, "views": views}


def with_gap(case, fill):
    """The case with the bytes between cells and view_stride set to `fill` (they are never read)."""
    out = dict(case)
    flags = case["flags"].copy()
    for v in range(case["n_views"]):
        flags[v * case["stride"] + case["cells"]: (v + 1) * case["stride"]] = fill
    out["flags"] = flags
    return out


def model(case, variant=None, par=None):
    return reach_goals(case["par"] if par is None else par, case["grid"], case["flags"], case["stride"], case["view_of"], case["n_views"],
                       case["vehicles"], case["occ"], case["m_origin"], case["m_res"], variant)


def frontier_model_of(case):
    """The model of fasterhip_frontier.h on the same tables (its params: the first five fields)."""
    par = abi.default_frontier_params(float(case["par"]["r_max"]))
    for k in ("r_avoid", "z_lo", "z_hi", "want"):
        par[k] = case["par"][k]
    return fm.frontier_goals(par, case["grid"], case["flags"], case["stride"], case["view_of"], case["n_views"], case["vehicles"], case["occ"],
                             case["m_origin"], case["m_res"])


def floor_case(free, marked, positions, par):
    """A lattice of two layers.  Layer 0 is known; its voxel (x, y) is free in the map where free[y][x].  Layer 1 is occupied, and
    unknown exactly above the `marked` voxels: those voxels of layer 0 (where free) are the candidates, and no other voxel is."""
    free = np.asarray(free, dtype=bool)
    ny, nx = free.shape
    view = np.zeros((2, ny, nx), dtype=np.uint8)
    occ = np.zeros((2, ny, nx), dtype=np.uint8)
    occ[0][~free] = 100
    occ[1][:] = 100
    for x, y in marked:
        view[1, y, x] = 1
    return make_case((nx, ny, 2), [view] * len(positions), [centre((x, y, 0)) for x, y in positions], occ, par)


def sealed_pocket():
    dims = (12, 8, 3)
    view = np.zeros((3, 8, 12), dtype=np.uint8)
    view[:, :, 8:] = 1
    view[:, 6, 2] = 1
    occ = np.zeros((3, 8, 12), dtype=np.uint8)
    for x, y in ((1, 5), (3, 5), (2, 4)):
        occ[:, y, x] = 100
    occ[0, 5, 2] = occ[2, 5, 2] = 100
    return make_case(dims, [view], [centre((2, 2, 1))], occ, reach_params(10.0))


def word_carry():
    """150 x 3 x 1: the row y = 1 is the only free one; vehicle 0 at its first voxel with the only unknown voxel beside its last one,
    vehicle 1 the other way round."""
    dims = (150, 3, 1)
    occ = np.full((1, 3, 150), 100, dtype=np.uint8)
    occ[0, 1, :] = 0
    a, b = np.zeros((1, 3, 150), dtype=np.uint8), np.zeros((1, 3, 150), dtype=np.uint8)
    a[0, 0, 149] = 1
    b[0, 0, 0] = 1
    return make_case(dims, [a, b], [centre((0, 1, 0)), centre((149, 1, 0))], occ, reach_params(100.0))


def row_ends():
    """70 x 3 x 2, all occupied but four voxels.  Vehicle 0 stands in the last voxel of row (y 0, z 0); the first voxel of the row after
    it is free and a candidate.  Vehicle 1 stands in the last voxel of the last row of slab 0; the first voxel of slab 1 is free and a
    candidate.  Neither has a face in common with its vehicle."""
    dims = (70, 3, 2)
    occ = np.full((2, 3, 70), 100, dtype=np.uint8)
    view = np.zeros((2, 3, 70), dtype=np.uint8)
    for x, y, z in ((69, 0, 0), (0, 1, 0), (69, 2, 0), (0, 0, 1)):
        occ[z, y, x] = 0
    view[0, 1, 1] = view[1, 0, 1] = 1   # unknown voxels beside the two candidates
    return make_case(dims, [view], [centre((69, 0, 0)), centre((69, 2, 0))], occ, reach_params(100.0), view_of=[0, 0])


def serpentine():
    """21 x 22 x 1: the even rows 0 .. 20 are free from end to end, the odd rows between them are walls with one gap, at alternating
    ends; row 21 is a wall whose last voxel is unknown.  240 steps from (0, 0) to the only candidate (20, 20)."""
    nx, ny = 21, 22
    occ = np.full((1, ny, nx), 100, dtype=np.uint8)
    for y in range(0, 21, 2):
        occ[0, y, :] = 0
    for k, y in enumerate(range(1, 20, 2)):
        occ[0, y, nx - 1 if k % 2 == 0 else 0] = 0
    view = np.zeros((1, ny, nx), dtype=np.uint8)
    view[0, 21, 20] = 1
    return make_case((nx, ny, 1), [view], [centre((0, 0, 0))], occ, reach_params(100.0))


def clipped_box():
    """6 x 5 x 5, res 0.5, r_max 1: vehicles in two opposite corners, boxes clipped on three sides each; the far half of x unknown for
    one and the near half for the other."""
    dims = (6, 5, 5)
    a, b = np.zeros((5, 5, 6), dtype=np.uint8), np.zeros((5, 5, 6), dtype=np.uint8)
    a[:, :, 2:] = 1
    b[:, :, :4] = 1
    occ = np.zeros((5, 5, 6), dtype=np.uint8)
    occ[0, 1, 1] = 100
    return make_case(dims, [a, b], [(0.1, 0.2, 0.3), (2.9, 2.4, 2.4)], occ, reach_params(1.0))


def one_voxel():
    return make_case((1, 1, 1), [np.zeros((1, 1, 1), dtype=np.uint8)], [(0.25, 0.25, 0.25)], np.zeros((1, 1, 1), dtype=np.uint8), reach_params(3.0))


def start_blocked():
    """6 x 6 x 2: the start of vehicle 0 is unknown in its view, the start of vehicle 1 is occupied in the map."""
    dims = (6, 6, 2)
    a, b = np.zeros((2, 6, 6), dtype=np.uint8), np.zeros((2, 6, 6), dtype=np.uint8)
    a[0, 2, 2] = 1
    a[:, :, 5] = 1
    b[:, 5, :] = 1
    occ = np.zeros((2, 6, 6), dtype=np.uint8)
    occ[1, 3, 3] = 100
    return make_case(dims, [a, b], [centre((2, 2, 0)), centre((3, 3, 1))], occ, reach_params(10.0))


def start_outside():
    """Vehicle 0 below the lattice in x, vehicle 1 above it in z, both within r_max of known frontier voxels; vehicle 2 inside."""
    dims = (6, 5, 3)
    view = np.zeros((3, 5, 6), dtype=np.uint8)
    view[:, 4, :] = 1
    occ = np.zeros((3, 5, 6), dtype=np.uint8)
    return make_case(dims, [view], [(-0.2, 1.0, 0.7), (1.0, 1.0, 1.5), (1.1, 1.2, 0.7)], occ, reach_params(4.0), view_of=[0, 0, 0])


def _slab(dims):
    view = np.zeros((dims[2], dims[1], dims[0]), dtype=np.uint8)
    view[:, :, dims[0] - 1] = 1
    return make_case(dims, [view], [centre((1, 1, 1))], np.zeros(view.shape, dtype=np.uint8), reach_params(100.0))


def box_too_large():
    return _slab((8, 41, 25))    # 1 x 41 x 25 = 1025 words


def box_at_cap():
    return _slab((8, 32, 32))    # 1 x 32 x 32 = 1024 words


def _max_hops(k):
    """10 x 1 x 1, the vehicle in voxel 0, voxels 6 .. 9 unknown: the only candidate is voxel 5, in level 5, which is the last level."""
    view = np.zeros((1, 1, 10), dtype=np.uint8)
    view[0, 0, 6:] = 1
    return make_case((10, 1, 1), [view], [centre((0, 0, 0))], np.zeros((1, 1, 10), dtype=np.uint8), reach_params(100.0, max_hops=k))


def ties_cell():
    """Candidates two steps to either side of the vehicle: equal hops, equal d2, the lower cell wins."""
    return floor_case(np.ones((3, 7), dtype=bool), [(1, 1), (5, 1)], [(3, 1)], reach_params(10.0))


def ties_d2():
    """Two steps each: (5, 1) straight ahead with d2 = 1, (4, 2) round the corner with d2 = 0.5.  The cell of the nearer one is larger."""
    return floor_case(np.ones((4, 7), dtype=bool), [(5, 1), (4, 2)], [(3, 1)], reach_params(10.0))


def ties_hops():
    """(6, 1): three steps, d2 = 2.25.  (3, 3): d2 = 1, but behind a wall (2 .. 4, 2): six steps.  Hops win."""
    free = np.ones((5, 8), dtype=bool)
    free[2, 2:5] = False
    return floor_case(free, [(6, 1), (3, 3)], [(3, 1)], reach_params(10.0))


def other_lattice():
    """A map with another origin and a res that is no multiple of the views', smaller than the lattice: the voxels of the rows iy = 0
    and of the last columns have their centres outside it.  Three vehicles, one view each, a known ball around each."""
    dims, res, origin = (20, 9, 4), 0.5, (-2.0, -1.5, 0.0)
    rng = np.random.default_rng(15)
    m_res, m_origin, m_dims = 0.3, (-1.87, -0.93, -0.11), (28, 13, 8)   # x up to 6.53 (the lattice: 8.0), y from -0.93 (-1.5), z up to 2.29 (2.0)
    occ = (rng.random((m_dims[2], m_dims[1], m_dims[0])) < 0.12).astype(np.uint8) * 100
    positions = [(0.3, 0.4, 0.9), (3.1, 1.6, 1.2), (6.9, 0.2, 0.4)]
    iz, iy, ix = np.meshgrid(np.arange(dims[2]), np.arange(dims[1]), np.arange(dims[0]), indexing="ij")
    q = np.stack([(ix + 0.5) * res + origin[0], (iy + 0.5) * res + origin[1], (iz + 0.5) * res + origin[2]], axis=-1)
    views = []
    for p in positions:
        view = np.ones((dims[2], dims[1], dims[0]), dtype=np.uint8)
        view[np.linalg.norm(q - np.array(p), axis=-1) < 2.2] = 0
        views.append(view)
    return make_case(dims, views, positions, occ, reach_params(3.0, z_lo=0.6, z_hi=1.4), res=res, origin=origin, m_origin=m_origin, m_res=m_res)


def shared_view():
    """Vehicles 0, 1, 2 and 4 read view 0, vehicle 3 names a view that does not exist; vehicle 4 has a NaN coordinate."""
    dims = (9, 7, 3)
    view = np.zeros((3, 7, 9), dtype=np.uint8)
    view[:, :, 7:] = 1
    view[2, 0, 0] = 1
    occ = np.zeros((3, 7, 9), dtype=np.uint8)
    occ[:, 3, 2:6] = 100
    positions = [(0.7, 0.6, 0.8), (2.3, 2.9, 0.3), (3.2, 0.4, 1.3), (1.0, 1.0, 1.0), (1.0, NAN, 1.0)]
    g = np.array(positions) + 0.3
    g[4] = (1.0, 1.0, 1.0)
    return make_case(dims, [view], positions, occ, reach_params(2.0, r_avoid=0.5), view_of=[0, 0, 0, 7, 0], g_term=g)


CASES = {"sealed_pocket": sealed_pocket, "word_carry": word_carry, "row_ends": row_ends, "serpentine": serpentine, "clipped_box": clipped_box,
         "one_voxel": one_voxel, "start_blocked": start_blocked, "start_outside": start_outside, "box_too_large": box_too_large,
         "box_at_cap": box_at_cap, "max_hops_before": lambda: _max_hops(4), "max_hops_at": lambda: _max_hops(5),
         "max_hops_after": lambda: _max_hops(6), "ties_cell": ties_cell, "ties_d2": ties_d2, "ties_hops": ties_hops,
         "other_lattice": other_lattice, "shared_view": shared_view}


def equality_as_case(name, gap=0):
    """frontier_model.equality_case under the parameter set `name` of frontier_model.PARAM_SETS, as a case of this module."""
    eq = fm.equality_case(gap)
    fp = fm.PARAM_SETS[name]
    par = reach_params(float(fp["r_max"]), float(fp["r_avoid"]), float(fp["z_lo"]), float(fp["z_hi"]), int(fp["want"]))
    return {"grid": eq["grid"], "flags": eq["flags"], "stride": fm.STRIDE, "cells": fm.CELLS, "view_of": eq["view_of"], "n_views": fm.N_VIEWS,
            "vehicles": eq["vehicles"], "occ": eq["occ"], "m_origin": np.asarray(eq["m_origin"], dtype=np.float64), "m_res": fm.MAP_RES, "par": par,
            "views": eq["views"]}


_BUILT = {}


def case(name):
    """The named case (or "equality:<parameter set>"), built once.  Treat it as read-only."""
    if name not in _BUILT:
        _BUILT[name] = equality_as_case(name.split(":", 1)[1]) if name.startswith("equality:") else CASES[name]()
    return _BUILT[name]


ALL_CASES = list(CASES) + ["equality:" + k for k in fm.PARAM_SETS]
_MODELS = {}


def expected(name):
    """The model's outputs of the named case, computed once.  Treat them as read-only."""
    if name not in _MODELS:
        _MODELS[name] = model(case(name))
    return _MODELS[name]
