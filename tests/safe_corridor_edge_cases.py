"""Inputs for fh_safe_corridor_batch_device (safe_path_kernel in faster_amd/csrc/fh_safe.hip.hpp, decomp_kernel with an UnknownLattice,
safe_finalize_kernel) at the edges of the march, of the voxel search and of the lattice.  numpy only: tests/test_safe_corridor_edge_cases.py
proves every property on the CPU against the restatements, tests/test_gpu_safe_corridor_edges.py runs the same inputs on the device.

A GROUP is one launch: a rule, a lattice, an occupied cloud, and PAIRS that each bring their own flags (a view of their own,
fh_set_unknown_views_device), their JPS_in path, their goal and a whole trajectory written by hand.

Rule mode 2 chooses R with findIndexH / findIndexR against the SAME unknown voxels, and a pair none of whose samples comes within
drone_radius of one needs no safe path at all.  So the whole trajectory of every mode-2 pair is a straight line at constant speed from the
start towards a flagged cell (its `trigger`), slow enough that every tenth sample is 0.1 m from the next, with a_max so small that the
vehicle can never brake before H: R is then sample 0 or close to it, and `choose_r` below restates the choice (with a margin on every
decision, so that it does not depend on a rounding)."""
import os
import re

import numpy as np

import decomp_edge_cases as dec
import sample_model as sm
from decomp_edge_cases import (CAP, CAP_GLOBAL, CAP_IDS, MARGIN_IN, MARGIN_OUT, MAX_FACES_POLY, MAX_POLY, MIN_DIST, box_aabb,  # noqa: F401
                               plane_depth, segment_dist)
from faster_amd import abi
from oracle import pair_glue

_t = open(os.path.join(dec.ROOT, "faster_amd", "csrc", "fh_safe.hip.hpp")).read()
_m = re.findall(r"^constexpr int SAFE_PATH_CAP = (\d+);", _t, flags=re.M)
assert len(_m) == 1, _m
SAFE_PATH_CAP = int(_m[0])

BBOX = dec.BBOX
DECOMP_RADIUS = dec.DRONE_RADIUS
N_SEG_SAFE = 6
SPEED, DC, TRAJ_N, A_MAX = 1.0, 0.01, 8, 0.05   # 0.1 m between tested samples; braking distance v^2 / (2 delta_a a_max) = 20 m


# ---- the whole trajectory and R ---------------------------------------------------------------------------------------------------------
def line_trajectory(start, target, speed=SPEED):
    """(problem, result): constant velocity from `start` to `target`, TRAJ_N segments (cubic and quadratic rows zero)."""
    start, target = np.asarray(start, dtype=np.float64), np.asarray(target, dtype=np.float64)
    dist = float(np.linalg.norm(target - start))
    dt = dist / (speed * TRAJ_N)
    v = (target - start) / (dt * TRAJ_N)
    pr = sm.synthetic_problem(TRAJ_N, DC)
    pr["a_max"] = A_MAX
    pr["x0"][:3] = start
    pr["xf"][:3] = target
    pr["f_init"], pr["f_final"], pr["f_inc"] = 1.0, 3.0, 0.5
    rs = np.zeros((), dtype=abi.result_dtype)
    rs["solved"], rs["dt"], rs["factor"] = 1, dt, 1.0
    for s in range(TRAJ_N):
        rs["coeff"][s, 6:9] = v
        rs["coeff"][s, 9:12] = start + v * (s * dt)
    return pr, rs


def state_k(problem, result, k):
    """(state, bound [9]) of sample k by tests/sample_model.py: the exact value rounded once and the bound of a double evaluation"""
    N, dt, dc = int(problem["n_seg"]), float(result["dt"]), float(problem["dc"])
    size = sm.count(N, dt, dc)
    ts, ivs = sm.clock(k + 1, dc, dt, N)
    coef = [[sm.Fraction(float(result["coeff"][ivs[k]][3 * r + a])) for r in range(4)] for a in range(3)]
    exact, bnd = sm.state_in_segment(coef, sm.Fraction(ts[k]), ivs[k], sm.Fraction(dt))
    st, bound = np.zeros(9), np.zeros(9)
    for a in range(3):
        for f in range(3):
            st[3 * f + a], bound[3 * f + a] = (0.0, 0.0) if (f > 0 and k == size - 1) else sm._round_with_bound(exact[a][f], bnd[a][f])
    return st, bound


def positions(problem, result):
    """pos and vel of every sample in doubles (the search for H and R: every decision is asserted to have a margin)"""
    N, dt, dc = int(problem["n_seg"]), float(result["dt"]), float(problem["dc"])
    size = sm.count(N, dt, dc)
    ts, ivs = sm.clock(size, dc, dt, N)
    c = result["coeff"]
    tau = np.array(ts) - np.array(ivs) * dt
    iv = np.array(ivs)
    pos = ((c[iv, 0:3] * tau[:, None] + c[iv, 3:6]) * tau[:, None] + c[iv, 6:9]) * tau[:, None] + c[iv, 9:12]
    vel = (3 * c[iv, 0:3] * tau[:, None] + 2 * c[iv, 3:6]) * tau[:, None] + c[iv, 6:9]
    return pos, vel


def nearest(pts, p):
    d = pts - p
    return float(np.sqrt(np.min(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])))


def choose_r(problem, result, rule, r_frac, unknown_pts, margin=1e-6):
    """-> (k, need): choose_r_index of fh_sample.hip.hpp.  Mode 0: sample (int)(r_frac size).  Mode 2: findIndexH (every tenth sample, the
    first one closer than drone_radius to an unknown voxel centre), then findIndexR (x and y only)."""
    pos, vel = positions(problem, result)
    size = len(pos)
    if rule["mode"] == 0:
        return min(max(int(r_frac * size), 0), size - 1), True
    assert rule["mode"] == 2
    if unknown_pts is None or not len(unknown_pts):
        return size - 1, False
    i_h = None
    for i in range(0, size, 10):
        d = nearest(unknown_pts, pos[i])
        assert abs(d - rule["drone_radius"]) > margin, (i, d)
        if d < rule["drone_radius"]:
            i_h = i
            break
    if i_h is None:
        return size - 1, False
    index_h = min(max(int(rule["delta_h"] * i_h), 0), size - 1)
    den = 2.0 * rule["delta_a"] * float(problem["a_max"])
    for i in range(index_h + 1):
        hit = False
        for a in range(2):
            diff = pos[index_h, a] - pos[i, a]
            w = vel[i, a] * diff
            lhs, rhs = np.sign(w) * vel[i, a] ** 2 / den, abs(diff)
            assert (lhs == 0 and rhs == 0) or abs(lhs - rhs) > 1e-9, (i, a, lhs, rhs)
            hit = hit or lhs > rhs
        if hit:
            return i, True
    return index_h, True


# ---- the lattice ----------------------------------------------------------------------------------------------------------------------------
def centres(origin, res, dims):
    """cell centres [nz][ny][nx][3] as the kernels form them: ((double)i + 0.5) * res + origin"""
    x = (np.arange(dims[0]) + 0.5) * res + origin[0]
    y = (np.arange(dims[1]) + 0.5) * res + origin[1]
    z = (np.arange(dims[2]) + 0.5) * res + origin[2]
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    return np.stack([X, Y, Z], axis=-1)


def flagged(group, flags):
    """the centres of the flagged cells, z-major and x fastest: the unknown cloud of a view"""
    return centres(group["origin"], group["res"], group["dims"])[np.asarray(flags) != 0]


def cell_of(group, p):
    return tuple(int(np.floor((p[a] - group["origin"][a]) / group["res"])) for a in range(3))


def lattice_range(origin, res, dims, lo, hi):
    """lattice_range of fh_decomp.hip.hpp: (x0, cx, y0, cy, z0, cz, total); total 0: empty, -1: more than 1024 cells on an axis"""
    out = []
    for a in range(3):
        first = int(np.floor((lo[a] - origin[a]) / res)) - 1
        first = 0 if first < 0 else (dims[a] if first > dims[a] else first)
        last = int(np.floor((hi[a] - origin[a]) / res)) + 1
        last = dims[a] - 1 if last > dims[a] - 1 else last
        out += [first, last - first + 1]
    cx, cy, cz = out[1], out[3], out[5]
    if cx <= 0 or cy <= 0 or cz <= 0:
        return tuple(out) + (0,)
    cells = cx * cy * cz
    return tuple(out) + (-1 if (cells > (1 << 28) or cx > 1024 or cy > 1024 or cz > 1024) else cells,)


def range_margin(origin, res, lo, hi):
    """how far (in cells) the nearest of the six floor() arguments of lattice_range is from an integer"""
    v = np.concatenate([(np.asarray(lo) - origin) / res, (np.asarray(hi) - origin) / res])
    return float(np.min(np.abs(v - np.round(v))))


def nearest_unknown(group, flags, p, cap=np.inf, widths=None):
    """nearest_unknown of fh_safe.hip.hpp: cubes of half-width w around p's cell; widths receives every w tried.
    -> (distance or a value above cap, 'found' | 'covered' | 'cap' | 'none')"""
    if flags is None:
        return np.inf, "none"
    o, res, (nx, ny, nz) = group["origin"], group["res"], group["dims"]
    cx, cy, cz = cell_of(group, p)
    wmax = max(cx, nx - 1 - cx, cy, ny - 1 - cy, cz, nz - 1 - cz, 0)
    cen = centres(o, res, group["dims"])
    w = 1
    while True:
        if widths is not None:
            widths.append(w)
        x0, x1, y0, y1, z0, z1 = max(cx - w, 0), min(cx + w, nx - 1), max(cy - w, 0), min(cy + w, ny - 1), max(cz - w, 0), min(cz + w, nz - 1)
        best = np.inf
        if x1 >= x0 and y1 >= y0 and z1 >= z0:
            sub = cen[z0:z1 + 1, y0:y1 + 1, x0:x1 + 1][flags[z0:z1 + 1, y0:y1 + 1, x0:x1 + 1] != 0]
            if len(sub):
                d = sub - p
                best = float(np.min(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]))
        d = float(np.sqrt(best))
        if w >= wmax:
            return d, "covered"
        if d <= (w + 0.5) * res:
            return d, "found"
        if (w + 0.5) * res > cap:
            return min(d, 1e300), "cap"
        need = int(np.ceil(d / res)) if best < np.inf else 2 * w + 1
        w = min(max(need, w + 1), wmax)


# ---- groups and pairs -----------------------------------------------------------------------------------------------------------------------
def group(name, mode, origin, res, dims, drone_radius=0.3, r_known=0.0, r_frac=0.5, max_points=SAFE_PATH_CAP, max_poly_safe=3, fpp=96,
          cloud=None, z_ground=0.0):
    return {"name": name, "rule": {"mode": mode, "r_known": r_known, "drone_radius": drone_radius, "delta_h": 1.0, "delta_a": 0.5},
            "r_frac": r_frac, "origin": np.asarray(origin, dtype=np.float64), "res": float(res), "dims": tuple(int(d) for d in dims),
            "max_points": max_points, "max_poly_safe": max_poly_safe, "fpp": fpp, "cloud": np.zeros((0, 3)) if cloud is None else cloud,
            "z_ground": z_ground, "bbox": BBOX, "decomp_radius": DECOMP_RADIUS, "pairs": []}


def no_flags(g):
    return np.zeros(g["dims"][::-1], dtype=np.uint8)


def flag_points(g, pts):
    """flags with exactly the cells of `pts` set; every point must be a cell centre of the lattice (to 1e-9: snap() gives its bits)"""
    f = no_flags(g)
    cen = centres(g["origin"], g["res"], g["dims"])
    for p in np.asarray(pts, dtype=np.float64).reshape(-1, 3):
        ix, iy, iz = cell_of(g, p)
        assert 0 <= ix < g["dims"][0] and 0 <= iy < g["dims"][1] and 0 <= iz < g["dims"][2], (p, (ix, iy, iz))
        assert np.abs(cen[iz, iy, ix] - p).max() < 1e-9, (p, cen[iz, iy, ix])
        f[iz, iy, ix] = 1
    return f


def snap(g, p):
    """the centre of the cell that holds p, as the kernels form it"""
    ix, iy, iz = cell_of(g, p)
    return centres(g["origin"], g["res"], g["dims"])[iz, iy, ix]


def add_pair(g, name, path, flags, trigger=None, goal=None, n_points=None, view=None, start=None, untouched=False, no_corridor=False):
    """path: the JPS_in vertices (n_points defaults to their number; fewer than two vertices are padded).  trigger: the point the whole
    trajectory heads for (mode 2: a flagged cell centre; default: the last vertex).  view: the view number of the pair (default: its own
    flags); flags None with a view outside the range: the caller's error the header describes.  untouched: the march must leave
    the vertices behind the first as they were; no_corridor: a segment of the pair reports failure, the pair gets n_seg = 0."""
    path = np.asarray(path, dtype=np.float64).reshape(-1, 3)
    n_pts = len(path) if n_points is None else n_points
    start = path[0] if start is None else np.asarray(start, dtype=np.float64)
    trigger = path[-1] if trigger is None else np.asarray(trigger, dtype=np.float64)
    if g["rule"]["mode"] == 2 and flags is not None and flags.any():
        trigger = snap(g, trigger)
        assert flags[cell_of(g, trigger)[::-1]], (name, "the trajectory heads for a cell that is not flagged")
        # a trajectory along an axis has the other coordinates constant to the bit: findIndexR then compares exact zeros, not roundings
        start = np.where(np.abs(start - trigger) < 1e-9, trigger, start)
    pr, rs = line_trajectory(start, trigger)
    g["pairs"].append({"name": name, "path": path, "n_points": int(n_pts), "flags": flags, "goal": path[-1] if goal is None else np.asarray(goal, dtype=np.float64),
                       "problem": pr, "result": rs, "view": view, "untouched": untouched, "no_corridor": no_corridor})
    return g["pairs"][-1]


def pair_named(g, name):
    (p,) = [p for p in g["pairs"] if p["name"] == name]
    return p


def expected(g, p, safe_path=pair_glue.safe_path, strict_r=True):
    """What the device must give for pair p, by the restatements: dict(live, k, R, R_bound, unknown, path (the safe path, R first), trace)"""
    rule = g["rule"]
    unk = None
    if rule["mode"] == 2:
        unk = flagged(g, p["flags"]) if p["flags"] is not None else None
    n_pts = p["n_points"]
    out = {"live": False, "unknown": unk, "path": None, "trace": [], "k": None}
    if not (2 <= n_pts <= SAFE_PATH_CAP) or not p["result"]["solved"]:
        return out
    k, need = choose_r(p["problem"], p["result"], rule, g["r_frac"], unk)
    if not need:
        return out
    R, bound = state_k(p["problem"], p["result"], k)
    out.update(live=True, k=k, R=R, R_bound=bound)
    out["path"] = safe_path(p["path"][:n_pts], p["problem"]["x0"][:3], R[:3], rule["r_known"], rule["drone_radius"], g["max_poly_safe"],
                            unknown_pts=unk if rule["mode"] == 2 else None, trace=out["trace"])
    return out


def full_march(g, p):
    """the cut path before R goes first and the legs are limited (max_poly_safe = SAFE_PATH_CAP)"""
    e = expected(g, p)
    tr = []
    full = pair_glue.safe_path(p["path"][:p["n_points"]], p["problem"]["x0"][:3], e["R"][:3], g["rule"]["r_known"], g["rule"]["drone_radius"],
                               SAFE_PATH_CAP, unknown_pts=e["unknown"] if g["rule"]["mode"] == 2 else None, trace=tr)
    return full, tr


def decomposition_cloud(g, p):
    """unknown points first (z-major), then the occupied cloud: what frontend.decompose is given"""
    rule = g["rule"]
    if rule["mode"] == 2:
        unk = flagged(g, p["flags"]) if p["flags"] is not None else np.zeros((0, 3))
    else:
        unk = pair_glue.unknown_voxels(g["origin"], g["res"], np.array(g["dims"]), p["problem"]["x0"][:3], rule["r_known"])
    return np.vstack([unk, g["cloud"]]), len(unk)


# ---- march cases (mode 2, drone_radius 0.3): cases 1, 2, 3, 5 and 14 ------------------------------------------------------------------------------
M_ORIGIN, M_RES, M_DIMS = (-1.0, -2.0, 0.0), 0.1, (100, 40, 30)   # x -1 .. 9, y -2 .. 2, z 0 .. 3


def zigzag(n, leg=0.25, dx=0.2, z=1.55, y0=0.05):
    dy = np.sqrt(leg * leg - dx * dx)
    return np.array([[0.05 + dx * i, y0 + (dy / 2 if i % 2 else -dy / 2), z] for i in range(n)])


def _corridor_flags(g, x_end, wall_y=1.05):
    """a wall of unknown cells beside the path (y = wall_y, one cell thick, z 1.0 .. 2.0) and a slab across it at x = x_end"""
    cen = centres(g["origin"], g["res"], g["dims"])
    band = (cen[..., 2] > 1.0) & (cen[..., 2] < 2.1)
    wall = band & (np.abs(cen[..., 1] - wall_y) < 0.01)
    slab = band & (np.abs(cen[..., 0] - x_end) < 0.01) & (np.abs(cen[..., 1]) < 1.0)
    return (wall | slab).astype(np.uint8)


def march_group(max_poly_safe):
    """vertex counts, the long march (truncated to max_poly_safe legs), the back-off across legs, nothing to hit, where xf lands"""
    g = group("march mps=%d" % max_poly_safe, 2, M_ORIGIN, M_RES, M_DIMS, max_poly_safe=max_poly_safe, fpp=40 * max_poly_safe)
    slab_far, slab_near = _corridor_flags(g, 6.05), _corridor_flags(g, 0.85)
    # 1. vertex counts: 2, CAP - 1, CAP vertices towards the far slab; 0, 1, -1, -2: no safe problem
    for n in (2, SAFE_PATH_CAP - 1, SAFE_PATH_CAP):
        path = zigzag(n) if n > 2 else np.array([[0.05, 0.05, 1.55], [7.05, 0.05, 1.55]])
        add_pair(g, "n_points=%d" % n, path, slab_far, trigger=[6.05, 0.05, 1.55])
    for n in (0, 1, -1, -2):
        add_pair(g, "n_points=%d" % n, zigzag(2), slab_far, trigger=[6.05, 0.05, 1.55], n_points=n)
    # 2. the long march is "n_points=40" above; the slab so near that the cut path is shorter than max_poly_safe + 1 (for FH_MAX_POLY)
    add_pair(g, "near slab", zigzag(SAFE_PATH_CAP), slab_near, trigger=[0.85, 0.05, 1.55])
    # 3. back-off across legs: one long leg, then legs of 0.05 m, one unknown voxel just off the path.  (Eleven vertices: what is left after
    # the back-off fits FH_MAX_POLY legs, so the device's output shows where the back-off ended.)
    back = np.array([[0.05, 0.0, 1.5]] + [[2.05 + 0.05 * i, 0.0, 1.5] for i in range(10)])
    add_pair(g, "back-off", back, flag_points(g, [[2.45, 0.05, 1.55]]), trigger=[2.45, 0.05, 1.55])
    # 5. nothing to hit
    add_pair(g, "no flags", zigzag(5), no_flags(g))
    add_pair(g, "far voxel", zigzag(5), flag_points(g, [[4.05, 0.05, 1.55]]), trigger=[4.05, 0.05, 1.55], untouched=True)
    add_pair(g, "view out of range", zigzag(5), None, view=10 ** 6)
    add_pair(g, "view negative", zigzag(5), None, view=-1)
    # 14. where xf lands: the path of "far voxel" at z = 0.85 (its polytope reaches the ground), G inside, outside, on the ground plane
    low = zigzag(5, z=0.85)
    far = flag_points(g, [[4.05, 0.05, 0.85]])
    last = low[min(max_poly_safe, 4)]
    add_pair(g, "G inside", low, far, trigger=[4.05, 0.05, 0.85], untouched=True, goal=last + [0.1, 0.1, 0.1])
    add_pair(g, "G outside", low, far, trigger=[4.05, 0.05, 0.85], untouched=True, goal=last + [0.0, 3.0, 0.0])
    add_pair(g, "G on the ground", low, far, trigger=[4.05, 0.05, 0.85], untouched=True, goal=[last[0], last[1], 0.0])
    return g


# ---- 4. the boundary of the cut and 6. the nearest voxel (mode 2, drone_radius 0.25, cells of 0.5 m: every number below is exact) ------------
B_ORIGIN, B_RES, B_DIMS = (0.0, 0.0, 0.0), 0.5, (16, 10, 5)


def boundary_group():
    g = group("boundary", 2, B_ORIGIN, B_RES, B_DIMS, drone_radius=0.25)
    c = np.array([2.25, 2.25, 1.25])   # the centre of cell (4, 4, 2)
    one = flag_points(g, [c])
    away = np.array([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0.5, 0], [3.0, 0.5, 0]])
    # 4. first vertex closer than drone_radius (0.2 m): the stub; exactly drone_radius away: `<` is strict, no stub; r = 0 at the first vertex
    add_pair(g, "stub", c + [0.2, 0, 0] + away, one, trigger=c)
    add_pair(g, "exactly drone_radius", c + [0.25, 0, 0] + away, one, trigger=c)
    add_pair(g, "on the first vertex", c + away, one, trigger=c + [0.0, 0.0, 0.0], start=c + [0.5, 0, 0])
    # a voxel centre exactly on the SECOND vertex, the first sphere passes through it: the crossing point is that vertex, r = 0 there
    add_pair(g, "on the second vertex", [c + [1.5, 0, 0], c, c + [0, 1.5, 0]], one, trigger=c)
    # 6. the vertex 0.49 res from its cell centre towards +x; flagged cells at offset (-1, -1, -1) and (+2, 0, 0) of its cell
    v = c + [0.49 * B_RES, 0, 0]
    two = flag_points(g, [c + np.array([-1, -1, -1]) * B_RES, c + np.array([2, 0, 0]) * B_RES])
    add_pair(g, "second cube", [v, v + [2.0, 0, 0], v + [3.0, 0.5, 0]], two, trigger=c + [1.0, 0, 0])
    # two voxels at exactly the same distance (2 cells either side along y), the path between them along x
    tie = flag_points(g, [c + [0, 1.0, 0], c + [0, -1.0, 0], c + [3.0, 0, 0]])
    add_pair(g, "equal distance", [c, c + [1.5, 0, 0], c + [3.5, 0, 0]], tie, trigger=c + [3.0, 0, 0])
    return g


def far_corner_group():
    """6. a lone voxel in the far corner of a 64 x 64 x 16 lattice, the path from the opposite corner through the lattice and out of it"""
    g = group("far corner", 2, (0.0, 0.0, 0.0), 0.1, (64, 64, 16))
    voxel = np.array([6.35, 6.35, 1.55])
    path = np.array([[0.25, 0.25, 0.25], [2.0, 2.2, 0.6], [4.0, 3.8, 1.0], [6.1, 6.2, 1.45], [7.5, 7.5, 1.6]])
    add_pair(g, "far corner", path, flag_points(g, [voxel]), trigger=voxel)
    return g


# ---- 7. lattice geometry: vertices outside the lattice, small lattices, an origin that is no multiple of res -------------------------------------
def outside_group(nz):
    dims = (7, 5, nz)
    g = group("outside 7x5x%d" % nz, 2, (0.13, -0.27, 0.41), 0.5, dims)
    cen = centres(g["origin"], g["res"], dims)
    v = cen[nz // 2, 2, 3]
    f = flag_points(g, [v])
    lo, hi = g["origin"], g["origin"] + g["res"] * np.array(dims)
    for a in range(3):
        for s in (-1, 1):
            first = v.copy()
            first[a] = (lo[a] - 1.0) if s < 0 else (hi[a] + 1.0)
            beyond = v + (v - first) / np.linalg.norm(v - first) * 0.8 + [0.02, 0.03, 0.01]
            add_pair(g, "outside %s%s" % ("-+"[s > 0], "xyz"[a]), [first, (first + v) / 2 + [0.01, 0.02, 0.0], beyond], f, trigger=v)
    add_pair(g, "100 m away", [v + [100.0, 0, 0], v + [50.0, 0.1, 0], v + [-0.7, 0.02, 0.01]], f, trigger=v, start=v + [2.0, 0, 0])
    return g


# ---- 8. modelled unknown space (mode 0): r = r_known - |p - A|, clamped at 0 ------------------------------------------------------------------
S_ORIGIN, S_RES, S_DIMS = (0.0, 0.0, 0.0), 0.2, (50, 50, 15)


def modelled_group(r_known):
    g = group("modelled r_known=%g" % r_known, 0, S_ORIGIN, S_RES, S_DIMS, r_known=r_known, r_frac=0.25)
    A = np.array([5.0, 5.0, 1.5])
    path = A + np.array([[0, 0, 0], [1.0, 0.2, 0.0], [1.9, 0.1, 0.1], [3.0, 0.4, 0.0], [4.0, 0.3, 0.0]])
    add_pair(g, "modelled", path, None, trigger=path[2], untouched=r_known > 50)
    return g


MODELLED_R_KNOWN = (2.5, 0.0, 100.0)


# ---- 9. every list home with lattice ids ----------------------------------------------------------------------------------------------------
H_RES = 0.125
H_ORIGIN, H_DIMS = (-2.5 - H_RES / 2, -2.5 - H_RES / 2, -H_RES / 2), (69, 41, 25)   # centres at multiples of 0.125: x -2.5 .. 6, y -2.5 .. 2.5, z 0 .. 3
H_PATH = np.array([dec.HORIZONTAL[:3], dec.HORIZONTAL[3:], [6.5, 0.0, 1.5]])
H_TRIGGER = np.array([5.5, 0.0, 1.5])
HOME_KS = [CAP - 1, CAP, CAP + 1, CAP_IDS - 1, CAP_IDS, CAP_IDS + 1, CAP_GLOBAL, CAP_GLOBAL + 1]


def home_segment(g):
    """the one leg the safe path keeps: R (sample 0 of the whole trajectory, on the x axis of the path) -> the second vertex"""
    p = {"path": H_PATH, "n_points": 3, "flags": flag_points(g, [H_TRIGGER]), "problem": None, "result": None}
    p["problem"], p["result"] = line_trajectory(H_PATH[0], H_TRIGGER)
    e = expected(g, p)
    assert e["k"] == 0 and len(e["path"]) == 2 and np.array_equal(e["path"][1], H_PATH[1])
    assert e["R"][1] == 0.0 and e["R"][2] == 1.5
    return np.concatenate([e["path"][0], e["path"][1]])


def eligible_cells(g, segment, min_dist=MIN_DIST):
    """(centres [n][3] in lattice order, flat indices): at least MARGIN_IN inside the local box of the segment, at least min_dist from the
    whole JPS_in path (so that the march is not cut before the second vertex)"""
    cen = centres(g["origin"], g["res"], g["dims"]).reshape(-1, 3)
    ok = plane_depth(segment, cen) >= MARGIN_IN
    for a, b in zip(H_PATH[:-1], H_PATH[1:]):
        ok &= segment_dist(np.concatenate([a, b]), cen) >= min_dist
    ok &= segment_dist(segment, cen) >= min_dist
    return cen[ok], np.nonzero(ok)[0]


def _home_flags(g, idx, k, seed):
    rng = np.random.default_rng(seed)
    f = flag_points(g, [H_TRIGGER]).reshape(-1)
    f[rng.choice(idx, size=k, replace=False)] = 1
    return f.reshape(g["dims"][::-1])


def assert_list_length(g, p, segment, k):
    """exactly k points of the pair's decomposition cloud (flagged cell centres, then occupied points) lie at least MARGIN_IN inside the
    local box of the segment; every other one is at least MARGIN_OUT outside its bounding box (an unflagged cell is never listed,
    wherever it lies)"""
    cloud, _ = decomposition_cloud(g, p)
    depth = plane_depth(segment, cloud)
    inside = depth >= MARGIN_IN
    assert int(inside.sum()) == k, (int(inside.sum()), k)
    assert np.all(dec.aabb_clearance(segment, cloud[~inside]) >= MARGIN_OUT)


def homes_group():
    g = group("homes", 2, H_ORIGIN, H_RES, H_DIMS, max_poly_safe=1, fpp=128)
    seg = home_segment(g)
    _, idx = eligible_cells(g, seg)
    for j, k in enumerate(HOME_KS):
        add_pair(g, "k=%d" % k, H_PATH, _home_flags(g, idx, k, 100 + j), trigger=H_TRIGGER, no_corridor=k > CAP_GLOBAL)
    g["segment"], g["n_eligible"] = seg, len(idx)
    return g


TIE_VOXEL, TIE_POINT = np.array([1.0, 0.75, 1.5]), np.array([1.0, -0.75, 1.5])


def split_group():
    """CAP + 1 and CAP_IDS + 1 list entries split between voxels and occupied points; in the first the voxel (1, 0.75, 1.5) and the occupied
    point (1, -0.75, 1.5) mirror each other about the segment and are the nearest of all: the voxel is listed first and wins the tie"""
    g = group("split", 2, H_ORIGIN, H_RES, H_DIMS, max_poly_safe=1, fpp=128)
    seg = home_segment(g)
    rng = np.random.default_rng(77)
    n_occ = 100
    occ = dec._inside_points(seg, n_occ - 1, rng, BBOX, dec.TIE_MIN_DIST)
    g["cloud"] = np.vstack([occ[:40], TIE_POINT, occ[40:], dec._outside_points(seg, 200, rng, BBOX)])
    _, idx = eligible_cells(g, seg, dec.TIE_MIN_DIST)
    for j, k in enumerate((CAP + 1, CAP_IDS + 1)):
        f = _home_flags(g, idx, k - n_occ - (1 if j == 0 else 0), 200 + j)
        if j == 0:
            f |= flag_points(g, [TIE_VOXEL])
        add_pair(g, "split k=%d" % k, H_PATH, f, trigger=H_TRIGGER)
    g["segment"] = seg
    return g


# ---- 10. sub-block sizes around the trips of 64 and the four-trip prefetch -------------------------------------------------------------------------
BLOCK_DIMS = [(1, 1, 1), (7, 3, 3), (4, 4, 4), (5, 13, 1), (5, 17, 3), (8, 8, 4), (257, 1, 1)]
BLOCK_GAP = np.array([0.6, 0.45, 0.3])


def block_group(dims):
    """A small lattice with every cell flagged, inside the local boxes of two legs along x: "first" ends short of the corner (0, 0, 0) of the
    block, coming from -x, -y, -z — the FIRST cell of the sweep is the nearest point and gives the first plane —, "last" leaves from beyond
    the opposite corner: the LAST cell of the sweep gives it.  The whole trajectories head for those two cells."""
    res = 0.005 if max(dims) > 64 else 0.05
    origin = np.array([3.0, 3.0, 1.5])
    g = group("block %dx%dx%d" % dims, 2, origin, res, dims, max_poly_safe=1, fpp=64)
    cen = centres(g["origin"], g["res"], dims)
    f = np.ones(dims[::-1], dtype=np.uint8)
    lo, hi = cen[0, 0, 0], cen[-1, -1, -1]
    add_pair(g, "first", [lo - BLOCK_GAP - [2.0, 0, 0], lo - BLOCK_GAP], f, trigger=lo, untouched=True)
    add_pair(g, "last", [hi + BLOCK_GAP, hi + BLOCK_GAP + [2.0, 0, 0]], f, trigger=hi, untouched=True)
    return g


# ---- 11. clipping: the local box sticks out of the lattice ----------------------------------------------------------------------------------------
C_ORIGIN, C_RES, C_DIMS = (0.0, 0.0, 0.0), 0.25, (48, 40, 12)   # x 0 .. 12, y 0 .. 10, z 0 .. 3


def clip_group(nz=C_DIMS[2]):
    dims = (C_DIMS[0], C_DIMS[1], nz)
    oz = 0.0 if nz > 1 else 1.375   # the lattice one cell thick: the layer around z = 1.5
    g = group("clip nz=%d" % nz, 2, (0.0, 0.0, oz), C_RES, dims, max_poly_safe=1, fpp=160)
    cen = centres(g["origin"], g["res"], dims)
    zc = cen[nz // 2, 0, 0, 2]
    rng = np.random.default_rng(31)
    sprinkle = rng.random(dims[::-1]) < (0.02 if nz > 1 else 0.3)

    def pair(name, p1, p2, p3):
        """a leg p1 -> p2 whose box is clipped, a second leg towards a flagged cell near p3"""
        p1, p2, p3 = (np.array(v, dtype=np.float64) for v in (p1, p2, p3))
        trig = cen[cell_of(g, p3)[::-1]]
        f = sprinkle.copy()
        c = cen.reshape(-1, 3)
        near = np.zeros(len(c), dtype=bool)
        for a, b in ((p1, p2), (p2, trig)):
            near |= segment_dist(np.concatenate([a, b]), c) < 0.45
        f.reshape(-1)[near] = False
        f = f.astype(np.uint8) | flag_points(g, [trig])
        add_pair(g, name, [p1, p2, trig + (trig - p2) / np.linalg.norm(trig - p2) * 0.5], f, trigger=trig)

    z = 1.5
    pair("-x", [0.5, 5.0, z], [1.5, 5.2, z], [4.5, 5.0, z])
    pair("+x", [11.5, 5.0, z], [10.5, 5.2, z], [7.5, 5.0, z])
    pair("-y", [6.0, 0.5, z], [6.2, 1.5, z], [6.0, 4.5, z])
    pair("+y", [6.0, 9.5, z], [6.2, 8.5, z], [6.0, 5.5, z])
    if nz > 1:
        pair("-z", [3.0, 3.0, 0.4], [4.0, 3.2, 0.5], [7.0, 3.0, 0.6])
        pair("+z", [3.0, 7.0, 2.6], [4.0, 7.2, 2.5], [7.0, 7.0, 2.4])
        # the box of the first leg entirely outside the lattice (x < -2.4): the sub-block is empty, the rows those of the occupied points
        pair("outside", [-6.0, 5.0, z], [-4.5, 5.1, z], [1.1, 5.1, z])
        g["cloud"] = np.array([[-5.0, 5.9, 1.6], [-5.5, 4.2, 1.2], [-4.0, 5.5, 2.1], [6.0, 5.0, 1.5]])
    g["zc"] = zc
    return g


# ---- 12. 1024 cells per axis -------------------------------------------------------------------------------------------------------------------
FINE_RES, FINE_ORIGIN = 0.00585, (-2.2, 0.5, 1.5)


def fine_group(cx_wanted):
    """A lattice of cx_wanted + 34 x 2 x 2 cells of 5.85 mm beside the first leg.  It begins before the local box and ends INSIDE it, so the
    sub-block of the leg runs from the cell before the box to the last cell of the lattice: cx_wanted cells along x (1024: the packed
    cell number needs all ten bits of x, and that last column is listed; 1025: the segment reports failure)."""
    path = np.array([[0.0, 0.0, 1.5], [2.0, 0.0, 1.5], [4.2, 0.55, 1.5]])
    probe = group("probe", 2, FINE_ORIGIN, FINE_RES, (4096, 2, 2))
    last = snap(probe, [3.5, 0.5, 1.5])
    R, _ = state_k(*line_trajectory(path[0], last), 0)
    lo, hi = box_aabb(np.concatenate([R[:3], path[1]]))
    x0 = lattice_range(probe["origin"], FINE_RES, probe["dims"], lo, hi)[0]
    g = group("fine cx=%d" % cx_wanted, 2, FINE_ORIGIN, FINE_RES, (x0 + cx_wanted, 2, 2), max_poly_safe=1, fpp=64)
    cen = centres(g["origin"], g["res"], g["dims"])
    trig = cen[0, 0, -1]   # the last column: the whole trajectory heads for it
    R, _ = state_k(*line_trajectory(path[0], trig), 0)
    seg = np.concatenate([R[:3], path[1]])
    lo, hi = box_aabb(seg)
    r = lattice_range(g["origin"], g["res"], g["dims"], lo, hi)
    assert r[0] == x0 and r[1] == cx_wanted and range_margin(g["origin"], g["res"], lo, hi) > 1e-3, r
    cols = [x0, x0 + 1, x0 + 63, x0 + 64, x0 + 511, x0 + 1022]
    pts = [cen[iz, iy, ix] for ix, iy, iz in zip(cols, (0, 1, 0, 1, 0, 1), (0, 0, 1, 1, 0, 1))] + [trig]
    add_pair(g, "fine", path, flag_points(g, pts), trigger=trig, no_corridor=cx_wanted > 1024)
    g["range"], g["segment"] = r, seg
    return g


# ---- 13. the sphere model (mode 0): a cell centre exactly r_known from A ----------------------------------------------------------------------------
def sphere_group(below):
    """cells of 0.5 m, A on a cell centre, the cell at offset (1.5, 2.0, 0) exactly 2.5 m away: not unknown for r_known = 2.5 (`>` is
    strict), unknown for the next double below"""
    r_known = float(np.nextafter(2.5, 0.0)) if below else 2.5
    g = group("sphere %s" % ("below" if below else "exact"), 0, (0.0, 0.0, 0.0), 0.5, (20, 20, 6), r_known=r_known, r_frac=0.1, max_poly_safe=1, fpp=128)
    A = np.array([4.25, 4.25, 1.25])
    add_pair(g, "sphere", [A, A + [0.9, 1.1, 0.1]], None, untouched=True)
    g["cell"] = A + [1.5, 2.0, 0.0]
    return g


# ---- 15. table sizes ---------------------------------------------------------------------------------------------------------------------------
def shell_group():
    """A leg of 1 m inside a shell of unknown cells (0.78 .. 0.82 m around its midpoint, cells of 0.04 m): every tangent plane cuts off
    little more than its own voxel, the polytope has more than FH_MAX_FACES_POLY rows: no corridor"""
    res = 0.04
    g = group("shell", 2, (-1.0 - res / 2, -1.0 - res / 2, 0.5 - res / 2), res, (76, 51, 51), drone_radius=0.1, max_poly_safe=1, fpp=512)
    cen = centres(g["origin"], g["res"], g["dims"])
    d = np.linalg.norm(cen - [0.5, 0.0, 1.5], axis=-1)
    f = ((d > 0.78) & (d < 0.82)).astype(np.uint8)
    trig = cen[cell_of(g, [1.3, 0.0, 1.5])[::-1]]
    assert f[cell_of(g, trig)[::-1]]
    add_pair(g, "shell", [[0.0, 0.0, 1.5], [1.0, 0.0, 1.5], [1.9, 0.0, 1.5]], f, trigger=trig, no_corridor=True)
    return g


def rows_group():
    """three pairs with different row totals (one, two and three legs kept before the cut) for faces_per_problem = T and T - 1"""
    g = group("rows", 2, M_ORIGIN, M_RES, M_DIMS, max_poly_safe=3, fpp=256)
    for name, x_end in (("one leg", 0.85), ("three legs", 6.05)):
        add_pair(g, name, zigzag(8, leg=0.5, dx=0.4), _corridor_flags(g, x_end), trigger=[x_end, 0.05, 1.55])
    add_pair(g, "no walls", zigzag(8, leg=0.5, dx=0.4), flag_points(g, [[6.05, 0.05, 1.55]]), trigger=[6.05, 0.05, 1.55])
    return g
