"""The model of include/fasterhip_frontier.h (fh_map_frontier_goals_device, fh_map_view_coverage_device) restated in numpy, brute force
over every cell of the lattice, operation for operation, for the tests that compare the device's outputs byte for byte.  Not a test file.

numpy evaluates a * a + b * b + c * c as ((a a) + (b b)) + (c c) with every operation rounded: IEEE double, no fused multiply-add, the
three products summed from left to right, as the header writes it.

`variant` names a deliberately WRONG model (VARIANTS): tests/test_frontier_model.py shows that the inputs of the GPU equality tests
(equality_case, PARAM_SETS) tell every one of them from the model, so a kernel that made one of these mistakes would not pass."""
import numpy as np

from faster_amd import abi

VARIANTS = ("le_rmax",           # d2 <= r_max^2
            "tie_larger",        # ties in d2 go to the larger cell
            "boundary_unknown",  # a face on the boundary of the lattice counts as unknown
            "flat_x",            # the x neighbours are the bytes c - 1 and c + 1, which wrap across rows
            "no_half",           # q = ix res + origin
            "no_map",            # no map test
            "le_avoid",          # e2 <= r_avoid^2 is excluded too
            "z_exclusive")       # z_lo < q.z < z_hi

GOAL_REACHED, NO_PATH = 2, 1


def frontier_mask(view, variant=None):
    """view: [nz][ny][nx] uint8.  True where the voxel is known (0) and one of its six face neighbours inside the lattice is not."""
    unk = view != 0
    edge = variant == "boundary_unknown"
    near = np.zeros(view.shape, dtype=bool)
    for axis in range(3):
        if axis == 2 and variant == "flat_x":
            flat = unk.ravel()
            near |= np.concatenate([[False], flat[:-1]]).reshape(view.shape)
            near |= np.concatenate([flat[1:], [False]]).reshape(view.shape)
            continue
        pad = [(0, 0)] * 3
        pad[axis] = (1, 1)
        padded = np.pad(unk, pad, constant_values=edge)
        n = view.shape[axis]
        near |= np.take(padded, np.arange(0, n), axis=axis)       # the neighbour below
        near |= np.take(padded, np.arange(2, n + 2), axis=axis)   # the neighbour above
    return ~unk & near


def views_of(flags, n_views, view_stride, dims):
    """[n_views][nz][ny][nx] from the flat table; the bytes between cells and view_stride are dropped."""
    nx, ny, nz = (int(d) for d in dims)
    cells = nx * ny * nz
    f = np.asarray(flags, dtype=np.uint8).reshape(-1)
    return np.stack([f[v * view_stride: v * view_stride + cells].reshape(nz, ny, nx) for v in range(n_views)])


def view_coverage(flags, n_views, view_stride, dims, variant=None):
    out = np.zeros(n_views, dtype=abi.view_coverage_dtype)
    for v, view in enumerate(views_of(flags, n_views, view_stride, dims)):
        out["known"][v] = int((view == 0).sum())
        out["frontier"][v] = int(frontier_mask(view, variant).sum())
    return out


def wanted(want, status, stage):
    return bool(((want & abi.FH_FRONTIER_WANT_REACHED) and status == GOAL_REACHED) or ((want & abi.FH_FRONTIER_WANT_NO_PATH) and stage == NO_PATH)
                or (want & abi.FH_FRONTIER_WANT_ALL))


def candidates_of(frontier, p, g, par, grid, occ, m_origin, m_res, variant=None):
    """(candidate mask [nz][ny][nx], d2 [nz][ny][nx], q as three broadcastable arrays) of one searched vehicle."""
    origin, res, dims = grid
    nx, ny, nz = (int(d) for d in dims)
    res = float(res)
    half = 0.0 if variant == "no_half" else 0.5
    qx = ((np.arange(nx) + half) * res + float(origin[0]))[None, None, :]
    qy = ((np.arange(ny) + half) * res + float(origin[1]))[None, :, None]
    qz = ((np.arange(nz) + half) * res + float(origin[2]))[:, None, None]
    z_lo, z_hi = float(par["z_lo"]), float(par["z_hi"])
    ok = frontier & ((z_lo < qz) & (qz < z_hi) if variant == "z_exclusive" else (z_lo <= qz) & (qz <= z_hi))
    r_max, r_avoid = np.float64(par["r_max"]), np.float64(par["r_avoid"])
    dx, dy, dz = qx - p[0], qy - p[1], qz - p[2]
    d2 = dx * dx + dy * dy + dz * dz
    ok = ok & ((d2 <= r_max * r_max) if variant == "le_rmax" else (d2 < r_max * r_max))
    ex, ey, ez = qx - g[0], qy - g[1], qz - g[2]
    e2 = ex * ex + ey * ey + ez * ez
    ok = ok & ~((e2 <= r_avoid * r_avoid) if variant == "le_avoid" else (e2 < r_avoid * r_avoid))
    if variant != "no_map":
        mz, my, mx = occ.shape
        m_res = float(m_res)
        fx, fy, fz = np.floor((qx - m_origin[0]) / m_res), np.floor((qy - m_origin[1]) / m_res), np.floor((qz - m_origin[2]) / m_res)
        inside = (fx >= 0) & (fx < mx) & (fy >= 0) & (fy < my) & (fz >= 0) & (fz < mz)
        inside = np.broadcast_to(inside, ok.shape)
        jx = np.broadcast_to(np.clip(fx, 0, mx - 1), ok.shape).astype(np.int64)
        jy = np.broadcast_to(np.clip(fy, 0, my - 1), ok.shape).astype(np.int64)
        jz = np.broadcast_to(np.clip(fz, 0, mz - 1), ok.shape).astype(np.int64)
        ok = ok & inside & (occ[jz, jy, jx] == 0)
    return ok, np.broadcast_to(d2, ok.shape), (qx, qy, qz)


def frontier_goals(par, grid, flags, view_stride, view_of, n_views, vehicles, occ, m_origin, m_res, variant=None):
    """-> (goals [n][3], mask [n] int32, records [n] abi.frontier_record_dtype).  par: an abi.frontier_params_dtype record; grid =
    (origin, res, dims); flags: the flat table of n_views rows, view_stride apart; vehicles: abi.vehicle_dtype; occ: [mz][my][mx],
    non-zero = occupied (what Map.occupancy returns)."""
    origin, res, dims = grid
    nx, ny, nz = (int(d) for d in dims)
    n = len(vehicles)
    views = views_of(flags, n_views, view_stride, dims)
    fronts = {}
    goals = np.zeros((n, 3), dtype=np.float64)
    mask = np.zeros(n, dtype=np.int32)
    rec = np.zeros(n, dtype=abi.frontier_record_dtype)
    for i in range(n):
        v = int(i if view_of is None else view_of[i])
        p, g = vehicles["state"]["pos"][i], vehicles["g_term"][i]
        flag = abi.FH_FRONTIER_WANTED if wanted(int(par["want"]), int(vehicles["status"][i]), int(vehicles["stage"][i])) else 0
        if not 0 <= v < n_views:
            flag |= abi.FH_FRONTIER_NO_VIEW
        if not (np.all(np.isfinite(p)) and np.all(np.isfinite(g))):
            flag |= abi.FH_FRONTIER_BAD_POS
        goals[i] = g   # (the bits: a copy)
        rec[i] = (flag, v, -1, 0, np.inf, 0.0)
        if flag != abi.FH_FRONTIER_WANTED:
            continue
        if v not in fronts:
            fronts[v] = frontier_mask(views[v], variant)
        with np.errstate(over="ignore", invalid="ignore"):
            ok, d2, (qx, qy, qz) = candidates_of(fronts[v], p, g, par, grid, occ, m_origin, m_res, variant)
        cells = np.nonzero(ok.ravel())[0]
        rec["candidates"][i] = len(cells)
        if not len(cells):
            continue
        dd = d2.ravel()[cells]
        tied = cells[dd == dd.min()]
        c = int(tied.max() if variant == "tie_larger" else tied.min())
        iz, iy, ix = c // (nx * ny), (c // nx) % ny, c % nx
        goals[i] = (qx[0, 0, ix], qy[0, iy, 0], qz[iz, 0, 0])
        mask[i] = 1
        rec["flags"][i] |= abi.FH_FRONTIER_FOUND
        rec["cell"][i], rec["d2"][i] = c, dd.min()
    return goals, mask, rec


def map_read(cloud, cells, res, center, z_ground, z_max):
    """fh_map_read_device without inflation: -> (occ [mz][my][mx] uint8 (0 / 100), origin [3], dims (mx, my, mz))."""
    dx, dy, dz = int(cells[0]), int(cells[1]), int(cells[2])
    down = up = int(dz / 2.0)
    if center[2] - res * dz / 2.0 < z_ground:
        down = max(int((center[2] - z_ground) / res), 0)
    if center[2] + res * dz / 2.0 > z_max:
        up = max(int((z_max - center[2]) / res), 1)
    dz = down + up
    origin = np.array([center[0] - res * dx / 2.0, center[1] - res * dy / 2.0, center[2] - res * down])
    occ = np.zeros((dz, dy, dx), dtype=np.uint8)
    for pt in np.asarray(cloud, dtype=np.float64).reshape(-1, 3):
        c = [max(int(np.round((pt[k] - origin[k]) / res - 0.5)), 0) for k in range(3)]   # (no point here lies half-way: round is C's round)
        idx = c[0] + dx * c[1] + dx * dy * c[2]
        if 0 <= idx < dx * dy * dz:
            occ.ravel()[idx] = 100
    return occ, origin, (dx, dy, dz)


# ---- the inputs of the GPU equality tests (tests/test_gpu_frontier.py), here so that the CPU test can show what they separate ----
DIMS, RES, ORIGIN = (70, 7, 5), 0.5, (-2.0, -1.5, 0.0)   # nx: more than one wavefront and no multiple of 64; a dyadic origin
CELLS = DIMS[0] * DIMS[1] * DIMS[2]
STRIDE = CELLS + 3
N_VIEWS = 5
# the map: another resolution, an origin that is no voxel corner, and it does not reach the row iy = 0 of the lattice (y = -1.25)
MAP_CELLS, MAP_RES, MAP_CENTER, MAP_Z = (118, 11, 10), 0.3, (15.6, 0.55, 1.3), (-10.0, 10.0)
INF, NAN = float("inf"), float("nan")


def _q(ix, iy, iz):
    return np.array([(ix + 0.5) * RES + ORIGIN[0], (iy + 0.5) * RES + ORIGIN[1], (iz + 0.5) * RES + ORIGIN[2]])


def _params(r_max, r_avoid, z_lo, z_hi, want):
    p = abi.default_frontier_params(r_max)
    p["r_avoid"], p["z_lo"], p["z_hi"], p["want"] = r_avoid, z_lo, z_hi, want
    return p


# name -> params.  "exact": vehicle 1 has a voxel at d2 == r_max^2, one at e2 == r_avoid^2, and its whole row at q.z == z_lo.
PARAM_SETS = {
    "exact": _params(1.5, 1.0, 0.75, 1.75, 4),
    "wide": _params(10.0, 0.0, -INF, INF, 4),
    "reached": _params(10.0, 0.0, -INF, INF, 1),
    "no_path": _params(10.0, 0.0, -INF, INF, 2),
    "reached_or_no_path": _params(10.0, 0.0, -INF, INF, 3),
    "mid": _params(3.0, 0.75, -INF, 1.25, 7),
}


def _ball(view, centre, r):
    nx, ny, nz = DIMS
    for iz in range(nz):
        for iy in range(ny):
            for ix in range(nx):
                d = _q(ix, iy, iz) - centre
                if d[0] * d[0] + d[1] * d[1] + d[2] * d[2] < r * r:
                    view[iz, iy, ix] = 0


def equality_case(gap):
    """The tables of the equality tests; the bytes between cells and view_stride hold `gap`.  -> dict(flags, view_of, vehicles, cloud,
    occ, m_origin, m_dims, grid)."""
    nx, ny, nz = DIMS
    views = np.ones((N_VIEWS, nz, ny, nx), dtype=np.uint8)
    # view 0: what five vehicles at ordinary positions have seen
    posts = [np.array(c) for c in ((4.1, 0.2, 1.1), (12.3, -0.4, 0.9), (12.9, 0.6, 1.4), (21.7, 0.1, 0.6), (27.2, -0.3, 1.9))]
    for c in posts:
        _ball(views[0], c, 1.3)
    # view 1: the edges.  A row along x (iy 3, iz 1) around vehicle 1, which stands on the centre of voxel 20 of it; a voxel at ix = 0; a
    # voxel in the row iy = 0 that the map does not reach; the last cell; and K = (69, 2, 2) with its five neighbours inside the lattice
    # known: K's only unknown "neighbour" is the byte after the end of its row, (0, 3, 2)
    views[1][1, 3, 18:24] = 0
    views[1][1, 1, 0] = 0
    views[1][1, 0, 5] = 0
    views[1][nz - 1, ny - 1, nx - 1] = 0
    for ix, iy, iz in ((69, 2, 2), (68, 2, 2), (69, 1, 2), (69, 3, 2), (69, 2, 1), (69, 2, 3)):
        views[1][iz, iy, ix] = 0
    views[2][:] = 0   # all known: no frontier
    #         3: all unknown: no frontier
    corner = np.array([0.0, 0.5, 1.0])   # a voxel corner: candidates tie exactly in d2
    _ball(views[4], corner, 1.0)
    flags = np.full(N_VIEWS * STRIDE, gap, dtype=np.uint8)
    for v in range(N_VIEWS):
        flags[v * STRIDE: v * STRIDE + CELLS] = views[v].ravel()
    n = 16
    veh = np.zeros(n, dtype=abi.vehicle_dtype)
    view_of = np.array([4, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, -1, N_VIEWS, 2, 3], dtype=np.int32)
    pos = np.zeros((n, 3))
    pos[0] = corner
    pos[1] = _q(20, 3, 1)
    pos[2] = (32.9, 0.1, 1.2)     # at the edge of the lattice: the box is clipped
    pos[3] = (-1.9, -0.8, 0.7)
    pos[4] = (-4.0, 0.3, 1.0)     # outside the lattice, within reach of it for r_max = 10
    for k, c in enumerate(posts):
        pos[5 + k] = c + np.array([0.3, -0.2, 0.1]) * (k - 2)
    pos[10] = (4.0, NAN, 1.0)
    pos[11] = posts[1]
    pos[12], pos[13] = posts[0], posts[2]
    pos[14], pos[15] = (10.0, 0.0, 1.0), (10.0, 0.0, 1.0)
    g = pos + np.array([0.4, 0.2, 0.0])
    g[1] = _q(21, 3, 1)           # voxels 19 and 23 of the row are at exactly 1.0 from it
    g[4] = (60.0, 0.0, 1.0)       # wholly outside, with every box empty
    g[10] = (4.0, 0.0, 1.0)
    g[11] = (INF, 0.0, 1.0)
    veh["state"]["pos"], veh["g_term"] = pos, g
    veh["status"] = np.arange(n) % 4                     # TRAVELING, GOAL_SEEN, GOAL_REACHED, YAWING
    veh["stage"] = np.array([1, 5, 0, 1, 5, 0, 1, 5, 0, 1, 5, 0, 1, 5, 0, 1])[:n]   # NO_PATH against every status
    # occupied: the centre of a frontier voxel of view 0 (the first one that the map reaches, near vehicle 5), the map cell beside the
    # one of another (the last one, near vehicle 7), and the centre of voxel 18 of vehicle 1's row
    front = [c for c in np.nonzero(frontier_mask(views[0]).ravel())[0] if (c // nx) % ny >= 1]
    occupied, beside = ((int(c % nx), int((c // nx) % ny), int(c // (nx * ny))) for c in (front[0], front[-1]))
    cloud = np.array([_q(*occupied), _q(*beside) + (MAP_RES, 0.0, 0.0), _q(18, 3, 1)])
    occ, m_origin, m_dims = map_read(cloud, MAP_CELLS, MAP_RES, MAP_CENTER, MAP_Z[0], MAP_Z[1])
    return {"flags": flags, "view_of": view_of, "vehicles": veh, "cloud": cloud, "occ": occ, "m_origin": m_origin, "m_dims": m_dims,
            "grid": (ORIGIN, RES, DIMS), "views": views, "occupied": occupied, "beside": beside}


def equality_model(case, par, variant=None, n=None):
    n = len(case["vehicles"]) if n is None else n
    return frontier_goals(par, case["grid"], case["flags"], STRIDE, case["view_of"][:n], N_VIEWS, case["vehicles"][:n], case["occ"],
                          case["m_origin"], MAP_RES, variant)
