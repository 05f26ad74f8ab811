"""The model of include/fasterhip_sight.h (fh_sight_goals_device) restated in Python, brute force: the flood, the box, the passable voxels
and the candidates are those of tests/reach_model.py and tests/frontier_model.py by import, the ball is that of tests/gain_model.py; for
every (candidate, unknown voxel of the box in the ball) the line is walked with the closed formula for r(a, k), one division per axis
and step — no remainders, no rows, no words, so it shares no structure with the kernel (numpy does all voxels of a candidate at once).
Not a test file.

`variant` names a deliberately WRONG model (VARIANTS): tests/test_sight_model.py shows that the named cases (CASES) tell every one of
them from the model, so a kernel that made one of these mistakes would not pass tests/test_gpu_sight.py."""
import numpy as np

from faster_amd import abi

import frontier_model as fm
import gain_model as gm
import reach_model as rm

VARIANTS = ("see_through",        # no voxel blocks: the gain is ball_gain
            "unknown_blocks",     # an unknown voxel on the line blocks too
            "floor",              # r(a, k) = sgn(a) floor(|a| k / m): no rounding
            "half_toward",        # a half rounds toward c
            "floor_signed",       # floor((2 a k + m) / (2 m)) on the signed a: a half rounds toward +
            "x_drives",           # m = |dx| whatever the other two are
            "occupied_unknown",   # an unknown voxel whose map cell is occupied is a wall
            "outside_free",       # a known voxel outside the map is no wall
            "parents",            # the line from u is walked parent by parent, each from its own offset, not by the closed formula
            "poor_on_ball",       # poor is judged on ball_gain
            "best_on_ball",       # best_gain is the largest ball_gain
            "walls_lattice")      # walls counts the whole lattice, not the box

INF = rm.INF
ALL = abi.FH_FRONTIER_WANT_ALL
WANTED, FOUND = abi.FH_FRONTIER_WANTED, abi.FH_FRONTIER_FOUND
DEAR = abi.FH_SIGHT_MAX_HOP_COST


def line_offsets(d, m, k, variant=None):
    """r(a, k) for the offsets d [N][3] with m [N] >= 1, by the closed formula."""
    a, s = np.abs(d), np.sign(d)
    mm = m[:, None]
    if variant == "floor":
        return s * ((a * k) // mm)
    if variant == "half_toward":
        return s * ((2 * a * k + mm - 1) // (2 * mm))
    if variant == "floor_signed":
        return (2 * d * k + mm) // (2 * mm)
    return s * ((2 * a * k + mm) // (2 * mm))


def _parents_visible(c, u, wall):
    cur = np.array(u, dtype=np.int64)
    c = np.array(c, dtype=np.int64)
    while True:
        d = cur - c
        m = int(np.abs(d).max())
        if m <= 1:
            return True
        cur = c + np.sign(d) * ((2 * np.abs(d) * (m - 1) + m) // (2 * m))
        if wall[cur[2], cur[1], cur[0]]:
            return False


def visible(c, us, wall, lo, hi, variant=None):
    """[N] bool: which of the voxels us [N][3] (x, y, z) are visible from c; wall [nz][ny][nx] bool over the lattice."""
    us = np.asarray(us, dtype=np.int64).reshape(-1, 3)
    if variant == "parents":
        return np.array([_parents_visible(c, u, wall) for u in us], dtype=bool)
    d = us - np.asarray(c, dtype=np.int64)[None, :]
    m = np.abs(d[:, 0]) if variant == "x_drives" else np.abs(d).max(axis=1)
    seen = np.ones(len(us), dtype=bool)
    lo, hi = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
    for k in range(1, int(m.max()) if len(m) else 0):
        on = k < m
        r = np.where(on[:, None], line_offsets(d, np.maximum(m, 1), k, variant), 0)   # (a line that has ended stays on c, which is no wall)
        p = np.asarray(c, dtype=np.int64)[None, :] + r
        if variant == "x_drives":   # (its voxels may leave the box: kept inside it)
            p = np.clip(p, lo[None, :], hi[None, :])
        seen &= ~(on & wall[p[:, 2], p[:, 1], p[:, 0]])
    return seen


def gains_of(c, lo, hi, unknown, wall, g, variant=None):
    """(gain, ball_gain) of the candidate c = (x, y, z)."""
    z, y, x = np.ogrid[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1]
    d = (x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2
    inside = (d <= g * g) & unknown[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1]
    zz, yy, xx = np.nonzero(inside)
    ball = len(xx)
    if ball == 0 or variant == "see_through":
        return ball, ball
    us = np.stack([xx + lo[0], yy + lo[1], zz + lo[2]], axis=1)
    return int(visible(c, us, wall, lo, hi, variant).sum()), ball


def sight_goals(par, grid, flags, view_stride, view_of, n_views, vehicles, occ, m_origin, m_res, variant=None, details=None):
    """-> (goals [n][3], mask [n] int32, records [n] abi.sight_record_dtype), the arguments of gain_model.gain_goals.  details: a dict that
    receives, per searched vehicle i, {cell: (hops, gain, ball_gain, utility)} of its reachable candidates."""
    origin, res, dims = grid
    nx, ny, nz = (int(d) for d in dims)
    n = len(vehicles)
    views = fm.views_of(flags, n_views, view_stride, dims)
    free, _ = rm.map_free(grid, occ, m_origin, m_res)
    in_map, _ = rm.map_free(grid, np.zeros_like(occ), m_origin, m_res)   # (the voxel's centre lies in a cell of the map)
    fronts = {}
    goals = np.zeros((n, 3), dtype=np.float64)
    mask = np.zeros(n, dtype=np.int32)
    rec = np.zeros(n, dtype=abi.sight_record_dtype)
    r_max, max_hops = float(par["r_max"]), int(par["max_hops"])
    g, hop_cost, min_gain = int(par["gain_radius"]), int(par["hop_cost"]), int(par["min_gain"])
    for i in range(n):
        v = int(i if view_of is None else view_of[i])
        p, gt = vehicles["state"]["pos"][i], vehicles["g_term"][i]
        flag = WANTED if fm.wanted(int(par["want"]), int(vehicles["status"][i]), int(vehicles["stage"][i])) else 0
        if not 0 <= v < n_views:
            flag |= abi.FH_FRONTIER_NO_VIEW
        if not (np.all(np.isfinite(p)) and np.all(np.isfinite(gt))):
            flag |= abi.FH_FRONTIER_BAD_POS
        goals[i] = gt   # (the bits: a copy)
        rec[i] = (flag, v, -1, -1, 0, 0, 0, 0, np.inf, -1, 0, 0, -1, -1, 0)
        if flag != WANTED:
            continue
        with np.errstate(all="ignore"):
            s = [np.floor((np.float64(p[k]) - np.float64(origin[k])) / np.float64(res)) for k in range(3)]
        if not all(0.0 <= s[k] < dims[k] for k in range(3)):
            rec["flags"][i] |= abi.FH_REACH_START_OUTSIDE
            continue
        start = tuple(int(x) for x in s)
        box = [rm.box_axis(p[k], r_max, origin[k], res, int(dims[k])) for k in range(3)]
        lo, hi = [b[0] for b in box], [b[1] for b in box]
        words = -(-(hi[0] - lo[0] + 1) // 64) * (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1)
        if words > abi.FH_REACH_MAX_WORDS:
            rec["flags"][i] |= abi.FH_REACH_BOX_TOO_LARGE
            continue
        if v not in fronts:
            fronts[v] = fm.frontier_mask(views[v])
        with np.errstate(over="ignore", invalid="ignore"):
            ok, d2, (qx, qy, qz) = fm.candidates_of(fronts[v], p, gt, par, grid, occ, m_origin, m_res)
        known = views[v] == 0
        passable = known & free
        hops = rm.flood(start, lo, hi, passable, max_hops)
        unknown = ~known
        wall = known & ~free
        if variant == "occupied_unknown":
            wall = ~free
        elif variant == "outside_free":
            wall = known & ~free & in_map
        elif variant == "unknown_blocks":
            wall = ~passable
        in_box = np.zeros_like(wall)
        in_box[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = True
        rec["walls"][i] = int((wall if variant == "walls_lattice" else wall & in_box).sum())
        rec["candidates"][i] = int(ok.sum())
        rec["reachable"][i] = int((ok & (hops >= 0)).sum())
        rec["reached"][i] = int((hops >= 0).sum())
        rec["levels"][i] = max(int(hops.max()), 0)
        if max_hops > 0 and int(hops.max()) == max_hops:
            rec["flags"][i] |= abi.FH_REACH_CUT
        cells = [int(c) for c in np.nonzero((ok & (hops >= 0)).ravel())[0]]
        if not cells:
            continue
        hh = {c: int(hops.ravel()[c]) for c in cells}
        rows, poor, most = [], 0, -1
        for c in cells:
            xyz = (c % nx, (c // nx) % ny, c // (nx * ny))
            gain, ball = gains_of(xyz, lo, hi, unknown, wall, g, variant)
            most = max(most, ball if variant == "best_on_ball" else gain)
            utility = gain - hop_cost * hh[c]
            if details is not None:
                details.setdefault(i, {})[c] = (hh[c], gain, ball, utility)
            if (ball if variant == "poor_on_ball" else gain) < min_gain:
                poor += 1
                continue
            dd = d2.ravel()[c]
            rows.append(((-utility, hh[c], dd, c), c, gain, ball, utility, dd))
        rec["poor"][i], rec["best_gain"][i] = poor, most
        if poor == len(cells):
            rec["flags"][i] |= abi.FH_SIGHT_ALL_POOR
        if not rows:
            continue
        _, c, gain, ball, utility, dd = sorted(rows, key=lambda r: r[0])[0]
        iz, iy, ix = c // (nx * ny), (c // nx) % ny, c % nx
        goals[i] = (qx[0, 0, ix], qy[0, iy, 0], qz[iz, 0, 0])
        mask[i] = 1
        rec["flags"][i] |= FOUND
        rec["cell"][i], rec["hops"][i], rec["d2"][i] = c, hh[c], dd
        rec["gain"][i], rec["utility"][i], rec["ball_gain"][i] = gain, utility, ball
    return goals, mask, rec


# ---- the named cases: the smallest shapes at which the kernel can still go wrong ------------------------------------------------------
def sight_params(r_max, g, hop_cost=1, min_gain=0, r_avoid=0.0, z_lo=-INF, z_hi=INF, want=ALL, max_hops=0):
    p = abi.default_sight_params(r_max, g)
    p["r_avoid"], p["z_lo"], p["z_hi"], p["want"], p["max_hops"], p["hop_cost"], p["min_gain"] = r_avoid, z_lo, z_hi, want, max_hops, hop_cost, min_gain
    return p


def sight_par_of(par):
    """The fh_sight_params with the fields of a fh_gain_params (the two have one layout)."""
    return sight_params(float(par["r_max"]), int(par["gain_radius"]), int(par["hop_cost"]), int(par["min_gain"]), float(par["r_avoid"]),
                        float(par["z_lo"]), float(par["z_hi"]), int(par["want"]), int(par["max_hops"]))


def gain_par_of(par):
    return gm.gain_params(float(par["r_max"]), int(par["gain_radius"]), int(par["hop_cost"]), int(par["min_gain"]), float(par["r_avoid"]),
                          float(par["z_lo"]), float(par["z_hi"]), int(par["want"]), int(par["max_hops"]))


def of_gain(case):
    """A case of gain_model with its params as a fh_sight_params."""
    out = dict(case)
    out["par"] = sight_par_of(case["par"])
    return out


def model(case, variant=None, par=None, details=None):
    return sight_goals(case["par"] if par is None else par, case["grid"], case["flags"], case["stride"], case["view_of"], case["n_views"],
                       case["vehicles"], case["occ"], case["m_origin"], case["m_res"], variant, details)


def gain_model_of(case):
    """The model of the gain chooser on the same tables."""
    return gm.model(case, par=gain_par_of(case["par"]))


def scene(dims, unknown, occupied, starts, g, r_max=100.0, **kw):
    """A lattice that is known and free but for the voxels (or (slice, slice, slice) blocks, in x, y, z) of `unknown` and `occupied`; one
    view, a vehicle at the centre of every voxel of `starts`.  make: the keywords of reach_model.make_case."""
    nx, ny, nz = dims
    view = np.zeros((nz, ny, nx), dtype=np.uint8)
    make = kw.pop("make", {})
    occ = np.zeros((nz, ny, nx) if "occ_dims" not in kw else kw.pop("occ_dims")[::-1], dtype=np.uint8)
    for x, y, z in unknown:
        view[z, y, x] = 1
    for x, y, z in occupied:
        occ[z, y, x] = 100
    return rm.make_case(dims, [view], [rm.centre(c) for c in starts], occ, sight_params(r_max, g, **kw), view_of=[0] * len(starts), **make)


ALLX = slice(None)

# hole before a wall: 15 x 9 x 3.  Unknown: the slab x <= 1, the plane x == 14 (the open edge) and the hole (4, 4, 1); the plane x == 2 is
# known and occupied.  The vehicle stands at (7, 4, 1).  HB_NEAR, between the wall and the hole, has the slab in its ball and sees none
# of it; HB_EDGE, six steps away like HB_NEAR, sees the open edge.
HB_DIMS, HB_HOLE, HB_START, HB_NEAR, HB_EDGE, HB_G = (15, 9, 3), (4, 4, 1), (7, 4, 1), (3, 4, 1), (13, 4, 1), 3


def hole_before_wall(**kw):
    return scene(HB_DIMS, [(slice(0, 2), ALLX, ALLX), (14, ALLX, ALLX), HB_HOLE], [(2, ALLX, ALLX)], [HB_START], kw.pop("g", HB_G), **kw)


# a plane: 9 x 7 x 3, the plane x == 4 known and occupied, x >= 5 unknown, a hole at (2, 3, 1) whose neighbour PL_NEAR touches the plane
PL_DIMS, PL_HOLE, PL_NEAR, PL_WINDOW = (9, 7, 3), (2, 3, 1), (3, 3, 1), (4, 3, 1)


def plane(window=False, pillar=False, **kw):
    """The vehicle stands on PL_NEAR and steps cost the most, so PL_NEAR is the choice unless it is poor.  closed: nothing behind the
    plane is seen, and the gain is the hole alone (a candidate always sees the unknown voxel it touches: m = 1).  window: the plane's
    voxel PL_WINDOW is free.  pillar: of the plane only the column (4, 3, *) stands."""
    occupied = [(4, 3, ALLX)] if pillar else [(4, ALLX, ALLX)]
    case = scene(PL_DIMS, [(slice(5, 9), ALLX, ALLX), PL_HOLE], occupied, [PL_NEAR], 3, hop_cost=DEAR, **kw)
    if window:
        case["occ"][PL_WINDOW[2], PL_WINDOW[1], PL_WINDOW[0]] = 0
    return case


PROBE_C = (8, 8, 8)


def probe(offsets, walls, extra=(), occupied_unknown=(), dims=(17, 17, 17), c=PROBE_C, g=8, **kw):
    """The vehicle stands on c, which is a candidate because c + (0, 0, -1) is unknown; steps cost the most, so c is the choice and
    the record's gain is its gain: 1 + the visible ones of the unknown voxels c + offsets (+ extra), the voxels c + walls being
    known and occupied.  occupied_unknown: offsets of unknown voxels whose map cell is occupied."""
    at = lambda d: (c[0] + d[0], c[1] + d[1], c[2] + d[2])   # noqa: E731
    unknown = [at((0, 0, -1))] + [at(d) for d in list(offsets) + list(extra) + list(occupied_unknown)]
    occupied = [at(d) for d in list(walls) + list(occupied_unknown)]
    return scene(dims, unknown, occupied, [c], g, hop_cost=DEAR, **kw)


def outside_map():
    """8 x 3 x 3, the map holds x <= 3 only: the vehicle at (2, 1, 1), (2, 1, 0) and (6, 1, 1) unknown.  The line to (6, 1, 1) crosses
    (4, 1, 1) and (5, 1, 1), known and outside the map: walls."""
    return scene((8, 3, 3), [(2, 1, 0), (6, 1, 1)], [], [(2, 1, 1)], 5, hop_cost=DEAR, occ_dims=(4, 3, 3))


def diagonal_leak():
    """A wall one voxel thick along x + y == 5 of layer 1 (and the same in the layers beside it): the line from (1, 1, 1) to (4, 4, 1)
    goes over (2, 2, 1) and (3, 3, 1) and slips through between (2, 3, 1) and (3, 2, 1)."""
    wall = [(x, 5 - x, z) for x in range(0, 6) for z in range(3)]
    return scene((6, 6, 3), [(1, 1, 0), (4, 4, 1)], wall, [(1, 1, 1)], 5, hop_cost=DEAR)


def word_lines():
    """132 x 5 x 3: vehicles at x = 62, 126 (lines to x + 4 with the wall at x + 2 = 64, 128, the first bit of the second word) and at
    x = 66, 130 (lines to x - 4 with the wall at 64, 128: the target lies in the first word), and one at x = 61 whose line to 65 is free."""
    unknown, occupied, starts = [], [], []
    for x, y, sgn in ((62, 1, 1), (126, 3, 1), (66, 3, -1), (130, 1, -1)):
        starts.append((x, y, 1))
        unknown += [(x, y, 0), (x + 4 * sgn, y, 1)]
        occupied.append((x + 2 * sgn, y, 1))
    starts.append((30, 2, 1))
    unknown += [(30, 2, 0), (34, 2, 1)]
    return scene((132, 5, 3), unknown, occupied, starts, 4, hop_cost=DEAR)


def row_ends():
    """70 x 3 x 3, gain_model.row_ends with walls where its unknown ends of rows are: (69, 1, 1) and (69, 2, 1) known and occupied, the
    starts of the rows that follow them in memory unknown, and (68, 0, 1), (68, 1, 0) unknown so that there are candidates.  The walls
    lie in balls and on no line to an unknown voxel: the lines are walked and every gain is ball_gain."""
    unknown = [(0, 2, 1), (1, 2, 1), (0, 0, 2), (1, 0, 2), (68, 0, 1), (68, 1, 0)]
    return scene((70, 3, 3), unknown, [(69, 1, 1), (69, 2, 1)], [(66, 1, 1), (66, 2, 1)], 2, max_hops=3)


def far_wall():
    """hole_before_wall without its plane and slab, and one wall voxel in a corner, in no candidate's ball."""
    return scene(HB_DIMS, [(14, ALLX, ALLX), HB_HOLE], [(0, 0, 0)], [HB_START], HB_G)


def _random_walled(dims, positions, r_max, g, seed, known_r, p_unknown=0.45, p_occ=0.2, res=0.5, **kw):
    """gain_model's random scene with occupied map cells at random: known ones are walls, unknown ones are not."""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    view = (rng.random((nz, ny, nx)) < p_unknown).astype(np.uint8)
    occ = ((rng.random((nz, ny, nx)) < p_occ) * 100).astype(np.uint8)
    z, y, x = np.ogrid[0:nz, 0:ny, 0:nx]
    for c in positions:
        near = (x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2 <= known_r * known_r
        view[near] = 0
        occ[near] = 0
    return rm.make_case(dims, [view], [rm.centre(c, res) for c in positions], occ, sight_params(r_max, g, **kw), res=res, view_of=[0] * len(positions))


def box_faces():
    """gain_model.box_faces with walls: balls and lines cut by every face of a box inside the lattice and by the lattice's corners."""
    positions = [(6, 6, 5), (0, 0, 0), (12, 11, 10), (0, 6, 5), (6, 11, 5), (6, 6, 0)]
    return _random_walled((13, 12, 11), positions, 1.6, 3, 23, 1.5)


def _radius(g):
    return _random_walled((63, 9, 3), [(31, 4, 1)], 100.0, g, 31, 1.0, p_unknown=0.3, p_occ=0.12, hop_cost=3)


CASES = {
    "hole_before_wall": hole_before_wall,
    "hole_before_wall_min_gain": lambda: hole_before_wall(min_gain=2),
    "closed_plane": plane,
    "closed_plane_all_poor": lambda: plane(min_gain=2),
    "window": lambda: plane(window=True),
    "pillar": lambda: plane(pillar=True),
    "round_plus": lambda: probe([(2, 1, 0)], [(1, 1, 0)]),
    "round_minus": lambda: probe([(2, -1, 0)], [(1, -1, 0)]),
    "round_3_of_6": lambda: probe([(6, 3, 0)], [(1, 1, 0)]),
    "round_negative_x": lambda: probe([(-1, 2, 0)], [(-1, 1, 0)]),
    "drive_y": lambda: probe([(1, 4, 0)], [(0, 1, 0)]),
    "drive_z": lambda: probe([(0, 1, 4)], [(0, 0, 1)]),
    "drive_z_oblique": lambda: probe([(4, 1, 6)], [(3, 1, 4)]),
    "transparent_unknown": lambda: probe([(4, 0, 0), (2, 0, 0), (0, 4, 0)], [], occupied_unknown=[(0, 2, 0)]),
    "outside_map": outside_map,
    "between_two_walls": lambda: probe([(1, 1, 0)], [(1, 0, 0), (0, 1, 0)]),
    "diagonal_leak": diagonal_leak,
    "parents_differ": lambda: probe([PARENTS_U], [PARENTS_WALL]),
    "word_lines": word_lines,
    "row_ends": row_ends,
    "far_wall": far_wall,
    "box_faces": box_faces,
    "radius_0": lambda: _radius(0),
    "radius_1": lambda: _radius(1),
    "radius_31": lambda: _radius(31),
}

# an offset whose closed line and whose chain of parents part: the closed line goes over PARENTS_WALL, the chain does not
PARENTS_U, PARENTS_WALL = (3, 1, 0), (1, 0, 0)   # closed: (1, 0, 0), (2, 1, 0); the parent of (3, 1, 0) is (2, 1, 0), whose parent is (1, 1, 0)

# the cases on which the variant that walks voxel by voxel in Python is tried (the others have thousands of pairs)
LARGE = ("radius_0", "radius_1", "radius_31", "gain:radius_0", "gain:radius_1", "gain:radius_31", "gain:box_at_cap")
_BUILT = {}


def case(name):
    """The named case; "gain:<case of gain_model>" (that case, its params as fh_sight_params); or "reduction:<case of reach_model>" (that
    case with g = 0, hop_cost = 1, min_gain = 0); built once.  Treat it as read-only."""
    if name not in _BUILT:
        if name.startswith("gain:"):
            _BUILT[name] = of_gain(gm.case(name.split(":", 1)[1]))
        elif name.startswith("reduction:"):
            _BUILT[name] = of_gain(gm.case(name))
        else:
            _BUILT[name] = CASES[name]()
    return _BUILT[name]


GAIN_CASES = ["gain:" + k for k in gm.CASES]
REDUCTIONS = list(gm.REDUCTIONS)
ALL_CASES = list(CASES) + GAIN_CASES + REDUCTIONS
_MODELS = {}


def expected(name):
    """The model's outputs of the named case, computed once.  Treat them as read-only."""
    if name not in _MODELS:
        _MODELS[name] = model(case(name))
    return _MODELS[name]


def wall_free(name):
    """Does no searched vehicle of the named case have a wall voxel in its box?"""
    return not expected(name)[2]["walls"].any()
