"""The model of include/fasterhip_gain.h (fh_gain_goals_device) restated in Python, brute force: the queue flood, the box, the passable
voxels and the candidates are those of tests/reach_model.py by import; the gain of a candidate is a count over every voxel of the box,
one squared distance each — no rows, no masks and no words, so it shares no structure with the kernel; the choice is a sort.  Not a
test file.

`variant` names a deliberately WRONG model (VARIANTS, also wrong_variants()): tests/test_gain_model.py shows that the named cases
(CASES) tell every one of them from the model, so a kernel that made one of these mistakes would not pass tests/test_gpu_gain.py."""
import numpy as np

from faster_amd import abi

import frontier_model as fm
import reach_model as rm

VARIANTS = ("cube",          # max(|dx|, |dy|, |dz|) <= g instead of the ball
            "lt",            # squared distance < g^2
            "x_wrap",        # the rows of the ball are not clipped to the box in x: they run on into the next row of the box's memory
            "first_word",    # of the (at most) two words of 64 box columns that a row of the ball touches only the first is counted
            "no_hops",       # utility = gain
            "poor_le",       # poor: gain <= min_gain
            "d2_first",      # equal utility: the smallest (d2, hops, c)
            "cell_largest",  # equal utility, hops and d2: the largest cell
            "map_known",     # a voxel whose map cell is occupied counts as known
            "first_level")   # only the candidates of the first level that holds one are looked at


def wrong_variants():
    return VARIANTS


INF, NAN = rm.INF, rm.NAN
ALL = abi.FH_FRONTIER_WANT_ALL
WANTED, FOUND = abi.FH_FRONTIER_WANTED, abi.FH_FRONTIER_FOUND


def isqrt_floor(v):
    h = 0
    while (h + 1) * (h + 1) <= v:
        h += 1
    return h


def gain_of(c, lo, hi, unknown, g, variant=None):
    """The unknown voxels of the box [lo, hi] within g voxels of c = (x, y, z): a plain triple loop over the box."""
    cx, cy, cz = c
    g2 = g * g
    bx, by, bz = hi[0] - lo[0] + 1, hi[1] - lo[1] + 1, hi[2] - lo[2] + 1
    total = 0
    if variant == "x_wrap":   # row by row of the ball, the x range not clipped: box memory order runs on into the next row
        flat = unknown[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1].ravel()
        for z in range(max(cz - g, lo[2]), min(cz + g, hi[2]) + 1):
            for y in range(max(cy - g, lo[1]), min(cy + g, hi[1]) + 1):
                rem = g2 - (y - cy) ** 2 - (z - cz) ** 2
                if rem < 0:
                    continue
                hx = isqrt_floor(rem)
                for x in range(cx - hx, cx + hx + 1):
                    f = ((z - lo[2]) * by + (y - lo[1])) * bx + (x - lo[0])
                    if 0 <= f < len(flat) and flat[f]:
                        total += 1
        return total
    for z in range(lo[2], hi[2] + 1):
        for y in range(lo[1], hi[1] + 1):
            first = None   # the word of the first voxel of this row that lies in the ball (variant first_word)
            for x in range(lo[0], hi[0] + 1):
                dx, dy, dz = x - cx, y - cy, z - cz
                d = dx * dx + dy * dy + dz * dz
                if variant == "cube":
                    inside = max(abs(dx), abs(dy), abs(dz)) <= g
                elif variant == "lt":
                    inside = d < g2
                else:
                    inside = d <= g2
                if not inside:
                    continue
                if first is None:
                    first = (x - lo[0]) // 64
                if variant == "first_word" and (x - lo[0]) // 64 != first:
                    continue
                if unknown[z, y, x]:
                    total += 1
    return total


def _fast_gain(c, lo, hi, unknown, g):
    """gain_of without a variant, with numpy over the box (the same count; tests/test_gain_model.py compares the two)."""
    z, y, x = np.ogrid[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1]
    d = (x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2
    return int(((d <= g * g) & unknown[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1]).sum())


def gain_goals(par, grid, flags, view_stride, view_of, n_views, vehicles, occ, m_origin, m_res, variant=None, details=None):
    """-> (goals [n][3], mask [n] int32, records [n] abi.gain_record_dtype), the arguments of reach_model.reach_goals with an
    abi.gain_params_dtype record.  details: a dict that receives, per searched vehicle i, {cell: (hops, gain, utility, d2)} of its
    reachable candidates."""
    origin, res, dims = grid
    nx, ny, nz = (int(d) for d in dims)
    n = len(vehicles)
    views = fm.views_of(flags, n_views, view_stride, dims)
    free, _ = rm.map_free(grid, occ, m_origin, m_res)
    fronts = {}
    goals = np.zeros((n, 3), dtype=np.float64)
    mask = np.zeros(n, dtype=np.int32)
    rec = np.zeros(n, dtype=abi.gain_record_dtype)
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
        rec[i] = (flag, v, -1, -1, 0, 0, 0, 0, np.inf, -1, 0, 0, -1, 0.0)
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
        passable = (views[v] == 0) & free
        hops = rm.flood(start, lo, hi, passable, max_hops)
        unknown = views[v] != 0
        if variant == "map_known":
            unknown = unknown & free
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
        looked = cells
        if variant == "first_level":
            looked = [c for c in cells if hh[c] == min(hh.values())]
        rows, poor, most = [], 0, -1
        for c in looked:
            xyz = (c % nx, (c // nx) % ny, c // (nx * ny))
            gain = _fast_gain(xyz, lo, hi, unknown, g) if variant is None or variant in ("no_hops", "poor_le", "d2_first", "cell_largest",
                                                                                         "map_known", "first_level") \
                else gain_of(xyz, lo, hi, unknown, g, variant)
            most = max(most, gain)
            utility = gain if variant == "no_hops" else gain - hop_cost * hh[c]
            if details is not None:
                details.setdefault(i, {})[c] = (hh[c], gain, utility, float(d2.ravel()[c]))
            if gain <= min_gain if variant == "poor_le" else gain < min_gain:
                poor += 1
                continue
            dd = d2.ravel()[c]
            if variant == "d2_first":
                key = (-utility, dd, hh[c], c)
            elif variant == "cell_largest":
                key = (-utility, hh[c], dd, -c)
            else:
                key = (-utility, hh[c], dd, c)
            rows.append((key, c, gain, utility, dd))
        rec["poor"][i], rec["best_gain"][i] = poor, most
        if poor == len(cells):
            rec["flags"][i] |= abi.FH_GAIN_ALL_POOR
        if not rows:
            continue
        _, c, gain, utility, dd = sorted(rows, key=lambda r: r[0])[0]
        iz, iy, ix = c // (nx * ny), (c // nx) % ny, c % nx
        goals[i] = (qx[0, 0, ix], qy[0, iy, 0], qz[iz, 0, 0])
        mask[i] = 1
        rec["flags"][i] |= FOUND
        rec["cell"][i], rec["hops"][i], rec["d2"][i] = c, hh[c], dd
        rec["gain"][i], rec["utility"][i] = gain, utility
    return goals, mask, rec


# ---- the named cases: the smallest shapes at which the kernel can still go wrong ------------------------------------------------------
def gain_params(r_max, g, hop_cost=1, min_gain=0, r_avoid=0.0, z_lo=-INF, z_hi=INF, want=ALL, max_hops=0):
    p = abi.default_gain_params(r_max, g)
    p["r_avoid"], p["z_lo"], p["z_hi"], p["want"], p["max_hops"], p["hop_cost"], p["min_gain"] = r_avoid, z_lo, z_hi, want, max_hops, hop_cost, min_gain
    return p


def with_gain(case, g, hop_cost=1, min_gain=0, max_hops=None):
    """A case of reach_model (or of this module) with the gain parameters set, the other fields of its params kept."""
    out = dict(case)
    old = case["par"]
    out["par"] = gain_params(float(old["r_max"]), g, hop_cost, min_gain, float(old["r_avoid"]), float(old["z_lo"]), float(old["z_hi"]),
                             int(old["want"]), int(old["max_hops"]) if max_hops is None else max_hops)
    return out


def packed(case):
    """The case with view_stride == cells: no byte between one view and the next."""
    out = dict(case)
    out["flags"] = np.concatenate([case["flags"][v * case["stride"]: v * case["stride"] + case["cells"]] for v in range(case["n_views"])])
    out["stride"] = case["cells"]
    return out


def reach_par_of(par):
    """The fh_reach_params that a fh_gain_params begins with."""
    return rm.reach_params(float(par["r_max"]), float(par["r_avoid"]), float(par["z_lo"]), float(par["z_hi"]), int(par["want"]), int(par["max_hops"]))


def model(case, variant=None, par=None, details=None):
    return gain_goals(case["par"] if par is None else par, case["grid"], case["flags"], case["stride"], case["view_of"], case["n_views"],
                      case["vehicles"], case["occ"], case["m_origin"], case["m_res"], variant, details)


def reach_model_of(case):
    """The model of fasterhip_reach.h on the same tables (its params: the first six fields)."""
    return rm.model(case, par=reach_par_of(case["par"]))


HOLE_DIMS, HOLE, HOLE_START = (16, 5, 3), (0, 2, 1), (3, 2, 1)
HOLE_NEAR, WALL_NEAR, WALL_X = (1, 2, 1), (11, 2, 1), 12   # the candidate beside the hole (2 steps), the middle one at the wall (8 steps)


def hole_and_wall(start=HOLE_START, occupied_wall=False, **kw):
    """16 x 5 x 3, all free.  One unknown voxel, HOLE, whose neighbour HOLE_NEAR is two steps from the vehicle; the slab x >= 12 is
    unknown, and its middle neighbour WALL_NEAR is eight steps away.  occupied_wall: the map cells of the slab are occupied."""
    nx, ny, nz = HOLE_DIMS
    view = np.zeros((nz, ny, nx), dtype=np.uint8)
    view[HOLE[2], HOLE[1], HOLE[0]] = 1
    view[:, :, WALL_X:] = 1
    occ = np.zeros((nz, ny, nx), dtype=np.uint8)
    if occupied_wall:
        occ[:, :, WALL_X:] = 100
    par = gain_params(100.0, kw.pop("g", 2), **kw)
    return rm.make_case(HOLE_DIMS, [view], [rm.centre(start)], occ, par)


WORD_XS = (0, 63, 64, 127, 128)


def word_edges():
    """132 x 3 x 3: the row (y 1, z 1) is a known corridor, free in the map; every other voxel is occupied in the map and unknown at
    random, those beside the corridor at x = 0, 63, 64, 127, 128 (y 0) and 62, 65, 126, 129 (y 2) for certain.  Five vehicles in
    the corridor at bit 0, 63 | 64 and 127 | 128, two levels of flood each: the rows of their candidates' balls lie across both
    word boundaries."""
    dims = (132, 3, 3)
    rng = np.random.default_rng(17)
    view = (rng.random((3, 3, 132)) < 0.5).astype(np.uint8)
    view[1, 1, :] = 0
    for x in WORD_XS:
        view[1, 0, x] = 1
    for x in (62, 65, 126, 129):
        view[1, 2, x] = 1
    occ = np.full((3, 3, 132), 100, dtype=np.uint8)
    occ[1, 1, :] = 0
    return rm.make_case(dims, [view], [rm.centre((x, 1, 1)) for x in WORD_XS], occ, gain_params(100.0, 3, max_hops=2), view_of=[0] * 5)


def row_ends():
    """70 x 3 x 3, all known and free but: (69, 1, 1), the end of a row, which makes (68, 1, 1) a candidate, with (0, 2, 1) and
    (1, 2, 1), the start of the next row in y, unknown too; and (69, 2, 1), the end of the last row of a slab, with (0, 0, 2) and
    (1, 0, 2), the start of the next slab.  Those starts are 68 voxels from the candidates at the ends."""
    dims = (70, 3, 3)
    view = np.zeros((3, 3, 70), dtype=np.uint8)
    for x, y, z in ((69, 1, 1), (0, 2, 1), (1, 2, 1), (69, 2, 1), (0, 0, 2), (1, 0, 2)):
        view[z, y, x] = 1
    occ = np.zeros((3, 3, 70), dtype=np.uint8)
    return rm.make_case(dims, [view], [rm.centre((66, 1, 1)), rm.centre((66, 2, 1))], occ, gain_params(100.0, 2, max_hops=3), view_of=[0, 0])


def _random_scene(dims, positions, r_max, g, seed, known_r, p_unknown=0.45, res=0.5, **kw):
    """Unknown at random, a known ball of known_r voxels around each vehicle (given as cells); no obstacle."""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    view = (rng.random((nz, ny, nx)) < p_unknown).astype(np.uint8)
    z, y, x = np.ogrid[0:nz, 0:ny, 0:nx]
    for c in positions:
        view[(x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2 <= known_r * known_r] = 0
    occ = np.zeros((nz, ny, nx), dtype=np.uint8)
    return rm.make_case(dims, [view], [rm.centre(c, res) for c in positions], occ, gain_params(r_max, g, **kw), res=res, view_of=[0] * len(positions))


def box_faces():
    """13 x 12 x 11, res 0.5, r_max 1.6 (a box of 9 voxels a side at most): a vehicle in the middle, whose box lies inside the lattice —
    unknown voxels beyond its faces are not counted — one at each of two opposite corners of the lattice and one at each of three
    faces: balls of radius 3 cut by every face of a box and by its corners."""
    positions = [(6, 6, 5), (0, 0, 0), (12, 11, 10), (0, 6, 5), (6, 11, 5), (6, 6, 0)]
    return _random_scene((13, 12, 11), positions, 1.6, 3, 23, 1.5)


def one_voxel():
    return with_gain(rm.one_voxel(), 3)


def one_layer():
    """9 x 9 x 1: the ball is a disc."""
    return _random_scene((9, 9, 1), [(4, 4, 0)], 100.0, 3, 29, 1.5)


def _radius(g):
    """63 x 9 x 3, the vehicle in the middle: with g = 31 the row of the ball through a candidate in the middle column is 63 wide."""
    return _random_scene((63, 9, 3), [(31, 4, 1)], 100.0, g, 31, 1.0, hop_cost=3)


EXACT_C, EXACT_G = (4, 4, 4), 3
EXACT_IN = [(3, 0, 0), (-3, 0, 0), (0, 3, 0), (0, 0, -3), (2, 2, 1), (-2, 1, 2), (1, -2, -2), (0, 0, 1)]   # squared distance 9, 9, ..., and 1
EXACT_OUT = [(3, 1, 0), (-3, 0, 1), (0, 3, -1), (1, 0, 3), (2, 2, 2), (-1, -3, 0)]                           # 10, 10, 10, 10, 12, 10


def exact_radius():
    """9 x 9 x 9, known and free but the voxels EXACT_IN and EXACT_OUT around EXACT_C, where the vehicle stands: with g = 3 the first
    lie at squared distance 9 exactly (and one at 1, which makes EXACT_C a candidate), the others at 10 or more."""
    view = np.zeros((9, 9, 9), dtype=np.uint8)
    for d in EXACT_IN + EXACT_OUT:
        view[EXACT_C[2] + d[2], EXACT_C[1] + d[1], EXACT_C[0] + d[0]] = 1
    return rm.make_case((9, 9, 9), [view], [rm.centre(EXACT_C)], np.zeros((9, 9, 9), dtype=np.uint8), gain_params(100.0, EXACT_G, hop_cost=1000))


def _floor(free, marked, positions, **kw):
    """reach_model.floor_case: the candidates are the free voxels of layer 0 below a marked voxel of layer 1.  With g = 2 the gain of a
    candidate is the number of marked voxels in the 3 x 3 above it."""
    return with_gain(rm.floor_case(free, marked, positions, rm.reach_params(10.0)), kw.pop("g", 2), **kw)


def ties_hops():
    """reach_model.ties_hops with gains: (6, 1), three steps, gain 1; (3, 3), behind the wall, six steps, gain 4; (2, 3) and (4, 3), five steps,
    gain 3: utility -2 each.  The fewest hops win, though (3, 3) is the nearest."""
    free = np.ones((5, 8), dtype=bool)
    free[2, 2:5] = False
    return _floor(free, [(6, 1), (3, 3), (2, 3), (4, 3), (3, 4)], [(3, 1)])


def ties_d2():
    """(5, 1) and (4, 2): two steps and gain 2 each.  The nearer one wins; its cell is the larger."""
    return _floor(np.ones((4, 7), dtype=bool), [(5, 1), (4, 2)], [(3, 1)])


def ties_cell():
    """(1, 1) and (5, 1): two steps, gain 1 and d2 1.0 each.  The lower cell wins."""
    return _floor(np.ones((3, 7), dtype=bool), [(1, 1), (5, 1)], [(3, 1)])


def many_levels():
    """26 x 8 x 2, a free floor under marks at random, the vehicle in a corner: candidates in more than twenty levels, spread over the
    rows, so every wavefront holds a best of its own when the four are merged."""
    rng = np.random.default_rng(37)
    marked = [(x, y) for y in range(8) for x in range(26) if rng.random() < 0.6 or (x + y) % 3 == 0]
    return _floor(np.ones((8, 26), dtype=bool), marked, [(0, 0)], hop_cost=0)


CASES = {
    "hole_and_wall": hole_and_wall,
    "hole_and_wall_dear_hops": lambda: hole_and_wall(hop_cost=abi.FH_GAIN_MAX_HOP_COST),
    "hole_and_wall_min_gain": lambda: hole_and_wall(min_gain=2),
    "hole_and_wall_min_gain_met": lambda: hole_and_wall(min_gain=1, hop_cost=abi.FH_GAIN_MAX_HOP_COST),
    "hole_and_wall_free_hops": lambda: hole_and_wall(hop_cost=0),
    "hole_and_wall_occupied": lambda: hole_and_wall(occupied_wall=True),
    "all_poor": lambda: hole_and_wall(min_gain=100),
    "none_reachable": lambda: with_gain(rm.row_ends(), 2),
    "max_hops_before": lambda: hole_and_wall(max_hops=7),
    "max_hops_at": lambda: hole_and_wall(max_hops=8),
    "max_hops_after": lambda: hole_and_wall(max_hops=9),
    "start_is_candidate": lambda: hole_and_wall(start=HOLE_NEAR, hop_cost=abi.FH_GAIN_MAX_HOP_COST),
    "start_blocked": lambda: with_gain(rm.start_blocked(), 2),
    "word_edges": word_edges,
    "row_ends": row_ends,
    "box_faces": box_faces,
    "one_voxel": one_voxel,
    "one_layer": one_layer,
    "radius_0": lambda: _radius(0),
    "radius_1": lambda: _radius(1),
    "radius_31": lambda: _radius(31),
    "exact_radius": exact_radius,
    "ties_hops": ties_hops,
    "ties_d2": ties_d2,
    "ties_cell": ties_cell,
    "serpentine_dear_hops": lambda: with_gain(rm.serpentine(), 2, hop_cost=abi.FH_GAIN_MAX_HOP_COST),
    "many_levels": many_levels,
    "shared_view": lambda: with_gain(rm.shared_view(), 2),
    "start_outside": lambda: with_gain(rm.start_outside(), 2),
    "box_too_large": lambda: with_gain(rm.box_too_large(), 2),
    "box_at_cap": lambda: with_gain(rm.box_at_cap(), 2),
    "other_lattice": lambda: with_gain(rm.other_lattice(), 2),
}

# the cases on which the variants that count voxel by voxel in Python are tried (the others have thousands of candidates or voxels)
LARGE = ("radius_0", "radius_1", "radius_31", "box_at_cap")
_BUILT = {}


def case(name):
    """The named case, or "reduction:<case of reach_model>" (that case with g = 0, hop_cost = 1, min_gain = 0), built once.  Treat it as
    read-only."""
    if name not in _BUILT:
        _BUILT[name] = with_gain(rm.case(name.split(":", 1)[1]), 0) if name.startswith("reduction:") else CASES[name]()
    return _BUILT[name]


REDUCTIONS = ["reduction:" + k for k in rm.ALL_CASES]
ALL_CASES = list(CASES) + REDUCTIONS
_MODELS = {}


def expected(name):
    """The model's outputs of the named case, computed once.  Treat them as read-only."""
    if name not in _MODELS:
        _MODELS[name] = model(case(name))
    return _MODELS[name]
