"""The model of include/fasterhip_team.h (fh_team_goals_device) restated in plain Python over the vehicles in index order: the classes,
the lists and the passes of tests/spread_model.py, the gain, the utility and the choice of tests/gain_model.py, the flood of
tests/reach_model.py and the candidates of tests/frontier_model.py, all by import.  What this header adds is written out here: the
widened interaction radius, the voxel of a claim, the covered voxels (a brute-force squared distance per voxel of the box and claim,
no rows, no masks, no words) and the choice over the candidates that are not claimed.  Not a test file.

`variant` names a deliberately WRONG model (VARIANTS): tests/test_team_model.py shows that the named cases (CASES) tell every one of
them from the model, so kernels that made one of these mistakes would not pass tests/test_gpu_team.py."""
import numpy as np

from faster_amd import abi

import frontier_model as fm
import gain_model as gm
import reach_model as rm
import spread_model as sm

VARIANTS = ("no_discount",        # the covered voxels are counted in the gains all the same
            "lt_claim",           # covered: squared distance < claim_radius^2
            "cube_claim",         # covered: a cube in place of the ball
            "round_voxel",        # the claim voxel by rounding to the nearest voxel, not by floor
            "covered_per_claim",  # `covered` summed claim by claim: the overlap of two balls counted twice
            "r_int_plain",        # the interaction radius not widened: K16's reach and near
            "higher_peers",       # the lists, and so the discounts, taken from the higher peers too
            "claimed_in_best",    # claimed candidates kept in best_gain and poor
            "x_unclipped",        # the rows of a claim's ball not clipped in x: they run on into the next row of the box's memory
            "poor_before")        # poor judged by the gain before the discount

INF = float("inf")
REACHED_WANT = abi.FH_FRONTIER_WANT_REACHED
SEARCHER, STANDING, NONE = sm.SEARCHER, sm.STANDING, sm.NONE
R, T = sm.R, sm.T


def r_int_of(par, res, variant=None):
    """The interaction radius, a double computed once."""
    r_spread, g, cr = np.float64(par["r_spread"]), int(par["gain_radius"]), int(par["claim_radius"])
    if cr < 0 or variant == "r_int_plain":
        return r_spread
    return max(r_spread, np.float64(g + cr + 1) * np.float64(res))


def claim_voxel(c, origin, res, variant=None):
    """floor((c - origin) / res) per axis: Python ints of any size."""
    out = []
    for k in range(3):
        q = (np.float64(c[k]) - np.float64(origin[k])) / np.float64(res)
        out.append(int(np.floor(q + 0.5 if variant == "round_voxel" else q)))
    return tuple(out)


def covered_of(voxels, lo, hi, unknown, cr, variant=None):
    """-> (cov [nz][ny][nx] bool: the unknown voxels of the box inside the ball of some claim voxel, count): one squared distance per
    voxel of the box and claim."""
    cov = np.zeros(unknown.shape, dtype=bool)
    count = 0
    if cr < 0:
        return cov, 0
    z, y, x = np.ogrid[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1]
    box = (slice(lo[2], hi[2] + 1), slice(lo[1], hi[1] + 1), slice(lo[0], hi[0] + 1))
    bx, by, bz = hi[0] - lo[0] + 1, hi[1] - lo[1] + 1, hi[2] - lo[2] + 1
    for kx, ky, kz in voxels:
        if any(k < lo[a] - cr or k > hi[a] + cr for a, k in enumerate((kx, ky, kz))):   # (too far for any voxel of the box: exact, and keeps the ints small)
            continue
        one = np.zeros(unknown.shape, dtype=bool)
        if variant == "x_unclipped":
            flat = np.zeros(bx * by * bz, dtype=bool)
            for vz in range(max(kz - cr, lo[2]), min(kz + cr, hi[2]) + 1):
                for vy in range(max(ky - cr, lo[1]), min(ky + cr, hi[1]) + 1):
                    rem = cr * cr - (vy - ky) ** 2 - (vz - kz) ** 2
                    if rem < 0:
                        continue
                    hx = gm.isqrt_floor(rem)
                    for vx in range(kx - hx, kx + hx + 1):
                        f = ((vz - lo[2]) * by + (vy - lo[1])) * bx + (vx - lo[0])
                        if 0 <= f < len(flat):
                            flat[f] = True
            one[box] = flat.reshape(bz, by, bx)
        else:
            dx, dy, dz = x - kx, y - ky, z - kz
            d = dx * dx + dy * dy + dz * dz
            if variant == "cube_claim":
                inside = np.maximum(np.maximum(np.abs(dx), np.abs(dy)), np.abs(dz)) <= cr
            elif variant == "lt_claim":
                inside = d < cr * cr
            else:
                inside = d <= cr * cr
            one[box] = inside
        one &= unknown
        count += int(one.sum())
        cov |= one
    return cov, (count if variant == "covered_per_claim" else int(cov.sum()))


def team_goals(par, grid, flags, view_stride, view_of, n_views, group, vehicles, occ, m_origin, m_res, variant=None, details=None):
    """-> (goals [n][3], mask [n] int32, records [n] abi.team_record_dtype): the arguments of spread_model.spread_goals with an
    abi.team_params_dtype record.  details: a dict that receives, per searched vehicle i, {"claims", "voxels", "cov", "unknown", "lo",
    "hi", "cands": {cell: (hops, gain, utility, d2)} of its candidates in some level that are not claimed, "claimed": cells}."""
    origin, res, dims = grid
    nx, ny, nz = (int(d) for d in dims)
    n = len(vehicles)
    r_max, r_spread, passes, max_hops = np.float64(par["r_max"]), np.float64(par["r_spread"]), int(par["passes"]), int(par["max_hops"])
    g, hop_cost, min_gain, cr = int(par["gain_radius"]), int(par["hop_cost"]), int(par["min_gain"]), int(par["claim_radius"])
    s2_max = r_spread * r_spread
    r_int = r_int_of(par, res, variant)
    reach, near = (r_max + r_max) + r_int, r_max + r_int
    reach2, near2 = reach * reach, near * near
    # what fasterhip_reach.h says about every vehicle alone: the outputs of those that are not searched, and who is searched
    _, _, base = rm.reach_goals(sm.reach_par_of(par), grid, flags, view_stride, view_of, n_views, vehicles, occ, m_origin, m_res)
    goals = vehicles["g_term"].copy()
    mask = np.zeros(n, dtype=np.int32)
    rec = np.zeros(n, dtype=abi.team_record_dtype)
    pos, g_term = vehicles["state"]["pos"], vehicles["g_term"]
    view = [int(i if view_of is None else view_of[i]) for i in range(n)]
    has_view = [0 <= view[i] < n_views for i in range(n)]
    grp = [(int(view[i] if group is None else group[view[i]]) if has_view[i] else 0) for i in range(n)]
    cls = []
    for i in range(n):
        f = int(base["flags"][i])
        wanted = bool(f & abi.FH_FRONTIER_WANTED)
        if (f & ~(abi.FH_FRONTIER_FOUND | abi.FH_REACH_CUT)) == abi.FH_FRONTIER_WANTED:
            cls.append(SEARCHER)
        elif not wanted and has_view[i] and int(vehicles["status"][i]) != sm.GOAL_REACHED and np.all(np.isfinite(g_term[i])):
            cls.append(STANDING)
        else:
            cls.append(NONE)

    def peers(i, k):
        return has_view[i] and has_view[k] and i != k and grp[i] == grp[k]

    lower, standing = {}, {}
    for i in range(n):
        for k in ("flags", "view"):
            rec[k][i] = base[k][i]
        rec["flags"][i] &= ~(abi.FH_FRONTIER_FOUND | abi.FH_REACH_CUT)
        rec["cell"][i], rec["hops"][i], rec["d2"][i], rec["group"][i] = -1, -1, np.inf, grp[i]
        rec["gain"][i], rec["best_gain"][i] = -1, -1
        if cls[i] != SEARCHER:
            continue
        ks = range(n) if variant == "higher_peers" else range(i)
        lower[i] = [k for k in ks if peers(i, k) and cls[k] == SEARCHER and sm.d2_of(pos[k], pos[i]) < reach2]
        standing[i] = [k for k in range(n) if peers(i, k) and cls[k] == STANDING and sm.d2_of(g_term[k], pos[i]) < near2]
        rec["lower"][i], rec["claims"][i] = len(lower[i]), len(standing[i])
        if len(lower[i]) + len(standing[i]) > abi.FH_TEAM_LIST:
            rec["flags"][i] |= abi.FH_TEAM_OVERFLOW
        else:
            rec["decided_pass"][i] = -1

    views = fm.views_of(flags, n_views, view_stride, dims)
    free, _ = rm.map_free(grid, occ, m_origin, m_res)
    fronts = {}

    def search(i, claims):
        """K17's search of vehicle i with the claimed candidates left out and the covered voxels not counted; writes the outputs of i."""
        v, p, gt = view[i], pos[i], g_term[i]
        start = tuple(int(np.floor((np.float64(p[k]) - np.float64(origin[k])) / np.float64(res))) for k in range(3))
        box = [rm.box_axis(p[k], r_max, origin[k], res, int(dims[k])) for k in range(3)]
        lo, hi = [b[0] for b in box], [b[1] for b in box]
        if v not in fronts:
            fronts[v] = fm.frontier_mask(views[v])
        with np.errstate(over="ignore", invalid="ignore"):
            ok, d2, (qx, qy, qz) = fm.candidates_of(fronts[v], p, gt, par, grid, occ, m_origin, m_res)
            taken = np.zeros(ok.shape, dtype=bool)
            for c in claims:
                sx, sy, sz = np.float64(c[0]) - qx, np.float64(c[1]) - qy, np.float64(c[2]) - qz
                s2 = (sx * sx + sy * sy) + sz * sz
                taken |= s2 < s2_max
        taken &= ok
        hops = rm.flood(start, lo, hi, (views[v] == 0) & free, max_hops)
        unknown = views[v] != 0
        voxels = [claim_voxel(c, origin, res, variant) for c in claims]
        cov, covered = covered_of(voxels, lo, hi, unknown, cr, variant)
        counted = unknown if variant == "no_discount" else unknown & ~cov
        open_ = ok & ~taken & (hops >= 0)
        looked = ok & (hops >= 0) if variant == "claimed_in_best" else open_
        rec["candidates"][i], rec["claimed"][i] = int(ok.sum()), int(taken.sum())
        rec["reachable"][i], rec["reached"][i], rec["levels"][i] = int(open_.sum()), int((hops >= 0).sum()), max(int(hops.max()), 0)
        rec["flags"][i] = abi.FH_FRONTIER_WANTED
        if max_hops > 0 and int(hops.max()) == max_hops:
            rec["flags"][i] |= abi.FH_REACH_CUT
        rec["claims"][i], rec["covered"][i] = len(claims), covered
        rows, poor, most = [], 0, -1
        info = {"claims": [tuple(float(x) for x in c) for c in claims], "voxels": voxels, "cov": cov, "unknown": unknown, "lo": lo, "hi": hi,
                "cands": {}, "claimed": [int(c) for c in np.nonzero(taken.ravel())[0]]}
        for c in (int(c) for c in np.nonzero(looked.ravel())[0]):
            xyz = (c % nx, (c // nx) % ny, c // (nx * ny))
            gain = gm._fast_gain(xyz, lo, hi, counted, g)
            hh, dd = int(hops.ravel()[c]), d2.ravel()[c]
            utility = gain - hop_cost * hh
            most = max(most, gain)
            judged = gm._fast_gain(xyz, lo, hi, unknown, g) if variant == "poor_before" else gain
            if judged < min_gain:
                poor += 1
                continue
            if open_.ravel()[c]:
                info["cands"][c] = (hh, gain, utility, float(dd))
                rows.append(((-utility, hh, dd, c), c, gain, utility, dd, hh))
        if details is not None:
            details[i] = info
        rec["poor"][i], rec["best_gain"][i] = poor, most
        if rec["reachable"][i] > 0 and poor == rec["reachable"][i]:
            rec["flags"][i] |= abi.FH_TEAM_ALL_POOR
        if not rows:
            if rec["claimed"][i] > 0:
                rec["flags"][i] |= abi.FH_TEAM_CLAIMED
            return
        _, c, gain, utility, dd, hh = sorted(rows, key=lambda r: r[0])[0]
        iz, iy, ix = c // (nx * ny), (c // nx) % ny, c % nx
        goals[i] = (qx[0, 0, ix], qy[0, iy, 0], qz[iz, 0, 0])
        mask[i] = 1
        rec["flags"][i] |= abi.FH_FRONTIER_FOUND
        rec["cell"][i], rec["hops"][i], rec["d2"][i] = c, hh, dd
        rec["gain"][i], rec["utility"][i] = gain, utility

    for p in range(1, passes + 1):
        before = rec["decided_pass"].copy()   # nothing a pass decides is seen by that same pass
        for i in range(n):
            if before[i] != -1:
                continue
            if not all(0 <= before[k] < p for k in lower[i] if variant != "higher_peers" or k < i):   # (a higher peer is not waited for)
                continue
            claims = [g_term[k] for k in standing[i]] + [goals[k].copy() for k in lower[i] if mask[k] == 1]
            search(i, claims)
            rec["decided_pass"][i] = p
    for i in range(n):
        if rec["decided_pass"][i] == -1:
            rec["flags"][i] |= abi.FH_TEAM_UNSETTLED
    return goals, mask, rec


# ---- parameters and the two reductions ----------------------------------------------------------------------------------------------------
def team_params(r_max, r_spread, g, cr=None, hop_cost=1, min_gain=0, passes=abi.FH_TEAM_DEFAULT_PASSES, r_avoid=0.0, z_lo=-INF, z_hi=INF,
                want=REACHED_WANT, max_hops=0):
    p = abi.default_team_params(r_max, r_spread, g, cr)
    p["r_avoid"], p["z_lo"], p["z_hi"], p["want"], p["max_hops"], p["passes"], p["hop_cost"], p["min_gain"] = r_avoid, z_lo, z_hi, want, max_hops, passes, hop_cost, min_gain
    return p


def with_par(case, **kw):
    """The case with fields of its team params replaced."""
    out = dict(case)
    out["par"] = case["par"].copy()
    for k, v in kw.items():
        out["par"][k] = v
    return out


def of_spread(case):
    """Reduction A: a case of spread_model under claim_radius -1, gain_radius 0, hop_cost 1, min_gain 0."""
    old = case["par"]
    out = dict(case)
    out["par"] = team_params(float(old["r_max"]), float(old["r_spread"]), 0, -1, 1, 0, int(old["passes"]), float(old["r_avoid"]), float(old["z_lo"]),
                             float(old["z_hi"]), int(old["want"]), int(old["max_hops"]))
    return out


def of_gain(case, r_spread=1.0, cr=None):
    """Reduction B: a case of gain_model with every vehicle a group of its own (spread_model.own_groups), so no searcher has a peer."""
    old = case["par"]
    out = sm.own_groups(case)
    out["par"] = team_params(float(old["r_max"]), r_spread, int(old["gain_radius"]), cr, int(old["hop_cost"]), int(old["min_gain"]),
                             abi.FH_TEAM_DEFAULT_PASSES, float(old["r_avoid"]), float(old["z_lo"]), float(old["z_hi"]), int(old["want"]),
                             int(old["max_hops"]))
    return out


def as_team_flags(flags):
    """The flags of a gain record read as those of a team record: bit 128 is bit 1024."""
    f = np.asarray(flags).astype(np.int64)
    return ((f & ~abi.FH_GAIN_ALL_POOR) | np.where(f & abi.FH_GAIN_ALL_POOR, abi.FH_TEAM_ALL_POOR, 0)).astype(np.int32)


def gain_par_of(par):
    return gm.gain_params(float(par["r_max"]), int(par["gain_radius"]), int(par["hop_cost"]), int(par["min_gain"]), float(par["r_avoid"]),
                          float(par["z_lo"]), float(par["z_hi"]), int(par["want"]), int(par["max_hops"]))


# ---- the named cases ------------------------------------------------------------------------------------------------------------------------
# spread_model.corridor: a floor length x 5 x 2 at res 0.5, layer 0 known and free, layer 1 occupied and unknown above x >= unknown_from.
# The candidates are the voxels of layer 0 below unknown ones; every unknown voxel is in layer 1, one voxel above: with radius r the
# ball of a voxel of layer 0 holds the unknown voxels of layer 1 with dx dx + dy dy <= r r - 1.
def hall(x_of, status, par, length=24, unknown_from=None, g_term=None, **kw):
    return sm.corridor(len(x_of), x_of, status, g_term=g_term, length=length, unknown_from=unknown_from, par=par, **kw)


def only_unknown(c, voxels):
    """The case of one view with layer 1 known but for `voxels` (they stay occupied in the map)."""
    nx, ny, nz = c["grid"][2]
    view = c["flags"][:c["cells"]].reshape(nz, ny, nx).copy()
    view[1] = 0
    for x, y, z in voxels:
        view[z, y, x] = 1
    flags = c["flags"].copy()
    flags[:c["cells"]] = view.ravel()
    c["flags"] = flags
    return c


def wall_pair(**kw):
    """Two searchers of one view in voxel (4, 2), before unknown space that begins at x = 8 (r_max 5: candidates up to x = 13)."""
    return hall([4, 4], [R, R], team_params(5.0, 0.4, 2, kw.pop("cr", 2), **kw), unknown_from=8)


def cut_ball():
    """wall_pair with a claim ball of radius 3 around the first vehicle's goal: it cuts the balls of radius 2 of the second's candidates."""
    return hall([4, 4], [R, R], team_params(5.0, 0.4, 2, 3), unknown_from=8)


EXACT_CLAIM, EXACT_R = (10, 2, 0), 3
EXACT_IN = [(12, 4, 1), (8, 0, 1), (12, 0, 1), (10, 4, 1), (12, 3, 1)]   # squared distance from EXACT_CLAIM: 9, 9, 9 (R^2 exactly), 5, 6
EXACT_OUT = [(13, 2, 1), (7, 2, 1), (13, 1, 1)]                          # 10, 10 (R^2 + 1), 11


def exact_claim():
    """Vehicle 1 travels to the centre of EXACT_CLAIM (a standing claim); vehicle 0 stands in (10, 2, 0).  Layer 1 is known but for the
    voxels at squared distance 9 (R^2), 10 (R^2 + 1) and some nearer ones from the claim voxel: the first are covered, the second not."""
    c = hall([10, 40], [R, T], team_params(3.0, 0.4, 4, EXACT_R), length=44, g_term=np.array([(1000.0,) * 3, rm.centre(EXACT_CLAIM)]))
    return only_unknown(c, EXACT_IN + EXACT_OUT)


def standing_in_unknown(cr):
    """Vehicle 1 travels to the centre of (10, 2, 1), an unknown voxel above the floor; vehicle 0 stands below it."""
    return hall([10, 40], [R, T], team_params(3.0, 0.4, 2, cr), length=44, g_term=np.array([(1000.0,) * 3, rm.centre((10, 2, 1))]))


def two_claims():
    """Two standing claims two voxels apart: their balls of radius 3 overlap, and `covered` counts the union once."""
    g = np.array([(1000.0,) * 3, rm.centre((9, 2, 0)), rm.centre((11, 2, 0))])
    return hall([10, 40, 41], [R, T, T], team_params(3.0, 0.4, 3, 3), length=44, g_term=g)


def claim_outside_box():
    """r_max 1.0: the box of vehicle 0 is small.  A standing claim at x = 16
    lies outside the box (x in 7 .. 13), inside near = 1 + 3.5, and its ball of radius 4 reaches the column 13."""
    g = np.array([(1000.0,) * 3, rm.centre((16, 2, 0))])
    return hall([10, 40], [R, T], team_params(1.0, 0.4, 2, 4), length=44, g_term=g)


def claim_outside_lattice():
    """The vehicle stands in voxel 1 of the floor; a standing claim at x = -2, before the lattice begins, inside near: its ball of
    radius 4 reaches the columns 0 .. 1."""
    g = np.array([(1000.0,) * 3, (-0.75, 1.25, 0.25)])
    return hall([1, 40], [R, T], team_params(1.0, 0.4, 2, 4), length=44, g_term=g)


def word_edge_claim():
    """132 voxels long, r_max 40: the box is the whole row, three words of 64.  Standing claims at x = 63 (a ball across bits 63 | 64),
    at x = 131, y = 2 (the end of a row in y) and at x = 130, y = 4 in layer 1 (the end of the last row of a slab, in z).  The starts of
    the rows that follow are unknown and not covered."""
    g = np.array([(1000.0,) * 3, rm.centre((63, 2, 0)), rm.centre((131, 2, 0)), rm.centre((130, 4, 1)), rm.centre((131, 4, 0))])
    return hall([66, 200, 201, 202, 203], [R, T, T, T, T], team_params(40.0, 0.4, 3, 5, max_hops=8), length=132, g_term=g)


def poor_by_discount(min_gain):
    """wall_pair with claim_radius 31: the first vehicle's ball covers all that the second can count."""
    return hall([4, 4], [R, R], team_params(5.0, 0.4, 2, 31, min_gain=min_gain), unknown_from=8)


def claimed_and_richest():
    """Two searchers in voxel (4, 2) below a patch of 3 x 3 unknown voxels around (9, 2, 1) and a lone one; steps cost nothing and claims
    cover nothing (claim_radius -1).  (9, 2, 0), gain 9, is the first vehicle's goal and the richest candidate of the second, and it
    is claimed; its neighbours count 6."""
    c = hall([4, 4], [R, R], team_params(5.0, 0.4, 2, -1, hop_cost=0))
    return only_unknown(c, [(x, y, 1) for x in (8, 9, 10) for y in (1, 2, 3)] + [(12, 2, 1)])


def chain(passes):
    """Three searchers a voxel apart before one wall: 1 waits for 0 and 2 for both; the third sees both discounts."""
    return hall([5, 6, 7], [R, R, R], team_params(3.0, 0.4, 2, 2, passes=passes), unknown_from=10)


def widened_reach(cr=3):
    """r_max 1.0, r_spread 0.4: K16's reach is 2.4, the widened one 2 + (2 + 3 + 1) 0.5 = 5.  Vehicles 8 voxels (4 m) apart."""
    return hall([4, 12], [R, R], team_params(1.0, 0.4, 2, cr))


def widened_overflow(cr=3):
    """33 standing claims 2.5 m from the vehicle: beyond K16's near (1.4), inside the widened one (4)."""
    n = 34
    g = np.full((n, 3), 1000.0)
    for k in range(1, n):
        g[k] = rm.centre((15, k % 5, 0))
    g[:, 0][1:] += 0.001 * np.arange(1, n)
    return hall([10] + [40] * 33, [R] + [T] * 33, team_params(1.0, 0.4, 2, cr), length=44, g_term=g)


def empty_lower_peer():
    """spread_model.finds_nothing: vehicle 0 finds nothing, claims nothing and covers nothing for vehicle 1."""
    return hall([2, 15], [R, R], team_params(3.0, 1.0, 3, 3), length=30, unknown_from=20)


CASES = {
    "wall_pair": wall_pair, "cut_ball": cut_ball, "exact_claim": exact_claim,
    "claim_radius_none": lambda: standing_in_unknown(-1), "claim_radius_0": lambda: standing_in_unknown(0), "claim_radius_31": lambda: standing_in_unknown(31),
    "two_claims": two_claims, "claim_outside_box": claim_outside_box, "claim_outside_lattice": claim_outside_lattice,
    "word_edge_claim": word_edge_claim, "poor_by_discount": lambda: poor_by_discount(5), "poor_by_discount_min_0": lambda: poor_by_discount(0),
    "claimed_and_richest": claimed_and_richest, "chain_passes_3": lambda: chain(3), "chain_passes_2": lambda: chain(2),
    "widened_reach": widened_reach, "widened_reach_plain": lambda: widened_reach(-1),
    "widened_overflow": widened_overflow, "widened_overflow_plain": lambda: widened_overflow(-1),
    "empty_lower_peer": empty_lower_peer,
}

_BUILT, _MODELS = {}, {}


def case(name):
    """The named case, "A:<case of spread_model>" or "B:<case of gain_model>" (the two reductions), built once.  Treat it as read-only."""
    if name not in _BUILT:
        if name.startswith("A:"):
            _BUILT[name] = of_spread(sm.case(name[2:]))
        elif name.startswith("B:"):
            _BUILT[name] = of_gain(gm.case(name[2:]))
        else:
            _BUILT[name] = CASES[name]()
    return _BUILT[name]


REDUCTIONS_A = ["A:" + k for k in sm.CASES]
REDUCTIONS_B = ["B:" + k for k in gm.CASES]


def model(case, variant=None, par=None, details=None):
    return team_goals(case["par"] if par is None else par, case["grid"], case["flags"], case["stride"], case["view_of"], case["n_views"],
                      case.get("group"), case["vehicles"], case["occ"], case["m_origin"], case["m_res"], variant, details)


def expected(name):
    """The model's outputs of the named case, computed once.  Treat them as read-only."""
    if name not in _MODELS:
        _MODELS[name] = model(case(name))
    return _MODELS[name]
