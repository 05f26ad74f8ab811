"""The model of include/fasterhip_bid.h (fh_bid_goals_device) restated in plain Python: the classes and the standing claims of
tests/spread_model.py, the interaction radius, the claim voxel and the covered voxels of tests/team_model.py, the gain of
tests/gain_model.py, the flood of tests/reach_model.py and the candidates of tests/frontier_model.py, all by import.  What this header
adds is written out here: the rivals on both sides of the index, the offers, the rounds and who settles in them; the search of a
vehicle under a list of claims is that of team_model.team_goals, statement by statement (bid_goals of a case without rivals is compared
with it in every byte: Reduction A).  greedy_goals() is the sequential rule that the rounds are a parallel form of.  Not a test file.

`variant` names a deliberately WRONG model (VARIANTS): tests/test_bid_model.py shows that the named cases (CASES) tell every one of
them from the model, so kernels that made one of these mistakes would not pass tests/test_gpu_bid.py."""
import numpy as np

from faster_amd import abi

import frontier_model as fm
import gain_model as gm
import reach_model as rm
import spread_model as sm
import team_model as tm

VARIANTS = ("index_order",       # the lower index beats the higher, whatever the offers
            "ties_high",         # equal (utility, hops): the higher index wins
            "ties_no_hops",      # equal utility: the lower index wins, whatever the hops
            "stale_offers",      # an offer is never searched again
            "decided_block",     # a decided rival with an offer still blocks
            "sees_own_round",    # the settling of a round, in index order, sees what that round has decided
            "no_offer_blocks",   # an undecided rival without an offer blocks for the round
            "overflow_blocks",   # an overflowed rival blocks
            "lower_only",        # the lists hold the lower rivals only
            "mask0_claims")      # a rival decided with d_mask 0 claims what its d_goals hold, and its decision makes a search due

INF = float("inf")
REACHED_WANT = abi.FH_FRONTIER_WANT_REACHED
SEARCHER, STANDING, NONE = sm.SEARCHER, sm.STANDING, sm.NONE
R, T = sm.R, sm.T
W, F = abi.FH_FRONTIER_WANTED, abi.FH_FRONTIER_FOUND


def beats(a, i, b, k, variant=None):
    """Offer a = (utility, hops) of vehicle i against offer b of vehicle k."""
    if variant == "index_order":
        return i < k
    if a[0] != b[0]:
        return a[0] > b[0]
    if variant != "ties_no_hops" and a[1] != b[1]:
        return a[1] < b[1]
    return i > k if variant == "ties_high" else i < k


class _Fleet:
    """What every rule below shares: the classes, the lists, the outputs of pass 0 and the search of one vehicle under claims."""

    def __init__(self, par, grid, flags, view_stride, view_of, n_views, group, vehicles, occ, m_origin, m_res, variant=None, details=None):
        self.par, self.grid, self.variant, self.details = par, grid, variant, details
        self.occ, self.m_origin, self.m_res = occ, m_origin, m_res
        origin, res, dims = grid
        n = self.n = len(vehicles)
        r_max = np.float64(par["r_max"])
        r_int = tm.r_int_of(par, res)
        reach, near = (r_max + r_max) + r_int, r_max + r_int
        reach2, near2 = reach * reach, near * near
        _, _, base = rm.reach_goals(sm.reach_par_of(par), grid, flags, view_stride, view_of, n_views, vehicles, occ, m_origin, m_res)
        self.goals = vehicles["g_term"].copy()
        self.mask = np.zeros(n, dtype=np.int32)
        rec = self.rec = np.zeros(n, dtype=abi.bid_record_dtype)
        pos, g_term = self.pos, self.g_term = vehicles["state"]["pos"], vehicles["g_term"]
        view = self.view = [int(i if view_of is None else view_of[i]) for i in range(n)]
        has_view = [0 <= view[i] < n_views for i in range(n)]
        grp = [(int(view[i] if group is None else group[view[i]]) if has_view[i] else 0) for i in range(n)]
        cls = self.cls = []
        for i in range(n):
            f = int(base["flags"][i])
            if (f & ~(F | abi.FH_REACH_CUT)) == W:
                cls.append(SEARCHER)
            elif not f & W and has_view[i] and int(vehicles["status"][i]) != sm.GOAL_REACHED and np.all(np.isfinite(g_term[i])):
                cls.append(STANDING)
            else:
                cls.append(NONE)

        def peers(i, k):
            return has_view[i] and has_view[k] and i != k and grp[i] == grp[k]

        self.rivals, self.standing, self.overflowed = {}, {}, set()
        for i in range(n):
            for k in ("flags", "view"):
                rec[k][i] = base[k][i]
            rec["flags"][i] &= ~(F | abi.FH_REACH_CUT)
            rec["cell"][i], rec["hops"][i], rec["d2"][i], rec["group"][i] = -1, -1, np.inf, grp[i]
            rec["gain"][i], rec["best_gain"][i] = -1, -1
            if cls[i] != SEARCHER:
                continue
            ks = range(i) if variant == "lower_only" else range(n)
            self.rivals[i] = [k for k in ks if peers(i, k) and cls[k] == SEARCHER and sm.d2_of(pos[k], pos[i]) < reach2]
            self.standing[i] = [k for k in range(n) if peers(i, k) and cls[k] == STANDING and sm.d2_of(g_term[k], pos[i]) < near2]
            rec["rivals"][i], rec["claims"][i] = len(self.rivals[i]), len(self.standing[i])
            if len(self.rivals[i]) + len(self.standing[i]) > abi.FH_BID_LIST:
                rec["flags"][i] |= abi.FH_BID_OVERFLOW
                self.overflowed.add(i)
            else:
                rec["decided_pass"][i] = -1
        self.views = fm.views_of(flags, n_views, view_stride, dims)
        self.free, _ = rm.map_free(grid, occ, m_origin, m_res)
        self.fronts = {}

    def bidders(self):
        return [i for i in range(self.n) if self.cls[i] == SEARCHER and i not in self.overflowed]

    def search(self, i, claims):
        """team_model's search of vehicle i under `claims`: writes the outputs of i and returns its offer (utility, hops), or None."""
        par, rec, goals, mask = self.par, self.rec, self.goals, self.mask
        origin, res, dims = self.grid
        nx, ny, nz = (int(d) for d in dims)
        r_max, r_spread, max_hops = np.float64(par["r_max"]), np.float64(par["r_spread"]), int(par["max_hops"])
        g, hop_cost, min_gain, cr = int(par["gain_radius"]), int(par["hop_cost"]), int(par["min_gain"]), int(par["claim_radius"])
        s2_max = r_spread * r_spread
        v, p, gt = self.view[i], self.pos[i], self.g_term[i]
        start = tuple(int(np.floor((np.float64(p[k]) - np.float64(origin[k])) / np.float64(res))) for k in range(3))
        box = [rm.box_axis(p[k], r_max, origin[k], res, int(dims[k])) for k in range(3)]
        lo, hi = [b[0] for b in box], [b[1] for b in box]
        if v not in self.fronts:
            self.fronts[v] = fm.frontier_mask(self.views[v])
        with np.errstate(over="ignore", invalid="ignore"):
            ok, d2, (qx, qy, qz) = fm.candidates_of(self.fronts[v], p, gt, par, self.grid, self.occ, self.m_origin, self.m_res)
            taken = np.zeros(ok.shape, dtype=bool)
            for c in claims:
                sx, sy, sz = np.float64(c[0]) - qx, np.float64(c[1]) - qy, np.float64(c[2]) - qz
                s2 = (sx * sx + sy * sy) + sz * sz
                taken |= s2 < s2_max
        taken &= ok
        hops = rm.flood(start, lo, hi, (self.views[v] == 0) & self.free, max_hops)
        unknown = self.views[v] != 0
        voxels = [tm.claim_voxel(c, origin, res) for c in claims]
        cov, covered = tm.covered_of(voxels, lo, hi, unknown, cr)
        counted = unknown & ~cov
        open_ = ok & ~taken & (hops >= 0)
        rec["candidates"][i], rec["claimed"][i] = int(ok.sum()), int(taken.sum())
        rec["reachable"][i], rec["reached"][i], rec["levels"][i] = int(open_.sum()), int((hops >= 0).sum()), max(int(hops.max()), 0)
        rec["flags"][i] = W
        if max_hops > 0 and int(hops.max()) == max_hops:
            rec["flags"][i] |= abi.FH_REACH_CUT
        rec["claims"][i], rec["covered"][i] = len(claims), covered
        rows, poor, most = [], 0, -1
        info = {"claims": [tuple(float(x) for x in c) for c in claims], "voxels": voxels, "cov": cov, "unknown": unknown, "lo": lo, "hi": hi, "cands": {}}
        for c in (int(c) for c in np.nonzero(open_.ravel())[0]):
            xyz = (c % nx, (c // nx) % ny, c // (nx * ny))
            gain = gm._fast_gain(xyz, lo, hi, counted, g)
            hh, dd = int(hops.ravel()[c]), d2.ravel()[c]
            utility = gain - hop_cost * hh
            most = max(most, gain)
            if gain < min_gain:
                poor += 1
                continue
            info["cands"][c] = (hh, gain, utility, float(dd))
            rows.append(((-utility, hh, dd, c), c, gain, utility, dd, hh))
        if self.details is not None:
            self.details[i] = info
        rec["poor"][i], rec["best_gain"][i] = poor, most
        goals[i], mask[i] = gt, 0
        rec["cell"][i], rec["hops"][i], rec["d2"][i], rec["gain"][i], rec["utility"][i] = -1, -1, np.inf, -1, 0
        if rec["reachable"][i] > 0 and poor == rec["reachable"][i]:
            rec["flags"][i] |= abi.FH_BID_ALL_POOR
        if not rows:
            if rec["claimed"][i] > 0:
                rec["flags"][i] |= abi.FH_BID_CLAIMED
            return None
        _, c, gain, utility, dd, hh = sorted(rows, key=lambda r: r[0])[0]
        iz, iy, ix = c // (nx * ny), (c // nx) % ny, c % nx
        goals[i] = (qx[0, 0, ix], qy[0, iy, 0], qz[iz, 0, 0])
        mask[i] = 1
        rec["flags"][i] |= F
        rec["cell"][i], rec["hops"][i], rec["d2"][i] = c, hh, dd
        rec["gain"][i], rec["utility"][i] = gain, utility
        return (utility, hh)

    def unsettle(self, i):
        """The outputs of a searcher that the last round left undecided: those of a vehicle that is not searched; rivals and searches stay."""
        rec = self.rec
        self.goals[i], self.mask[i] = self.g_term[i], 0
        rec["flags"][i] = W | abi.FH_BID_UNSETTLED
        rec["cell"][i], rec["hops"][i], rec["d2"][i] = -1, -1, np.inf
        for k in ("candidates", "reachable", "reached", "levels", "claimed", "utility", "poor", "covered"):
            rec[k][i] = 0
        rec["gain"][i], rec["best_gain"][i], rec["decided_pass"][i], rec["claims"][i] = -1, -1, -1, len(self.standing[i])

    def out(self):
        return self.goals, self.mask, self.rec


def bid_goals(par, grid, flags, view_stride, view_of, n_views, group, vehicles, occ, m_origin, m_res, variant=None, details=None, trace=None):
    """-> (goals [n][3], mask [n] int32, records [n] abi.bid_record_dtype): the arguments of team_model.team_goals with an
    abi.bid_params_dtype record.  details: per searched vehicle, what its LAST search saw (as team_model's).  trace: a dict that
    receives "searched": {round: [i]}, "decided": {round: [i]}, "offers": {round: {i: (utility, hops) or None}} and "ties": the pairs of
    undecided rivals whose offers of one round were equal in (utility, hops)."""
    fl = _Fleet(par, grid, flags, view_stride, view_of, n_views, group, vehicles, occ, m_origin, m_res, variant, details)
    rec, goals, mask, n = fl.rec, fl.goals, fl.mask, fl.n
    passes = int(par["passes"])
    offer = {}
    if trace is not None:
        trace.update(searched={}, decided={}, offers={}, ties=[])
    for p in range(1, passes + 1):
        before, goals_before, mask_before = rec["decided_pass"].copy(), goals.copy(), mask.copy()   # nothing a round decides is seen by that same round
        undecided = [i for i in fl.bidders() if before[i] == -1]

        def claiming(k):
            return 1 <= before[k] < p and (mask_before[k] == 1 or variant == "mask0_claims")

        searched = []
        for i in undecided:
            due = p == 1 or any(before[k] == p - 1 and claiming(k) for k in fl.rivals[i])
            if variant == "stale_offers":
                due = p == 1
            if not due:
                continue
            claims = [fl.g_term[k] for k in fl.standing[i]] + [goals_before[k].copy() for k in fl.rivals[i] if claiming(k)]
            offer[i] = fl.search(i, claims)
            rec["searches"][i] += 1
            searched.append(i)
        now = before.copy()
        for i in undecided:
            if offer[i] is not None:
                blocked = False
                for k in fl.rivals[i]:
                    state = now if variant == "sees_own_round" else before
                    if k in fl.overflowed:
                        blocked |= variant == "overflow_blocks"
                    elif state[k] == -1:
                        if offer[k] is None:
                            blocked |= variant == "no_offer_blocks"
                        else:
                            blocked |= beats(offer[k], k, offer[i], i, variant)
                            if trace is not None and offer[k] == offer[i] and k < i:
                                trace["ties"].append((p, k, i))
                    elif variant == "decided_block" and offer.get(k) is not None:
                        blocked |= beats(offer[k], k, offer[i], i, variant)
                if blocked:
                    continue
            now[i] = p
        rec["decided_pass"][:] = now
        if trace is not None:
            trace["searched"][p], trace["offers"][p] = searched, {i: offer[i] for i in undecided}
            trace["decided"][p] = [i for i in undecided if now[i] == p]
    for i in fl.bidders():
        if rec["decided_pass"][i] == -1:
            fl.unsettle(i)
    return fl.out()


def greedy_goals(par, grid, flags, view_stride, view_of, n_views, group, vehicles, occ, m_origin, m_res):
    """The sequential rule: search every undecided searcher under the goals decided so far; a searcher without an offer is decided at
    once; of the others the ONE whose offer beats all others is decided; repeat.  decided_pass counts the steps and `searches` the
    searches of this rule: neither is comparable with bid_goals'."""
    fl = _Fleet(par, grid, flags, view_stride, view_of, n_views, group, vehicles, occ, m_origin, m_res)
    rec, goals, mask = fl.rec, fl.goals, fl.mask
    step = 0
    while True:
        undecided = [i for i in fl.bidders() if rec["decided_pass"][i] == -1]
        if not undecided:
            break
        step += 1
        offer = {}
        for i in undecided:
            claims = [fl.g_term[k] for k in fl.standing[i]] + [goals[k].copy() for k in fl.rivals[i] if rec["decided_pass"][k] >= 1 and mask[k] == 1]
            offer[i] = fl.search(i, claims)
            rec["searches"][i] += 1
        none = [i for i in undecided if offer[i] is None]
        for i in none:
            rec["decided_pass"][i] = step
        if none:
            continue   # (they claim nothing: the offers of the others stand, and are searched again all the same)
        best = undecided[0]
        for i in undecided[1:]:
            if beats(offer[i], i, offer[best], best):
                best = i
        rec["decided_pass"][best] = step
    return fl.out()


# ---- parameters -----------------------------------------------------------------------------------------------------------------------------
def bid_params(r_max, r_spread, g, cr=None, hop_cost=1, min_gain=0, passes=abi.FH_BID_DEFAULT_PASSES, r_avoid=0.0, z_lo=-INF, z_hi=INF,
               want=REACHED_WANT, max_hops=0):
    p = abi.default_bid_params(r_max, r_spread, g, cr)
    p["r_avoid"], p["z_lo"], p["z_hi"], p["want"], p["max_hops"], p["passes"], p["hop_cost"], p["min_gain"] = r_avoid, z_lo, z_hi, want, max_hops, passes, hop_cost, min_gain
    return p


def with_par(case, **kw):
    """The case with fields of its params replaced."""
    out = dict(case)
    out["par"] = case["par"].copy()
    for k, v in kw.items():
        out["par"][k] = v
    return out


def of_team(case):
    """A case of team_model (or one made by its reductions) with the same bytes as fh_bid_params."""
    out = dict(case)
    out["par"] = np.array(case["par"]).view(abi.bid_params_dtype).reshape(()).copy()
    return out


def as_team(case):
    """The reverse: the case for team_model."""
    out = dict(case)
    out["par"] = np.array(case["par"]).view(abi.team_params_dtype).reshape(()).copy()
    return out


def as_team_records(rec):
    """The records with `searches` zeroed, as abi.team_record_dtype (rivals at `lower`)."""
    r = rec.copy()
    r["searches"] = 0
    return r.view(abi.team_record_dtype)


def relabelled(case, perm):
    """The case with vehicle perm[j] in place j (views and groups are per view: they stay)."""
    perm = np.asarray(perm)
    out = dict(case)
    out["vehicles"] = case["vehicles"][perm].copy()
    out["view_of"] = None if case["view_of"] is None else np.ascontiguousarray(np.asarray(case["view_of"])[perm])
    if case["view_of"] is None:
        out["view_of"] = perm.astype(np.int32)
    return out


# ---- the named cases ------------------------------------------------------------------------------------------------------------------------
# team_model.hall: a floor length x 5 x 2 at res 0.5, layer 0 known and free, layer 1 occupied and unknown; team_model.only_unknown keeps
# of layer 1 only the listed voxels unknown.  A patch of unknown voxels above the floor is what a vehicle below it can gain.  With r_max
# 3, gain_radius 2 and claim_radius 2 the interaction radius is 2.5 and reach = 8.5: vehicles less than 17 voxels apart are rivals.
def hall(x_of, status, par, length=24, unknown_from=None, g_term=None, **kw):
    return sm.corridor(len(x_of), x_of, status, g_term=g_term, length=length, unknown_from=unknown_from, par=par, **kw)


def patch(cx, half=1, ys=(1, 2, 3)):
    """Unknown voxels of layer 1 above (cx - half .. cx + half, ys)."""
    return [(x, y, 1) for x in range(cx - half, cx + half + 1) for y in ys]


def nearer_higher(hop_cost=1):
    """Two searchers of one view before one hall that begins at x = 10; vehicle 1, in voxel 7, is nearer than vehicle 0 in voxel 4."""
    return hall([4, 7], [R, R], bid_params(5.0, 0.4, 2, 2, hop_cost=hop_cost), unknown_from=10)


def same_voxel():
    """Both in voxel (4, 2): equal offers, the lower index wins."""
    return hall([4, 4], [R, R], bid_params(5.0, 0.4, 2, 2), unknown_from=8)


def chain(passes=8):
    """Three mutual rivals before one hall, the higher the index the nearer: offers fall against the index."""
    return hall([4, 6, 8], [R, R, R], bid_params(5.0, 0.4, 2, 2, passes=passes), unknown_from=11)


def path_four():
    """Rivals 0 - 1 - 2 - 3, ten voxels apart (twenty are none), each before a patch of its own: 9, 1, 9 and 1 voxels."""
    c = hall([5, 15, 25, 35], [R, R, R, R], bid_params(3.0, 0.4, 2, 2), length=44)
    return tm.only_unknown(c, patch(7) + [(17, 2, 1)] + patch(27) + [(37, 2, 1)])


def keeps_offer(passes=8):
    """Rivals A = 0 - B = 1 - L = 2 with patches of 9, 6 and 1 voxels, and N = 3, a rival of L alone that finds nothing (no unknown
    voxel near it).  Round 1 decides A and N; B, beaten by A, and L, beaten by B, wait.  In round 2 B is searched again and L is not:
    none of its rivals won a goal (N was decided with d_mask 0)."""
    c = hall([5, 15, 25, 38], [R, R, R, R], bid_params(3.0, 0.4, 2, 2, passes=passes), length=48)
    return tm.only_unknown(c, patch(7) + patch(17, ys=(1, 2)) + [(27, 2, 1)])


def flip():
    """A = 0 in voxel 11 and B = 1 in voxel 16 before one patch of 9 at x = 13; C = 2 in voxel 28, a rival of B alone, before a patch
    of 4; B has a lone voxel behind it.  Round 1: A beats B beats C.  Under A's claim B's offer falls below C's: C is decided in round 2
    and B in round 3, under both claims."""
    c = hall([11, 16, 28], [R, R, R], bid_params(3.0, 0.4, 2, 2), length=40)
    return tm.only_unknown(c, patch(13) + [(18, 2, 1)] + [(30, 1, 1), (30, 2, 1), (30, 3, 1), (31, 2, 1)])


def no_offer_poor():
    """min_gain 3: vehicle 0 stands before a lone unknown voxel (every open candidate poor), its rival, vehicle 1, before a patch of 9."""
    c = hall([5, 15], [R, R], bid_params(3.0, 0.4, 2, 2, min_gain=3), length=24)
    return tm.only_unknown(c, [(7, 2, 1)] + patch(17))


def no_offer_unreachable():
    """spread_model.finds_nothing: the sphere of vehicle 0 holds no candidate; vehicle 1, thirteen voxels away, is its rival."""
    return hall([2, 15], [R, R], bid_params(3.0, 0.4, 2, 2), length=30, unknown_from=20)


def listed(n_standing, far_rival=False):
    """Vehicle 0, in voxel 10, with n_standing vehicles that travel to goals within 2.5 m of it (their claim balls all touch its box),
    and two rivals beside it (voxels 9 and 11) that list them too; far_rival: one more searcher in voxel 24, a rival of all three that is
    too far for the standing claims."""
    n = 3 + n_standing + (1 if far_rival else 0)
    g = np.full((n, 3), 1000.0)
    for k in range(n_standing):
        g[3 + k] = rm.centre((8 + k % 5, k % 5, 0))
        g[3 + k][0] += 0.001 * (k + 1)
    x_of = [10, 9, 11] + [60] * n_standing + ([24] if far_rival else [])
    status = [R, R, R] + [T] * n_standing + ([R] if far_rival else [])
    return hall(x_of, status, bid_params(3.0, 0.4, 2, 2), length=64, g_term=g)


def reach_edge(inside):
    """reach = 3 + 3 + 2.5 = 8.5: voxel centres 17 voxels apart are exactly 8.5 apart, no rivals; 16 voxels: rivals, by both."""
    c = hall([5, 21 if inside else 22], [R, R], bid_params(3.0, 0.4, 2, 2), length=32)
    return tm.only_unknown(c, patch(7) + [(23, 2, 1)])


def claims_both_sides():
    """Vehicles 0 and 3 travel (standing claims below and above), 1 and 2 are searchers before one patch, 2 the nearer: vehicle 1 is
    searched again under the two standing claims and the goal of the rival above it."""
    g = np.array([rm.centre((3, 1, 0)), (1000.0,) * 3, (1000.0,) * 3, rm.centre((4, 3, 0))])
    c = hall([40, 6, 9, 41], [T, R, R, T], bid_params(3.0, 0.4, 2, 2), length=44, g_term=g)
    return tm.only_unknown(c, patch(11) + [(2, 2, 1), (3, 0, 1), (5, 4, 1)])


def word_edge_winner():
    """132 voxels long, r_max 40: every box is the whole lattice, three words of 64 a row, and all three are rivals.  Vehicle 0 (voxel
    61) wins a goal at x = 63: its claim ball of radius 5 lies across bits 63 | 64.  Vehicle 2 (voxel 131) wins the voxel it stands in, the end
    of a row; the starts of the rows that follow are unknown and not covered.  Vehicle 1 (voxel 67) is searched under both."""
    c = hall([61, 67, 131], [R, R, R], bid_params(40.0, 0.4, 3, 5, max_hops=8), length=132)
    unknown = [(x, y, 1) for x in (62, 63, 64, 65) for y in (1, 2, 3)] + [(131, 1, 1), (131, 2, 1), (131, 3, 1), (130, 2, 1)]
    return tm.only_unknown(c, unknown + [(72, 2, 1), (0, 3, 1), (0, 4, 1), (1, 3, 1)])


CASES = {
    "nearer_higher": nearer_higher, "fewer_hops": lambda: nearer_higher(hop_cost=0), "same_voxel": same_voxel,
    "chain": chain, "chain_passes_2": lambda: chain(2), "path_four": path_four,
    "keeps_offer": keeps_offer, "keeps_offer_passes_2": lambda: keeps_offer(2), "flip": flip,
    "no_offer_poor": no_offer_poor, "no_offer_unreachable": no_offer_unreachable,
    "listed_64": lambda: listed(62), "listed_65": lambda: listed(62, far_rival=True), "listed_33": lambda: of_team(tm.case("widened_overflow")),
    "outside_reach": lambda: reach_edge(False), "inside_reach": lambda: reach_edge(True),
    "claims_both_sides": claims_both_sides, "word_edge_winner": word_edge_winner,
}

_BUILT, _MODELS = {}, {}


def case(name):
    """The named case, or "A:<case>" (Reduction A: a case of gain_model with every vehicle a group of its own, or a case of team_model
    without peers), built once.  Treat it as read-only."""
    if name not in _BUILT:
        if name.startswith("A:gain:"):
            _BUILT[name] = of_team(tm.case("B:" + name[7:]))
        elif name.startswith("A:team:"):
            _BUILT[name] = of_team(tm.case(name[7:]))
        else:
            _BUILT[name] = CASES[name]()
    return _BUILT[name]


REDUCTIONS_A = ["A:gain:" + k for k in gm.CASES] + ["A:team:" + k for k in ("exact_claim", "claim_radius_none", "claim_radius_0", "claim_radius_31", "two_claims",
                                                                            "claim_outside_box", "claim_outside_lattice", "word_edge_claim")]


def _args(case, par=None):
    return (case["par"] if par is None else par, case["grid"], case["flags"], case["stride"], case["view_of"], case["n_views"], case.get("group"),
            case["vehicles"], case["occ"], case["m_origin"], case["m_res"])


def model(case, variant=None, par=None, details=None, trace=None):
    return bid_goals(*_args(case, par), variant=variant, details=details, trace=trace)


def greedy(case):
    return greedy_goals(*_args(case))


def expected(name):
    """The model's outputs of the named case, computed once.  Treat them as read-only."""
    if name not in _MODELS:
        _MODELS[name] = model(case(name))
    return _MODELS[name]
