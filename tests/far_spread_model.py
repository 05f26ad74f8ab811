"""The model of include/fasterhip_apart.h (fh_apart_goals_device) restated in Python over the vehicles in index order, on the
pieces of tests/far_model.py (summary, flood, block_d2, pack): no passes, no bitmaps and no chunks, so it shares no structure with the
kernels.  A searcher's claims are the g_term of its standing peers and the goals this loop has already given to the searching peers
below it.  Not a test file.

`variant` names a deliberately WRONG model (VARIANTS): tests/test_far_spread_model.py shows that the named cases (CASES) tell every one of
them from the model, so a kernel that made one of these mistakes would not pass tests/test_gpu_far_spread.py."""
import numpy as np

from faster_amd import abi

import far_model as fa
import frontier_model as fm
import reach_model as rm

VARIANTS = ("no_standing",      # standing claims ignored
            "higher_peers",     # the searching peers ABOVE i claim (the higher index chooses first)
            "le",               # G2 <= r_spread^2 is claimed too
            "non_peers",        # every vehicle with a view claims, whatever its group
            "group_by_view",    # the labels are ignored: group = view
            "same_pass",        # a searcher is decided in pass lower(i), with the peer just below it: a pass sees its own decisions
            "centre",           # claimed by the distance to the centre of the block, not to the block
            "cut_links",        # a claimed block is closed to the flood
            "reached_claims",   # a skipped vehicle claims whatever its status
            "voxel_only")       # a block is claimed iff the voxel that would be chosen in it is within r_spread of a claim

INF, NAN = float("inf"), float("nan")
ALL, REACHED, WANT_NO_PATH = abi.FH_FRONTIER_WANT_ALL, abi.FH_FRONTIER_WANT_REACHED, abi.FH_FRONTIER_WANT_NO_PATH
TRAVELING, YAWING = abi.FH_VEHICLE_TRAVELING, abi.FH_VEHICLE_YAWING
UNSETTLED, CLAIMED = abi.FH_APART_UNSETTLED, abi.FH_APART_CLAIMED
NONE, SEARCHER, STANDING = 0, 1, 2


def work_bytes(dims, B, n_views, n):
    far = fa.work_bytes(dims, B, n_views)
    return 0 if far == 0 or n < 0 else far + ((n + 63) & ~63) + 4 * n + 4 * n


def judge(par, grid, view_of, n_views, skip, group, vehicles, variant=None):
    """Per vehicle (flags, view, class, group, start voxel or None): fasterhip_far.h's judgement and the classes of this header."""
    origin, res, dims = grid
    out = []
    for i in range(len(vehicles)):
        v = int(i if view_of is None else view_of[i])
        p, g = vehicles["state"]["pos"][i], vehicles["g_term"][i]
        status = int(vehicles["status"][i])
        wanted = fm.wanted(int(par["want"]), status, int(vehicles["stage"][i]))
        flag = abi.FH_FRONTIER_WANTED if wanted else 0
        has_view = 0 <= v < n_views
        if not has_view:
            flag |= abi.FH_FRONTIER_NO_VIEW
        if not (np.all(np.isfinite(p)) and np.all(np.isfinite(g))):
            flag |= abi.FH_FRONTIER_BAD_POS
        eligible = flag == abi.FH_FRONTIER_WANTED
        skipped = skip is not None and int(skip[i]) != 0
        if skipped:
            flag |= abi.FH_FAR_SKIPPED
        start = None
        if eligible and not skipped:
            with np.errstate(all="ignore"):
                s = [np.floor((np.float64(p[k]) - np.float64(origin[k])) / np.float64(res)) for k in range(3)]
            if all(0.0 <= s[k] < dims[k] for k in range(3)):
                start = tuple(int(x) for x in s)
            else:
                flag |= abi.FH_REACH_START_OUTSIDE
        cls = NONE
        if start is not None:
            cls = SEARCHER
        elif has_view and np.all(np.isfinite(g)) and (not wanted or skipped):
            if status != fm.GOAL_REACHED or (variant == "reached_claims" and skipped):
                cls = STANDING
        if not has_view:
            grp = 0
        elif group is None or variant == "group_by_view":
            grp = v
        else:
            grp = int(group[v])
        out.append((flag, v, cls, grp, start))
    return out


def far_spread_goals(par, grid, flags, view_stride, view_of, n_views, skip, group, vehicles, occ, m_origin, m_res, variant=None):
    """-> (goals [n][3], mask [n] int32, records [n] abi.far_spread_record_dtype, sums {view: [4][W] uint64 of the needed views}, need
    [(n_views + 63) & ~63] uint8): the arguments of far_model.far_goals with an abi.far_spread_params_dtype record and the labels."""
    origin, res, dims = grid
    nx, ny, nz = (int(d) for d in dims)
    B = int(par["block"])
    C, wx, W = fa.blocks_of(dims, B)
    assert W <= abi.FH_FAR_MAX_WORDS
    n = len(vehicles)
    views = fm.views_of(flags, n_views, view_stride, dims)
    free, qz_of = rm.map_free(grid, occ, m_origin, m_res)
    qx = (np.arange(nx) + 0.5) * float(res) + float(origin[0])
    qy = (np.arange(ny) + 0.5) * float(res) + float(origin[1])
    qz = (np.arange(nz) + 0.5) * float(res) + float(origin[2])
    done = {}
    goals = np.zeros((n, 3), dtype=np.float64)
    mask = np.zeros(n, dtype=np.int32)
    rec = np.zeros(n, dtype=abi.far_spread_record_dtype)
    need = np.zeros((n_views + 63) & ~63, dtype=np.uint8)
    max_hops, passes = int(par["max_hops"]), int(par["passes"])
    r_avoid, r_spread = np.float64(par["r_avoid"]), np.float64(par["r_spread"])
    a2, s2 = r_avoid * r_avoid, r_spread * r_spread
    who = judge(par, grid, view_of, n_views, skip, group, vehicles, variant)

    def peers(i, k):   # (asked of vehicles with a class: both have a view in range)
        return k != i and (variant == "non_peers" or who[k][3] == who[i][3])

    for i in range(n):
        flag, v, cls, grp, start = who[i]
        goals[i] = vehicles["g_term"][i]   # (the bits: a copy)
        rec[i] = (flag, v, -1, -1, -1, 0, 0, 0, 0, 0, (0, 0), np.inf, np.inf, grp, 0, 0, 0, 0, 0, (0, 0))
        if cls == SEARCHER:
            need[v] = 1
            if v not in done:
                done[v] = fa.summary(views[v], free, qz_of, par, B)
    order = range(n - 1, -1, -1) if variant == "higher_peers" else range(n)
    before = (lambda k, i: k > i) if variant == "higher_peers" else (lambda k, i: k < i)
    for i in order:
        flag, v, cls, grp, start = who[i]
        if cls != SEARCHER:
            continue
        p, g = vehicles["state"]["pos"][i], vehicles["g_term"][i]
        low = [k for k in range(n) if who[k][2] == SEARCHER and before(k, i) and peers(i, k)]
        stand = [k for k in range(n) if who[k][2] == STANDING and peers(i, k)]
        rec["lower"][i], rec["standing"][i] = len(low), len(stand)
        if len(low) > passes if variant == "same_pass" else len(low) >= passes:
            rec["flags"][i] |= UNSETTLED
            rec["decided_pass"][i], rec["claims"][i] = -1, len(stand)
            continue
        rec["decided_pass"][i] = max(len(low), 1) if variant == "same_pass" else len(low) + 1
        claims = [] if variant == "no_standing" else [vehicles["g_term"][k] for k in stand]
        claims += [goals[k].copy() for k in low if mask[k] == 1]
        rec["claims"][i] = len(stand) + sum(1 for k in low if mask[k] == 1)
        maps, passable, target = done[v]
        T = maps[0]

        def nearest_voxel(b):
            best, members = None, 0
            for iz in range(b[2] * B, min(b[2] * B + B, nz)):
                for iy in range(b[1] * B, min(b[1] * B + B, ny)):
                    for ix in range(b[0] * B, min(b[0] * B + B, nx)):
                        if not target[iz, iy, ix]:
                            continue
                        members += 1
                        dx, dy, dz = qx[ix] - p[0], qy[iy] - p[1], qz[iz] - p[2]
                        d2 = (dx * dx + dy * dy) + dz * dz
                        c = (iz * ny + iy) * nx + ix
                        if best is None or (d2, c) < best[0]:
                            best = ((d2, c), c, d2, (ix, iy, iz))
            return best, members

        mine = np.zeros(T.shape, dtype=bool)      # the target blocks of this vehicle, claimed or not
        covered = np.zeros(T.shape, dtype=bool)   # those of them that are claimed
        for bz, by, bx in zip(*np.nonzero(T)):
            b = (int(bx), int(by), int(bz))
            if fa.block_d2(b, B, grid, g) < a2:
                continue
            mine[bz, by, bx] = True
            for c in claims:
                if variant == "voxel_only":
                    ix, iy, iz = nearest_voxel(b)[0][3]
                    e = [np.float64(c[0]) - qx[ix], np.float64(c[1]) - qy[iy], np.float64(c[2]) - qz[iz]]
                    g2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
                else:
                    g2 = fa.block_d2(b, B, grid, c, "centre" if variant == "centre" else None)
                if g2 <= s2 if variant == "le" else g2 < s2:
                    covered[bz, by, bx] = True
                    break
        sb = tuple(c // B for c in start)
        if variant == "cut_links":
            _, LX, LY, LZ = (m.copy() for m in maps)
            LX[:, :, :-1] &= ~covered[:, :, :-1] & ~covered[:, :, 1:]
            LY[:, :-1, :] &= ~covered[:, :-1, :] & ~covered[:, 1:, :]
            LZ[:-1, :, :] &= ~covered[:-1, :, :] & ~covered[1:, :, :]
            hops = fa.flood(sb, (T, LX, LY, LZ), max_hops)
        else:
            hops = fa.flood(sb, maps, max_hops)
        open_ = mine & ~covered
        rec["targets"][i] = int(mine.sum())
        rec["claimed"][i] = int(covered.sum())
        rec["reachable"][i] = int((open_ & (hops >= 0)).sum())
        rec["reached"][i] = int((hops >= 0).sum())
        rec["levels"][i] = max(int(hops.max()), 0)
        if max_hops > 0 and int(hops.max()) == max_hops:
            rec["flags"][i] |= abi.FH_REACH_CUT
        found = [(int(bx), int(by), int(bz)) for bz, by, bx in zip(*np.nonzero(open_ & (hops >= 0)))]
        if not found:
            if rec["claimed"][i] > 0:
                rec["flags"][i] |= CLAIMED
            continue
        keyed = []
        for b in found:
            D2, h, idx = fa.block_d2(b, B, grid, p), int(hops[b[2], b[1], b[0]]), (b[2] * C[1] + b[1]) * C[0] + b[0]
            keyed.append(((h, D2, idx), b, D2, h, idx))
        _, b, D2, h, idx = min(keyed, key=lambda k: k[0])
        best, members = nearest_voxel(b)
        assert best is not None   # (a set bit of T: the block holds a target voxel)
        _, c, d2, (ix, iy, iz) = best
        goals[i] = (qx[ix], qy[iy], qz[iz])
        mask[i] = 1
        rec["flags"][i] |= abi.FH_FRONTIER_FOUND
        rec["cell"][i], rec["block_cell"][i], rec["hops"][i], rec["members"][i], rec["d2"][i], rec["block_d2"][i] = c, idx, h, members, d2, D2
    sums = {v: fa.pack(done[v][0], wx) for v in done}
    return goals, mask, rec, sums, need


def far_part(par):
    """The fh_far_params of an fh_apart_params record: its first 64 bytes."""
    out = np.zeros((), dtype=abi.far_params_dtype)
    for k in abi.far_params_dtype.names:
        out[k] = par[k]
    return out


def far_outputs(case):
    """What far_model.far_goals gives on the same inputs (no claims)."""
    return fa.far_goals(far_part(case["par"]), case["grid"], case["flags"], case["stride"], case["view_of"], case["n_views"], case["skip"],
                        case["vehicles"], case["occ"], case["m_origin"], case["m_res"])


# ---- the named cases: the smallest shapes at which the kernels can still go wrong -----------------------------------------------------------
def fsp(block, r_spread, passes=None, r_avoid=0.0, z_lo=-INF, z_hi=INF, want=ALL, max_hops=0):
    p = abi.default_far_spread_params(block, r_spread)
    p["r_avoid"], p["z_lo"], p["z_hi"], p["want"], p["max_hops"] = r_avoid, z_lo, z_hi, want, max_hops
    if passes is not None:
        p["passes"] = passes
    return p


centre = rm.centre
NEAR, MID, END = (8, 0), (16, 0), (23, 0)   # the target voxels of `hall`: the blocks 4, 8 and 11 at B = 2


def hall(positions, par, marks=(NEAR, MID), view_of=None, n_views=1, skip=None, g_term=None, group=None, status=None, stage=None, free=None):
    """far_model.floor on a free hall of 24 x 2 voxels (12 x 1 blocks at B = 2), the same target voxels in every view.  Vehicles read view 0
    unless stated.  status / stage: per vehicle, TRAVELING and 0 unless stated."""
    n = len(positions)
    free = np.ones((2, 24), dtype=bool) if free is None else free
    case = fa.floor(free, [list(marks)] * n_views, positions, par, view_of=[0] * n if view_of is None else view_of, skip=skip, g_term=g_term)
    case["group"] = None if group is None else np.asarray(group, dtype=np.int32)
    if status is not None:
        case["vehicles"]["status"] = status
    if stage is not None:
        case["vehicles"]["stage"] = stage
    return case


def _with_term(positions, terms):
    """g_term per vehicle: far away (as reach_model.make_case) but for the vehicles in `terms` {k: point}."""
    pts = [centre((q[0], q[1], 0)) if len(q) == 2 else q for q in positions]
    g = np.asarray(pts, dtype=np.float64) + 1000.0
    for k, t in terms.items():
        g[k] = t
    return g


AT_NEAR = centre((8, 0, 0))


def pair_one_view():
    return hall([(1, 0), (1, 0)], fsp(2, 2.0))


def pair_two_groups():
    return hall([(1, 0), (1, 0)], fsp(2, 2.0), view_of=[0, 1], n_views=2)


def chain_of_three():
    return hall([(1, 0), (1, 0), (1, 0)], fsp(2, 2.0), marks=(NEAR, MID, END))


def chain_two_passes():
    return hall([(1, 0), (1, 0), (1, 0)], fsp(2, 2.0, passes=2), marks=(NEAR, MID, END))


def lower_finds_nothing():
    """Vehicle 0 stands behind a wall (x = 2, 3) and reaches no target; vehicle 1, its peer, is decided in pass 2 with no claim."""
    free = np.ones((2, 24), dtype=bool)
    free[:, 2:4] = False
    return hall([(0, 0), (5, 0)], fsp(2, 2.0), free=free)


def higher_claims_nothing():
    """Vehicle 1 stands beside the near target; vehicle 0, far from it, still chooses first and takes it."""
    return hall([(1, 0), (7, 0)], fsp(2, 2.0))


def standing_claim():
    """Vehicle 1 was given the near target by an earlier chooser (skipped, TRAVELING): vehicle 0 flies to the next one."""
    pos = [(1, 0), (3, 1)]
    return hall(pos, fsp(2, 2.0), skip=[0, 1], g_term=_with_term(pos, {1: AT_NEAR}))


def standing_non_peer():
    pos = [(1, 0), (3, 1)]
    return hall(pos, fsp(2, 2.0), view_of=[0, 1], n_views=2, skip=[0, 1], g_term=_with_term(pos, {1: AT_NEAR}))


def standing_reached():
    """want = no_path: vehicle 0 has no path and searches; vehicle 1 is not wanted but GOAL_REACHED: it holds no goal."""
    pos = [(1, 0), (3, 1)]
    return hall(pos, fsp(2, 2.0, want=WANT_NO_PATH), g_term=_with_term(pos, {1: AT_NEAR}), status=[TRAVELING, fm.GOAL_REACHED], stage=[fm.NO_PATH, 0])


def standing_travels():
    """The same with vehicle 1 TRAVELING and not wanted: it claims."""
    pos = [(1, 0), (3, 1)]
    return hall(pos, fsp(2, 2.0, want=WANT_NO_PATH), g_term=_with_term(pos, {1: AT_NEAR}), status=[TRAVELING, TRAVELING], stage=[fm.NO_PATH, 0])


def standing_nan():
    pos = [(1, 0), (3, 1)]
    return hall(pos, fsp(2, 2.0), skip=[0, 1], g_term=_with_term(pos, {1: (AT_NEAR[0], NAN, AT_NEAR[2])}))


def skipped_yawing():
    pos = [(1, 0), (3, 1)]
    return hall(pos, fsp(2, 2.0), skip=[0, -3], g_term=_with_term(pos, {1: AT_NEAR}), status=[TRAVELING, YAWING])


def skipped_reached():
    """A skipped vehicle that is still GOAL_REACHED (the earlier chooser's goal was not applied): no claim."""
    pos = [(1, 0), (3, 1)]
    return hall(pos, fsp(2, 2.0), skip=[0, 1], g_term=_with_term(pos, {1: AT_NEAR}), status=[TRAVELING, fm.GOAL_REACHED])


def radius_edge():
    """r_spread = 1.  Block 4 ends at x = 4.75.  Vehicle 2, the standing peer of vehicle 0, holds x = 5.75: G2 == r_spread^2, kept.  Vehicle
    3, that of vehicle 1 in another view, holds one nextafter less: claimed."""
    pos = [(1, 0), (1, 0), (3, 1), (3, 1)]
    g = _with_term(pos, {2: (5.75, 0.25, 0.25), 3: (np.nextafter(5.75, 0.0), 0.25, 0.25)})
    return hall(pos, fsp(2, 1.0), view_of=[0, 1, 0, 1], n_views=2, skip=[0, 0, 1, 1], g_term=g)


def all_claimed():
    pos = [(1, 0), (3, 1)]
    return hall(pos, fsp(2, 2.0), marks=(NEAR,), skip=[0, 1], g_term=_with_term(pos, {1: AT_NEAR}))


def avoid_and_claim():
    """r_avoid = 1 around vehicle 0's own g_term, which lies in block 4, and a peer's claim on the same block: no target, so not `claimed`."""
    pos = [(1, 0), (3, 1)]
    return hall(pos, fsp(2, 2.0, r_avoid=1.0), skip=[0, 1], g_term=_with_term(pos, {0: AT_NEAR, 1: AT_NEAR}))


def route_through_claim():
    """24 x 1 voxels: the claimed block 4 is the only way to block 8, and the flood walks through it."""
    pos = [(1, 0), (3, 0)]
    return hall(pos, fsp(2, 1.5), skip=[0, 1], g_term=_with_term(pos, {1: AT_NEAR}), free=np.ones((1, 24), dtype=bool))


def gap_not_centre():
    """B = 4: block 2 covers x = 4.25 .. 5.75 and holds the target voxel (11, 0).  A claim at x = 7 with r_spread 1.5: the gap is 1.25, the
    centre of the block 2.0 away."""
    pos = [(1, 0), (3, 1)]
    return hall(pos, fsp(4, 1.5), marks=((11, 0), (20, 0)), skip=[0, 1], g_term=_with_term(pos, {1: (7.0, 0.25, 0.25)}))


def block_not_voxel():
    """The same with the target voxel (8, 0) at x = 4.25, 2.75 from the claim: the block is claimed all the same."""
    pos = [(1, 0), (3, 1)]
    return hall(pos, fsp(4, 1.5), marks=((8, 0), (20, 0)), skip=[0, 1], g_term=_with_term(pos, {1: (7.0, 0.25, 0.25)}))


def _many(n_standing):
    """Vehicle 0 searches; n_standing peers stand with goals far outside the lattice, but for the LAST of them, which holds the near target."""
    pos = [(1, 0)] + [(3, 1)] * n_standing
    terms = {k: (100.0 + k, 0.25, 0.25) for k in range(1, n_standing)}
    terms[n_standing] = AT_NEAR
    return hall(pos, fsp(2, 2.0), skip=[0] + [1] * n_standing, g_term=_with_term(pos, terms))


def _fleet(n):
    """want = no_path.  Searchers (stage NO_PATH) at 0, 64, 256 (if there) and n - 1, all peers: a chain.  Standing peers (TRAVELING) at 63,
    255 and n - 2 with goals on the targets at x = 8, 12 and 16.  Every other vehicle has reached its goal and is not wanted: none."""
    status = np.full(n, fm.GOAL_REACHED, dtype=np.int32)
    stage = np.zeros(n, dtype=np.int32)
    pos = [(1, 0)] * n
    terms = {}
    for k in sorted({0, 64, 256, n - 1}):
        if k < n:
            stage[k] = fm.NO_PATH
            status[k] = TRAVELING
    for k, at in ((63, (8, 0, 0)), (255, (12, 0, 0)), (n - 2, (16, 0, 0))):
        if 0 <= k < n and stage[k] == 0:
            status[k] = TRAVELING
            terms[k] = centre(at)
    marks = ((8, 0), (12, 0), (16, 0), (20, 0), (23, 0), (4, 1), (0, 1))
    return hall(pos, fsp(2, 1.0, want=WANT_NO_PATH), marks=marks, g_term=_with_term(pos, terms), status=status, stage=stage)


def two_words():
    """65 x 2 at B = 1: Cx = 65, two words a row.  Target voxels 63 and 64 in both rows; a claim between them in row 0 with r_spread 0.5
    clears a bit in both words of row 0 and nothing in row 1 (G2 = 0.0625 + 0.25)."""
    pos = [(0, 0), (1, 1)]
    case = fa.floor(np.ones((2, 65), dtype=bool), [[(63, 0), (64, 0), (63, 1), (64, 1)]], pos, fsp(1, 0.5), view_of=[0, 0], skip=[0, 1],
                    g_term=_with_term(pos, {1: (32.0, 0.25, 0.25)}))
    case["group"] = None
    return case


def partial_block():
    """13 x 2 at B = 4: the last block is the voxel column 12 alone, its lo = hi = 6.25.  A claim at x = 8 with r_spread 1.5 is 1.75 away
    (with hi taken as the centre of voxel 15 it would be 0.25).  A second pair in another view with the claim at x = 7.5: claimed."""
    pos = [(9, 0), (9, 0), (3, 1), (3, 1)]
    g = _with_term(pos, {2: (8.0, 0.25, 0.25), 3: (7.5, 0.25, 0.25)})
    case = fa.floor(np.ones((2, 13), dtype=bool), [[(12, 0), (0, 0)]] * 2, pos, fsp(4, 1.5), view_of=[0, 1, 0, 1], skip=[0, 0, 1, 1], g_term=g)
    case["group"] = None
    return case


def claim_outside():
    """A claim below the lattice in x and y: r_spread 3 reaches the blocks 0 and 1 (x up to 1.75), which hold the near target (2, 0)."""
    pos = [(9, 0), (3, 1)]
    return hall(pos, fsp(2, 3.0), marks=((2, 0), (22, 0)), skip=[0, 1], g_term=_with_term(pos, {1: (-1.5, -0.5, 0.25)}))


def block_1():
    return hall([(1, 0), (1, 0)], fsp(1, 2.0))


def block_16():
    """40 x 18 at B = 16: blocks 0, 1 and the partial 2; the pair starts in block 0 and the targets lie in 1 and 2."""
    case = fa.floor(np.ones((18, 40), dtype=bool), [[(20, 3), (39, 17)]], [(0, 0), (0, 0)], fsp(16, 2.0), view_of=[0, 0])
    case["group"] = None
    return case


def cap():
    """64 x 64 x 8 at B = 1: W = 512, every thread owns two words.  All free; unknown voxels in two far corners; a pair in the first voxel."""
    dims = (64, 64, 8)
    view = np.zeros((8, 64, 64), dtype=np.uint8)
    view[7, 63, 63] = view[0, 0, 63] = 1
    case = rm.make_case(dims, [view], [centre((0, 0, 0)), centre((0, 0, 0))], np.zeros((8, 64, 64), dtype=np.uint8), fsp(1, 2.0), view_of=[0, 0])
    case["skip"] = case["group"] = None
    return case


def labels():
    """Three views; the labels join the views 0 and 2 (a negative label) and leave view 1 alone (the largest int32)."""
    return hall([(1, 0), (1, 0), (1, 0)], fsp(2, 2.0), view_of=[0, 1, 2], n_views=3, group=[-7, 2 ** 31 - 1, -7])


def labels_null():
    """The same without labels: three groups."""
    return hall([(1, 0), (1, 0), (1, 0)], fsp(2, 2.0), view_of=[0, 1, 2], n_views=3)


def shared_and_invalid_view():
    """Vehicles 0 and 2 share view 0; vehicle 1 has no view (and claims nothing, though it is skipped and holds the near target); vehicle 3
    reads view 1."""
    pos = [(1, 0), (3, 1), (1, 0), (1, 0)]
    return hall(pos, fsp(2, 2.0), view_of=[0, 5, 0, 1], n_views=2, skip=[0, 1, 0, 0], g_term=_with_term(pos, {1: AT_NEAR}))


def one_vehicle():
    return hall([(1, 0)], fsp(2, 2.0))


CASES = {"pair_one_view": pair_one_view, "pair_two_groups": pair_two_groups, "chain_of_three": chain_of_three, "chain_two_passes": chain_two_passes,
         "lower_finds_nothing": lower_finds_nothing, "higher_claims_nothing": higher_claims_nothing, "standing_claim": standing_claim,
         "standing_non_peer": standing_non_peer, "standing_reached": standing_reached, "standing_travels": standing_travels,
         "standing_nan": standing_nan, "skipped_yawing": skipped_yawing, "skipped_reached": skipped_reached, "radius_edge": radius_edge,
         "all_claimed": all_claimed, "avoid_and_claim": avoid_and_claim, "route_through_claim": route_through_claim,
         "gap_not_centre": gap_not_centre, "block_not_voxel": block_not_voxel, "standing_33": lambda: _many(33), "standing_300": lambda: _many(300),
         "fleet_255": lambda: _fleet(255), "fleet_256": lambda: _fleet(256), "fleet_257": lambda: _fleet(257), "fleet_513": lambda: _fleet(513),
         "two_words": two_words, "partial_block": partial_block, "claim_outside": claim_outside, "block_1": block_1, "block_16": block_16,
         "cap": cap, "labels": labels, "labels_null": labels_null, "shared_and_invalid_view": shared_and_invalid_view, "one_vehicle": one_vehicle}

# the cases named for a claim: their outputs must differ from far_model's on the same inputs
CLAIM_CASES = ("pair_one_view", "chain_of_three", "chain_two_passes", "higher_claims_nothing", "standing_claim", "standing_travels",
               "skipped_yawing", "radius_edge", "all_claimed", "route_through_claim", "gap_not_centre", "block_not_voxel", "standing_33",
               "standing_300", "fleet_255", "fleet_256", "fleet_257", "fleet_513", "two_words", "partial_block", "claim_outside", "block_1",
               "block_16", "cap", "labels")


def model(case, variant=None, par=None):
    return far_spread_goals(case["par"] if par is None else par, case["grid"], case["flags"], case["stride"], case["view_of"], case["n_views"],
                            case["skip"], case["group"], case["vehicles"], case["occ"], case["m_origin"], case["m_res"], variant)


with_gap = rm.with_gap

_BUILT, _MODELS = {}, {}


def case(name):
    """The named case, built once.  Treat it as read-only."""
    if name not in _BUILT:
        _BUILT[name] = CASES[name]()
    return _BUILT[name]


def expected(name):
    """The model's outputs of the named case, computed once.  Treat them as read-only."""
    if name not in _MODELS:
        _MODELS[name] = model(case(name))
    return _MODELS[name]


def has_peers(case):
    """Some searcher of the case has a peer (searching or standing, of any index)."""
    who = judge(case["par"], case["grid"], case["view_of"], case["n_views"], case["skip"], case["group"], case["vehicles"])
    for i, a in enumerate(who):
        if a[2] == SEARCHER and any(k != i and b[2] != NONE and b[3] == a[3] for k, b in enumerate(who)):
            return True
    return False


def random_fleet(seed):
    """A small random fleet in the hall: 2 .. 9 vehicles over 1 .. 3 views with random labels, classes, goals and radii."""
    rng = np.random.default_rng(seed)
    n, n_views = int(rng.integers(2, 10)), int(rng.integers(1, 4))
    pos = [(int(rng.integers(0, 24)), int(rng.integers(0, 2))) for _ in range(n)]
    marks = tuple({(int(rng.integers(0, 24)), int(rng.integers(0, 2))) for _ in range(int(rng.integers(1, 7)))})
    skip = [int(rng.integers(0, 3) == 0) for _ in range(n)]
    terms = {k: centre((int(rng.integers(0, 24)), int(rng.integers(0, 2)), 0)) for k in range(n) if skip[k]}
    status = [int(rng.choice([TRAVELING, fm.GOAL_REACHED, YAWING])) for _ in range(n)]
    par = fsp(int(rng.choice([1, 2, 3, 4])), float(rng.choice([0.5, 1.0, 1.75, 3.0])), passes=16)
    group = None if rng.integers(0, 2) else [int(rng.integers(-1, 2)) for _ in range(n_views)]
    return hall(pos, par, marks=marks, view_of=[int(rng.integers(0, n_views)) for _ in range(n)], n_views=n_views, skip=skip,
                g_term=_with_term(pos, terms), group=group, status=status)
