"""The model of include/fasterhip_stake.h (fh_stake_goals_device) restated in Python over the vehicles in index order, on the pieces of
tests/far_model.py (summary, flood, block_d2, pack), tests/far_spread_model.py (judge: the classes and groups) and tests/far_gain_model.py
(unknown_counts, pack_counts): no passes, no bitmaps, no chunks and no words, so it shares no structure with the kernels.  The covered set
of a searcher is a boolean array over the blocks, the gain a triple loop over the clipped cube that skips covered blocks.  Not a test file.

`variant` names a deliberately WRONG model (VARIANTS): tests/test_far_team_model.py shows that the named cases (CASES) tell every one of
them from the model, so a kernel that made one of these mistakes would not pass tests/test_gpu_far_team.py."""
import numpy as np

from faster_amd import abi

import far_gain_model as fg
import far_model as fa
import far_spread_model as fs
import frontier_model as fm
import reach_model as rm

VARIANTS = ("cover_by_gap",        # a claim covers the blocks whose gap distance from it is below (k - 1) B res + res, not the cube
            "cover_removes",       # a covered block is no target
            "cover_non_peers",     # the goals of vehicles of other groups cover too
            "mask0_covers",        # a lower searching peer that found nothing covers around its g_term
            "standing_no_cover",   # the g_term of a standing peer claims target blocks but covers nothing
            "row_wrap",            # a row of the covered cube is 2 k - 1 consecutive blocks IN MEMORY: it runs into the next row of x
            "union_twice",         # covered and removed are summed per claim: a block that two claims cover counts twice
            "poor_uncovered",      # poor is judged on the gain without the covered set
            "own_block",           # the cube is centred on the vehicle's own block, not on the claim's
            "removed_cube")        # removed = what the covered set takes out of the chosen block's cube, not the sum over the covered set

INF, NAN = fa.INF, fa.NAN
ALL, REACHED = fa.ALL, fa.REACHED
NONE, SEARCHER, STANDING = fs.NONE, fs.SEARCHER, fs.STANDING
UNSETTLED, CLAIMED, ALL_POOR = abi.FH_STAKE_UNSETTLED, abi.FH_STAKE_CLAIMED, abi.FH_STAKE_ALL_POOR
centre = rm.centre


def work_bytes(dims, B, n_views, n):
    pro = fg.work_bytes(dims, B, n_views)
    return 0 if pro == 0 or n < 0 else pro + ((n + 63) & ~63) + 4 * n + 4 * n


def cover_of(shape, cb, k, variant=None):
    """[Cz][Cy][Cx] bool: the blocks b' with |b'_a - cb_a| < k on every axis, clipped; cb = (bx, by, bz)."""
    cz, cy, cx = shape
    out = np.zeros(shape, dtype=bool)
    for dz in range(-k + 1, k):
        for dy in range(-k + 1, k):
            for dx in range(-k + 1, k):
                x, y, z = cb[0] + dx, cb[1] + dy, cb[2] + dz
                if not (0 <= y < cy and 0 <= z < cz):
                    continue
                if variant == "row_wrap":
                    f = (z * cy + y) * cx + x
                    if not 0 <= f < cx * cy * cz:
                        continue
                    x, y, z = f % cx, (f // cx) % cy, f // (cx * cy)
                elif not 0 <= x < cx:
                    continue
                out[z, y, x] = True
    return out


def gain_of(U, b, g, covered):
    """The sum of U over the cube of edge 2 g - 1 blocks around b = (bx, by, bz), clipped, without the covered blocks."""
    cz, cy, cx = U.shape
    total = 0
    for z in range(max(b[2] - g + 1, 0), min(b[2] + g - 1, cz - 1) + 1):
        for y in range(max(b[1] - g + 1, 0), min(b[1] + g - 1, cy - 1) + 1):
            for x in range(max(b[0] - g + 1, 0), min(b[0] + g - 1, cx - 1) + 1):
                if not covered[z, y, x]:
                    total += int(U[z, y, x])
    return total


def far_team_goals(par, grid, flags, view_stride, view_of, n_views, skip, group, vehicles, occ, m_origin, m_res, variant=None):
    """-> (goals [n][3], mask [n] int32, records [n] abi.far_team_record_dtype, sums {view: [4][W] uint64 of the needed views}, need
    [(n_views + 63) & ~63] uint8, counts {view: [64 W] uint16 of the needed views}, cls [n] uint8, grp [n] int32, lower [n] int32): the
    arguments of far_spread_model.far_spread_goals with an abi.far_team_params_dtype record."""
    origin, res, dims = grid
    nx, ny, nz = (int(d) for d in dims)
    B = int(par["block"])
    g, hop_cost, min_gain, k = int(par["gain_blocks"]), int(par["hop_cost"]), int(par["min_gain"]), int(par["claim_blocks"])
    assert 0 <= g <= abi.FH_STAKE_MAX_BLOCKS and 0 <= hop_cost <= abi.FH_STAKE_MAX_HOP_COST and min_gain >= 0
    assert 0 <= k <= abi.FH_STAKE_MAX_CLAIM_BLOCKS
    C, wx, W = fa.blocks_of(dims, B)
    assert W <= abi.FH_STAKE_MAX_WORDS
    n = len(vehicles)
    views = fm.views_of(flags, n_views, view_stride, dims)
    free, qz_of = rm.map_free(grid, occ, m_origin, m_res)
    qx = (np.arange(nx) + 0.5) * float(res) + float(origin[0])
    qy = (np.arange(ny) + 0.5) * float(res) + float(origin[1])
    qz = (np.arange(nz) + 0.5) * float(res) + float(origin[2])
    done, counts = {}, {}
    goals = np.zeros((n, 3), dtype=np.float64)
    mask = np.zeros(n, dtype=np.int32)
    rec = np.zeros(n, dtype=abi.far_team_record_dtype)
    need = np.zeros((n_views + 63) & ~63, dtype=np.uint8)
    max_hops, passes = int(par["max_hops"]), int(par["passes"])
    r_avoid, r_spread = np.float64(par["r_avoid"]), np.float64(par["r_spread"])
    a2, s2 = r_avoid * r_avoid, r_spread * r_spread
    who = fs.judge(par, grid, view_of, n_views, skip, group, vehicles)
    cls = np.array([w[2] for w in who], dtype=np.uint8)
    grp = np.array([w[3] for w in who], dtype=np.int32)
    low_of = np.zeros(n, dtype=np.int32)

    for i in range(n):
        flag, v, c, gr, start = who[i]
        goals[i] = vehicles["g_term"][i]   # (the bits: a copy)
        rec[i] = (flag, v, -1, -1, -1, 0, 0, 0, 0, 0, (0, 0), np.inf, np.inf, gr, 0, 0, 0, 0, 0, (0, 0), -1, 0, 0, -1, 0, 0, (0, 0))
        if c == SEARCHER:
            need[v] = 1
            if v not in done:
                done[v] = fa.summary(views[v], free, qz_of, par, B)
                counts[v] = fg.unknown_counts(views[v], B)

    def block_of_point(c):
        """The block of the voxel of point c, or None where the voxel lies outside the lattice."""
        with np.errstate(all="ignore"):
            s = [np.floor((np.float64(c[a]) - np.float64(origin[a])) / np.float64(res)) for a in range(3)]
        if not all(0.0 <= s[a] < dims[a] for a in range(3)):
            return None
        return tuple(int(x) // B for x in s)

    for i in range(n):
        flag, v, c, gr, start = who[i]
        if c != SEARCHER:
            continue
        p, gt = vehicles["state"]["pos"][i], vehicles["g_term"][i]
        low = [j for j in range(n) if who[j][2] == SEARCHER and j < i and who[j][3] == gr]
        stand = [j for j in range(n) if who[j][2] == STANDING and j != i and who[j][3] == gr]
        rec["lower"][i], rec["standing"][i] = len(low), len(stand)
        low_of[i] = len(low)
        if len(low) >= passes:
            rec["flags"][i] |= UNSETTLED
            rec["decided_pass"][i], rec["claims"][i] = -1, len(stand)
            continue
        rec["decided_pass"][i] = len(low) + 1
        standing_claims = [vehicles["g_term"][j].copy() for j in stand]
        lower_claims = [goals[j].copy() for j in low if mask[j] == 1]
        claims = standing_claims + lower_claims
        rec["claims"][i] = len(claims)
        maps, passable, target = done[v]
        T, U = maps[0], counts[v]
        # ---- the covered set ----
        covering = list(lower_claims) if variant == "standing_no_cover" else list(claims)
        if variant == "mask0_covers":
            covering += [goals[j].copy() for j in low if mask[j] == 0]   # (a decided searcher has no UNSETTLED lower peer: one chain a group)
        if variant == "cover_non_peers":
            for j in range(n):
                if j == i or who[j][2] == NONE or who[j][3] == gr:
                    continue
                if who[j][2] == STANDING:
                    covering.append(vehicles["g_term"][j].copy())
                elif j < i and mask[j] == 1:
                    covering.append(goals[j].copy())
        covered = np.zeros(T.shape, dtype=bool)
        cover_sum, removed_sum = 0, 0
        for c_pt in covering:
            if variant == "cover_by_gap":
                one = np.zeros(T.shape, dtype=bool)
                if k > 0:
                    lim = np.float64((k - 1) * B * float(res) + float(res))
                    for bz in range(T.shape[0]):
                        for by in range(T.shape[1]):
                            for bx in range(T.shape[2]):
                                one[bz, by, bx] = fa.block_d2((bx, by, bz), B, grid, c_pt) < lim * lim
            else:
                cb = block_of_point(c_pt)
                if cb is None:
                    continue
                if variant == "own_block":
                    cb = tuple(s // B for s in start)
                one = cover_of(T.shape, cb, k, variant)
            covered |= one
            cover_sum += int(one.sum())
            removed_sum += int(U[one].sum())
        if variant != "union_twice":
            cover_sum, removed_sum = int(covered.sum()), int(U[covered].sum())
        rec["covered"][i], rec["removed"][i] = cover_sum, removed_sum
        # ---- the target blocks of the vehicle, and the claimed ones among them ----
        mine = np.zeros(T.shape, dtype=bool)
        claimed = np.zeros(T.shape, dtype=bool)
        for bz, by, bx in zip(*np.nonzero(T)):
            b = (int(bx), int(by), int(bz))
            if fa.block_d2(b, B, grid, gt) < a2:
                continue
            if variant == "cover_removes" and covered[bz, by, bx]:
                continue
            mine[bz, by, bx] = True
            for c_pt in claims:
                if fa.block_d2(b, B, grid, c_pt) < s2:
                    claimed[bz, by, bx] = True
                    break
        hops = fa.flood(tuple(s // B for s in start), maps, max_hops)
        open_ = mine & ~claimed
        rec["targets"][i] = int(mine.sum())
        rec["claimed"][i] = int(claimed.sum())
        rec["reachable"][i] = int((open_ & (hops >= 0)).sum())
        rec["reached"][i] = int((hops >= 0).sum())
        rec["levels"][i] = max(int(hops.max()), 0)
        if max_hops > 0 and int(hops.max()) == max_hops:
            rec["flags"][i] |= abi.FH_REACH_CUT
        found = [(int(bx), int(by), int(bz)) for bz, by, bx in zip(*np.nonzero(open_ & (hops >= 0)))]
        nothing = np.zeros(T.shape, dtype=bool)
        keyed, poor, best_gain = [], 0, -1
        for b in found:
            gain = gain_of(U, b, g, covered)
            judged = gain_of(U, b, g, nothing) if variant == "poor_uncovered" else gain
            best_gain = max(best_gain, gain)
            if judged < min_gain:
                poor += 1
                continue
            h = int(hops[b[2], b[1], b[0]])
            D2, idx = fa.block_d2(b, B, grid, p), (b[2] * C[1] + b[1]) * C[0] + b[0]
            utility = gain - hop_cost * h
            keyed.append(((-utility, h, D2, idx), b, D2, h, idx, gain, utility))
        rec["poor"][i], rec["best_gain"][i] = poor, best_gain
        if found and poor == len(found):
            rec["flags"][i] |= ALL_POOR
        if not keyed:
            if rec["claimed"][i] > 0:
                rec["flags"][i] |= CLAIMED
            continue
        _, b, D2, h, idx, gain, utility = min(keyed, key=lambda q: q[0])
        if variant == "removed_cube":
            rec["removed"][i] = gain_of(U, b, g, nothing) - gain
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
        assert best is not None   # (a set bit of T: the block holds a target voxel)
        _, c, d2, (ix, iy, iz) = best
        goals[i] = (qx[ix], qy[iy], qz[iz])
        mask[i] = 1
        rec["flags"][i] |= abi.FH_FRONTIER_FOUND
        rec["cell"][i], rec["block_cell"][i], rec["hops"][i], rec["members"][i], rec["d2"][i], rec["block_d2"][i] = c, idx, h, members, d2, D2
        rec["gain"][i], rec["utility"][i] = gain, utility
    sums = {v: fa.pack(done[v][0], wx) for v in done}
    return goals, mask, rec, sums, need, {v: fg.pack_counts(counts[v], wx) for v in counts}, cls, grp, low_of


# ---- params of this chooser from those of the others, and back ------------------------------------------------------------------------------
_FAR_FIELDS = ("r_avoid", "z_lo", "z_hi", "reserved_d", "want", "max_hops")


def ftp(block, r_spread, gain_blocks, hop_cost=1, min_gain=0, claim_blocks=None, passes=None, r_avoid=0.0, z_lo=-INF, z_hi=INF, want=ALL, max_hops=0):
    p = abi.default_far_team_params(block, r_spread, gain_blocks)
    p["r_avoid"], p["z_lo"], p["z_hi"], p["want"], p["max_hops"] = r_avoid, z_lo, z_hi, want, max_hops
    p["hop_cost"], p["min_gain"] = hop_cost, min_gain
    if claim_blocks is not None:
        p["claim_blocks"] = claim_blocks
    if passes is not None:
        p["passes"] = passes
    return p


def from_gain_params(gp, r_spread=1.0, claim_blocks=None, passes=abi.FH_STAKE_MAX_PASSES):
    """The params of this chooser with the fields of an fh_prospect_params record."""
    p = ftp(int(gp["block"]), r_spread, int(gp["gain_blocks"]), int(gp["hop_cost"]), int(gp["min_gain"]), claim_blocks, passes)
    for f in _FAR_FIELDS:
        p[f] = gp[f]
    return p


def from_spread_params(sp, claim_blocks=0, hop_cost=1):
    """The params under which this chooser is far_spread_model's: gain_blocks 0, hop_cost >= 1, min_gain 0."""
    p = ftp(int(sp["block"]), float(sp["r_spread"]), 0, hop_cost, 0, claim_blocks, int(sp["passes"]))
    for f in _FAR_FIELDS:
        p[f] = sp[f]
    return p


def far_part(par):
    """The fh_far_params of an fh_stake_params record."""
    out = abi.default_far_params(int(par["block"]))
    for f in _FAR_FIELDS:
        out[f] = par[f]
    return out


def gain_part(par):
    """The fh_prospect_params of an fh_stake_params record."""
    out = abi.default_far_gain_params(int(par["block"]), int(par["gain_blocks"]))
    for f in _FAR_FIELDS + ("hop_cost", "min_gain"):
        out[f] = par[f]
    return out


def spread_part(par):
    """The fh_apart_params of an fh_stake_params record."""
    out = abi.default_far_spread_params(int(par["block"]), float(par["r_spread"]))
    for f in _FAR_FIELDS + ("passes",):
        out[f] = par[f]
    return out


def gain_outputs(case, par=None):
    par = case["par"] if par is None else par
    return fg.far_gain_goals(gain_part(par), case["grid"], case["flags"], case["stride"], case["view_of"], case["n_views"], case["skip"],
                             case["vehicles"], case["occ"], case["m_origin"], case["m_res"])


def spread_outputs(case, par=None):
    par = case["par"] if par is None else par
    return fs.far_spread_goals(spread_part(par), case["grid"], case["flags"], case["stride"], case["view_of"], case["n_views"], case["skip"],
                               case.get("group"), case["vehicles"], case["occ"], case["m_origin"], case["m_res"])


# ---- the named cases: the smallest shapes at which the kernels can still go wrong -----------------------------------------------------------
def scene(dims, unknown, positions, par, group=None, status=None, **kw):
    case = fg.scene(dims, unknown, positions, par, **kw)
    case["group"] = None if group is None else np.asarray(group, dtype=np.int32)
    if status is not None:
        case["vehicles"]["status"] = status
    return case


def _term(positions, terms):
    """g_term per vehicle: far away but for the vehicles in `terms` {k: point}."""
    pts = [centre(q) if all(isinstance(c, (int, np.integer)) for c in q) else q for q in positions]
    g = np.asarray(pts, dtype=np.float64) + 1000.0
    for k, t in terms.items():
        g[k] = t
    return g


# TWO HALLS in K23's lattice of 24 x 2 x 2 voxels at B = 2, twelve blocks in a row: the RICH hall is the blocks 8 .. 11 (x >= 16), wholly
# unknown, its edge the target block 7; the POORER hall is block 0 (x < 2), wholly unknown, its edge the target block 1.  The vehicles
# stand in block 4 (x = 8, 9), three steps from either edge.  At g = 3: gain(7) = U(5 .. 9) = 16, gain(1) = U(0 .. 3) = 8.
def _halls_unknown():
    rich = [(x, y, z) for x in range(16, 24) for y in range(2) for z in range(2)]
    poorer = [(x, y, z) for x in range(0, 2) for y in range(2) for z in range(2)]
    return rich + poorer


def halls(par, positions=((8, 0, 0), (9, 0, 0)), extra=(), **kw):
    n = len(positions)
    kw.setdefault("view_of", [0] * n)
    return scene((24, 2, 2), [_halls_unknown() + list(extra)] * (max(kw["view_of"]) + 1 if kw.get("n_views") is None else kw.pop("n_views")),
                 positions, par, **kw)


def two_halls():
    """g = k = 3, hop_cost 1, r_spread 1: vehicle 0 takes the rich hall's edge (block 7, gain 16, three steps, utility 13 against 5); its
    goal, a voxel of block 7, claims that block and covers the blocks 5 .. 9 (removed: U(8) + U(9) = 16), and vehicle 1 takes the poorer
    hall's edge, block 1 with gain 8."""
    return halls(ftp(2, 1.0, 3, 1))


def wide_hall():
    """The same with the rich hall wider than r_spread along its edge: 24 x 6 x 2, both halls three blocks wide in y, the pair in block
    column 5, two steps from the rich hall's edge and four from the poorer one's.  K22's rule parts the pair by r_spread = 1 inside the
    rich hall (another block of its edge); this chooser sends the second to the poorer hall: the first one's goal covers the blocks
    5 .. 9 of all three rows."""
    rich = [(x, y, z) for x in range(16, 24) for y in range(6) for z in range(2)]
    poorer = [(x, y, z) for x in range(0, 2) for y in range(6) for z in range(2)]
    return scene((24, 6, 2), [rich + poorer], [(10, 2, 0), (11, 2, 0)], ftp(2, 1.0, 3, 1), view_of=[0, 0])


def standing_covers():
    """Vehicle 1 stands (skipped, TRAVELING) with its goal in the rich hall's edge: vehicle 0 finds block 7 claimed and the blocks 5 .. 9
    covered, and takes the poorer hall."""
    pos = [(8, 0, 0), (9, 1, 0)]
    return halls(ftp(2, 1.0, 3, 1), pos, skip=[0, 1], g_term=_term(pos, {1: centre((15, 0, 0))}))


def lower_mask0():
    """Vehicle 0 is walled in (x = 6, 7 and x = 10, 11 occupied around its block 4; it stands at 8) and finds nothing: mask 0, and its
    g_term lies in the rich hall's edge.  Vehicle 1, outside the walls at x = 12, has a lower peer that covers nothing."""
    pos = [(8, 0, 0), (12, 0, 0)]
    walls = [(x, y, z) for x in (6, 7, 10, 11) for y in range(2) for z in range(2)]
    return halls(ftp(2, 1.0, 3, 1), pos, occupied=walls, g_term=_term(pos, {0: centre((15, 0, 0))}))


def lower_unsettled():
    """passes = 1: vehicle 1 is UNSETTLED, with its g_term in the poorer hall; vehicle 2 (passes would have to be 3) is UNSETTLED too.
    With passes = 2 (chain_short) vehicle 1 is decided and vehicle 2 is not.  One chain a group: nobody that is decided stands behind an
    UNSETTLED peer, so all the case can show is that an UNSETTLED record carries covered = removed = 0."""
    pos = [(8, 0, 0), (9, 0, 0), (8, 1, 0)]
    return halls(ftp(2, 1.0, 3, 1, passes=1), pos, g_term=_term(pos, {1: centre((3, 0, 0))}))


def chain_short():
    pos = [(8, 0, 0), (9, 0, 0), (8, 1, 0)]
    return halls(ftp(2, 1.0, 3, 1, passes=2), pos, g_term=_term(pos, {1: centre((3, 0, 0))}))


def other_group():
    """Two views with the same content, one vehicle each, and a standing vehicle of view 1 with its goal in the rich hall: vehicle 0 has no
    peer, nothing is covered, both searchers take the rich hall."""
    pos = [(8, 0, 0), (9, 0, 0), (9, 1, 0)]
    return halls(ftp(2, 1.0, 3, 1), pos, view_of=[0, 1, 1], skip=[0, 0, 1], g_term=_term(pos, {2: centre((15, 0, 0))}))


def labels_join():
    """The same with labels that join the two views: one group, a chain of two and a standing peer."""
    pos = [(8, 0, 0), (9, 0, 0), (9, 1, 0)]
    return halls(ftp(2, 1.0, 3, 1), pos, view_of=[0, 1, 1], skip=[0, 0, 1], g_term=_term(pos, {2: centre((15, 0, 0))}), group=[-7, -7])


def claim_outside():
    """The standing peer's goal lies beyond the lattice in x (x = 12.4, the lattice ends at 12.0): its voxel is outside, it covers
    nothing, but with r_spread 1 it still claims block 11 — no target here — and with r_spread 3 the rich hall's edge is out of reach of
    it too; r_spread 5, as here, claims block 7 (gap 12.4 - 7.75 = 4.65)."""
    pos = [(8, 0, 0), (9, 1, 0)]
    return halls(ftp(2, 5.0, 2, 1), pos, skip=[0, 1], g_term=_term(pos, {1: (12.4, 0.25, 0.25)}))


def claim_on_face():
    """A standing peer's goal lies exactly on the plane x = 8.0 (between the blocks 7 and 8: voxel 16, block 8) and on the faces y = 0 and
    z = 0 of the lattice: floor gives the voxel (16, 0, 0), inside, and k = 1 covers block 8 alone.  The goal of a second standing peer
    lies one nextafter below the face y = 0: outside, it covers nothing, and it claims block 1 all the same."""
    pos = [(8, 0, 0), (9, 1, 0), (9, 1, 1)]
    return halls(ftp(2, 0.4, 3, 1, claim_blocks=1), pos, skip=[0, 1, 1],
                 g_term=_term(pos, {1: (8.0, 0.0, 0.0), 2: (1.5, np.nextafter(0.0, -1.0), 0.25)}))


def six_faces():
    """K23's `faces`: 10 x 10 x 10 at B = 2, the shell unknown but for three bars.  Six searchers in the ends of the bars and six standing
    peers whose goals lie in the corner blocks and face blocks of the lattice: every cover cube (k = 2) is clipped, at all six faces."""
    base = fg.case("faces")
    pos = [tuple(base["vehicles"]["state"]["pos"][i]) for i in range(6)]
    goals = [(0, 0, 0), (9, 9, 9), (0, 9, 0), (9, 0, 9), (4, 4, 0), (5, 5, 9)]
    positions = pos + [centre((5, 5, 5))] * 6
    g = _term(positions, {6 + j: centre(q) for j, q in enumerate(goals)})
    return scene((10, 10, 10), [base["views"][0]], positions, ftp(2, 0.4, 2, 1), view_of=[0] * 12, skip=[0] * 6 + [1] * 6, g_term=g)


def word_edge(cx_blocks):
    """B = 2, one row of 65 or 130 blocks (Cx = 65: 130 voxels; Cx = 130: 260 voxels).  All unknown from block 60 on.  A standing peer
    holds a goal in block 63 and another in block 64: their cubes (k = 3) are 61 .. 65 and 62 .. 66, astride the words 0 | 1.  The searcher
    stands at block 50; the target block is 59, whose cube (g = 4) is 56 .. 62."""
    nx = 2 * cx_blocks
    unknown = [(x, 0, 0) for x in range(120, nx)]
    pos = [(100, 0, 0), (101, 0, 0), (102, 0, 0)]
    g = _term(pos, {1: centre((127, 0, 0)), 2: centre((128, 0, 0))})
    return scene((nx, 1, 1), [unknown], pos, ftp(2, 0.4, 4, 1, claim_blocks=3), view_of=[0] * 3, skip=[0, 1, 1], g_term=g)


def row_edge():
    """K23's `row_edge` lattice, 8 x 4 x 1 at B = 2 (two rows of four blocks), g = 2.  A standing peer's goal lies in block (3, 0), the end
    of row 0; k = 2 covers (2, 0), (3, 0), (2, 1), (3, 1) and must not reach block (0, 1), the next in memory, which is wholly unknown: the
    gain of block (0, 0) keeps its 4."""
    unknown = [(0, 2, 0), (1, 2, 0), (0, 3, 0), (1, 3, 0), (7, 0, 0)]
    pos = [(3, 0, 0), (4, 1, 0)]
    return scene((8, 4, 1), [unknown], pos, ftp(2, 0.3, 2, 1), view_of=[0, 0], skip=[0, 1], g_term=_term(pos, {1: centre((6, 1, 0))}),
                 occupied=[(x, 2, 0) for x in range(2, 8)] + [(x, 3, 0) for x in range(2, 8)])


def overlap():
    """Two standing peers with goals in the blocks 8 and 9 of the two halls at k = 2: the cubes 7 .. 9 and 8 .. 10 overlap in two blocks;
    covered = 4, removed = U(7 .. 10) = 24.  The vehicle takes block 1, whose cube holds none of them."""
    pos = [(8, 0, 0), (9, 1, 0), (9, 1, 1)]
    return halls(ftp(2, 0.4, 3, 1, claim_blocks=2), pos, skip=[0, 1, 1], g_term=_term(pos, {1: centre((16, 0, 0)), 2: centre((18, 0, 0))}))


def cover_width(k):
    """A standing peer's goal in block 9 of the two halls, r_spread small: k = 0 covers nothing and the vehicle takes block 7 with gain 16;
    k = 5 covers the blocks 5 .. 11 (clipped: 7 blocks, removed 32) and it takes block 1."""
    pos = [(8, 0, 0), (9, 1, 0)]
    return halls(ftp(2, 0.4, 3, 1, claim_blocks=k), pos, skip=[0, 1], g_term=_term(pos, {1: centre((18, 0, 0))}))


def covered_target():
    """The standing peer's goal lies in block 9, r_spread 0.4, k = 3: block 7, the edge, is covered (7 .. 11) but not claimed (gap 0.75),
    and it stays a target block (targets = reachable = 2): its gain is U(5) + U(6) = 0, utility -3, against the poorer hall's block 1
    at 8 - 3.  With hop_cost 0 and only the rich hall unknown (covered_target_chosen) it is chosen, with gain 0."""
    pos = [(8, 0, 0), (9, 1, 0)]
    return halls(ftp(2, 0.4, 3, 1, claim_blocks=3), pos, skip=[0, 1], g_term=_term(pos, {1: centre((18, 0, 0))}))


def covered_target_chosen():
    rich = [(x, y, z) for x in range(16, 24) for y in range(2) for z in range(2)]
    pos = [(8, 0, 0), (9, 1, 0)]
    return scene((24, 2, 2), [rich], pos, ftp(2, 0.4, 2, 0, claim_blocks=3), view_of=[0, 0], skip=[0, 1],
                 g_term=_term(pos, {1: centre((18, 0, 0))}))


def poor_edge(min_gain):
    """g = 3, k = 1: the standing peer's goal in block 8 covers that block alone, so gain(7) = U(5 .. 9) - U(8) = 16 - 8 = 8.  min_gain 8:
    kept, and chosen before block 1 (equal utility and hops, the vehicle stands at x = 9, nearer to block 7); 9: poor (on the uncovered
    gain, 16, it would be kept), and so is block 1: ALL_POOR."""
    pos = [(9, 0, 0), (9, 1, 0)]
    return halls(ftp(2, 0.2, 3, 1, min_gain=min_gain, claim_blocks=1), pos, skip=[0, 1], g_term=_term(pos, {1: centre((17, 1, 1))}))


def poor_and_claimed():
    """Only the rich hall is unknown; its edge, block 7, is claimed by the standing peer (r_spread 1 around x = 15), and the hole (1, 1, 1)
    makes the blocks 0 and 1 targets of gain 1 < min_gain 2: ALL_POOR and CLAIMED together."""
    rich = [(x, y, z) for x in range(16, 24) for y in range(2) for z in range(2)]
    pos = [(8, 0, 0), (9, 1, 0)]
    return scene((24, 2, 2), [rich + [(1, 1, 1)]], pos, ftp(2, 1.0, 2, 1, min_gain=2), view_of=[0, 0], skip=[0, 1],
                 g_term=_term(pos, {1: centre((15, 0, 0))}))


def many_claims():
    """n = 300: vehicle 0 searches, 299 peers stand; all hold goals far outside but the last two, in the blocks 8 and 9 of the halls: the
    scan takes two chunks, and the claims of the second chunk cover (k = 2: covered 4, removed 24)."""
    n = 300
    pos = [(8, 0, 0)] + [(9, 1, 0)] * (n - 1)
    terms = {j: (100.0 + j, 0.25, 0.25) for j in range(1, n - 2)}
    terms[n - 2], terms[n - 1] = centre((16, 0, 0)), centre((18, 1, 1))
    return halls(ftp(2, 0.4, 3, 1, claim_blocks=2), pos, skip=[0] + [1] * (n - 1), g_term=_term(pos, terms))


def block_1():
    """K23's 9 x 3 x 1 at B = 1: a block is a voxel; a pair."""
    unknown = [(8, y, 0) for y in range(3)] + [(2, 2, 0)]
    return scene((9, 3, 1), [unknown], [(0, 0, 0), (1, 0, 0)], ftp(1, 0.6, 2, 1), view_of=[0, 0])


def block_3():
    """K23's 130 x 2 x 1 at B = 3 (Cx = 44, blocks astride the runs of 64 voxels, a partial last block): a pair and a standing peer."""
    unknown = [(x, 1, 0) for x in range(62, 67)] + [(x, y, 0) for x in range(127, 130) for y in range(2)]
    pos = [(0, 0, 0), (100, 0, 0), (50, 0, 0)]
    return scene((130, 2, 1), [unknown], pos, ftp(3, 1.0, 2, 1), view_of=[0] * 3, skip=[0, 0, 1], g_term=_term(pos, {2: centre((64, 0, 0))}))


def block_16():
    """K23's 48 x 32 x 16 at B = 16: block (1, 0, 0) is wholly unknown, U = 4096; a pair in block (0, 1, 0)."""
    view = np.zeros((16, 32, 48), dtype=np.uint8)
    view[:, :16, 16:32] = 1
    return scene((48, 32, 16), [view], [(2, 20, 3), (3, 20, 3)], ftp(16, 2.0, 2, 64, claim_blocks=1), view_of=[0, 0])


def partial_block():
    """K23's 13 x 7 x 3 at B = 4, the last block along every axis partial, the corner unknown: a pair, the first goal lies in the partial
    blocks."""
    view = np.zeros((3, 7, 13), dtype=np.uint8)
    view[:, 5:, 11:] = 1
    view[:, :2, :2] = 1
    return scene((13, 7, 3), [view], [(6, 3, 1), (7, 3, 1)], ftp(4, 0.6, 2, 1), view_of=[0, 0])


def cap():
    """64 x 64 x 8 at B = 1: W = 512, every thread owns two words of every bitmap.  Two unknown regions in far corners; a pair."""
    view = np.zeros((8, 64, 64), dtype=np.uint8)
    view[5:, 60:, 60:] = 1
    view[0, 8:10, 8:10] = 1
    return scene((64, 64, 8), [view], [(0, 0, 0), (1, 0, 0)], ftp(1, 1.0, 3, 0, claim_blocks=4), view_of=[0, 0])


def not_searched():
    """K23's five kinds of vehicle that are not searched (skipped, not wanted, no view, a NaN position, a start outside), and a pair."""
    par = ftp(2, 1.0, 3, 1, want=REACHED)
    pos = [(8, 0, 0), (8, 0, 0), (8, 0, 0), (0.25, NAN, 0.25), (-3.0, 0.25, 0.25), (8, 0, 0), (9, 0, 0)]
    case = halls(par, pos, view_of=[0, 0, 5, 0, 0, 0, 0], skip=[1, 0, 0, 0, 0, 0, 0], n_views=1)
    case["vehicles"]["status"] = (fm.GOAL_REACHED, 0, fm.GOAL_REACHED, fm.GOAL_REACHED, fm.GOAL_REACHED, fm.GOAL_REACHED, fm.GOAL_REACHED)
    case["vehicles"]["g_term"][3] = (1.0, 1.0, 0.3)
    return case


def fleet_of(n):
    """n searchers of one group in the known part of the two halls: a chain of n, 64 passes."""
    pos = [(6 + i % 8, (i // 8) % 2, (i // 16) % 2) for i in range(n)]
    return halls(ftp(2, 1.0, 3, 1, passes=64), pos)


def unneeded_view():
    """Three views; vehicles 0 and 1 read view 0, vehicle 2 reads view 2; view 1 is needed by nobody."""
    a = np.zeros((2, 2, 24), dtype=np.uint8)
    for x, y, z in _halls_unknown():
        a[z, y, x] = 1
    b = np.ones_like(a)
    c = np.zeros_like(a)
    c[:, :, :2] = 1
    return scene((24, 2, 2), [a, b, c], [(8, 0, 0), (9, 1, 0), (23, 0, 0)], ftp(2, 1.0, 3, 1), view_of=[0, 0, 2])


CASES = {"two_halls": two_halls, "wide_hall": wide_hall, "standing_covers": standing_covers, "lower_mask0": lower_mask0,
         "lower_unsettled": lower_unsettled, "chain_short": chain_short, "other_group": other_group, "labels_join": labels_join,
         "claim_outside": claim_outside, "claim_on_face": claim_on_face, "six_faces": six_faces, "word_edge_65": lambda: word_edge(65),
         "word_edge_130": lambda: word_edge(130), "row_edge": row_edge, "overlap": overlap, "cover_0": lambda: cover_width(0),
         "cover_5": lambda: cover_width(5), "covered_target": covered_target, "covered_target_chosen": covered_target_chosen,
         "min_gain_equal": lambda: poor_edge(8), "min_gain_above": lambda: poor_edge(9), "poor_and_claimed": poor_and_claimed,
         "many_claims": many_claims, "block_1": block_1, "block_3": block_3, "block_16": block_16, "partial_block": partial_block, "cap": cap,
         "not_searched": not_searched, "fleet_1": lambda: fleet_of(1), "fleet_257": lambda: fleet_of(257), "unneeded_view": unneeded_view}


def model(case, variant=None, par=None):
    return far_team_goals(case["par"] if par is None else par, case["grid"], case["flags"], case["stride"], case["view_of"], case["n_views"],
                          case["skip"], case.get("group"), case["vehicles"], case["occ"], case["m_origin"], case["m_res"], variant)


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
    who = fs.judge(case["par"], case["grid"], case["view_of"], case["n_views"], case["skip"], case.get("group"), case["vehicles"])
    for i, a in enumerate(who):
        if a[2] == SEARCHER and any(j != i and b[2] != NONE and b[3] == a[3] for j, b in enumerate(who)):
            return True
    return False


def random_fleet(seed):
    """A small random fleet in a lattice of 24 x 4 x 2 with random unknown boxes: 2 .. 7 vehicles over 1 .. 3 views with random labels,
    classes, goals, radii and widths."""
    rng = np.random.default_rng(seed)
    n, n_views = int(rng.integers(2, 8)), int(rng.integers(1, 4))
    dims = (24, 4, 2)
    views = []
    for _ in range(n_views):
        v = np.zeros((2, 4, 24), dtype=np.uint8)
        for _ in range(int(rng.integers(1, 4))):
            x0, y0 = int(rng.integers(0, 22)), int(rng.integers(0, 4))
            v[int(rng.integers(0, 2)):, y0:y0 + int(rng.integers(1, 4)), x0:x0 + int(rng.integers(1, 8))] = 1
        views.append(v)
    pos = [(int(rng.integers(0, 24)), int(rng.integers(0, 4)), int(rng.integers(0, 2))) for _ in range(n)]
    skip = [int(rng.integers(0, 3) == 0) for _ in range(n)]
    terms = {j: centre((int(rng.integers(0, 24)), int(rng.integers(0, 4)), int(rng.integers(0, 2)))) for j in range(n) if skip[j]}
    status = [int(rng.choice([fs.TRAVELING, fm.GOAL_REACHED, fs.YAWING])) for _ in range(n)]
    B = int(rng.choice([1, 2, 3, 4]))
    par = ftp(B, float(rng.choice([0.5, 1.0, 1.75, 3.0])), int(rng.integers(0, 4)), int(rng.integers(0, 2 * B * B + 1)), int(rng.integers(0, 3)),
              int(rng.integers(0, 4)), passes=16)
    group = None if rng.integers(0, 2) else [int(rng.integers(-1, 2)) for _ in range(n_views)]
    return scene(dims, views, pos, par, group=group, status=status, view_of=[int(rng.integers(0, n_views)) for _ in range(n)], skip=skip,
                 g_term=_term(pos, terms))
