"""The model of include/fasterhip_prospect.h (fh_prospect_goals_device) restated in Python on the pieces of tests/far_model.py (summary,
flood, block_d2, blocks_of): the unknown voxels of a block by reshaping the view, the gain of a block a triple loop over the clipped cube
of blocks, the choice a minimum over every target block of every level.  No words and no bit tricks, so it shares no structure with the
kernels.  Not a test file.

`variant` names a deliberately WRONG model (VARIANTS): tests/test_far_gain_model.py shows that the named cases (CASES) tell every one of
them from the model, so a kernel that made one of these mistakes would not pass tests/test_gpu_far_gain.py."""
import numpy as np

from faster_amd import abi

import far_model as fa
import frontier_model as fm
import reach_model as rm

VARIANTS = ("delta_le",          # the cube takes |b'_a - b_a| <= g: an edge of 2 g + 1 blocks
            "ball",              # a ball of blocks, the squared block distance <= (g - 1)^2, instead of the cube
            "row_wrap",          # a row of the cube is 2 g - 1 consecutive blocks IN MEMORY: it runs from the end of a row of x into the next
            "full_block",        # a partial last block counts the voxels it would have outside the lattice as unknown
            "free_only",         # an unknown voxel whose map cell is occupied is not counted
            "z_filter",          # an unknown voxel outside z_lo <= q.z <= z_hi is not counted
            "poor_le",           # gain <= min_gain is poor
            "d2_first",          # among equal utilities the smallest (D2, hops, b)
            "first_level",       # the choice is confined to the first level that holds a target block, as the chooser without a gain does
            "avoid_removed",     # a block that r_avoid takes out of the targets does not feed the gains of its neighbours either
            "best_gain_rich")    # best_gain leaves the poor blocks out

INF, NAN = fa.INF, fa.NAN
ALL, REACHED = fa.ALL, fa.REACHED
centre = rm.centre


def work_bytes(dims, B, n_views):
    far = fa.work_bytes(dims, B, n_views)
    return 0 if far == 0 else far + n_views * 64 * fa.blocks_of(dims, B)[2] * 2


def unknown_counts(view, B, counted=None, variant=None):
    """[nz][ny][nx] uint8 -> [Cz][Cy][Cx] int: the voxels of each block, inside the lattice, whose flag is not 0."""
    nz, ny, nx = view.shape
    C = [-(-n // B) for n in (nz, ny, nx)]
    p = np.full((C[0] * B, C[1] * B, C[2] * B), variant == "full_block", dtype=bool)
    p[:nz, :ny, :nx] = (view != 0) if counted is None else ((view != 0) & counted)
    return p.reshape(C[0], B, C[1], B, C[2], B).sum(axis=(1, 3, 5)).astype(np.int64)


def gain_of(U, b, g, variant=None, zero=None):
    """The sum of U over the cube of edge 2 g - 1 blocks around b = (bx, by, bz), clipped to the lattice of blocks.  zero: blocks whose
    count is taken as 0 (a wrong variant's)."""
    cz, cy, cx = U.shape
    reach = g if variant == "delta_le" else g - 1
    total = 0
    for dz in range(-reach, reach + 1):
        for dy in range(-reach, reach + 1):
            for dx in range(-reach, reach + 1):
                if variant == "ball" and dx * dx + dy * dy + dz * dz > (g - 1) * (g - 1):
                    continue
                x, y, z = b[0] + dx, b[1] + dy, b[2] + dz
                if not (0 <= y < cy and 0 <= z < cz):
                    continue
                if variant == "row_wrap":
                    f = (z * cy + y) * cx + x
                    if not 0 <= f < cx * cy * cz:
                        continue
                    x, y, z = f % cx, (f // cx) % cy, f // (cx * cy)
                elif not 0 <= x < cx:
                    continue
                if zero is not None and zero[z, y, x]:
                    continue
                total += int(U[z, y, x])
    return total


def pack_counts(U, wx):
    """[Cz][Cy][Cx] -> [64 W] uint16: entry 64 word + bit of the block whose bit of the summary that is; 0 beyond Cx."""
    cz, cy, cx = U.shape
    out = np.zeros((cz, cy, wx * 64), dtype=np.uint16)
    out[:, :, :cx] = U
    return out.reshape(-1)


def far_gain_goals(par, grid, flags, view_stride, view_of, n_views, skip, vehicles, occ, m_origin, m_res, variant=None):
    """-> (goals [n][3], mask [n] int32, records [n] abi.far_gain_record_dtype, sums {view: [4][W] uint64 of the needed views}, need
    [(n_views + 63) & ~63] uint8, counts {view: [64 W] uint16 of the needed views}): the arguments of far_model.far_goals with an
    abi.far_gain_params_dtype record."""
    origin, res, dims = grid
    nx, ny, nz = (int(d) for d in dims)
    B = int(par["block"])
    g, hop_cost, min_gain = int(par["gain_blocks"]), int(par["hop_cost"]), int(par["min_gain"])
    assert 0 <= g <= abi.FH_PROSPECT_MAX_BLOCKS and 0 <= hop_cost <= abi.FH_PROSPECT_MAX_HOP_COST and min_gain >= 0
    C, wx, W = fa.blocks_of(dims, B)
    assert W <= abi.FH_PROSPECT_MAX_WORDS
    n = len(vehicles)
    views = fm.views_of(flags, n_views, view_stride, dims)
    free, qz_of = rm.map_free(grid, occ, m_origin, m_res)
    qx = (np.arange(nx) + 0.5) * float(res) + float(origin[0])
    qy = (np.arange(ny) + 0.5) * float(res) + float(origin[1])
    qz = (np.arange(nz) + 0.5) * float(res) + float(origin[2])
    done, counts = {}, {}
    goals = np.zeros((n, 3), dtype=np.float64)
    mask = np.zeros(n, dtype=np.int32)
    rec = np.zeros(n, dtype=abi.far_gain_record_dtype)
    need = np.zeros((n_views + 63) & ~63, dtype=np.uint8)
    max_hops = int(par["max_hops"])
    r_avoid = np.float64(par["r_avoid"])
    a2 = r_avoid * r_avoid
    counted = None
    if variant == "free_only":
        counted = free
    elif variant == "z_filter":
        counted = np.broadcast_to((float(par["z_lo"]) <= qz_of) & (qz_of <= float(par["z_hi"])), free.shape)
    for i in range(n):
        v = int(i if view_of is None else view_of[i])
        p, gt = vehicles["state"]["pos"][i], vehicles["g_term"][i]
        flag = abi.FH_FRONTIER_WANTED if fm.wanted(int(par["want"]), int(vehicles["status"][i]), int(vehicles["stage"][i])) else 0
        if not 0 <= v < n_views:
            flag |= abi.FH_FRONTIER_NO_VIEW
        if not (np.all(np.isfinite(p)) and np.all(np.isfinite(gt))):
            flag |= abi.FH_FRONTIER_BAD_POS
        eligible = flag == abi.FH_FRONTIER_WANTED
        skipped = skip is not None and int(skip[i]) != 0
        if skipped:
            flag |= abi.FH_PROSPECT_SKIPPED
        goals[i] = gt   # (the bits: a copy)
        rec[i] = (flag, v, -1, -1, -1, 0, 0, 0, 0, 0, (0, 0), np.inf, np.inf, -1, 0, 0, -1)
        if not eligible or skipped:
            continue
        with np.errstate(all="ignore"):
            s = [np.floor((np.float64(p[k]) - np.float64(origin[k])) / np.float64(res)) for k in range(3)]
        if not all(0.0 <= s[k] < dims[k] for k in range(3)):
            rec["flags"][i] |= abi.FH_REACH_START_OUTSIDE
            continue
        start = tuple(int(x) for x in s)
        need[v] = 1
        if v not in done:
            done[v] = fa.summary(views[v], free, qz_of, par, B)
            counts[v] = unknown_counts(views[v], B, counted, variant)
        maps, passable, target = done[v]
        T, U = maps[0], counts[v]
        mine = np.zeros(T.shape, dtype=bool)   # the target blocks of this vehicle
        for bz, by, bx in zip(*np.nonzero(T)):
            mine[bz, by, bx] = not (fa.block_d2((bx, by, bz), B, grid, gt) < a2)
        hops = fa.flood(tuple(c // B for c in start), maps, max_hops)
        rec["targets"][i] = int(mine.sum())
        rec["reachable"][i] = int((mine & (hops >= 0)).sum())
        rec["reached"][i] = int((hops >= 0).sum())
        rec["levels"][i] = max(int(hops.max()), 0)
        if max_hops > 0 and int(hops.max()) == max_hops:
            rec["flags"][i] |= abi.FH_REACH_CUT
        found = [(int(bx), int(by), int(bz)) for bz, by, bx in zip(*np.nonzero(mine & (hops >= 0)))]
        if not found:
            continue
        zero = (T & ~mine) if variant == "avoid_removed" else None
        keyed, poor, best_gain = [], 0, -1
        first = min(int(hops[b[2], b[1], b[0]]) for b in found)
        for b in found:
            gain = gain_of(U, b, g, variant, zero)
            is_poor = gain <= min_gain if variant == "poor_le" else gain < min_gain
            if not (is_poor and variant == "best_gain_rich"):
                best_gain = max(best_gain, gain)
            if is_poor:
                poor += 1
                continue
            h = int(hops[b[2], b[1], b[0]])
            if variant == "first_level" and h != first:
                continue
            D2, idx = fa.block_d2(b, B, grid, p), (b[2] * C[1] + b[1]) * C[0] + b[0]
            utility = gain - hop_cost * h
            keyed.append(((-utility, D2, h, idx) if variant == "d2_first" else (-utility, h, D2, idx), b, D2, h, idx, gain, utility))
        rec["poor"][i], rec["best_gain"][i] = poor, best_gain
        if poor == len(found):
            rec["flags"][i] |= abi.FH_PROSPECT_ALL_POOR
        if not keyed:
            continue
        _, b, D2, h, idx, gain, utility = min(keyed, key=lambda k: k[0])
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
    return goals, mask, rec, sums, need, {v: pack_counts(counts[v], wx) for v in counts}


def far_part(par):
    """The fh_far_params of an fh_prospect_params record: its fields, the three new ones back to reserved zeros."""
    out = abi.default_far_params(int(par["block"]))
    for k in ("r_avoid", "z_lo", "z_hi", "reserved_d", "want", "max_hops"):
        out[k] = par[k]
    return out


def far_outputs(case):
    """What far_model.far_goals gives on the same inputs (no gain)."""
    return fa.far_goals(far_part(case["par"]), case["grid"], case["flags"], case["stride"], case["view_of"], case["n_views"], case["skip"],
                        case["vehicles"], case["occ"], case["m_origin"], case["m_res"])


def reduction_params(far_par, hop_cost=1):
    """The params under which this chooser is far_model's: gain_blocks 0, hop_cost >= 1, min_gain 0."""
    p = abi.default_far_gain_params(int(far_par["block"]), 0)
    for k in ("r_avoid", "z_lo", "z_hi", "reserved_d", "want", "max_hops"):
        p[k] = far_par[k]
    p["hop_cost"], p["min_gain"] = hop_cost, 0
    return p


# ---- the named cases: the smallest shapes at which the kernels can still go wrong -----------------------------------------------------------
def fgp(block, gain_blocks, hop_cost=1, min_gain=0, r_avoid=0.0, z_lo=-INF, z_hi=INF, want=ALL, max_hops=0):
    p = abi.default_far_gain_params(block, gain_blocks)
    p["r_avoid"], p["z_lo"], p["z_hi"], p["want"], p["max_hops"] = r_avoid, z_lo, z_hi, want, max_hops
    p["hop_cost"], p["min_gain"] = hop_cost, min_gain
    return p


def scene(dims, unknown, positions, par, occupied=(), view_of=None, skip=None, g_term=None, n_views=None):
    """A lattice that is free in the map but for the voxels `occupied`, and known but for the voxels `unknown`: one list of (x, y, z) (or
    one bool array [nz][ny][nx]) per view.  positions: voxels (their centres) or points."""
    nx, ny, nz = dims
    occ = np.zeros((nz, ny, nx), dtype=np.uint8)
    for x, y, z in occupied:
        occ[z, y, x] = 100
    views = []
    for u in unknown:
        if isinstance(u, np.ndarray):
            views.append(u.astype(np.uint8))
            continue
        view = np.zeros((nz, ny, nx), dtype=np.uint8)
        for x, y, z in u:
            view[z, y, x] = 1
        views.append(view)
    pts = [centre(q) if all(isinstance(c, (int, np.integer)) for c in q) else q for q in positions]
    case = rm.make_case(dims, views, pts, occ, par, view_of=view_of, g_term=g_term)
    case["skip"] = None if skip is None else np.asarray(skip, dtype=np.int32)
    return case


def _hall(par, positions=((0, 0, 0),), extra=(), **kw):
    """24 x 2 x 2 at B = 2: a row of twelve blocks of eight voxels.  The HOLE is the unknown voxel (3, 1, 1), in block 1: the blocks 1 and
    2 hold target voxels beside it.  The HALL is everything from x = 10 on, the blocks 5 .. 11, wholly unknown: block 4 is its edge.  From
    block 0 the hole's block is one step away and the hall's edge four."""
    unknown = [(3, 1, 1)] + [(x, y, z) for x in range(10, 24) for y in range(2) for z in range(2)] + list(extra)
    return scene((24, 2, 2), [unknown], positions, par, **kw)


def hole_vs_hall(hop_cost=1):
    """g = 3: gain(1) = U(0..3) = 1 and gain(4) = U(2..6) = 16, so utility(1) = 1 - c and utility(4) = 16 - 4 c: the hall wins up to
    c = 4, at c = 5 both are -4 and the fewer hops win, from c = 6 on the hole wins outright."""
    return _hall(fgp(2, 3, hop_cost))


def later_level():
    """g = 2 at hop_cost 1: block 1 (level 1) has utility 1 - 1, block 2 (level 2) 1 - 2, block 4 (level 4) 8 - 4: the best block is in
    the third level that holds a target."""
    return _hall(fgp(2, 2, 1))


def ties_hops():
    """far_model.ties_hops with a second layer, at B = 1 and g = 2, hop_cost 1: 8 x 5 x 2, layer 1 occupied.  The vehicle at (3, 1); the
    target voxel (6, 1) is three links away with D2 = 2.25 and one unknown voxel above it: utility 1 - 3.  The target voxel (3, 3), behind
    the wall y = 2, is six links away with D2 = 1; above it and above the three occupied voxels of the row behind it four voxels are
    unknown: utility 4 - 6.  Equal utilities: the fewer hops win, although D2 and the gain of the other are better."""
    occupied = [(x, y, 1) for x in range(8) for y in range(5)] + [(2, 2, 0), (3, 2, 0), (4, 2, 0), (2, 4, 0), (3, 4, 0), (4, 4, 0)]
    unknown = [(6, 1, 1), (3, 3, 1), (2, 4, 1), (3, 4, 1), (4, 4, 1)]
    return scene((8, 5, 2), [unknown], [(3, 1, 0)], fgp(1, 2, 1), occupied=occupied)


def ties_d2():
    """24 x 2 x 2 at B = 2, g = 1, hop_cost 1: the vehicle at x = 5.6 in block 5; the blocks 3 and 7 hold two unknown voxels each, both
    two steps away: equal utilities and hops; block 7 is nearer (D2), block 3 has the smaller index."""
    unknown = [(6, 0, 0), (6, 1, 0), (15, 0, 0), (15, 1, 0)]
    return scene((24, 2, 2), [unknown], [(5.6, 0.25, 0.25)], fgp(2, 1, 1))


def ties_block():
    """As ties_d2 with the vehicle in the middle of block 5 (x = 5.5): equal utility, hops and D2, the smaller b wins."""
    unknown = [(6, 0, 0), (6, 1, 0), (15, 0, 0), (15, 1, 0)]
    return scene((24, 2, 2), [unknown], [(5.5, 0.25, 0.25)], fgp(2, 1, 1))


def min_gain_edge(min_gain):
    """The hall at g = 2, hop_cost 1: gain(4) = 8, gain(1) = gain(2) = 1.  min_gain 8: block 4 is not poor, the others are; 9: all are."""
    return _hall(fgp(2, 2, 1, min_gain))


def block_alone():
    """g = 1: block 4, the hall's edge, is a target block and knows every one of its own voxels: gain 0, all of it in block 5.  Block 1
    holds the hole itself: gain 1."""
    return _hall(fgp(2, 1, 0))


def widest():
    """g = 5: gain(1) = U(0..5) = 1 + 8, gain(4) = U(0..8) = 1 + 32."""
    return _hall(fgp(2, 5, 1))


def faces():
    """10 x 10 x 10 at B = 2, g = 2: the outer shell of blocks is unknown but for three known bars along the axes, which end in the
    six faces of the lattice; the core is known.  The target blocks at the ends of the bars have cubes that are clipped at x = 0, x = 4,
    y = 0, y = 4, z = 0 and z = 4.  Six vehicles, one in each of those blocks."""
    n = 10
    view = np.ones((n, n, n), dtype=np.uint8)
    view[2:8, 2:8, 2:8] = 0
    view[4:6, 4:6, :] = 0
    view[4:6, :, 4:6] = 0
    view[:, 4:6, 4:6] = 0
    pos = [(0, 4, 4), (9, 5, 5), (4, 0, 4), (5, 9, 5), (4, 4, 0), (5, 5, 9)]
    return scene((n, n, n), [view], pos, fgp(2, 2, 1), view_of=[0] * 6)


def partial_block():
    """13 x 7 x 3 at B = 4: the last block along every axis is partial.  The corner x >= 11, y >= 5 is unknown on all three layers: block
    (3, 1, 0) has 1 x 3 x 3 voxels inside the lattice and counts the 1 x 2 x 3 unknown ones of them, block (2, 1, 0) another 1 x 2 x 3."""
    view = np.zeros((3, 7, 13), dtype=np.uint8)
    view[:, 5:, 11:] = 1
    return scene((13, 7, 3), [view], [(1, 1, 1), (12, 3, 1)], fgp(4, 2, 1), view_of=[0, 0])


def word_edge():
    """130 x 1 x 1 at B = 2: Cx = 65, two words.  Unknown: x = 124 .. 129 (the blocks 62, 63 | 64).  The vehicle at x = 100; the cube of
    the target block 61 at g = 4 is 58 .. 64, astride the words 0 | 1."""
    unknown = [(x, 0, 0) for x in range(124, 130)]
    return scene((130, 1, 1), [unknown], [(100, 0, 0)], fgp(2, 4, 1))


def row_edge():
    """8 x 4 x 1 at B = 2, g = 2: two rows of four blocks.  Block (0, 1), the first of row 1, is wholly unknown; the rest of row 1 is
    occupied.  In row 0 the voxel (7, 0) is unknown: block (3, 0) ends row 0, block (0, 1) follows it in memory, and the cube of (3, 0)
    must not reach there: gain(3, 0) = 1.  Block (0, 0), below the unknown block, has gain 4."""
    unknown = [(0, 2, 0), (1, 2, 0), (0, 3, 0), (1, 3, 0), (7, 0, 0)]
    return scene((8, 4, 1), [unknown], [(3, 0, 0)], fgp(2, 2, 1), occupied=[(x, 2, 0) for x in range(2, 8)] + [(x, 3, 0) for x in range(2, 8)])


def block_3():
    """130 x 2 x 1 at B = 3: Cx = 44 and the blocks 21 (x = 63 .. 65) and 42 (x = 126 .. 128) straddle the runs of 64 voxels; the last
    block (x = 129) is partial.  Unknown: x = 62 .. 66 in row 1, and x >= 127 in both rows."""
    unknown = [(x, 1, 0) for x in range(62, 67)] + [(x, y, 0) for x in range(127, 130) for y in range(2)]
    return scene((130, 2, 1), [unknown], [(0, 0, 0), (100, 0, 0)], fgp(3, 2, 1), view_of=[0, 0])


def block_1():
    """9 x 3 x 1 at B = 1: a block is a voxel, U is the flag itself."""
    unknown = [(8, y, 0) for y in range(3)] + [(2, 2, 0)]
    return scene((9, 3, 1), [unknown], [(0, 0, 0)], fgp(1, 2, 1))


def block_16():
    """48 x 32 x 16 at B = 16: block (1, 0, 0) is wholly unknown, U = 4096; the other five blocks are known and free."""
    view = np.zeros((16, 32, 48), dtype=np.uint8)
    view[:, :16, 16:32] = 1
    return scene((48, 32, 16), [view], [(2, 20, 3)], fgp(16, 2, 64))


def cap():
    """64 x 64 x 8 at B = 1: W = 512.  All free, the far corner column unknown."""
    view = np.zeros((8, 64, 64), dtype=np.uint8)
    view[5:, 63, 63] = 1
    view[0, 10, 10] = 1
    return scene((64, 64, 8), [view], [(0, 0, 0)], fgp(1, 3, 0))


def occupied_unknown():
    """The hall with its unknown voxels from x = 12 on occupied in the map: they count as before."""
    return _hall(fgp(2, 3, 1), occupied=[(x, y, z) for x in range(12, 24) for y in range(2) for z in range(2)])


def outside_z():
    """The hall with z_lo = z_hi = the centre of layer 0: the unknown voxels of layer 1 count as before (the hole lies in layer 1; the
    target voxels are those of layer 0)."""
    return _hall(fgp(2, 3, 1, z_lo=0.25, z_hi=0.25), extra=[(3, 1, 0)])


def avoided_feeds():
    """The hall at g = 2 with a second hole (7, 1, 1) in block 3, beside block 4, and g_term in block 3 with r_avoid 0.3: block 3 is no
    target of the vehicle, but its unknown voxel still counts in gain(4) = U(3) + U(4) + U(5) = 1 + 0 + 8, and in gain(2)."""
    g = np.array([centre((7, 1, 1))])
    return _hall(fgp(2, 2, 1, r_avoid=0.3), extra=[(7, 1, 1)], g_term=g)


def max_hops_cut():
    """The hall at g = 3 with max_hops 3: block 4 (level 4, gain 16) is beyond the cut — not chosen, not in best_gain; FH_REACH_CUT."""
    return _hall(fgp(2, 3, 1, max_hops=3))


def max_hops_poor():
    """max_hops 1 and min_gain 2: block 1 is poor; block 2 (level 2, gain 1) would be, but lies beyond the cut and is not counted."""
    return _hall(fgp(2, 3, 1, min_gain=2, max_hops=1))


def shared_view():
    """Three views of the hall's lattice; vehicles 0 and 1 read view 0, vehicle 2 reads view 2; view 1 is needed by nobody."""
    a = _hall(fgp(2, 3, 1))["views"][0]
    b = np.ones_like(a)
    c = np.zeros_like(a)
    c[:, :, :2] = 1
    return scene((24, 2, 2), [a, b, c], [(0, 0, 0), (9, 1, 0), (23, 0, 0)], fgp(2, 3, 1), view_of=[0, 0, 2])


def not_searched():
    """Skipped, not wanted, no view, a NaN position, a start outside, and one vehicle that is searched."""
    par = fgp(2, 3, 1, want=REACHED)
    case = _hall(par, positions=[(0, 0, 0), (0, 0, 0), (0, 0, 0), (0.25, NAN, 0.25), (-3.0, 0.25, 0.25), (0, 0, 0)], view_of=[0, 0, 5, 0, 0, 0],
                 skip=[1, 0, 0, 0, 0, 0])
    case["vehicles"]["status"] = (fm.GOAL_REACHED, 0, fm.GOAL_REACHED, fm.GOAL_REACHED, fm.GOAL_REACHED, fm.GOAL_REACHED)
    case["vehicles"]["g_term"][3] = (1.0, 1.0, 0.3)
    return case


def fleet_of(n):
    """n vehicles spread along the known part of the hall, one view."""
    pos = [(i % 10, (i // 10) % 2, (i // 20) % 2) for i in range(n)]
    return _hall(fgp(2, 3, 1), positions=pos, view_of=[0] * n)


CASES = {"hole_vs_hall": hole_vs_hall, "break_even_below": lambda: hole_vs_hall(4), "break_even": lambda: hole_vs_hall(5),
         "break_even_above": lambda: hole_vs_hall(6), "later_level": later_level, "ties_hops": ties_hops, "ties_d2": ties_d2,
         "ties_block": ties_block, "min_gain_equal": lambda: min_gain_edge(8), "all_poor": lambda: min_gain_edge(9),
         "no_gain": lambda: _hall(fgp(2, 0, 1)), "block_alone": block_alone, "widest": widest, "faces": faces,
         "partial_block": partial_block, "word_edge": word_edge, "row_edge": row_edge, "block_3": block_3, "block_1": block_1,
         "block_16": block_16, "cap": cap, "occupied_unknown": occupied_unknown, "outside_z": outside_z, "avoided_feeds": avoided_feeds,
         "max_hops_cut": max_hops_cut, "max_hops_poor": max_hops_poor, "shared_view": shared_view, "not_searched": not_searched, "fleet_1": lambda: fleet_of(1),
         "fleet_257": lambda: fleet_of(257)}


def model(case, variant=None, par=None):
    return far_gain_goals(case["par"] if par is None else par, case["grid"], case["flags"], case["stride"], case["view_of"], case["n_views"],
                          case["skip"], case["vehicles"], case["occ"], case["m_origin"], case["m_res"], variant)


with_gap = rm.with_gap   # the case with the bytes between cells and view_stride set (they are never read)

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
