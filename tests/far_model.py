"""The model of include/fasterhip_far.h (fh_far_goals_device) restated in Python, brute force: the summaries by numpy over whole arrays of
voxels, the flood a queue over blocks, one block at a time — no words and no bit tricks in the search, so it shares no structure with the
kernels.  The frontier mask, the wanted rule and the passable voxel are those of tests/frontier_model.py and tests/reach_model.py.  Not a
test file.

`variant` names a deliberately WRONG model (VARIANTS): tests/test_far_model.py shows that the named cases (CASES) tell every one of them
from the model, so a kernel that made one of these mistakes would not pass tests/test_gpu_far.py."""
from collections import deque

import numpy as np

from faster_amd import abi

import frontier_model as fm
import reach_model as rm

VARIANTS = ("links_any_free",     # two neighbouring blocks are linked when both hold a passable voxel
            "one_way",            # a link is followed from the lower block to the upper one only
            "row_wrap",           # the last block of a row of x is linked to the first block of the next row (the voxels next in memory)
            "no_carry",           # no step between the blocks 63 | 64, 127 | 128, ... of a row: no carry between the words
            "full_hi",            # hi of a block is the centre of voxel b B + B - 1, inside the lattice or not
            "centre",             # the distance to the centre of the block, not to the block
            "d2_first",           # the smallest (D2, hops, b)
            "avoid_le",           # E2 <= r_avoid^2 is excluded too
            "avoid_first_voxel",  # E2 is the distance to the first voxel of the block
            "z_ignored",          # T without z_lo <= q.z <= z_hi
            "z_exclusive",        # z_lo < q.z < z_hi
            "start_passable",     # a start that is not passable floods nothing
            "voxel_c")            # in the chosen block the target voxel with the smallest c

INF, NAN = float("inf"), float("nan")
ALL, REACHED = abi.FH_FRONTIER_WANT_ALL, abi.FH_FRONTIER_WANT_REACHED


def blocks_of(dims, B):
    """((Cx, Cy, Cz), wx, W) of a lattice under blocks of edge B."""
    C = tuple(-(-int(n) // B) for n in dims)
    wx = -(-C[0] // 64)
    return C, wx, wx * C[1] * C[2]


def work_bytes(dims, B, n_views):
    if any(int(d) < 1 for d in dims) or not 1 <= B <= 16 or n_views < 1:
        return 0
    W = blocks_of(dims, B)[2]
    return 0 if W > abi.FH_FAR_MAX_WORDS else n_views * 4 * W * 8 + ((n_views + 63) & ~63)


def block_any(a, B):
    """[nz][ny][nx] bool -> [Cz][Cy][Cx] bool: some voxel of the block is set."""
    nz, ny, nx = a.shape
    C = [-(-n // B) for n in (nz, ny, nx)]
    p = np.zeros((C[0] * B, C[1] * B, C[2] * B), dtype=bool)
    p[:nz, :ny, :nx] = a
    return p.reshape(C[0], B, C[1], B, C[2], B).any(axis=(1, 3, 5))


def summary(view, free, qz, par, B, variant=None):
    """(T, LX, LY, LZ), each [Cz][Cy][Cx] bool, and the passable and the target voxels [nz][ny][nx] of one view."""
    passable = (view == 0) & free
    z_lo, z_hi = float(par["z_lo"]), float(par["z_hi"])
    if variant == "z_ignored":
        z_ok = np.ones(qz.shape, dtype=bool)
    elif variant == "z_exclusive":
        z_ok = (z_lo < qz) & (qz < z_hi)
    else:
        z_ok = (z_lo <= qz) & (qz <= z_hi)
    target = passable & fm.frontier_mask(view) & z_ok
    T = block_any(target, B)
    links = []
    for axis in (2, 1, 0):   # x, y, z
        n = view.shape[axis]
        lower = np.take(passable, np.arange(0, n - 1), axis=axis) & np.take(passable, np.arange(1, n), axis=axis)
        pair = np.zeros(view.shape, dtype=bool)   # set at the lower voxel of a passable pair that straddles two blocks
        idx = [slice(None)] * 3
        idx[axis] = slice(0, n - 1)
        pair[tuple(idx)] = lower
        last = (np.arange(n) + 1) % B == 0
        shape = [1, 1, 1]
        shape[axis] = n
        L = block_any(pair & last.reshape(shape), B)
        if variant == "links_any_free":
            has = block_any(passable, B)
            L = np.zeros(has.shape, dtype=bool)
            idx = [slice(None)] * 3
            idx[axis] = slice(0, has.shape[axis] - 1)
            L[tuple(idx)] = np.take(has, np.arange(0, has.shape[axis] - 1), axis=axis) & np.take(has, np.arange(1, has.shape[axis]), axis=axis)
        links.append(L)
    LX, LY, LZ = links
    if variant == "row_wrap":   # the last block of a row and the first of the next: a voxel of the block's last column and the voxel after it in memory
        nz, ny, nx = view.shape
        flat = passable.ravel()
        nxt = np.concatenate([flat[1:], [False]]).reshape(view.shape)
        col = np.zeros(view.shape, dtype=bool)
        col[:, :, nx - 1] = passable[:, :, nx - 1] & nxt[:, :, nx - 1]
        LX = LX | block_any(col, B)
    return (T, LX, LY, LZ), passable, target


def pack(maps, wx):
    """[4][Cz][Cy][Cx] bool -> [4][W] uint64: the bit of b is bit bx & 63 of word (bz Cy + by) wx + (bx >> 6)."""
    out = []
    for m in maps:
        cz, cy, cx = m.shape
        p = np.zeros((cz, cy, wx * 64), dtype=np.uint8)
        p[:, :, :cx] = m
        out.append(np.packbits(p.reshape(-1, 64), axis=1, bitorder="little").reshape(-1).view(np.uint64))
    return np.stack(out)


def gap2(x, first, last, res, o):
    lo, hi = (np.float64(first) + 0.5) * np.float64(res) + np.float64(o), (np.float64(last) + 0.5) * np.float64(res) + np.float64(o)
    x = np.float64(x)
    g = lo - x if x < lo else (x - hi if x > hi else np.float64(0.0))
    return g * g


def block_d2(b, B, grid, point, variant=None):
    """D2 of block b = (bx, by, bz) from `point`: the three squared gaps summed x, y, z."""
    origin, res, dims = grid
    terms = []
    for k in range(3):
        first = b[k] * B
        last = first + B - 1 if variant == "full_hi" else min(first + B, int(dims[k])) - 1
        if variant == "centre":
            lo, hi = (np.float64(first) + 0.5) * res + origin[k], (np.float64(last) + 0.5) * res + origin[k]
            g = np.float64(point[k]) - (lo + hi) / 2
            terms.append(g * g)
        else:
            terms.append(gap2(point[k], first, last, res, origin[k]))
    return (terms[0] + terms[1]) + terms[2]


def flood(start, maps, max_hops, variant=None):
    """hops [Cz][Cy][Cx] int, -1 where the flood does not come: a queue, block by block.  start: (bx, by, bz)."""
    _, LX, LY, LZ = maps
    cz, cy, cx = LX.shape
    hops = np.full(LX.shape, -1, dtype=np.int64)
    hops[start[2], start[1], start[0]] = 0
    queue = deque([start])
    while queue:
        x, y, z = queue.popleft()
        h = int(hops[z, y, x])
        if max_hops > 0 and h >= max_hops:
            continue
        near = []
        if LX[z, y, x] and x + 1 < cx and not (variant == "no_carry" and (x + 1) % 64 == 0):
            near.append((x + 1, y, z))
        if x > 0 and LX[z, y, x - 1] and variant != "one_way" and not (variant == "no_carry" and x % 64 == 0):
            near.append((x - 1, y, z))
        if variant == "row_wrap":
            f = (z * cy + y) * cx + x
            if x == cx - 1 and LX[z, y, x] and f + 1 < cx * cy * cz:
                near.append(((f + 1) % cx, ((f + 1) // cx) % cy, (f + 1) // (cx * cy)))
            if x == 0 and f > 0 and LX.ravel()[f - 1]:
                near.append(((f - 1) % cx, ((f - 1) // cx) % cy, (f - 1) // (cx * cy)))
        if LY[z, y, x] and y + 1 < cy:
            near.append((x, y + 1, z))
        if y > 0 and LY[z, y - 1, x] and variant != "one_way":
            near.append((x, y - 1, z))
        if LZ[z, y, x] and z + 1 < cz:
            near.append((x, y, z + 1))
        if z > 0 and LZ[z - 1, y, x] and variant != "one_way":
            near.append((x, y, z - 1))
        for u, v, w in near:
            if hops[w, v, u] < 0:
                hops[w, v, u] = h + 1
                queue.append((u, v, w))
    return hops


def far_goals(par, grid, flags, view_stride, view_of, n_views, skip, vehicles, occ, m_origin, m_res, variant=None):
    """-> (goals [n][3], mask [n] int32, records [n] abi.far_record_dtype, sums {view: [4][W] uint64 of the needed views}, need
    [(n_views + 63) & ~63] uint8), the arguments of reach_model.reach_goals with an abi.far_params_dtype record and the skip words."""
    origin, res, dims = grid
    nx, ny, nz = (int(d) for d in dims)
    B = int(par["block"])
    C, wx, W = blocks_of(dims, B)
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
    rec = np.zeros(n, dtype=abi.far_record_dtype)
    need = np.zeros((n_views + 63) & ~63, dtype=np.uint8)
    max_hops = int(par["max_hops"])
    r_avoid = np.float64(par["r_avoid"])
    a2 = r_avoid * r_avoid
    for i in range(n):
        v = int(i if view_of is None else view_of[i])
        p, g = vehicles["state"]["pos"][i], vehicles["g_term"][i]
        flag = abi.FH_FRONTIER_WANTED if fm.wanted(int(par["want"]), int(vehicles["status"][i]), int(vehicles["stage"][i])) else 0
        if not 0 <= v < n_views:
            flag |= abi.FH_FRONTIER_NO_VIEW
        if not (np.all(np.isfinite(p)) and np.all(np.isfinite(g))):
            flag |= abi.FH_FRONTIER_BAD_POS
        eligible = flag == abi.FH_FRONTIER_WANTED
        skipped = skip is not None and int(skip[i]) != 0
        if skipped:
            flag |= abi.FH_FAR_SKIPPED
        goals[i] = g   # (the bits: a copy)
        rec[i] = (flag, v, -1, -1, -1, 0, 0, 0, 0, 0, (0, 0), np.inf, np.inf)
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
            done[v] = summary(views[v], free, qz_of, par, B, variant)
        maps, passable, target = done[v]
        T = maps[0]
        # the target blocks of this vehicle
        mine = np.zeros(T.shape, dtype=bool)
        for bz, by, bx in zip(*np.nonzero(T)):
            if variant == "avoid_first_voxel":
                e = [np.float64(g[k]) - ((np.float64((bx, by, bz)[k] * B) + 0.5) * res + origin[k]) for k in range(3)]
                e2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
            else:
                e2 = block_d2((bx, by, bz), B, grid, g, "full_hi" if variant == "full_hi" else None)
            mine[bz, by, bx] = not (e2 <= a2 if variant == "avoid_le" else e2 < a2)
        sb = tuple(c // B for c in start)
        if variant == "start_passable" and not passable[start[2], start[1], start[0]]:
            hops = np.full(T.shape, -1, dtype=np.int64)
        else:
            hops = flood(sb, maps, max_hops, variant)
        rec["targets"][i] = int(mine.sum())
        rec["reachable"][i] = int((mine & (hops >= 0)).sum())
        rec["reached"][i] = int((hops >= 0).sum())
        rec["levels"][i] = max(int(hops.max()), 0)
        if max_hops > 0 and int(hops.max()) == max_hops:
            rec["flags"][i] |= abi.FH_REACH_CUT
        found = [(int(bx), int(by), int(bz)) for bz, by, bx in zip(*np.nonzero(mine & (hops >= 0)))]
        if not found:
            continue
        keyed = []
        for b in found:
            D2, h, idx = block_d2(b, B, grid, p, variant if variant in ("full_hi", "centre") else None), int(hops[b[2], b[1], b[0]]), (b[2] * C[1] + b[1]) * C[0] + b[0]
            keyed.append(((D2, h, idx) if variant == "d2_first" else (h, D2, idx), b, D2, h, idx))
        _, b, D2, h, idx = min(keyed, key=lambda k: k[0])
        best = None
        members = 0
        for iz in range(b[2] * B, min(b[2] * B + B, nz)):
            for iy in range(b[1] * B, min(b[1] * B + B, ny)):
                for ix in range(b[0] * B, min(b[0] * B + B, nx)):
                    if not target[iz, iy, ix]:
                        continue
                    members += 1
                    dx, dy, dz = qx[ix] - p[0], qy[iy] - p[1], qz[iz] - p[2]
                    d2 = (dx * dx + dy * dy) + dz * dz
                    c = (iz * ny + iy) * nx + ix
                    key = (c,) if variant == "voxel_c" else (d2, c)
                    if best is None or key < best[0]:
                        best = (key, c, d2, (ix, iy, iz))
        assert best is not None or variant is not None   # (a set bit of T: the block holds a target voxel)
        if best is None:
            continue
        _, c, d2, (ix, iy, iz) = best
        goals[i] = (qx[ix], qy[iy], qz[iz])
        mask[i] = 1
        rec["flags"][i] |= abi.FH_FRONTIER_FOUND
        rec["cell"][i], rec["block_cell"][i], rec["hops"][i], rec["members"][i], rec["d2"][i], rec["block_d2"][i] = c, idx, h, members, d2, D2
    sums = {v: pack(done[v][0], wx) for v in done}
    return goals, mask, rec, sums, need


# ---- the named cases: the smallest shapes at which the kernels can still go wrong -----------------------------------------------------------
def far_params(block, r_avoid=0.0, z_lo=-INF, z_hi=INF, want=ALL, max_hops=0):
    p = abi.default_far_params(block)
    p["r_avoid"], p["z_lo"], p["z_hi"], p["want"], p["max_hops"] = r_avoid, z_lo, z_hi, want, max_hops
    return p


centre = rm.centre


def floor(free, marks, positions, par, view_of=None, skip=None, g_term=None):
    """A lattice of two layers, res 0.5, origin 0.  Layer 0 is known; its voxel (x, y) is free in the map where free[y][x].  Layer 1 is
    occupied, and in view v unknown exactly above the voxels marks[v]: those voxels of layer 0 (where free) are the target voxels of
    view v, and no other voxel is.  positions: (x, y) voxels of layer 0, or points."""
    free = np.asarray(free, dtype=bool)
    ny, nx = free.shape
    occ = np.zeros((2, ny, nx), dtype=np.uint8)
    occ[0][~free] = 100
    occ[1][:] = 100
    views = []
    for marked in marks:
        view = np.zeros((2, ny, nx), dtype=np.uint8)
        for x, y in marked:
            view[1, y, x] = 1
        views.append(view)
    pts = [centre((q[0], q[1], 0)) if len(q) == 2 else q for q in positions]
    case = rm.make_case((nx, ny, 2), views, pts, occ, par, view_of=view_of, g_term=g_term)
    case["skip"] = None if skip is None else np.asarray(skip, dtype=np.int32)
    return case


def solid(dims, free_voxels, unknown_voxels, positions, par, view_of=None):
    """A lattice that is occupied but for `free_voxels`, known but for `unknown_voxels` (one list per view)."""
    nx, ny, nz = dims
    occ = np.full((nz, ny, nx), 100, dtype=np.uint8)
    for x, y, z in free_voxels:
        occ[z, y, x] = 0
    views = []
    for unknown in unknown_voxels:
        view = np.zeros((nz, ny, nx), dtype=np.uint8)
        for x, y, z in unknown:
            view[z, y, x] = 1
        views.append(view)
    case = rm.make_case(dims, views, [centre(q) if isinstance(q[0], int) else q for q in positions], occ, par, view_of=view_of)
    case["skip"] = None
    return case


def stranded():
    """20 x 4, a known free room; the only target voxel is (19, 1), 18 voxels (9 m) from the vehicle: beyond r_max = 2 of REACH_R."""
    return floor(np.ones((4, 20), dtype=bool), [[(19, 1)]], [(1, 1)], far_params(4))


REACH_R = 2.0   # the r_max with which the voxel flood finds nothing in `stranded`


def detour():
    """10 x 2 at B = 2.  The vehicle in block 2; block 3 holds a target voxel (7, 0) behind a wall (x = 6): no link 2 | 3.  Block 0 holds
    one too, two links away."""
    free = np.ones((2, 10), dtype=bool)
    free[:, 6] = False
    return floor(free, [[(7, 0), (0, 0)]], [(5, 0)], far_params(2))


def diagonal_gap():
    """4 x 2 at B = 2: (0, 0), (1, 0) free in block 0, (2, 1), (3, 1) free in block 1; (1, 0) and (2, 1) touch by an edge only."""
    free = np.zeros((2, 4), dtype=bool)
    free[0, 0] = free[0, 1] = free[1, 2] = free[1, 3] = True
    return floor(free, [[(3, 1)]], [(0, 0)], far_params(2))


def corner_link():
    """5 x 3 x 3 at B = 2: block (0, 1, 1) is one row (y = 2) of one layer (z = 2); its only link is the pair (1, 2, 2) | (2, 2, 2)."""
    return solid((5, 3, 3), [(0, 2, 2), (1, 2, 2), (2, 2, 2), (3, 2, 2)], [[(4, 2, 2)]], [(0, 2, 2)], far_params(2))


def partial_blocks():
    """13 x 7 x 3 at B = 4, all free, one unknown voxel (12, 5, 2): three of its neighbours lie in the last, partial block (3, 1, 0), one
    in block (2, 1, 0).  Vehicle 0 stands in the last voxel of the lattice, beyond the centre of the last voxel along x and y; vehicle 1 at
    the other end."""
    dims = (13, 7, 3)
    view = np.zeros((3, 7, 13), dtype=np.uint8)
    view[2, 5, 12] = 1
    case = rm.make_case(dims, [view], [(6.45, 3.45, 0.75), centre((1, 1, 1))], np.zeros((3, 7, 13), dtype=np.uint8), far_params(4), view_of=[0, 0])
    case["skip"] = None
    return case


def word_carry():
    """65 x 1 at B = 1: a free row.  Vehicle 0 at its first voxel with the target at its last one; vehicle 1 the other way round."""
    return floor(np.ones((1, 65), dtype=bool), [[(64, 0)], [(0, 0)]], [(0, 0), (64, 0)], far_params(1))


def row_end():
    """64 x 2 at B = 1, all occupied but (63, 0) and (0, 1), which follow each other in memory and have no face in common.  Vehicle 0 at
    (63, 0) with the target (0, 1), vehicle 1 the other way round."""
    free = np.zeros((2, 64), dtype=bool)
    free[0, 63] = free[1, 0] = True
    return floor(free, [[(0, 1)], [(63, 0)]], [(63, 0), (0, 1)], far_params(1))


def z_links():
    """2 x 2 x 6 at B = 2, all free: three blocks above each other; the unknown voxel is at the top, the vehicle at the bottom."""
    dims = (2, 2, 6)
    view = np.zeros((6, 2, 2), dtype=np.uint8)
    view[5, 0, 0] = 1
    case = rm.make_case(dims, [view], [centre((0, 0, 0))], np.zeros((6, 2, 2), dtype=np.uint8), far_params(2))
    case["skip"] = None
    return case


def own_block():
    return floor(np.ones((4, 4), dtype=bool), [[(3, 3)]], [(0, 0)], far_params(4))


def start_blocked():
    """6 x 2 at B = 2: the vehicle stands in an occupied voxel; the other three voxels of its block are free."""
    free = np.ones((2, 6), dtype=bool)
    free[0, 0] = False
    return floor(free, [[(5, 0)]], [(0, 0)], far_params(2))


def _open(positions, par, **kw):
    n_views = kw.pop("n_views", len(positions))
    return floor(np.ones((4, 6), dtype=bool), [[(5, 3)]] * n_views, positions, par, **kw)


def start_outside():
    """Vehicle 0 below the lattice in x, vehicle 1 above it in z, vehicle 2 inside."""
    return _open([(-0.2, 1.0, 0.3), (1.0, 1.0, 1.2), (1.1, 1.2, 0.3)], far_params(2))


def no_view():
    return _open([(0, 0), (1, 1), (2, 2)], far_params(2), view_of=[0, 2, -1], n_views=2)


def bad_pos():
    case = _open([(0, 0), (1.0, NAN, 0.3), (2, 2)], far_params(2))
    case["vehicles"]["g_term"][1] = (1.0, 1.0, 0.3)
    case["vehicles"]["g_term"][2] = (INF, 1.0, 0.3)
    return case


def not_wanted():
    """want = reached: vehicle 0 has reached its goal, vehicle 1 travels, vehicle 2 has no path."""
    case = _open([(0, 0), (1, 1), (2, 2)], far_params(2, want=REACHED))
    case["vehicles"]["status"] = (fm.GOAL_REACHED, 0, 0)
    case["vehicles"]["stage"] = (0, 0, fm.NO_PATH)
    return case


def skipped():
    """Vehicles 1 and 2 are skipped; vehicle 2 has a NaN coordinate too, vehicle 3 is outside and not skipped."""
    case = _open([(0, 0), (1, 1), (1.0, NAN, 0.3), (-5.0, 0.0, 0.3)], far_params(2), skip=[0, 7, -1, 0], view_of=[0, 0, 0, 0], n_views=1)
    case["vehicles"]["g_term"][2] = (1.0, 1.0, 0.3)
    return case


def avoid_edge():
    """12 x 2 at B = 2, r_avoid = 1.  The vehicles stand in block 2; block 4 holds a target voxel at a gap of 1.5, block 0 at 2.0, both two
    links away.  g_term of vehicle 0 is exactly 1.0 from block 4 (E2 == r_avoid^2: kept), that of vehicle 1 one nextafter nearer."""
    g = np.array([[5.75, 0.5, 0.5], [np.nextafter(5.75, 0.0), 0.5, 0.5]])
    return floor(np.ones((2, 12), dtype=bool), [[(8, 0), (0, 0)]], [(5, 0), (5, 0)], far_params(2, r_avoid=1.0), view_of=[0, 0], g_term=g)


def z_edges():
    """2 x 1 x 6 at B = 2, z_lo = 0.75 and z_hi = 1.75, the centres of the layers 1 and 3.  Column x = 1 is unknown in the layers 1, 3 and
    5: the frontier voxels are (0, 0, 1 | 3 | 5) and (1, 0, 0 | 2 | 4).  (1, 0, 2) is occupied.  Block 0 has one target voxel, at z_lo;
    block 1 one, at z_hi; the frontier voxels of block 2 all lie above z_hi."""
    dims = (2, 1, 6)
    view = np.zeros((6, 1, 2), dtype=np.uint8)
    view[1, 0, 1] = view[3, 0, 1] = view[5, 0, 1] = 1
    occ = np.zeros((6, 1, 2), dtype=np.uint8)
    occ[2, 0, 1] = 100
    case = rm.make_case(dims, [view], [centre((0, 0, 0)), centre((0, 0, 5))], occ, far_params(2, z_lo=0.75, z_hi=1.75), view_of=[0, 0])
    case["skip"] = None
    return case


def other_lattice():
    """reach_model.other_lattice: a map with another origin and a res that is no multiple of the views', smaller than the lattice."""
    case = dict(rm.case("other_lattice"))
    case["par"] = far_params(4, z_lo=0.6, z_hi=1.4)
    case["skip"] = None
    return case


def ties_hops():
    """reach_model.ties_hops at B = 1: (6, 1) three links away with D2 = 2.25, (3, 3) with D2 = 1 behind a wall, six links away."""
    free = np.ones((5, 8), dtype=bool)
    free[2, 2:5] = False
    return floor(free, [[(6, 1), (3, 3)]], [(3, 1)], far_params(1))


def ties_block_d2():
    """B = 1, two links each: (5, 1) with D2 = 1, (4, 2) with D2 = 0.5, whose index is larger."""
    return floor(np.ones((4, 7), dtype=bool), [[(5, 1), (4, 2)]], [(3, 1)], far_params(1))


def ties_block():
    """10 x 2 at B = 2: the vehicle at x = 2.5 in block 2, the blocks 1 and 3 one link away and both at a gap of 0.75."""
    return floor(np.ones((2, 10), dtype=bool), [[(2, 0), (7, 0)]], [(2.5, 0.25, 0.25)], far_params(2))


def ties_voxel():
    """8 x 4 at B = 4: the vehicle at (1, 2); in block 1 the target voxels (5, 1) and (5, 3) at equal distances, and (7, 0), which is
    farther and has the smallest cell index."""
    return floor(np.ones((4, 8), dtype=bool), [[(5, 1), (5, 3), (7, 0)]], [(1, 2)], far_params(4))


def _max_hops(k):
    """12 x 2 at B = 2: the vehicle in block 0, the target in block 3: level 3."""
    return floor(np.ones((2, 12), dtype=bool), [[(6, 0)]], [(0, 0)], far_params(2, max_hops=k))


def sealed():
    free = np.ones((2, 6), dtype=bool)
    free[:, 2:4] = False
    return floor(free, [[(5, 0)]], [(0, 0)], far_params(2))


def shared_view():
    """Vehicles 0 and 1 read view 0, vehicle 2 reads view 2; view 1 is needed by nobody."""
    return floor(np.ones((4, 9), dtype=bool), [[(8, 3)], [(4, 0)], [(0, 3)]], [(0, 0), (7, 1), (8, 0)], far_params(2), view_of=[0, 0, 2])


def block_1():
    """reach_model.sealed_pocket at B = 1."""
    case = dict(rm.case("sealed_pocket"))
    case["par"] = far_params(1)
    case["skip"] = None
    return case


def block_16():
    return floor(np.ones((18, 20), dtype=bool), [[(19, 17)]], [(0, 0)], far_params(16))


def cap():
    """64 x 64 x 8 at B = 1: W = 512.  All free, one unknown voxel in the far corner."""
    dims = (64, 64, 8)
    view = np.zeros((8, 64, 64), dtype=np.uint8)
    view[7, 63, 63] = 1
    case = rm.make_case(dims, [view], [centre((0, 0, 0))], np.zeros((8, 64, 64), dtype=np.uint8), far_params(1))
    case["skip"] = None
    return case


OVER_CAP = (64, 57, 9)   # W = 513 at B = 1

CASES = {"stranded": stranded, "detour": detour, "diagonal_gap": diagonal_gap, "corner_link": corner_link, "partial_blocks": partial_blocks,
         "word_carry": word_carry, "row_end": row_end, "z_links": z_links, "own_block": own_block, "start_blocked": start_blocked,
         "start_outside": start_outside, "no_view": no_view, "bad_pos": bad_pos, "not_wanted": not_wanted, "skipped": skipped,
         "avoid_edge": avoid_edge, "z_edges": z_edges, "other_lattice": other_lattice, "ties_hops": ties_hops, "ties_block_d2": ties_block_d2,
         "ties_block": ties_block, "ties_voxel": ties_voxel, "max_hops": lambda: _max_hops(3), "max_hops_short": lambda: _max_hops(2),
         "sealed": sealed, "shared_view": shared_view, "block_1": block_1, "block_16": block_16, "cap": cap}


def model(case, variant=None, par=None):
    return far_goals(case["par"] if par is None else par, case["grid"], case["flags"], case["stride"], case["view_of"], case["n_views"],
                     case["skip"], case["vehicles"], case["occ"], case["m_origin"], case["m_res"], variant)


with_gap = rm.with_gap   # the case with the bytes between cells and view_stride set (they are never read)


def reduced(case):
    """(the case at B = 1, the reach_model params of the reduction), or None where the case does not qualify: somebody is skipped, more
    than FH_FAR_MAX_WORDS words at B = 1, or a searched vehicle whose start voxel is not passable."""
    if case["skip"] is not None and np.any(case["skip"] != 0):
        return None
    origin, res, dims = case["grid"]
    if blocks_of(dims, 1)[2] > abi.FH_FAR_MAX_WORDS:
        return None
    par = case["par"].copy()
    par["block"] = 1
    one = dict(case)
    one["par"] = par
    _, _, rec, _, _ = model(one)
    views = fm.views_of(case["flags"], case["n_views"], case["stride"], dims)
    free, _ = rm.map_free(case["grid"], case["occ"], case["m_origin"], case["m_res"])
    searched = np.nonzero((rec["flags"] & ~(abi.FH_FRONTIER_FOUND | abi.FH_REACH_CUT)) == abi.FH_FRONTIER_WANTED)[0]
    for i in searched:
        p = case["vehicles"]["state"]["pos"][i]
        s = [int(np.floor((p[k] - origin[k]) / res)) for k in range(3)]
        v = int(i if case["view_of"] is None else case["view_of"][i])
        if views[v][s[2], s[1], s[0]] != 0 or not free[s[2], s[1], s[0]]:
            return None
    rpar = rm.reach_params(1e6, float(par["r_avoid"]), float(par["z_lo"]), float(par["z_hi"]), int(par["want"]), int(par["max_hops"]))
    return one, rpar


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
