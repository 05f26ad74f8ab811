"""An independent model of the voxel path search (faster_amd/csrc/fh_path.hip.hpp, host/corridor_frontend.cpp: plan_path,
plan_path_jps) in float64: numpy, heapq and scipy.sparse.csgraph.  No quantised keys, no heuristic, no jump rules, no tables: what the
device and the host restatement share by construction is not shared with this file.  One thing is borrowed: the crossing of a leg with the
sphere (single-precision arithmetic of the reference) is the Python restatement oracle/pair_glue.py already has, not a third copy.

Grids are occ[nz][ny][nx] int8 (0 free, 100 occupied) as Map.occupancy() returns them; cells are (x, y, z) integers."""
import heapq
import math

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import dijkstra as _sp_dijkstra

SQ2, SQ3 = math.sqrt(2.0), math.sqrt(3.0)
OFFSETS = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]
HASH = 2654435761
FAR = 1 << 40   # the "cell" of a coordinate no lattice reaches (a non-finite one)


def c_round(v):
    """C's round(): halves away from zero (numpy rounds halves to even).  v - trunc(v) is exact, so the tie test is too."""
    v = np.asarray(v, dtype=np.float64)
    t = np.trunc(v)
    return t + np.where(np.abs(v - t) >= 0.5, np.sign(v), 0.0)


# ---- the lattice ---------------------------------------------------------------------------------------------------------------------------
def geometry(cells, res, center, z_ground, z_max, inflation):
    """MapUtil::readMap's dimensions: x and y widened by int(5 * inflation / res), z clipped to [z_ground, z_max] -> ((nx, ny, nz), origin)"""
    dx, dy, dz = int(cells[0]) + int(5 * inflation / res), int(cells[1]) + int(5 * inflation / res), int(cells[2])
    down = up = int(dz / 2.0)
    if center[2] - res * dz / 2.0 < z_ground:
        down = max(int((center[2] - z_ground) / res), 0)
    if center[2] + res * dz / 2.0 > z_max:
        up = max(int((z_max - center[2]) / res), 1)
    dz = down + up
    origin = np.array([center[0] - res * dx / 2.0, center[1] - res * dy / 2.0, center[2] - res * down])
    return (dx, dy, dz), origin


def cell_of(p, origin, res):
    """MapUtil::floatToInt: (int)round((p - origin) / res - 0.5) per axis; a non-finite coordinate gives a cell outside every lattice"""
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        v = c_round((p - origin) / res - 0.5)
    out = np.where(np.isfinite(v), np.clip(np.nan_to_num(v), -FAR, FAR), -FAR)
    return tuple(int(c) for c in out)


def to_cell(p, origin, res):
    """the cell of a start or a goal: z below zero is clamped first (jps_manager.cpp:143-144); non-finite: outside"""
    p = np.array(p, dtype=np.float64)
    if not np.all(np.isfinite(p)):
        return (-FAR, -FAR, -FAR)
    p[2] = max(p[2], 0.0)
    return cell_of(p, origin, res)


def center_of(c, origin, res):
    return np.array([(c[0] + 0.5) * res + origin[0], (c[1] + 0.5) * res + origin[1], (c[2] + 0.5) * res + origin[2]])


def inside(c, dims):
    return all(0 <= c[k] < dims[k] for k in range(3))


def occupancy(cloud, cells, res, center, z_ground, z_max, inflation):
    """MapUtil::readMap: every point marks its cell (negative cell coordinates clamped to 0) and the cube of +-floor(inflation / res)
    cells around it; a cube cell is taken by its FLAT index (no per-axis clipping: a cube that sticks out in x comes back in on the next
    row); a point with a coordinate that is not finite marks nothing.  The one model of that contract is tests/map_read_model.py.
    -> (occ [nz][ny][nx] int8, dims, origin)"""
    import map_read_model

    return map_read_model.occupancy(cloud, cells, res, center, z_ground, z_max, inflation)


def m_free(inflation, res):
    """setFreeVoxelAndSurroundings(center, const float d): round(float32(inflation) / res + 0.5) cells"""
    return int(c_round(float(np.float32(inflation)) / res + 0.5))


def freed(occ, s, t, m):
    """the grid a query searches: the cubes of +-m cells around the start and the goal cell are free.  MapUtil::setFree takes a cube cell
    by its FLAT index, as readMap does: a cube that sticks out of the lattice in x or y frees cells of the next row or layer."""
    out = occ.copy().ravel()
    nz, ny, nx = occ.shape
    r = np.arange(-m, m + 1)
    ox, oy, oz = (a.ravel() for a in np.meshgrid(r, r, r, indexing="ij"))
    for c in (s, t):
        ids = (c[0] + ox) + nx * (c[1] + oy) + nx * ny * (c[2] + oz)
        out[ids[(ids >= 0) & (ids < out.size)]] = 0
    return out.reshape(occ.shape)


# ---- the search ----------------------------------------------------------------------------------------------------------------------------
_EDGES = {}


def _lattice_edges(shape):
    """every pair of neighbouring cells of the lattice once (half of the 26 offsets), with its step cost"""
    if shape not in _EDGES:
        nz, ny, nx = shape
        ids = np.arange(nx * ny * nz).reshape(nz, ny, nx)
        rows, cols, w = [], [], []
        for dx, dy, dz in OFFSETS:
            if (dz, dy, dx) <= (0, 0, 0):
                continue
            a = (slice(max(-dz, 0), nz - max(dz, 0)), slice(max(-dy, 0), ny - max(dy, 0)), slice(max(-dx, 0), nx - max(dx, 0)))
            b = (slice(max(dz, 0), nz - max(-dz, 0)), slice(max(dy, 0), ny - max(-dy, 0)), slice(max(dx, 0), nx - max(-dx, 0)))
            rows.append(ids[a].ravel())
            cols.append(ids[b].ravel())
            w.append(np.full(rows[-1].size, math.sqrt(dx * dx + dy * dy + dz * dz)))
        _EDGES.clear()   # (one lattice at a time: the big ones are big)
        _EDGES[shape] = (np.concatenate(rows), np.concatenate(cols), np.concatenate(w))
    return _EDGES[shape]


def _graph(free):
    """the 26-connected graph of the free cells, undirected"""
    rows, cols, w = _lattice_edges(free.shape)
    f = free.ravel()
    both = f[rows] & f[cols]
    return coo_matrix((w[both], (rows[both], cols[both])), shape=(f.size, f.size)).tocsr()


def cost_of(a, b, c):
    return a + b * SQ2 + c * SQ3


def dijkstra(occ, s, t, m):
    """Shortest path s -> t on the 26-connected grid with the two cubes freed, Euclidean step costs.
    -> (reachable, cost in cells, (a, b, c) straight / plane-diagonal / space-diagonal moves of an optimal path).
    1, sqrt 2 and sqrt 3 are independent over the rationals, so every optimal path has the same (a, b, c) — and two different triples
    below 4096 moves differ by far more than the rounding of a float64 sum, so the path scipy returns has THE triple; the cost is then
    computed from the triple, not accumulated."""
    nz, ny, nx = occ.shape
    dims = (nx, ny, nz)
    if not inside(s, dims) or not inside(t, dims):
        return False, math.inf, None
    free = freed(occ, s, t, m) == 0
    sid, tid = s[0] + nx * s[1] + nx * ny * s[2], t[0] + nx * t[1] + nx * ny * t[2]
    if sid == tid:
        return True, 0.0, (0, 0, 0)
    dist, pred = tree(free, sid)
    if not np.isfinite(dist[tid]):
        return False, math.inf, None
    counts = moves_along(pred, sid, tid, nx, ny)
    return True, cost_of(*counts), counts


def tree(free, sid):
    """(distance, predecessor) of every cell from cell sid over the free cells [nz][ny][nx] bool"""
    return _sp_dijkstra(_graph(free), directed=False, indices=sid, return_predecessors=True)


def moves_along(pred, sid, tid, nx, ny):
    """(a, b, c) of the tree path sid -> tid"""
    counts = [0, 0, 0]
    i = tid
    while i != sid:
        j = int(pred[i])
        d = abs(i % nx - j % nx) + abs(i // nx % ny - j // nx % ny) + abs(i // (nx * ny) - j // (nx * ny))
        counts[d - 1] += 1
        i = j
    return tuple(counts)


def leg_blocked(grid, origin, res, a, b, first=False):
    """Planner::blocked / VoxelGrid::blocked on the grid a query searches (cubes freed): samples a + (diff / steps) * n, n = 1 .. steps - 1
    with steps = int(max |diff| / res / 0.8); the walk stops at the first sample outside the grid.  first=True: the number of the first
    occupied sample instead (None: not blocked)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nz, ny, nx = grid.shape
    diff = b - a
    steps = int(np.max(np.abs(diff)) / res / 0.8)
    if steps <= 1:
        return None if first else False
    n = np.arange(1, steps, dtype=np.float64)
    pts = a[None, :] + (diff * (1.0 / steps))[None, :] * n[:, None]
    c = c_round((pts - origin) / res - 0.5).astype(np.int64)
    out = (c < 0).any(axis=1) | (c[:, 0] >= nx) | (c[:, 1] >= ny) | (c[:, 2] >= nz)
    stop = int(np.argmax(out)) if out.any() else len(c)
    c = c[:stop]
    hit = grid[c[:, 2], c[:, 1], c[:, 0]] != 0
    if first:
        return int(np.argmax(hit)) + 1 if hit.any() else None
    return bool(hit.any())


def polyline_length(v):
    v = np.asarray(v, dtype=np.float64)
    return float(np.sqrt(((v[1:] - v[:-1]) ** 2).sum(axis=1)).sum())


# ---- the lane-0 epilogue of plan_kernel ----------------------------------------------------------------------------------------------------
def _dist(a, b):
    x, y, z = a[0] - b[0], a[1] - b[1], a[2] - b[2]
    return math.sqrt(x * x + y * y + z * z)


def clip_to_sphere(path, ra):
    """The path up to its first vertex farther than ra (strictly) from the first one, then the crossing point with the sphere; the radius
    as it is (fh_map_plan_batch_radius_device; fh_map_set_sphere passes min(|goal - start| - 0.001, Ra))."""
    from oracle.pair_glue import _sphere_crossing

    path = [np.array(p, dtype=np.float64) for p in path]
    for i in range(1, len(path)):
        if _dist(path[i], path[0]) > ra:
            return path[:i] + [_sphere_crossing(path[i - 1], path[i], ra, path[0])]
    return path


def more_vertexes(path, max_vertex_dist, max_poly=0):
    """Faster::createMoreVertexes: a leg longer than the spacing gets floor(d / spacing) vertices, each one spacing beyond the last (added
    up, not multiplied); a vertex closer than 1e-9 to the last kept one is dropped; then the clip to max_poly + 1 vertices."""
    out = [np.array(path[0], dtype=np.float64)]
    for a, b in zip(path[:-1], path[1:]):
        a, b = np.array(a, dtype=np.float64), np.array(b, dtype=np.float64)
        new = []
        if max_vertex_dist > 0.0:
            d = _dist(b, a)
            if d > max_vertex_dist:
                v, q = (b - a) / d, a.copy()
                for _ in range(int(math.floor(d / max_vertex_dist))):
                    q = q + v * max_vertex_dist
                    new.append(q.copy())
        for p in new + [b]:
            if max_vertex_dist > 0.0 and _dist(p, out[-1]) < 1e-9:
                continue
            out.append(p)
    if max_poly > 0 and len(out) > max_poly + 1:
        out = out[:max_poly + 1]
    return np.array(out)


# ---- an instrument: what the A* open list of the device goes through -----------------------------------------------------------------------------
def sub_of(cell_id):
    return ((cell_id * HASH) & 0xffffffff) >> 24


def astar_open_profile(occ, s, t, m):
    """A* in the device's total order (key int(f * 2^20) with the exact empty-grid distance as heuristic, squared distance to the goal,
    cell index), lazy duplicates as the device keeps them.  Not a reference: it only says which mechanisms of the open list a scene
    reaches.  -> dict(pops: expanded cells, found, peak [256]: the largest size of every sub-list, drained_after_peak [256]: it was empty
    again later, shared_inserts: expansions that put two neighbours into one sub-list, max_open)"""
    nz, ny, nx = occ.shape
    free = (freed(occ, s, t, m) == 0).ravel()
    nxy = nx * ny

    def heur(x, y, z):
        a, b, c = sorted((abs(x - t[0]), abs(y - t[1]), abs(z - t[2])), reverse=True)
        return c * SQ3 + (b - c) * SQ2 + (a - b)

    def h2(x, y, z):
        return (x - t[0]) ** 2 + (y - t[1]) ** 2 + (z - t[2]) ** 2

    sid, tid = s[0] + nx * s[1] + nxy * s[2], t[0] + nx * t[1] + nxy * t[2]
    g = {sid: 0.0}
    closed = set()
    size = [0] * 256
    peak = [0] * 256
    drained = [False] * 256
    heap = [(int(heur(*s) * 1048576.0), h2(*s), sid)]
    size[sub_of(sid)] = peak[sub_of(sid)] = 1
    pops = shared = max_open = 0
    found = False
    steps = [(dx, dy, dz, math.sqrt(dx * dx + dy * dy + dz * dz)) for dx, dy, dz in OFFSETS]
    while heap:
        max_open = max(max_open, len(heap))
        _, _, cur = heapq.heappop(heap)
        sb = sub_of(cur)
        size[sb] -= 1
        if size[sb] == 0 and peak[sb] > 128:
            drained[sb] = True
        if cur in closed:
            continue
        closed.add(cur)
        if cur == tid:
            found = True
            break
        pops += 1
        cz, rem = divmod(cur, nxy)
        cy, cx = divmod(rem, nx)
        gc = g[cur]
        seen = set()
        for dx, dy, dz, w in steps:
            x, y, z = cx + dx, cy + dy, cz + dz
            if x < 0 or y < 0 or z < 0 or x >= nx or y >= ny or z >= nz:
                continue
            i = x + nx * y + nxy * z
            if not free[i] or i in closed:
                continue
            ng = gc + w
            if i in g and not ng < g[i]:
                continue
            g[i] = ng
            heapq.heappush(heap, (int((ng + heur(x, y, z)) * 1048576.0), h2(x, y, z), i))
            sb = sub_of(i)
            size[sb] += 1
            peak[sb] = max(peak[sb], size[sb])
            if sb in seen:
                shared += 1
            seen.add(sb)
    return {"pops": pops, "found": found, "peak": peak, "drained_after_peak": drained, "shared_inserts": shared, "max_open": max_open}
