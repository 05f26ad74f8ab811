"""Scenes for the voxel path search at its jump, list, limit and lattice edges (tests/test_gpu_path_edges.py on the device,
tests/test_path_edge_cases.py on the CPU, where every scene's reason to exist is asserted against tests/path_model.py).

Every scene is an explicit occupancy pattern turned into a cloud of cell-centre points.  The resolution is 0.25 m and every origin a
multiple of it, so cell centres, faces and the lattice arithmetic of readMap are exact in binary: a scene means what it draws.
With inflation 0 readMap marks exactly the pattern and the cubes freed around start and goal are +-1 cell (m_free = 1); with
inflation 0.25 m every point marks its 3 x 3 x 3 cube, the grid is 5 cells wider in x and y, and m_free = 2."""
import functools

import numpy as np

import path_model as pm

RES = 0.25


class Scene:
    """One map and its queries.  pattern: the intended occupancy [nz][ny][nx] bool (inflation 0: readMap marks exactly this)."""

    def __init__(self, name, pattern, starts, goals, inflation=0.0, oz=0.0, **meta):
        nz, ny, nx = pattern.shape
        self.name, self.pattern, self.inflation = name, pattern, inflation
        k = int(5 * inflation / RES)
        down = nz // 2
        self.cells = (nx - k, ny - k, 2 * nz)
        self.center = np.array([RES * nx / 2.0, RES * ny / 2.0, oz + RES * down])
        self.z_ground, self.z_max = oz, oz + RES * nz
        self.dims, self.origin = pm.geometry(self.cells, RES, self.center, self.z_ground, self.z_max, inflation)
        assert self.dims == (nx, ny, nz) and np.array_equal(self.origin, [0.0, 0.0, oz]), (name, self.dims, self.origin)
        z, y, x = np.nonzero(pattern)
        self.cloud = np.column_stack([(x + 0.5) * RES, (y + 0.5) * RES, (z + 0.5) * RES + oz]).reshape(-1, 3)
        self.starts, self.goals = np.asarray(starts, dtype=np.float64).reshape(-1, 3), np.asarray(goals, dtype=np.float64).reshape(-1, 3)
        self.m_free = pm.m_free(inflation, RES)
        self.meta = meta

    def map_args(self):
        return self.cloud, self.cells, RES, self.center, self.z_ground, self.z_max, self.inflation

    @functools.cached_property
    def occ(self):
        return pm.occupancy(*self.map_args())[0]

    def centre(self, c):
        return pm.center_of(c, self.origin, RES)

    def cell(self, p):
        return pm.to_cell(p, self.origin, RES)


def centres(cells_xyz, oz=0.0):
    c = np.asarray(cells_xyz, dtype=np.float64).reshape(-1, 3)
    return (c + 0.5) * RES + np.array([0.0, 0.0, oz])


# ---- the properties of any answer (P1 - P4) ---------------------------------------------------------------------------------------------
_MODEL = {}


def check_answer(sc, q, path, n_points, what, optimal=True, legs=True):
    """What the model gives for the answer to query q of scene sc (max_vertex_dist 0, no sphere, no limit applies): P1 n_points > 0 iff
    the goal is reachable; P2 the first vertex is the start and the last the goal, bit for bit; P3 no leg between interior vertices is
    blocked; P4 the polyline is no longer than res * optimal cost + |start - centre(s)| + |goal - centre(t)| + 1e-9 m (the clean-up only
    ever replaces two legs by a shorter one; the margin covers the rounding of the sums) — what fails if the search is not optimal.
    legs=False: without P3 — a leg that IS the raw path (a diagonal corridor one cell wide) was never tested: its samples sit on cell corners
    and may round into the walls.
    -> the optimal cost in cells, None: unreachable"""
    s, t = sc.cell(sc.starts[q]), sc.cell(sc.goals[q])
    if (sc.name, q) not in _MODEL:   # (the reference is computed once and shared: by the searches, the entry points, the record settings)
        _MODEL[(sc.name, q)] = pm.dijkstra(sc.occ, s, t, sc.m_free)[:2]
    reach, cost = _MODEL[(sc.name, q)]
    assert (n_points > 0) == reach, (what, sc.name, q, s, t, int(n_points), reach)                       # P1
    if not reach:
        return None
    v = path[:n_points]
    st, gl = sc.starts[q].copy(), sc.goals[q].copy()
    st[2], gl[2] = max(st[2], 0.0), max(gl[2], 0.0)
    assert n_points >= 2 and np.array_equal(v[0], st) and np.array_equal(v[-1], gl), (what, sc.name, q, v)   # P2
    grid = pm.freed(sc.occ, s, t, sc.m_free)
    for i in range(1, n_points - 2 if legs else 0):                                                    # P3: legs between interior vertices
        assert not pm.leg_blocked(grid, sc.origin, RES, v[i], v[i + 1]), (what, sc.name, q, i, v)
    if optimal:                                                                                        # P4
        bound = RES * cost + np.linalg.norm(st - sc.centre(s)) + np.linalg.norm(gl - sc.centre(t)) + 1e-9
        length = pm.polyline_length(v)
        assert length <= bound, (what, sc.name, q, s, t, length, bound)
    return cost


# ---- a. exhaustive tiny grids ------------------------------------------------------------------------------------------------------------------
TINY_DIMS = (8, 7, 5)
TINY_NAMES = ["empty/m1", "random/m1", "wall/m1", "empty/m2", "random/m2", "wall/m2"]
TINY_SAMPLE = 2000


def _tiny_pattern(kind, m):
    nx, ny, nz = TINY_DIMS
    p = np.zeros((nz, ny, nx), dtype=bool)
    rng = np.random.default_rng(5)
    if kind == "random":
        if m == 1:
            p[:] = rng.random(p.shape) < 0.25
        else:   # seeds: every one becomes a 3 x 3 x 3 cube (about a quarter of the grid in the end)
            p[rng.integers(0, nz, 5), rng.integers(0, ny, 5), rng.integers(0, nx, 5)] = True
    elif kind == "wall":
        if m == 1:   # the plane x = 5 with one hole, and a one-cell pocket at (2, 3, 2) in a shell two cells thick: the cube freed
            p[:, :, 5] = True           # around a start in the pocket stays closed
            p[2, 5, 5] = False
            p[:, 1:6, 0:5] = True
            p[2, 3, 2] = False
        else:        # seeds in the plane x = 5 except around (y, z) = (5, 2): the cubes leave a hole of one cell there and fill x = 4 .. 6;
            p[:, :, 5] = True   # five seeds two cells from (1, 3, 2) close a pocket around it
            p[1:4, 4:7, 5] = False
            for d in ((2, 0, 0), (0, 2, 0), (0, -2, 0), (0, 0, 2), (0, 0, -2)):
                p[2 + d[2], 3 + d[1], 1 + d[0]] = True
    return p


@functools.lru_cache(maxsize=None)
def tiny_scene(name):
    """all ordered pairs of cell centres of an 8 x 7 x 5 grid, start = goal included: query i * total + j goes from cell i to cell j"""
    kind, m = name.split("/m")
    m = int(m)
    nx, ny, nz = TINY_DIMS
    total = nx * ny * nz
    ids = np.arange(total)
    cells = np.column_stack([ids % nx, ids // nx % ny, ids // (nx * ny)])
    i, j = np.divmod(np.arange(total * total), total)
    return Scene("tiny " + name, _tiny_pattern(kind, m), centres(cells[i]), centres(cells[j]), inflation=0.0 if m == 1 else RES, cells_of=cells)


def tiny_sample(name):
    total = int(np.prod(TINY_DIMS))
    return np.sort(np.random.default_rng(11).choice(total * total, TINY_SAMPLE, replace=False))


def tiny_counts(sc):
    """pairs whose freed cubes overlap, pairs with a cube clipped by the border, pairs whose goal lies on a straight ray from the start"""
    c, m = sc.meta["cells_of"], sc.m_free
    total = len(c)
    i, j = np.divmod(np.arange(total * total), total)
    d = np.abs(c[i] - c[j])
    overlap = (d <= 2 * m).all(axis=1)
    clipped_cell = ((c < m) | (c + m >= np.array(TINY_DIMS))).any(axis=1)
    on_ray = ((d > 0).sum(axis=1) == 1)
    return int(overlap.sum()), int((clipped_cell[i] | clipped_cell[j]).sum()), int(on_ray.sum())


# ---- b. jump lengths at the lane batches -------------------------------------------------------------------------------------------------------
# A straight jump tests 64 ray cells at once, a plane-diagonal jump 32 diagonal cells, a space-diagonal jump 8 — but only where the jump
# table may not be used.  `near`: one occupied cell inside the cube freed around the start, beside the first ray cell (straight) or in
# the cone (diagonal): the boxes matter, tube_contact / cone_dirty say so, and the jump is examined cell by cell from the start, in
# batches.  Without it the same jump comes from the table.
JUMP_START = {1: (2, 6, 6), 2: (2, 2, 1), 3: (2, 2, 2)}
JUMP_DIMS = {1: (140, 12, 12), 2: (80, 80, 4), 3: (24, 24, 24)}
JUMP_DIR = {1: (1, 0, 0), 2: (1, 1, 0), 3: (1, 1, 1)}
JUMP_NEAR = {1: (3, 7, 6), 2: (3, 2, 2), 3: (3, 2, 2)}
JUMP_LENGTHS = {1: (63, 64, 65, 127, 128, 129), 2: (31, 32, 33, 64, 65), 3: (7, 8, 9, 16, 17)}
JUMP_CASES = [(n1, kind, L, near) for n1 in (1, 2, 3) for kind in (("goal", "hole", "blocked", "beside") if n1 == 1 else ("goal", "hole", "blocked"))
              for L in JUMP_LENGTHS[n1] for near in (False, True)]
FREED_TUBE_CASES = [64, 65]


@functools.lru_cache(maxsize=None)
def jump_scene(n1, kind, L, near):
    """A jump of norm-1 n1 from JUMP_START that ends exactly L cells out.
    goal: the goal is the L-th cell of the ray (two vertices, two popped nodes).  hole (straight): the plane x = start + L with one hole
    on the ray — the cells around the hole are the forced neighbours; the goal lies behind the wall off the ray, so the hole is the first
    vertex after the start.  hole (diagonal): the plane one cell behind the L-th diagonal cell, its hole straight ahead (+x) of that
    cell: the diagonal cells before it see only the wall, the L-th one has a straight jump into the hole (forced neighbours all around
    it), so the diagonal jump ends there, and the hole — the only way through — is the first vertex after the start.
    blocked: the whole plane x = start + L, the goal behind it (no path).  beside (straight): one occupied cell beside ray cell L and
    nothing else, the goal on the ray five cells further: a straight ray in free space has a jump point only where an occupied cell lies
    beside it, so the one node popped between start and goal (three popped nodes) is ray cell L — and it stays in the answer as the first vertex after the start."""
    nx, ny, nz = JUMP_DIMS[n1]
    s, d = np.array(JUMP_START[n1]), np.array(JUMP_DIR[n1])
    p = np.zeros((nz, ny, nx), dtype=bool)
    end = s + L * d
    if kind == "goal":
        t = end
    elif kind == "hole" and n1 == 1:
        p[:, :, end[0]] = True
        p[end[2], end[1], end[0]] = False
        t = end + (3, 3, 0)
    elif kind == "hole":
        p[:, :, end[0] + 1] = True
        p[end[2], end[1], end[0] + 1] = False
        t = end + (4, -3, 0)
    elif kind == "blocked":
        p[:, :, end[0]] = True
        t = np.minimum(end + (3, 0, 0), (nx - 1, ny - 1, nz - 1))
    else:
        p[end[2], end[1] + 1, end[0]] = True
        t = end + (5, 0, 0)
    if near:
        c = JUMP_NEAR[n1]
        p[c[2], c[1], c[0]] = True
    return Scene("jump n1=%d %s L=%d%s" % (n1, kind, L, " near" if near else ""), p, centres(s), centres(t), L=L, end=tuple(int(v) for v in end))


@functools.lru_cache(maxsize=None)
def freed_tube_scene(k):
    """One occupied cell beside ray cell k of the straight jump — a forced neighbour on the map as read, so the table says the jump ends k
    cells out — inside the cube freed around the goal: for this query it is free.  tube_contact must hand over to the cell-by-cell
    walk exactly at ray cell k (64: the last cell the table covers is 63; 65: 64)."""
    nx, ny, nz = JUMP_DIMS[1]
    s = np.array(JUMP_START[1])
    p = np.zeros((nz, ny, nx), dtype=bool)
    o = s + (k, 1, 0)
    p[o[2], o[1], o[0]] = True
    t = o + (1, 1, 0)
    return Scene("freed tube k=%d" % k, p, centres(s), centres(t), k=k, obstacle=tuple(int(v) for v in o))


# ---- c. the clean-up in batches ----------------------------------------------------------------------------------------------------------------
RAW_LENGTHS = (63, 64, 65, 128, 129)


@functools.lru_cache(maxsize=None)
def staircase_scene(n_raw):
    """A corridor one cell wide and one layer high that alternates +x and +x+y moves, n_raw cells long, in an otherwise full grid: the
    raw path is the corridor, and its interior cells survive removeLinePts (the direction changes at every cell), so the compaction
    count carries from one pass of 64 lanes to the next."""
    xs = np.arange(n_raw)
    ys = xs // 2
    nx, ny = n_raw + 4, int(ys[-1]) + 5
    p = np.ones((1, ny, nx), dtype=bool)
    p[0, ys + 2, xs + 2] = False
    return Scene("staircase %d" % n_raw, p, centres((2, 2, 0)), centres((xs[-1] + 2, ys[-1] + 2, 0)), n_raw=n_raw)


@functools.lru_cache(maxsize=None)
def straight_raw_scene():
    """a straight raw path of 129 cells in an empty grid: removeLinePts removes all but the ends"""
    return Scene("straight raw 129", np.zeros((1, 3, 140), dtype=bool), centres((4, 1, 0)), centres((4 + 128, 1, 0)), n_raw=129)


# (leg in cells, the sample of the refused shortcut that is the first occupied one): 52 cells are 65 steps — samples 1 .. 64, the last
# lane of the first pass of 64; 80, 81 and 160 cells are 100, 101 and 200 steps — sample 64 ends the first pass, 65 begins the second.
# (81, 64) cannot be built: samples 63 and 64 of a leg of 81 cells along an axis fall into one cell, so 64 is never the first.
# (52, 64) cannot either: sample 64 of 65 steps lies in the cell next to b, and whatever corridor enters b touches the pocket that
# leads up to that cell — the pocket becomes the route.  The leg of 52 cells is refused at sample 40 instead: a ray test of 64 samples,
# every lane of its one pass in use.
LEG_CASES = [(52, 40), (80, 64), (80, 65), (81, 65), (160, 64), (160, 65)]


@functools.lru_cache(maxsize=None)
def leg_scene(L, h):
    """The shortcut removeCornerPts tries is refused by ONE occupied cell, hit first by sample h of the ray test.
    A full grid, one layer.  The path is carved one cell wide: five cells straight from the start to P (so that P is a corner of the
    path, away from the cube freed around the start), then a V: from P diagonally down k1 = ceil(L / 2) cells to the apex A,
    diagonally up k2 = floor(L / 2) cells to b, then six cells straight on to the goal — the only route, and no corner of it can be cut,
    so the raw path is that corridor and removeLinePts leaves P, A and b next to each other.  The shortcut start -> A runs into the walls, P stays and
    becomes the point shortcuts are tried from, and the next one tried is P -> b:
    a leg of L cells.  Every cell its samples visit is carved free — two dead-end pockets, reaching in from P and from b — except the
    cell of sample h: the shortcut is refused there, by the lane that holds sample h, and A stays a vertex.  If the ray test missed that
    sample the shortcut would be taken and A would vanish from the answer."""
    k1, k2 = (L + 1) // 2, L // 2
    x0, y0 = 8, k1 + 3
    nx, ny = L + 19, k1 + 7
    p = np.ones((1, ny, nx), dtype=bool)
    p[0, y0, x0 - 5:x0] = False
    for i in range(k1 + 1):
        p[0, y0 - i, x0 + i] = False
    for j in range(1, k2 + 1):
        p[0, y0 - k1 + j, x0 + k1 + j] = False
    bx, by = x0 + L, y0 - k1 + k2
    p[0, by, bx:bx + 7] = False
    P, b = centres((x0, y0, 0))[0], centres((bx, by, 0))[0]
    steps = int(L / 0.8)
    n = np.arange(1, steps, dtype=np.float64)
    pts = P[None, :] + ((b - P) * (1.0 / steps))[None, :] * n[:, None]
    c = pm.c_round(pts / RES - 0.5).astype(np.int64)
    p[0, c[:, 1], c[:, 0]] = False
    o = tuple(int(v) for v in c[h - 1]) + (0,)
    p[0, o[1], o[0]] = True
    return Scene("leg %d sample %d" % (L, h), p, centres((x0 - 5, y0, 0)), centres((bx + 6, by, 0)), L=L, h=h, steps=steps, P=P, A=centres((x0 + k1, y0 - k1, 0))[0], b=b,
                 obstacle=o)


# ---- d. the A* open list beyond its first chunks --------------------------------------------------------------------------------------------------
COMB_NXY = (26, 421)   # 26 * 421 = 10946, a Fibonacci number
COMB_LEN = 310


@functools.lru_cache(maxsize=None)
def comb_scene():
    """The open list of A* has 256 sub-lists picked by (cell * 2654435761 mod 2^32) >> 24.  A flood of an empty box around a sealed goal,
    the obvious scene, does not get a sub-list past its first chunk at a size that runs quickly: the exact heuristic keeps the
    open list a shell, spread evenly over the sub-lists.  Measured with astar_open_profile on a box of 64 x 64 x 16 cells (start in a
    corner, the goal sealed in the middle): 65 411 expanded cells, at most 9 121 open entries, the largest sub-list 60 entries; more than
    128 in one sub-list need a box of some 250 000 cells and as many pops.  This scene reaches the mechanism in 643 pops instead:
      * 2654435761 / 2^32 is close to the golden ratio's fraction, so a stride of a Fibonacci number of cells moves the hash by almost
        nothing: with nx * ny = 10946 consecutive cells of a z column are 0.0049 sub-lists apart, 203 cells to a sub-list, so a column
        of 310 cells puts at least 155 cells into one sub-list wherever it starts;
      * a corridor C of 310 cells along z, next to it a column S of 310 cells, walls two cells thick around both (the cube freed around
        the start does not open them); the goal lies straight above the corridor, outside the walls: unreachable.  Along C f is constant,
        every S cell has f larger by 0.83, so A* runs up the corridor first and leaves the whole of S open — three chained chunks in one
        sub-list — then pops S from that sub-list until it is empty: the head chunk is released and handed out again;
      * 17 expansions open two cells of one sub-list at once (neighbours one layer apart): they take turns in the claim rounds.
    Query 1 goes from outside the walls to the far corner (reachable).
    The exhaustion of all 2048 chunks (total_new > ftop) needs an open list of about 10^5 entries — millions of pops: out of scope."""
    nx, ny = COMB_NXY
    L = COMB_LEN
    nz = L + 12
    x0, y0, z1 = 10, 200, 4
    p = np.zeros((nz, ny, nx), dtype=bool)
    p[z1 - 2:z1 + L + 2, y0 - 2:y0 + 3, x0 - 2:x0 + 4] = True
    p[z1:z1 + L, y0, x0:x0 + 2] = False
    starts = centres([(x0, y0, z1), (2, 2, 2)])
    goals = centres([(x0, y0, z1 + L + 5), (nx - 3, ny - 3, nz - 3)])
    return Scene("comb", p, starts, goals, column=(x0 + 1, y0, z1, z1 + L))


# ---- e. limits at their boundary -----------------------------------------------------------------------------------------------------------------
KEY_LIMIT = 2040


@functools.lru_cache(maxsize=None)
def key_range_scene(which):
    """The key range of A*: a query ends with -2 as soon as a cell with f >= 2040 cells is opened (include/fasterhip.h).
    end: a map of 2100 x 1 x 1 cells, the start in cell x = 0 — nothing lies behind it, so every opened cell has f = the distance d
    exactly: d = 2039 is a path, d = 2040 ends at the test of the start cell (f = 2040.0: `>` for `>=` would let it through).
    middle: a map of 2100 x 3 x 3 cells, the start in cell (10, 1, 1): the neighbours behind the start are opened with
    f = d + 2 sqrt 3 (one space-diagonal step back, one more to make up for), so d = 2036 is a path and d = 2037 ends at the test in
    the relaxation; d = 2039 and 2040, where only the start cell's own f was thought of, both end there too."""
    if which == "end":
        return Scene("key range end", np.zeros((1, 1, 2100), dtype=bool), centres([(0, 0, 0)] * 2), centres([(2039, 0, 0), (2040, 0, 0)]),
                     limit=[False, True])
    return Scene("key range middle", np.zeros((3, 3, 2100), dtype=bool), centres([(10, 1, 1)] * 4),
                 centres([(10 + d, 1, 1) for d in (2036, 2037, 2039, 2040)]), limit=[False, True, True, True])


MAXRAW = 4096


RAW_START = 2


@functools.lru_cache(maxsize=None)
def raw_limit_scene():
    """MAXRAW bounds the parent chain that finish_path walks back from the goal.  For A* that is a cell per move, and out of reach: 4095
    moves cost more than the 2040 cells of the key range.  For the jump point search it is a jump point per entry, so the scene is a
    corridor one cell wide between two walls (4110 x 3 x 1 cells): every corridor cell has occupied cells beside it, which jps3d takes
    for forced neighbours, so every cell is a jump point and is popped — except the two cells next to the start and the goal, whose
    neighbours lie in the freed cubes.  A goal d cells from the start has d + 1 raw cells in the model and a chain of d - 1 entries:
    queries 1 and 2 have chains of exactly 4096 and 4097 entries (the host restatement's popped-node counts say so), queries 0 and 3 are
    short neighbours whose rows must not be touched by the failing one."""
    p = np.zeros((1, 3, 4110), dtype=bool)
    p[0, 0, :] = p[0, 2, :] = True
    x0 = RAW_START
    return Scene("raw limit", p, centres([(x0, 1, 0)] * 4), centres([(x0 + d, 1, 0) for d in (9, MAXRAW + 1, MAXRAW + 2, 12)]),
                 chain=[8, MAXRAW, MAXRAW + 1, 11])


@functools.lru_cache(maxsize=None)
def max_points_scene():
    """An empty 12 x 5 x 3 grid: query 0 a straight leg of 6 cells (1.5 m: with a spacing of 0.25 m 7 vertices), query 1 start = goal
    (2 vertices), query 2 a leg of 2 cells."""
    return Scene("max points", np.zeros((3, 5, 12), dtype=bool), centres([(2, 2, 1), (4, 2, 1), (2, 3, 1)]), centres([(8, 2, 1), (4, 2, 1), (4, 3, 1)]))


# ---- f. the vertex epilogue -----------------------------------------------------------------------------------------------------------------------
# (max_vertex_dist, what): on the tiny grids, res 0.25: legs between cell centres are multiples of 0.25 m along an axis
SPACINGS = [(0.25, "legs of 0.5, 0.75 ... m are exact multiples: the 1e-9 duplicate rule"), (0.5, "legs of 1.0 and 1.5 m are exact multiples"),
            (0.6, "no axis leg is a multiple"), (100.0, "larger than every leg: nothing is added")]


# ---- g. the lattice faces and bad numbers -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lattice_scene():
    """An empty 8 x 7 x 5 grid whose origin is (0, 0, -0.5): starts (the goal is the centre of cell (4, 3, 2)) and goals (the start is that
    centre) exactly on the low and the high face of the lattice along each axis, one ulp inside and one ulp outside; on the interior
    cell borders (ties of round); z below zero (clamped to 0: cell z = 2); -0.0; and non-finite coordinates."""
    nx, ny, nz = TINY_DIMS
    oz = -0.5
    mid = centres((4, 3, 2), oz)[0]
    pts, kinds = [], []
    lo, hi = np.array([0.0, 0.0, oz]), np.array([nx * RES, ny * RES, oz + nz * RES])
    for k in range(3):
        for face in (lo[k], hi[k]):
            for v in (face, np.nextafter(face, -np.inf), np.nextafter(face, np.inf)):
                if k == 2 and v < 0.0:
                    continue   # (clamped to 0: listed below)
                p = mid.copy()
                p[k] = v
                pts.append(p)
                kinds.append("face")
        for border in (1, 2, 3):
            for v in (lo[k] + border * RES, np.nextafter(lo[k] + border * RES, -np.inf)):
                p = mid.copy()
                p[k] = v
                pts.append(p)
                kinds.append("border")
    for z in (-0.0, -1e-300, -0.3, -1e300):
        pts.append(np.array([mid[0], mid[1], z]))
        kinds.append("clamped")
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(3):
            p = mid.copy()
            p[k] = bad
            pts.append(p)
            kinds.append("nonfinite")
        pts.append(np.full(3, bad))
        kinds.append("nonfinite")
    pts = np.array(pts)
    n = len(pts)
    starts = np.vstack([pts, np.tile(mid, (n, 1))])
    goals = np.vstack([np.tile(mid, (n, 1)), pts])
    return Scene("lattice", np.zeros((nz, ny, nx), dtype=bool), starts, goals, oz=oz, kinds=kinds + kinds, mid=mid)
