"""The scene and the hand cases of the radio link with a line of sight (include/fasterhip_link_los.h), shared by
tests/test_link_los_model.py (the model on the CPU) and tests/test_gpu_link_los.py (every byte of the device against the model).  Not a
test file.

THE SCENE.  A map of 20 x 20 x 10 cells of 0.2 m, x and y in [-2, 2), z in [0, 2): the origin (-2, -2, 0) is exact, so the cell
boundaries are the doubles nearest to the multiples of 0.2 and a sample that lands on one can fall to either side of it.  A cloud of points
at cell centres builds a wall across the whole map at x cell 10 with a gap of three cells at y cells 13 .. 15, and a pillar at cell (2, 2);
both over all z.  The map inflates by one cell, so the occupied cells are: the wall, x cells 9 .. 11 (x in [-0.2, 0.4)) except the door,
y cell 14 (y in [0.8, 1.0)), one cell wide; and the pillar, x and y cells 1 .. 3 (x and y in [-1.8, -1.2))."""
import numpy as np

import link_model as lm

RES = 0.2
READ = dict(cells=(15, 15, 10), res=RES, center=(0.0, 0.0, 1.0), z_ground=-1.0, z_max=5.0, inflation=0.2)   # 15 + int(5 * 0.2 / 0.2) = 20
DIMS = (20, 20, 10)
ORIGIN = (-2.0, -2.0, 0.0)


def centre(ix, iy, iz):
    return ((ix + 0.5) * RES + ORIGIN[0], (iy + 0.5) * RES + ORIGIN[1], (iz + 0.5) * RES + ORIGIN[2])


def cloud():
    pts = [centre(10, iy, iz) for iy in range(20) if iy not in (13, 14, 15) for iz in range(10)]
    pts += [centre(2, 2, iz) for iz in range(10)]
    return np.array(pts, dtype=np.float64)


def expected_occupancy():
    """[10][20][20] int8, 0 free / 100 occupied: what the docstring says the map holds."""
    occ = np.zeros((10, 20, 20), dtype=np.int8)
    occ[:, :, 9:12] = 100
    occ[:, 14, 9:12] = 0
    occ[:, 1:4, 1:4] = 100
    return occ


NAN, INF = float("nan"), float("inf")

# name -> (positions, view_of or None, n_views, range, passes, labels, info): labels and info are what the model must give, written by hand
CASES = {
    # A and B at one height on either side of the wall, 2 m apart
    "across_the_wall": ([(-1.0, -1.0, 0.5), (1.0, -1.0, 0.5)], None, 2, 3.0, 4, [0, 1], [0, 2, 0, 1]),
    "on_one_side": ([(-1.0, -1.0, 0.5), (-1.5, 0.3, 0.7)], None, 2, 3.0, 4, [0, 0], [0, 1, 1, 0]),
    # along y = 0.9, the middle of the door; and to y = 1.07 on the far side: the ray rises past y = 1.0 (y cell 15) at x = 0.18, so of
    # the wall's three x cells it meets an occupied one only in the last, x cell 11
    "through_the_door": ([(-1.0, 0.9, 0.5), (1.0, 0.9, 0.5)], None, 2, 3.0, 4, [0, 0], [0, 1, 1, 0]),
    "clips_the_jamb": ([(-1.0, 0.9, 0.5), (1.0, 1.07, 0.5)], None, 2, 3.0, 4, [0, 1], [0, 2, 0, 1]),
    # vehicle 0 stands in the wall's inflated x cell 9; the samples in its own cell are not tested and the rest of the ray is free
    "inside_an_inflated_cell": ([(-0.1, -1.0, 0.5), (-1.0, -1.0, 0.5)], None, 2, 3.0, 4, [0, 0], [0, 1, 1, 0]),
    # ... and so is the far end's cell (vehicle 1 in the wall): q's cell is exempt as p's is
    "far_end_inside_an_inflated_cell": ([(-1.0, -1.0, 0.5), (-0.1, -1.0, 0.5)], None, 2, 3.0, 4, [0, 0], [0, 1, 1, 0]),
    # both in the occupied cell (10, 4, 2): K = 2, the one sample is in the ends' cell
    "two_in_one_cell": ([(0.05, -1.05, 0.5), (0.15, -1.12, 0.5)], None, 2, 3.0, 4, [0, 0], [0, 1, 1, 0]),
    # 0.04 m apart in two occupied cells (x cells 10 and 11): K = 1, no sample at all
    "nearer_than_half_a_cell": ([(0.18, -1.0, 0.5), (0.22, -1.0, 0.5)], None, 2, 3.0, 4, [0, 0], [0, 1, 1, 0]),
    # (a straight ray cannot leave a box and come back into it: the three ways a ray meets the outside)  0 - 1: both ends above the map, over
    # the wall: every sample is outside, free.  2 - 3: from above the map on one side down into it and through the wall: outside, then
    # inside and blocked there.  4 - 5: from outside the map in y to inside, free all the way.  The three pairs are out of each other's
    # range (1.8).
    "outside_the_map": ([(-0.4, -1.0, 2.3), (0.6, -1.0, 2.3), (-0.4, 1.8, 2.3), (0.6, 1.8, 1.5), (-1.9, -2.9, 0.5), (-1.9, -1.7, 0.5),
                         ], None, 6, 1.8, 4, [0, 0, 2, 3, 4, 4], [0, 4, 2, 1]),
    # 1.5 m apart with range 1.5: d2 == range range is not in range, and not blocked either (vehicle 2 keeps info[2] from being 0)
    "exactly_at_range": ([(-1.0, -1.0, 0.5), (-1.0, 0.5, 0.5), (-1.0, -0.5, 0.5)], None, 3, 1.5, 4, [0, 0, 0], [0, 1, 2, 0]),
    # vehicles that do not speak cast no ray and are counted nowhere: 1, 2, 3 have no finite position; 0 - 4 are linked, 0 - 5 and 4 - 5 blocked
    "nan_and_infinite_positions": ([(-1.0, -1.0, 0.5), (NAN, -1.0, 0.5), (-1.0, INF, 0.5), (-1.0, -1.0, -INF), (-1.0, -0.5, 0.5),
                                    (1.0, -1.0, 0.5)], None, 6, 3.0, 4, [0, 1, 2, 3, 0, 5], [0, 5, 1, 2]),
    # views -1 and 3 are out of range of n_views = 3: vehicles 1 and 2 do not speak; 0 - 3 linked (views 0 and 2), 0 - 4 and 3 - 4 blocked
    "a_view_out_of_range": ([(-1.0, -1.0, 0.5), (-1.0, -0.8, 0.5), (-1.0, -0.6, 0.5), (-1.0, -0.4, 0.5), (1.0, -1.0, 0.5)],
                            [0, -1, 3, 2, 1], 3, 3.0, 4, [0, 1, 0], [0, 2, 1, 2]),
    # A - B - C: B stands in the doorway and sees both, A and C at y = 0.6 see each other through the wall only
    "a_relay_in_the_doorway": ([(-1.0, 0.6, 0.5), (0.1, 0.9, 0.5), (1.0, 0.6, 0.5)], None, 3, 3.0, 4, [0, 0, 0], [0, 1, 2, 1]),
    # past the corner of the pillar (its corner is at (-1.2, -1.2)): a chord shorter than a cell, met by a half-cell step only
    "clips_the_pillar": ([(-1.05, -1.32, 0.5), (-1.79, -0.89, 0.5)], None, 2, 3.0, 4, [0, 1], [0, 2, 0, 1]),
}

# the hand case each variant of tests/link_los_model.py changes (labels or info); "from_observer" is told by the pair of the seeded search
TELLS = {
    "ends_tested": "inside_an_inflated_cell",
    "q_only": "inside_an_inflated_cell",
    "full_cell_step": "clips_the_pillar",
    "outside_blocks": "outside_the_map",
    "le": "exactly_at_range",
    "blocked_counts_twice": "across_the_wall",
}


def case(name):
    """(par, vehicles, view_of, n_views, labels int32, info int64)"""
    pos, view_of, n_views, range_, passes, labels, info = CASES[name]
    v, vo = lm.fleet(pos, view_of)
    return lm.params(range_, passes), v, vo, n_views, np.array(labels, dtype=np.int32), np.array(info, dtype=np.int64)


# ---- random fleets ---------------------------------------------------------------------------------------------------------------------------
def forest_cloud(seed=7, pillars=14):
    """A small random forest on the scene's lattice: `pillars` columns of points at cell centres, over all z (each inflates to 3 x 3 cells)."""
    rng = np.random.default_rng(seed)
    cols = rng.integers(1, 19, size=(pillars, 2))
    return np.array([centre(int(ix), int(iy), iz) for ix, iy in cols for iz in range(10)], dtype=np.float64)


def forest_fleet(seed=3, n=96, n_views=24):
    """(positions [n][3], view_of [n] int32): n vehicles in n_views views all over the map, some of them a little outside it; the first
    half on a 0.1 m grid, where samples land on cell boundaries and pairs stand exactly at range."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform((-2.1, -2.1, 0.1), (2.1, 2.1, 1.9), size=(n, 3))
    pos[:n // 2] = np.round(pos[:n // 2] * 10.0) / 10.0
    return pos, rng.integers(0, n_views, size=n).astype(np.int32)


def room_fleet(seed=5):
    """80 vehicles, a view each, in the scene of the hand cases: 72 in the room left of the wall (clear of the pillar), 8 in the room right
    of it, all within one range of 8 m.  Every vehicle on the left has 71 neighbours in line of sight and more, a row of FH_LINK_LIST = 64
    does not hold them; the two rooms see each other through the door only."""
    rng = np.random.default_rng(seed)
    left = rng.uniform((-1.9, -1.0, 0.2), (-0.3, 1.9, 1.8), size=(72, 3))
    right = rng.uniform((0.5, -1.9, 0.2), (1.9, 1.9, 1.8), size=(8, 3))
    return np.concatenate([right[:4], left, right[4:]])   # (the rooms mixed in index order: the labels need the passes)


# ---- the pair whose answer depends on the orientation of the ray ---------------------------------------------------------------------------
SEARCH_SEED = 2027     # (the first such pair is try 836 of this seed; seeds 2025 and 2026 find theirs at tries 596 and 327)
SEARCH_TRIES = 4000
SEARCH_LO, SEARCH_HI = (-2.3, -2.3, 0.1), (-0.6, -0.8, 1.1)   # around the pillar


def orientation_pair(occ, m_origin, m_res, blocked):
    """Seeded search: the first random pair on a 0.1 m grid around the pillar whose ray is blocked from one end and free from the
    other (`blocked` is link_los_model.blocked).  Returns (p, q, tries) with the ray p -> q free and q -> p blocked, or None."""
    rng = np.random.default_rng(SEARCH_SEED)
    for t in range(SEARCH_TRIES):
        pq = np.round(rng.uniform(SEARCH_LO + SEARCH_LO, SEARCH_HI + SEARCH_HI) * 10.0) / 10.0
        p, q = pq[:3], pq[3:]
        a, b = blocked(p, q, occ, m_origin, m_res), blocked(q, p, occ, m_origin, m_res)
        if a != b:
            return (q, p, t + 1) if a else (p, q, t + 1)
    return None
