"""Inputs for the decomposition kernel (faster_amd/csrc/fh_decomp.hip.hpp) where a segment's point list changes home and where its caps
bite, and for corridor_assemble_kernel's failure clauses.  numpy only: tests/test_decomp_edge_cases.py proves every property on the CPU
against the host restatement, tests/test_gpu_decomp_edges.py runs the same inputs on the device.

Every cloud is built so that the number of points in a segment's local box is known exactly: a point is either at least MARGIN_IN inside
all six planes of the box or at least MARGIN_OUT outside the bounding box of the box.  The kernel decides a point farther than its band
(about 1e-5 m) from the planes without the exact tests, DecompUtil's epsilon is 1e-10: both implementations list the same points."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _caps():
    text = open(os.path.join(ROOT, "faster_amd", "csrc", "fh_decomp.hip.hpp")).read()
    out = {}
    for name in ("FH_DECOMP_CAP", "FH_DECOMP_CAP_IDS", "FH_DECOMP_CAP_GLOBAL", "FH_DECOMP_BLIST"):
        m = re.findall(r"^#define\s+%s\s+(\d+)\b" % name, text, flags=re.M)
        assert len(m) == 1, (name, m)
        out[name] = int(m[0])
    return out


_C = _caps()
CAP, CAP_IDS, CAP_GLOBAL, BLIST = _C["FH_DECOMP_CAP"], _C["FH_DECOMP_CAP_IDS"], _C["FH_DECOMP_CAP_GLOBAL"], _C["FH_DECOMP_BLIST"]
assert 64 < CAP < CAP_IDS < CAP_GLOBAL and CAP % 64 == 0 and CAP_IDS % 64 == 0

_h = open(os.path.join(ROOT, "include", "fasterhip.h")).read()
MAX_FACES_POLY = int(re.search(r"^#define\s+FH_MAX_FACES_POLY\s+(\d+)", _h, flags=re.M).group(1))
MAX_POLY = int(re.search(r"^#define\s+FH_MAX_POLY\s+(\d+)", _h, flags=re.M).group(1))

BBOX = (2.0, 2.0, 1.0)
DRONE_RADIUS = 0.05
MARGIN_IN, MARGIN_OUT, MIN_DIST = 0.05, 1.0, 0.4
BLOCK = 64  # cloud points per block box (cloud_blocks_kernel)
MIN_BLOCKS = 8  # decompose_device uses block boxes from this many blocks upwards

HORIZONTAL = np.array([0.0, 0.0, 1.5, 2.0, 0.0, 1.5])
OBLIQUE = np.array([0.0, 0.0, 1.0, 1.5, 0.5, 1.7])
VERTICAL = np.array([1.5, 0.5, 1.2, 1.5, 0.5, 2.4])


def shifted(segment, dx):
    """the segment moved dx metres along x (several segments over one cloud are kept far apart)"""
    s = np.array(segment, dtype=np.float64)
    s[[0, 3]] += dx
    return s


# ---- the local box of a segment, as the kernel and the host build it ---------------------------------------------------------------------
def frame(segment):
    """(p1, p2, dh, dir, dv, length): the frame of the local box at p1 (line_segment.h:57-98)"""
    p1, p2 = np.asarray(segment[:3], dtype=np.float64), np.asarray(segment[3:], dtype=np.float64)
    L = np.linalg.norm(p2 - p1)
    d = (p2 - p1) / L
    dh = np.array([d[1], -d[0], 0.0])
    if np.linalg.norm(dh) == 0:
        dh = np.array([-1.0, 0.0, 0.0])
    dh = dh / np.linalg.norm(dh)
    return p1, p2, dh, d, np.cross(d, dh), L


def plane_depth(segment, pts, bbox=BBOX):
    """for every point the smallest distance INSIDE the six planes of the local box (negative: outside one of them)"""
    p1, p2, dh, d, dv, L = frame(segment)
    r = np.asarray(pts, dtype=np.float64).reshape(-1, 3) - p1
    u, a, w = r @ dh, r @ d, r @ dv
    return np.minimum.reduce([bbox[1] - u, bbox[1] + u, L + bbox[0] - a, a + bbox[0], bbox[2] - w, bbox[2] + w])


def segment_dist(segment, pts):
    p1, p2, _, d, _, L = frame(segment)
    r = np.asarray(pts, dtype=np.float64).reshape(-1, 3) - p1
    t = np.clip(r @ d, 0.0, L)
    return np.linalg.norm(r - t[:, None] * d, axis=1)


def box_aabb(segment, bbox=BBOX):
    """(lo, hi) of the eight corners of the local box: what decomp_kernel tests the block boxes against"""
    p1, p2, dh, d, dv, _ = frame(segment)
    corners = np.array([(p2 + d * bbox[0] if c & 1 else p1 - d * bbox[0]) + dh * (bbox[1] if c & 2 else -bbox[1]) + dv * (bbox[2] if c & 4 else -bbox[2])
                        for c in range(8)])
    return corners.min(axis=0), corners.max(axis=0)


def aabb_clearance(segment, pts, bbox=BBOX):
    """for every point its distance outside the bounding box of the local box, in the largest axis (<= 0: inside the bounding box)"""
    lo, hi = box_aabb(segment, bbox)
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    return np.maximum(lo - pts, pts - hi).max(axis=1)


def _inside_points(segment, k, rng, bbox, min_dist):
    p1, p2, dh, d, dv, L = frame(segment)
    m = MARGIN_IN + 0.01
    out = np.zeros((0, 3))
    while len(out) < k:
        n = 2 * (k - len(out)) + 64
        u, w = rng.uniform(-bbox[1] + m, bbox[1] - m, n), rng.uniform(-bbox[2] + m, bbox[2] - m, n)
        a = rng.uniform(-bbox[0] + m, L + bbox[0] - m, n)
        q = p1 + u[:, None] * dh + a[:, None] * d + w[:, None] * dv
        out = np.vstack([out, q[segment_dist(segment, q) >= min_dist + 0.02]])
    return out[:k]


def _outside_points(segment, n, rng, bbox):
    lo, hi = box_aabb(segment, bbox)
    out = np.zeros((0, 3))
    while len(out) < n:
        q = rng.uniform(lo - 4.0, hi + 4.0, size=(2 * (n - len(out)) + 64, 3))
        out = np.vstack([out, q[aabb_clearance(segment, q, bbox) >= MARGIN_OUT + 0.02]])
    return out[:n]


def _interleave(inside, outside, rng):
    """one cloud with the inside points in their order at seeded positions; -> (cloud, cloud index of every inside point)"""
    k, n = len(inside), len(outside)
    slots = np.sort(rng.choice(k + n, size=k, replace=False))
    cloud = np.zeros((k + n, 3))
    rest = np.ones(k + n, dtype=bool)
    rest[slots] = False
    cloud[slots], cloud[rest] = inside, outside
    return cloud, slots


def assert_exact(segment, cloud, k_inside, bbox=BBOX, min_dist=MIN_DIST):
    """the margins that make the list length exact, by this module's own dot products"""
    depth, clear = plane_depth(segment, cloud, bbox), aabb_clearance(segment, cloud, bbox)
    inside = depth >= MARGIN_IN
    assert int(inside.sum()) == k_inside, (int(inside.sum()), k_inside)
    assert np.all(clear[~inside] >= MARGIN_OUT), float(clear[~inside].min())
    if k_inside:
        assert segment_dist(segment, cloud[inside]).min() >= min_dist
    return inside


def exact_cloud(segment, k_inside, n_outside, seed, bbox=BBOX, near_from=None):
    """k_inside points at least MARGIN_IN inside every plane of the segment's local box and at least MIN_DIST from the segment, n_outside
    points at least MARGIN_OUT outside the bounding box of the box, interleaved under a seeded shuffle: the list of the segment holds
    exactly k_inside points, in cloud order, from many blocks of 64.
    near_from: the inside points at list positions >= near_from are the ones nearest the segment (the separating planes then keep
    mostly entries of the tail, and the compaction moves them to the front)."""
    rng = np.random.default_rng(seed)
    inside, outside = _inside_points(segment, k_inside, rng, bbox, MIN_DIST), _outside_points(segment, n_outside, rng, bbox)
    if near_from is not None and k_inside > near_from:
        order = np.argsort(-segment_dist(segment, inside), kind="stable")  # farthest first
        head, tail = order[:near_from], order[near_from:]
        inside = np.vstack([inside[rng.permutation(head)], inside[rng.permutation(tail)]])
    cloud, _ = _interleave(inside, outside, rng)
    assert_exact(segment, cloud, k_inside, bbox)
    return cloud


def merged_cloud(segments, clouds, seed, bbox=BBOX):
    """The clouds of several segments (far apart) as ONE cloud: a seeded interleave that keeps every cloud's own order.  Asserts that
    a segment's list is still exactly its own inside points: every point of another cloud is MARGIN_OUT outside its bounding box."""
    rng = np.random.default_rng(seed)
    owner = rng.permutation(np.repeat(np.arange(len(clouds)), [len(c) for c in clouds]))
    cloud = np.zeros((len(owner), 3))
    for j, c in enumerate(clouds):
        cloud[owner == j] = c
    for j, s in enumerate(segments):
        if np.isnan(s[0]):
            continue
        k = int((plane_depth(s, clouds[j], bbox) >= MARGIN_IN).sum())
        assert_exact(s, cloud, k, bbox)
    return cloud


# ---- exact ties ------------------------------------------------------------------------------------------------------------------------
TIE_SEGMENT = np.array([0.0, 0.0, 1.0, 2.0, 0.0, 1.0])
TIE_PAIR = np.array([[1.0, 0.75, 1.0], [1.0, -0.75, 1.0]])
TIE_MIN_DIST = 1.2  # the other points: outside the initial sphere (radius 1 around the midpoint), inflated or not


def tie_cloud(pos_a, pos_b, k_inside, n_outside, seed, swap=False, bbox=BBOX):
    """A cloud over TIE_SEGMENT whose list holds k_inside points, with the mirror images (1, +0.75, 1) and (1, -0.75, 1) at list positions
    pos_a < pos_b (swap: the other way round).  All coordinates of the segment and the pair are exactly representable, the inflation moves
    both by the same amount towards the midpoint, so every ellipsoid distance of the two is bit-equal; every other inside point is at
    least TIE_MIN_DIST from the segment and so strictly farther from the ellipsoid (asserted below): the pair is the first choice of every
    arg-min, and which of the two wins is decided by the tie rule alone.  -> cloud"""
    assert 0 <= pos_a < pos_b < k_inside
    rng = np.random.default_rng(seed)
    inside = _inside_points(TIE_SEGMENT, k_inside, rng, bbox, TIE_MIN_DIST)
    inside[pos_a], inside[pos_b] = (TIE_PAIR[1], TIE_PAIR[0]) if swap else (TIE_PAIR[0], TIE_PAIR[1])
    cloud, slots = _interleave(inside, _outside_points(TIE_SEGMENT, n_outside, rng, bbox), rng)
    assert_exact(TIE_SEGMENT, cloud, k_inside, bbox)
    # the ellipsoid the pair leaves: centre c, axes (1, 0.7, 1) along x, y, z (the sphere of radius 1 shrunk along y to the inflated pair).
    # Every other point, inflated towards c, is outside the initial sphere and farther from the final ellipsoid than the pair (distance 1)
    c = np.array([1.0, 0.0, 1.0])
    others = np.delete(inside, [pos_a, pos_b], axis=0) - c
    infl = others - np.sign(others) * DRONE_RADIUS
    assert np.linalg.norm(infl, axis=1).min() > 1.05
    assert np.linalg.norm(infl / np.array([1.0, 0.75 - DRONE_RADIUS, 1.0]), axis=1).min() > 1.05
    assert np.array_equal(cloud[slots[pos_a]] * [1, -1, 1], cloud[slots[pos_b]])
    return cloud


# ---- the candidate-block list -------------------------------------------------------------------------------------------------------------
BLOCK_SEGMENT = HORIZONTAL


def block_cloud(n_hit_blocks, seed, n_pad_blocks=37, last=17, bbox=BBOX):
    """A cloud of n_hit_blocks + n_pad_blocks blocks of 64 points over BLOCK_SEGMENT: a hit block holds ONE point of the local box (exact, as
    above) and 63 points far away on the +x side, a pad block only far points; the last block is a hit block of `last` < 64 points, so
    n_cloud % 64 != 0.  The list holds n_hit_blocks points, one per hit block."""
    assert n_hit_blocks >= 1 and 1 <= last < BLOCK
    rng = np.random.default_rng(seed)
    n_blocks = n_hit_blocks + n_pad_blocks
    hit = np.zeros(n_blocks, dtype=bool)
    hit[rng.choice(n_blocks - 1, size=n_hit_blocks - 1, replace=False)] = True
    hit[-1] = True
    n_cloud = (n_blocks - 1) * BLOCK + last
    lo, hi = box_aabb(BLOCK_SEGMENT, bbox)
    cloud = np.column_stack([rng.uniform(hi[0] + 5.0, hi[0] + 15.0, n_cloud), rng.uniform(-5.0, 5.0, n_cloud), rng.uniform(-3.0, 6.0, n_cloud)])
    inside = _inside_points(BLOCK_SEGMENT, n_hit_blocks, rng, bbox, MIN_DIST)
    size = np.full(n_blocks, BLOCK)
    size[-1] = last
    at = np.nonzero(hit)[0] * BLOCK + rng.integers(0, size[hit])
    cloud[at] = inside
    assert n_cloud % BLOCK != 0 and at[-1] >= (n_blocks - 1) * BLOCK
    assert_exact(BLOCK_SEGMENT, cloud, n_hit_blocks, bbox)
    return cloud


def blocks_meeting_box(segment, cloud, bbox=BBOX):
    """how many block boxes (min / max over 64 consecutive points, the last block over what it has: cloud_blocks_kernel) meet the bounding
    box of the local box widened by 1e-6: decomp_kernel's candidate test"""
    lo, hi = box_aabb(segment, bbox)
    n = 0
    for b0 in range(0, len(cloud), BLOCK):
        blk = cloud[b0:b0 + BLOCK]
        mn, mx = blk.min(axis=0), blk.max(axis=0)
        n += bool(np.all(mn <= hi + 1e-6) and np.all(mx >= lo - 1e-6))
    return n


# ---- corridor assembly --------------------------------------------------------------------------------------------------------------------
CORRIDOR_MAX_POLY = 3
MANY_FACES_PATH = 25  # the path whose second leg has more than FH_MAX_FACES_POLY rows


def corridor_case(seed=5, n=64):
    """n paths of up to CORRIDOR_MAX_POLY + 1 vertices over one cloud: n_points runs over -2 .. 4, path MANY_FACES_PATH ends in a leg
    inside a shell of points that each give a row.  -> dict(cloud, paths [n][4][3], n_points [n], many = (path, leg))"""
    rng = np.random.default_rng(seed)
    mp = CORRIDOR_MAX_POLY + 1
    n_points = np.array([(-2, -1, 0, 1, 2, 3, 4, 3, 4, 2)[i % 10] for i in range(n)], dtype=np.int32)
    paths = np.zeros((n, mp, 3))
    for i in range(n):
        v = np.array([rng.uniform(2, 18), rng.uniform(2, 18), rng.uniform(1.0, 2.0)])
        for j in range(mp):
            paths[i, j] = v
            step = rng.normal(size=3) * [1, 1, 0.25]
            v = v + step / np.linalg.norm(step) * rng.uniform(0.8, 2.0)
            v[2] = min(max(v[2], 0.8), 2.4)
    cloud = rng.uniform([-1, -1, 0.0], [21, 21, 3.2], size=(3500, 3))
    # the many-faces leg: 140 points on a sphere of radius 0.8 around the midpoint of a 1 m leg.  The ellipsoid is the sphere of radius
    # 0.5 on the leg, every tangent plane cuts off little more than its own point
    centre = np.array([40.5, 0.0, 1.5])
    paths[MANY_FACES_PATH, :3] = [[40.0, -3.5, 1.5], [40.0, 0.0, 1.5], [41.0, 0.0, 1.5]]
    n_points[MANY_FACES_PATH] = 3
    i = np.arange(140) + 0.5
    phi, th = np.arccos(1 - 2 * i / 140), np.pi * (1 + 5 ** 0.5) * i
    shell = centre + 0.8 * np.column_stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)])
    cloud = np.vstack([cloud, shell])
    keep = np.ones(len(cloud), dtype=bool)
    for i in range(n):
        for j in range(max(min(int(n_points[i]), mp) - 1, 0)):
            keep &= segment_dist(np.concatenate([paths[i, j], paths[i, j + 1]]), cloud) > 0.35
    cloud = cloud[keep][rng.permutation(int(keep.sum()))]
    return {"cloud": cloud, "paths": paths, "n_points": n_points, "many": (MANY_FACES_PATH, 1), "max_poly": CORRIDOR_MAX_POLY}


def legs_of(case, i):
    """the vertices of path i that the corridor keeps (None: the path is unusable)"""
    k = int(case["n_points"][i])
    return case["paths"][i, :min(k, case["max_poly"] + 1)] if k >= 2 else None


# ---- the cases of tests/test_gpu_decomp_edges.py (proved in tests/test_decomp_edge_cases.py) ------------------------------------------------
SPACING = 40.0  # metres between the segments of one cloud: far more than a local box and its outside points reach


def _case(segments, ks, seed, **kw):
    """segments[j] moved to its own place, a cloud whose list for segment j holds exactly ks[j] points -> (segments [n][6], cloud, ks)"""
    segs = [shifted(s, SPACING * j) for j, s in enumerate(segments)]
    nears = kw.get("near_from", [None] * len(segs))
    clouds = [exact_cloud(s, k, min(max(64, k // 4), 1024), seed + 101 * j, near_from=nf) for j, (s, k, nf) in enumerate(zip(segs, ks, nears))]
    return np.array(segs), merged_cloud(segs, clouds, seed + 7), list(ks)


def list_length_case():
    """a list of every length at which the kernel switches, one below and one above; CAP_GLOBAL + 1 must report -1"""
    ks = [0, 1, 63, 64, 65, CAP - 1, CAP_IDS - 1, CAP_IDS + 63, CAP_IDS + 64, CAP_IDS + 65]
    segments = [OBLIQUE] * len(ks)
    for s in (HORIZONTAL, OBLIQUE, VERTICAL):
        ks += [CAP, CAP + 1, CAP_IDS, CAP_IDS + 1]
        segments += [s] * 4
    return _case(segments, ks, seed=1000)


def list_cap_case():
    """the three largest: one below the capacity of the hybrid list, at it, and beyond it (count -1)"""
    return _case([OBLIQUE] * 3, [CAP_GLOBAL - 1, CAP_GLOBAL, CAP_GLOBAL + 1], seed=2000)


def compaction_case():
    """lists of 3000 and 6000 points, each also with the points nearest the segment behind position CAP_IDS"""
    return _case([OBLIQUE, HORIZONTAL, OBLIQUE, HORIZONTAL], [3000, 6000, 3000, 6000], seed=3000, near_from=[None, None, CAP_IDS, CAP_IDS])


TIE_CASES = [  # (pos_a, pos_b, list length): the pair on either side of a lane, a block of 64, the coordinate/id home, the LDS/HBM border
    (0, 1, 200), (63, 64, 200), (10, 700, 1000), (CAP_IDS - 1, CAP_IDS, 6000), (100, CAP_IDS, 6000), (CAP_IDS, CAP_IDS + 64, 6000), (1800, 5000, 6000)]


def tie_case(j, swap):
    a, b, k = TIE_CASES[j]
    return tie_cloud(a, b, k, 256, seed=4000 + j, swap=swap)


BLOCK_EDGE_SIZES = [MIN_BLOCKS * BLOCK - 65, MIN_BLOCKS * BLOCK - 64, MIN_BLOCKS * BLOCK - 63, MIN_BLOCKS * BLOCK]  # 447, 448, 449, 512


def block_edge_cloud(n_cloud):
    """n_cloud points around the switch to block boxes (8 blocks), 100 of them in the list"""
    return exact_cloud(BLOCK_SEGMENT, 100, n_cloud - 100, seed=5000 + n_cloud)


def block_list_cloud(n_hit_blocks):
    return block_cloud(n_hit_blocks, seed=6000 + n_hit_blocks)


def max_faces_case():
    """a segment with a polytope of a few dozen rows, then one whose box is empty (7 rows)"""
    return _case([HORIZONTAL, OBLIQUE], [200, 0], seed=7000)


HOMES_LENGTHS = [30, CAP, CAP + 1, 1000, CAP_IDS, CAP_IDS + 1, 2500]


def homes_case():
    """seven segments whose lists live in all three homes over one cloud (the test tiles them, with NaN slots, over a launch larger than the grid)"""
    return _case([OBLIQUE, HORIZONTAL, VERTICAL, OBLIQUE, HORIZONTAL, VERTICAL, OBLIQUE], HOMES_LENGTHS, seed=8000)


EXACT_CASES = {"list_length": list_length_case, "list_cap": list_cap_case, "compaction": compaction_case, "max_faces": max_faces_case,
               "homes": homes_case}
