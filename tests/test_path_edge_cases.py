"""The scenes of tests/test_gpu_path_edges.py proved on the CPU: every scene's reason to exist is an assertion here (against
tests/path_model.py), and the host restatement (frontend.plan_batch) satisfies on every scene what the device is asked for —
reachable iff the model says so (P1), ends on start and goal (P2), no blocked leg (P3), no longer than the optimal cost allows (P4)."""
import math

import numpy as np
import pytest

import path_edge_cases as pe
import path_model as pm
from faster_amd import frontend

RES = pe.RES


@pytest.fixture(scope="module", autouse=True)
def built():
    from faster_amd import build as fb

    fb.build_frontend()


def host(sc, search, sphere=0.0, idx=None, **kw):
    """frontend.plan_batch on the scene's map -> (paths, n_points, expansions, occupancy)"""
    starts, goals = (sc.starts, sc.goals) if idx is None else (sc.starts[idx], sc.goals[idx])
    with frontend.host_settings(search, sphere):
        p, n, ex, occ, dims, origin = frontend.plan_batch(*sc.map_args(), starts, goals, want_grid=True, **kw)
    assert tuple(dims) == sc.dims and np.array_equal(origin, sc.origin)
    return p, n, ex, occ


def assert_grid(sc, occ):
    """the model's grid is the host's; with inflation 0 it is exactly the pattern that was drawn"""
    assert np.array_equal(occ, sc.occ), sc.name
    if sc.inflation == 0.0:
        assert np.array_equal(sc.occ != 0, sc.pattern), sc.name


# ---- a ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pe.TINY_NAMES)
def test_tiny_grids(name):
    sc = pe.tiny_scene(name)
    assert sc.m_free == int(name[-1])
    overlap, clipped, on_ray = pe.tiny_counts(sc)
    print("%s: pairs with overlapping cubes %d, with a clipped cube %d, goal on a straight ray %d" % (name, overlap, clipped, on_ray))
    assert min(overlap, clipped, on_ray) >= 100
    sample = pe.tiny_sample(name)
    got = {}
    for search in ("astar", "jps"):
        p, n, ex, occ = host(sc, search, max_points=16)
        assert_grid(sc, occ)
        assert n.min() >= 0
        got[search] = n
        for q in sample:
            pe.check_answer(sc, q, p[q], n[q], "host " + search)
    assert np.array_equal(got["astar"] > 0, got["jps"] > 0)
    if name == "wall/m1":
        assert 100 < int((got["astar"][sample] == 0).sum()) < len(sample) - 100   # P1 is tried both ways


# ---- b ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("j", range(len(pe.JUMP_CASES)), ids=lambda j: "%d-%s-%d-%s" % pe.JUMP_CASES[j])
def test_jump_scenes(j):
    n1, kind, L, near = pe.JUMP_CASES[j]
    sc = pe.jump_scene(n1, kind, L, near)
    s, t = sc.cell(sc.starts[0]), sc.cell(sc.goals[0])
    assert pm.inside(t, sc.dims) and s == pe.JUMP_START[n1]
    if near:   # occupied on the map as read, inside the cube freed around the start, off the ray
        c = pe.JUMP_NEAR[n1]
        assert sc.occ[c[2], c[1], c[0]] != 0 and max(abs(c[k] - s[k]) for k in range(3)) <= sc.m_free
        assert pm.freed(sc.occ, s, t, sc.m_free)[c[2], c[1], c[0]] == 0
    for search in ("jps", "astar"):
        p, n, ex, occ = host(sc, search, max_points=16)
        assert_grid(sc, occ)
        cost = pe.check_answer(sc, 0, p[0], n[0], "host " + search)
        print("%s %s: n_points %d expansions %d cost %s" % (sc.name, search, n[0], ex[0], cost))
        if kind == "goal":   # one jump of L cells: the start and the goal are the only popped nodes, the cost is L moves of the jump's kind
            assert n[0] == 2 and cost == L * math.sqrt(n1)
            if search == "jps":
                assert ex[0] == 2
        elif kind == "hole" and n1 == 1:   # the first vertex after the start is the hole, L cells out on the ray
            assert n[0] == 3 and np.array_equal(p[0, 1], sc.centre(sc.meta["end"])) and np.array_equal((p[0, 1] - p[0, 0]) / RES, [L, 0, 0])
        elif kind == "hole":   # the first vertex after the start is the hole straight ahead of the L-th diagonal cell; the optimal cost is
            e = sc.meta["end"]  # L diagonal moves, one into the hole, then three diagonal ones and one straight to the goal
            assert n[0] == 3 and np.array_equal(p[0, 1], sc.centre((e[0] + 1, e[1], e[2])))
            assert cost == pm.cost_of(1, L + 3, 0) if n1 == 2 else cost == pm.cost_of(1, 3, L)
        elif kind == "blocked":
            assert n[0] == 0 and cost is None
        else:   # the only occupied cell beside the ray is beside ray cell L: the one jump point between start and goal
            e = sc.meta["end"]
            assert sc.occ[e[2], e[1] + 1, e[0]] != 0 and int((sc.occ != 0).sum()) == 1 + int(near) and cost == L + 5
            if search == "jps":   # (the jump point stays a vertex: collinear, but its two legs differ in length; A* has no such vertex)
                assert ex[0] == 3 and n[0] == 3 and np.array_equal(p[0, 1], sc.centre(e))


@pytest.mark.parametrize("k", pe.FREED_TUBE_CASES)
def test_freed_tube_scenes(k):
    sc = pe.freed_tube_scene(k)
    s, t, o = sc.cell(sc.starts[0]), sc.cell(sc.goals[0]), sc.meta["obstacle"]
    assert o == (s[0] + k, s[1] + 1, s[2]) and sc.occ[o[2], o[1], o[0]] != 0            # beside ray cell k
    assert max(abs(o[i] - t[i]) for i in range(3)) <= sc.m_free                         # in the goal's cube: free for this query
    assert not (pm.freed(sc.occ, s, t, sc.m_free) != 0).any()
    for search in ("jps", "astar"):
        p, n, ex, occ = host(sc, search, max_points=16)
        assert_grid(sc, occ)
        assert pe.check_answer(sc, 0, p[0], n[0], "host " + search) is not None


# ---- c ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_raw", pe.RAW_LENGTHS)
def test_staircase_scenes(n_raw):
    sc = pe.staircase_scene(n_raw)
    reach, _, abc = pm.dijkstra(sc.occ, sc.cell(sc.starts[0]), sc.cell(sc.goals[0]), sc.m_free)
    assert reach and sum(abc) + 1 == n_raw and abc[2] == 0 and abs(abc[0] - abc[1]) <= 1
    p, n, ex, occ = host(sc, "astar", max_points=160)
    assert_grid(sc, occ)
    pe.check_answer(sc, 0, p[0], n[0], "host astar")
    print("%s: %d vertices" % (sc.name, n[0]))
    assert n[0] > n_raw // 4   # the clean-up keeps a long list: the count carries over the passes of 64 lanes


@pytest.mark.parametrize("L,h", pe.LEG_CASES)
def test_leg_scenes(L, h):
    sc = pe.leg_scene(L, h)
    P, A, b, o = sc.meta["P"], sc.meta["A"], sc.meta["b"], sc.meta["obstacle"]
    s, t = sc.cell(sc.starts[0]), sc.cell(sc.goals[0])
    grid = pm.freed(sc.occ, s, t, sc.m_free)
    assert sc.meta["steps"] == {52: 65, 80: 100, 81: 101, 160: 200}[L]
    assert np.array_equal((np.abs(b - P) / RES).max(), L)
    assert pm.leg_blocked(grid, sc.origin, RES, P, b, first=True) == h           # the intended sample is the first occupied one
    assert grid[o[2], o[1], o[0]] != 0
    grid[o[2], o[1], o[0]] = 0
    assert not pm.leg_blocked(grid, sc.origin, RES, P, b)                        # ... and that one cell is all that refuses the shortcut
    reach, _, abc = pm.dijkstra(sc.occ, s, t, sc.m_free)
    assert reach and abc == (11, L, 0)                                           # the corridor: the only route
    for search in ("astar", "jps"):
        p, n, ex, occ = host(sc, search, max_points=16)
        assert_grid(sc, occ)
        pe.check_answer(sc, 0, p[0], n[0], "host " + search, legs=False)
        print("%s %s: %d vertices %s" % (sc.name, search, n[0], (p[0, :n[0], :2] / RES - 0.5).tolist()))
        k = [i for i in range(n[0]) if np.array_equal(p[0, i], P)]
        assert len(k) == 1 and np.array_equal(p[0, k[0] + 1], A) and np.array_equal(p[0, k[0] + 2], b)   # P -> b was refused: A is still there


def test_straight_raw_scene():
    sc = pe.straight_raw_scene()
    reach, _, abc = pm.dijkstra(sc.occ, sc.cell(sc.starts[0]), sc.cell(sc.goals[0]), sc.m_free)
    assert reach and abc == (128, 0, 0)
    p, n, ex, occ = host(sc, "astar", max_points=160)
    assert n[0] == 2
    pe.check_answer(sc, 0, p[0], n[0], "host astar")


# ---- d ------------------------------------------------------------------------------------------------------------------------------------
def test_comb_scene_reaches_chained_chunks():
    sc = pe.comb_scene()
    s, t = sc.cell(sc.starts[0]), sc.cell(sc.goals[0])
    prof = pm.astar_open_profile(sc.occ, s, t, sc.m_free)
    peak = np.array(prof["peak"])
    drained = np.array(prof["drained_after_peak"])
    print("comb: %d pops, open list <= %d, largest sub-lists %s, shared inserts %d" % (prof["pops"], prof["max_open"], np.sort(peak)[-3:], prof["shared_inserts"]))
    assert not prof["found"]
    assert peak.max() > 128 and drained[np.argmax(peak)]      # two chained chunks behind the head, released when it has drained
    assert prof["shared_inserts"] >= 10                       # two neighbours of one expansion in one sub-list: the claim rounds
    assert prof["pops"] < 2000
    x, y, z0, z1 = sc.meta["column"]
    ids = x + sc.dims[0] * y + sc.dims[0] * sc.dims[1] * np.arange(z0, z1)
    assert np.bincount([pm.sub_of(int(i)) for i in ids]).max() > 128
    p, n, ex, occ = host(sc, "astar", max_points=16)
    assert_grid(sc, occ)
    assert n[0] == 0 and ex[0] == prof["pops"]
    # (P1 from the instrument: its search is exhaustive, and a shortest-path tree over the 3.5 M cells of this lattice is not worth its memory)
    far = pm.astar_open_profile(sc.occ, sc.cell(sc.starts[1]), sc.cell(sc.goals[1]), sc.m_free)
    assert far["found"] and n[1] >= 2 and ex[1] == far["pops"]
    assert np.array_equal(p[1, 0], sc.starts[1]) and np.array_equal(p[1, n[1] - 1], sc.goals[1])


# ---- e ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["end", "middle"])
def test_key_range_scenes(which):
    sc = pe.key_range_scene(which)
    s = sc.cell(sc.starts[0])
    limit = sc.meta["limit"]
    for q, lim in enumerate(limit):   # the largest f among the start and the cells opened from it, by the model's own arithmetic
        t = sc.cell(sc.goals[q])
        f = [float(t[0] - s[0])]
        for dx, dy, dz in pm.OFFSETS:
            c = (s[0] + dx, s[1] + dy, s[2] + dz)
            if pm.inside(c, sc.dims):
                a, b, cc = sorted((abs(c[0] - t[0]), abs(c[1] - t[1]), abs(c[2] - t[2])), reverse=True)
                f.append(math.sqrt(dx * dx + dy * dy + dz * dz) + cc * pm.SQ3 + (b - cc) * pm.SQ2 + (a - b))
        assert (max(f) >= pe.KEY_LIMIT) == lim, (which, q, max(f))
    p, n, ex, occ = host(sc, "astar", max_points=16)
    assert_grid(sc, occ)
    print("%s: host A* n_points %s expansions %s" % (sc.name, n, ex))
    assert list(n) == [0 if lim else 2 for lim in limit]   # the host restatement refuses where the device reports -2
    p, n, ex, occ = host(sc, "jps", max_points=16)          # the jump point search has no such limit
    assert list(n) == [2] * len(limit)
    for q in range(len(limit)):
        pe.check_answer(sc, q, p[q], n[q], "host jps")


def test_raw_limit_scene():
    sc = pe.raw_limit_scene()
    chain = sc.meta["chain"]
    assert chain[1] == pe.MAXRAW and chain[2] == pe.MAXRAW + 1
    p, n, ex, occ = host(sc, "jps", max_points=16)   # the host has no limit on the chain: all four are paths
    assert_grid(sc, occ)
    print("raw limit: host jps n_points %s popped nodes %s" % (n, ex))
    assert list(ex) == chain and n.min() >= 2   # every popped node lies on the path: the chain is as long as the pops
    for q in range(4):
        reach, cost, abc = pm.dijkstra(sc.occ, sc.cell(sc.starts[q]), sc.cell(sc.goals[q]), sc.m_free)
        assert reach and abc == (chain[q] + 1, 0, 0)
        pe.check_answer(sc, q, p[q], n[q], "host jps")
    # A* cannot get there: a path of 4096 cells costs at least 4095 > 2040 cells, the key range ends the query first
    p, n, ex, occ = host(sc, "astar", max_points=16)
    assert n[0] >= 2 and n[3] >= 2 and list(n[1:3]) == [0, 0]


def test_max_points_scene():
    """(start = goal with a spacing: the goal is a duplicate of the start by the 1e-9 rule, one vertex is left)"""
    sc = pe.max_points_scene()
    for search in ("astar", "jps"):
        assert list(host(sc, search, max_points=16)[1]) == [2, 2, 2]
        assert list(host(sc, search, max_points=16, max_vertex_dist=0.25)[1]) == [7, 1, 3]
        assert list(host(sc, search, max_points=7, max_vertex_dist=0.25)[1]) == [7, 1, 3]
        assert list(host(sc, search, max_points=6, max_vertex_dist=0.25)[1]) == [-1, 1, 3]
        # the clip to max_poly + 1 comes before the test against max_points
        assert list(host(sc, search, max_points=6, max_vertex_dist=0.25, max_poly=4)[1]) == [5, 1, 3]
        assert list(host(sc, search, max_points=2, max_vertex_dist=0.25, max_poly=4)[1]) == [-1, 1, -1]
        assert list(host(sc, search, max_points=2)[1]) == [2, 2, 2]


# ---- f ------------------------------------------------------------------------------------------------------------------------------------
def epilogue_sample(name, k=400):
    return pe.tiny_sample(name)[:k]


@pytest.mark.parametrize("name", ["wall/m1", "random/m2"])
def test_vertex_epilogue_against_its_model(name):
    """createMoreVertexes, the duplicate rule and the clip to max_poly + 1 of the host restatement are what more_vertexes makes of the
    plain path, bit for bit; among the legs are exact multiples of the spacing, which exercise the duplicate rule."""
    sc = pe.tiny_scene(name)
    idx = epilogue_sample(name)
    plain, n0, _, _ = host(sc, "jps", idx=idx, max_points=16)
    for spacing, _ in pe.SPACINGS:
        exact = 0
        for max_poly in (0, 3):
            p, n, _, _ = host(sc, "jps", idx=idx, max_points=64, max_vertex_dist=spacing, max_poly=max_poly)
            for q in range(len(idx)):
                if n0[q] == 0:
                    assert n[q] == 0
                    continue
                want = pm.more_vertexes(plain[q, :n0[q]], spacing, max_poly)
                assert n[q] == len(want) and np.array_equal(p[q, :n[q]], want), (name, spacing, max_poly, idx[q], p[q, :n[q]], want)
                legs = np.linalg.norm(np.diff(plain[q, :n0[q]], axis=0), axis=1)
                exact += int(np.any((legs > spacing) & (legs / spacing == np.floor(legs / spacing))))
        print("%s spacing %g: %d paths with a leg that is an exact multiple" % (name, spacing, exact))
        if spacing in (0.25, 0.5):
            assert exact >= (20 if spacing == 0.25 else 2)
        if spacing == 100.0:
            assert exact == 0


def sphere_cases(sc, plain, n0, idx):
    """(query, Ra) pairs: vertex 1 exactly on the sphere, a sphere inside the first leg, the goal inside the sphere"""
    out = []
    for q in range(len(idx)):
        if n0[q] >= 3 and len(out) < 60:
            v = plain[q, :n0[q]]
            d = float(np.linalg.norm(v[-1] - v[0]))
            r1 = pm._dist(v[1], v[0])
            if r1 < d - 0.001:
                out.append((q, r1))
            out.append((q, 0.5 * r1))
            out.append((q, d + 1.0))
    return out


def test_sphere_clip_against_its_model():
    """JPS_in of the host restatement against clip_to_sphere: the strict `>` (a vertex exactly on the sphere is inside), the crossing
    point, no crossing point when the goal is inside."""
    sc = pe.tiny_scene("wall/m1")
    idx = epilogue_sample("wall/m1")
    plain, n0, _, _ = host(sc, "jps", idx=idx, max_points=16)
    cases = sphere_cases(sc, plain, n0, idx)
    assert len(cases) >= 40
    on_sphere = 0
    for q, ra in cases:
        v = plain[q, :n0[q]]
        p, n, _, _ = host(sc, "jps", sphere=ra, idx=idx[q:q + 1], max_points=16)
        want = np.array(pm.clip_to_sphere(v, min(pm._dist(v[-1], v[0]) - 0.001, ra)))
        assert n[0] == len(want) and np.array_equal(p[0, :n[0]], want), (idx[q], ra, p[0, :n[0]], want)
        assert np.all(np.isfinite(want))
        if ra == pm._dist(v[1], v[0]):
            on_sphere += 1
            assert n[0] >= 3 and np.array_equal(p[0, 1], v[1])   # vertex 1 is kept: the crossing lies on a later leg
    assert on_sphere >= 10


# ---- g ------------------------------------------------------------------------------------------------------------------------------------
def test_lattice_scene():
    sc = pe.lattice_scene()
    kinds = sc.meta["kinds"]
    assert {"face", "border", "clamped", "nonfinite"} == set(kinds)
    want = np.array([pm.inside(sc.cell(a), sc.dims) and pm.inside(sc.cell(b), sc.dims) for a, b in zip(sc.starts, sc.goals)])
    faces = np.array([k == "face" for k in kinds])
    assert want[faces].any() and (~want[faces]).any()
    assert want[[k in ("border", "clamped") for k in kinds]].all() and not want[[k == "nonfinite" for k in kinds]].any()
    # the low face itself is outside (round(-0.5) = -1) and so is the point one ulp inside it (-0.5 + 2^-1074 is -0.5); the high face is
    # outside (round(n - 0.5) = n), one ulp inside it is inside
    assert sc.cell([0.0, 0.8, 0.1])[0] == -1 and sc.cell([np.nextafter(0.0, 1.0), 0.8, 0.1])[0] == -1
    assert sc.cell([2.0, 0.8, 0.1])[0] == 8 and sc.cell([np.nextafter(2.0, 0.0), 0.8, 0.1])[0] == 7
    assert sc.cell([0.5, 0.8, -7.0])[2] == 2   # clamped to z = 0: (0 + 0.5) / 0.25 - 0.5 = 1.5 rounds away from zero
    for search in ("astar", "jps"):
        p, n, ex, occ = host(sc, search, max_points=16)
        assert np.array_equal(n > 0, want), (search, np.nonzero((n > 0) != want)[0])
        assert not ex[~want].any()
        for q in np.nonzero(want)[0]:
            pe.check_answer(sc, q, p[q], n[q], "host " + search)
