"""The voxel path search on the device (faster_amd/csrc/fh_path.hip.hpp: plan_kernel, plan_views_kernel, the launch-order kernels, the
jump tables) at its jump, list, limit and lattice edges — through fh_map_plan_batch_device, fh_map_plan_batch_radius_device and
fh_map_plan_batch_radius_views_device.

Every comparison with the host restatement (frontend.plan_batch) is exact: n_points, expansions and every vertex bit for bit (P5).  Where no
limit is documented to apply the answers also get the properties an independent model gives (tests/path_model.py; P1 - P4 in
path_edge_cases.check_answer).  Every output buffer has one guard row in front and one behind and starts as the byte 0xA5: the guards
must still be 0xA5 after the launch, and so must the row of a query that searched nothing.  The scenes come from
tests/path_edge_cases.py; why each of them means something is asserted on the CPU in tests/test_path_edge_cases.py."""
import numpy as np
import pytest
import torch  # noqa: F401  (before libfasterhip.so is loaded: one HIP runtime per process)

import path_edge_cases as pe
import path_model as pm
from faster_amd import capi, frontend

pytestmark = pytest.mark.gpu

POISON = 0xA5
DEV = "cuda:0"
MODES = [("astar", 0), ("jps", 0), ("jps", 1024)]   # (search, fh_map_set_records)
MODE_IDS = ["astar", "jps", "jps-hashed"]


@pytest.fixture(scope="module", autouse=True)
def built():
    from faster_amd import build as fb

    fb.build_frontend()


@pytest.fixture(scope="module")
def m():
    vmap = capi.Map(0)
    yield vmap
    vmap.close()


@pytest.fixture(scope="module")
def ms():
    """a Map with one wavefront per CU: the scenes of a few queries switch search and records all the time, and every switch rebuilds
    the workspace of every wavefront"""
    vmap = capi.Map(0)
    vmap.set_sched(waves_per_cu=1)
    yield vmap
    vmap.close()


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


_HOST = {}


def host(sc, search, sphere=0.0, idx=None, key=None, **kw):
    """the host restatement's answer (computed once per key)"""
    k = (sc.name, search, sphere, key, tuple(sorted(kw.items()))) if key is not None or idx is None else None
    if k is not None and k in _HOST:
        return _HOST[k]
    starts, goals = (sc.starts, sc.goals) if idx is None else (sc.starts[idx], sc.goals[idx])
    with frontend.host_settings(search, sphere):
        out = frontend.plan_batch(*sc.map_args(), starts, goals, **kw)
    if k is not None:
        _HOST[k] = out
    return out


def read(vmap, sc, search, records):
    vmap.set_search(search)
    vmap.set_records(records if search == "jps" else 0)
    vmap.read(*sc.map_args())
    dims, origin = vmap.dims()
    assert tuple(dims) == sc.dims and np.array_equal(origin, sc.origin)


def plan(vmap, starts, goals, max_points=16, entry="plain", radius=None, active=None, view_of=None, n_views=0, **kw):
    """One launch into poisoned buffers with a guard row on either side -> (paths [n][max_points][3], n_points [n], expansions [n], untouched [n]:
    the row of the query is still all 0xA5)."""
    n = len(starts)
    d_s, d_g = to_dev(np.asarray(starts, dtype=np.float64)), to_dev(np.asarray(goals, dtype=np.float64))
    row = max_points * 24
    d_paths = torch.full(((n + 2) * row,), POISON, dtype=torch.uint8, device=DEV)
    d_np = torch.full(((n + 2) * 4,), POISON, dtype=torch.uint8, device=DEV)
    d_ex = torch.full(((n + 2) * 8,), POISON, dtype=torch.uint8, device=DEV)
    args = (n, max_points, d_paths.data_ptr() + row, d_np.data_ptr() + 4)
    if entry == "plain":
        vmap.plan_batch_device(d_s.data_ptr(), d_g.data_ptr(), *args, d_ex.data_ptr() + 8, **kw)
    else:
        d_r = to_dev(np.full(n, 1e9) if radius is None else np.asarray(radius, dtype=np.float64))
        d_a = None if active is None else to_dev(np.asarray(active, dtype=np.int32))
        pa = d_a.data_ptr() if d_a is not None else None
        if entry == "radius":
            vmap.plan_batch_radius_device(d_s.data_ptr(), d_g.data_ptr(), d_r.data_ptr(), pa, *args, d_ex.data_ptr() + 8, **kw)
        else:
            d_v = to_dev(np.asarray(view_of, dtype=np.int32))
            vmap.plan_batch_radius_views_device(d_s.data_ptr(), d_g.data_ptr(), d_r.data_ptr(), pa, *args, d_v.data_ptr(), n_views,
                                                d_ex.data_ptr() + 8, **kw)
    vmap.sync()
    for d, per in ((d_paths, row), (d_np, 4), (d_ex, 8)):
        assert bool((d[:per] == POISON).all()) and bool((d[(n + 1) * per:] == POISON).all()), "a guard row was written"
    body = d_paths[row:(n + 1) * row].view(n, row)
    untouched = (body == POISON).all(dim=1).cpu().numpy()
    paths = body.cpu().numpy().view(np.float64).reshape(n, max_points, 3)
    return paths, d_np[4:(n + 1) * 4].cpu().numpy().view(np.int32).copy(), d_ex[8:(n + 1) * 8].cpu().numpy().view(np.int64).copy(), untouched


def assert_p5(dev, hst, what, skip=()):
    """P5: n_points, expansions and every vertex equal the host restatement's, bit for bit"""
    dp, dn, dex = dev[:3]
    hp, hn, hex_ = hst[:3]
    keep = np.ones(len(hn), dtype=bool)
    keep[list(skip)] = False
    assert np.array_equal(dn[keep], hn[keep]), (what, np.nonzero((dn != hn) & keep)[0][:8], dn[(dn != hn) & keep][:8], hn[(dn != hn) & keep][:8])
    assert np.array_equal(dex[keep], hex_[keep]), (what, np.nonzero((dex != hex_) & keep)[0][:8])
    live = (np.arange(hp.shape[1])[None, :] < np.maximum(hn, 0)[:, None]) & keep[:, None]
    # bit for bit; a zero of either sign is a zero (fmax(-0.0, 0.0) may return either)
    same = ((dp.view(np.int64) == hp.view(np.int64)) | ((dp == 0.0) & (hp == 0.0))).all(axis=2)
    assert same[live].all(), (what, np.nonzero((~same & live).any(axis=1))[0][:8])


def assert_same_bytes(a, b, what):
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), what
    assert np.array_equal(a[0].view(np.int64), b[0].view(np.int64)), what


def model_checks(sc, dev, queries, what):
    for q in queries:
        pe.check_answer(sc, q, dev[0][q], dev[1][q], what)


# ---- a. exhaustive tiny grids, h. one kernel text, three entry points -------------------------------------------------------------------------------
def read_views(vmap, sc, n_views=2):
    """view 0 knows every point, view 1 none (an empty map)"""
    n_cloud = len(sc.cloud)
    words = max((n_cloud + 31) // 32, 1)
    mask = np.zeros((n_views, words), dtype=np.uint32)
    mask[0] = 0xffffffff
    d_cloud, d_mask = to_dev(sc.cloud), to_dev(mask)
    cloud, cells, res, center, zg, zmax, infl = sc.map_args()
    vmap.read_views_device(d_cloud.data_ptr() if n_cloud else None, n_cloud, d_mask.data_ptr() if n_cloud else None, words, n_views, cells, res,
                           center, zg, zmax, infl)
    vmap.sync()
    return d_cloud, d_mask


@pytest.mark.parametrize("mode", range(3), ids=MODE_IDS)
@pytest.mark.parametrize("name", pe.TINY_NAMES)
def test_tiny_grids_all_pairs(m, name, mode):
    """All 78 400 ordered pairs of cells of an 8 x 7 x 5 grid — cubes clipped by every face, edge and corner, overlapping and nested cubes,
    the goal on, beside and behind every ray and cone that tube_contact, cone_dirty and goal_on_ray reason about: P5 for all of them, P1 -
    P4 for a fixed sample of 2000.  Then the same queries through the other two entry points: the radius entry point (radius large,
    every query active) and the view entry point on two views (0: every point, 1: none) give the same bytes with view_of = 0, zero
    vertices for view_of = -1 and = n_views, and with view_of = 1 what the plain entry point gives on an empty cloud."""
    search, records = MODES[mode]
    sc = pe.tiny_scene(name)
    read(m, sc, search, records)
    assert np.array_equal(m.occupancy(), sc.occ)
    dev = plan(m, sc.starts, sc.goals)
    assert_p5(dev, host(sc, search, max_points=16), "%s %s" % (name, MODE_IDS[mode]))
    model_checks(sc, dev, pe.tiny_sample(name), "device " + MODE_IDS[mode])
    n = len(sc.starts)
    assert_same_bytes(plan(m, sc.starts, sc.goals, entry="radius", active=np.ones(n)), dev, "radius entry point")
    keep = read_views(m, sc)
    assert np.array_equal(m.view_occupancy(0), sc.occ) and not m.view_occupancy(1).any()
    view_of = np.zeros(n, dtype=np.int32)
    assert_same_bytes(plan(m, sc.starts, sc.goals, entry="views", view_of=view_of, n_views=2), dev, "view entry point, view 0")
    sub = pe.tiny_sample(name)
    view_of = np.where(np.arange(len(sub)) % 2 == 0, -1, 2)
    none = plan(m, sc.starts[sub], sc.goals[sub], entry="views", view_of=view_of, n_views=2)
    assert not none[1].any() and not none[2].any() and none[3].all()
    empty = pe.tiny_scene("empty/m%d" % sc.m_free)
    one = plan(m, sc.starts[sub], sc.goals[sub], entry="views", view_of=np.ones(len(sub)), n_views=2)
    hst = host(empty, search, max_points=16)
    assert_p5(one, tuple(a[sub] for a in hst[:3]), "view 1: the empty map")
    del keep


# ---- b. jump lengths at the lane batches ------------------------------------------------------------------------------------------------------
_EMPTY = {}


def empty_twin(sc):
    """the scene's queries on the same lattice without a cloud: what view 1 holds"""
    if sc.name not in _EMPTY:
        _EMPTY[sc.name] = pe.Scene(sc.name + " (empty)", np.zeros_like(sc.pattern), sc.starts, sc.goals, inflation=sc.inflation, oz=sc.origin[2])
    return _EMPTY[sc.name]


def other_entry_points(vmap, sc, search, dev, what, skip=(), radius=None, **kw):
    """One kernel text, three entry points: the launch `dev` of the plain entry point (map read, search and records set) again through
    fh_map_plan_batch_radius_device (every query active) and through fh_map_plan_batch_radius_views_device on two views (0: every
    point, 1: none): the same bytes with view_of = 0, zero vertices for view_of = -1 and = n_views, and with view_of = 1 the host's
    answer on the empty lattice (skip: queries at a limit the host does not have).  radius: the clip radii `dev` was made with."""
    n = len(sc.starts)
    if radius is None:
        assert_same_bytes(plan(vmap, sc.starts, sc.goals, entry="radius", active=np.ones(n), **kw), dev, what + ": radius entry point")
    keep = read_views(vmap, sc)
    got = plan(vmap, sc.starts, sc.goals, entry="views", radius=radius, view_of=np.zeros(n), n_views=2, **kw)
    assert_same_bytes(got, dev, what + ": view entry point, view 0")
    for v in (-1, 2):
        none = plan(vmap, sc.starts, sc.goals, entry="views", radius=radius, view_of=np.full(n, v), n_views=2, **kw)
        assert not none[1].any() and not none[2].any() and none[3].all(), (what, v)
    if radius is None:
        one = plan(vmap, sc.starts, sc.goals, entry="views", view_of=np.ones(n), n_views=2, **kw)
        hkw = dict(kw)
        hkw.setdefault("max_points", 16)
        assert_p5(one, host(empty_twin(sc), search, **hkw), what + ": view 1, the empty map", skip=skip)
    del keep


def scene_all_modes(m, sc, max_points=16, modes=(0, 1, 2), legs=True):
    out = []
    for mode in modes:
        search, records = MODES[mode]
        read(m, sc, search, records)
        if mode == modes[0]:
            assert np.array_equal(m.occupancy(), sc.occ)
        dev = plan(m, sc.starts, sc.goals, max_points=max_points)
        print("%s %s: n_points %s expansions %s" % (sc.name, MODE_IDS[mode], dev[1][:8], dev[2][:8]))
        assert_p5(dev, host(sc, search, max_points=max_points), "%s %s" % (sc.name, MODE_IDS[mode]))
        for q in range(len(sc.starts)):
            pe.check_answer(sc, q, dev[0][q], dev[1][q], "device " + MODE_IDS[mode], legs=legs)
        other_entry_points(m, sc, search, dev, "%s %s" % (sc.name, MODE_IDS[mode]), max_points=max_points)
        out.append(dev)
    return out


@pytest.mark.parametrize("j", range(len(pe.JUMP_CASES)), ids=lambda j: "%d-%s-%d-%s" % pe.JUMP_CASES[j])
def test_jump_lengths_at_the_lane_batches(ms, j):
    """A straight jump that ends 63 / 64 / 65 / 127 / 128 / 129 cells out (64 ray cells are tested at once), a plane-diagonal one at 31 / 32
    / 33 / 64 / 65 (32 diagonal cells), a space-diagonal one at 7 / 8 / 9 / 16 / 17 (8) — ended by the goal, by forced neighbours (a hole in a
    wall; straight jumps also one occupied cell beside the ray), by a wall —
    from the jump table (near = False) and cell by cell in batches (near = True: an occupied cell inside the start's freed cube makes
    the boxes matter from the first cell on)."""
    n1, kind, L, near = pe.JUMP_CASES[j]
    sc = pe.jump_scene(n1, kind, L, near)
    for dev in scene_all_modes(ms, sc):
        if kind == "goal":
            assert dev[1][0] == 2
        elif kind == "hole":
            e = sc.meta["end"]
            assert dev[1][0] == 3 and np.array_equal(dev[0][0, 1], sc.centre(e if n1 == 1 else (e[0] + 1, e[1], e[2])))
        elif kind == "blocked":
            assert dev[1][0] == 0


@pytest.mark.parametrize("k", pe.FREED_TUBE_CASES)
def test_tube_contact_at_the_batch_boundary(ms, k):
    """The table says the jump ends at ray cell 64 (65), but the cell that forces it lies in the goal's freed cube: the table holds up to
    cell 63 (64), the walk goes on cell by cell from there.  Without the + 1 margin of tube_contact the jump would end at the obstacle."""
    scene_all_modes(ms, pe.freed_tube_scene(k))


# ---- c. the clean-up in batches ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_raw", pe.RAW_LENGTHS)
def test_clean_up_of_a_staircase(ms, n_raw):
    """a raw path of 63 / 64 / 65 / 128 / 129 cells that changes direction at every cell: removeLinePts keeps them, 64 lanes a pass"""
    scene_all_modes(ms, pe.staircase_scene(n_raw), max_points=160)


@pytest.mark.parametrize("L,h", pe.LEG_CASES)
def test_ray_test_at_its_pass_boundary(ms, L, h):
    """Planner::blocked samples 64 points a pass.  pe.leg_scene: the shortcut P -> b that removeCornerPts tries is a leg of 52 / 80 / 81 /
    160 cells (65 / 100 / 101 / 200 steps), and one occupied cell, first met by sample 64 (the last lane of the first pass) or 65 (the
    first lane of the second), refuses it.  A ray test that misses that sample takes the shortcut: the apex A vanishes from the answer."""
    sc = pe.leg_scene(L, h)
    for dev in scene_all_modes(ms, sc, legs=False):
        v = dev[0][0, :dev[1][0]]
        k = [i for i in range(len(v)) if np.array_equal(v[i], sc.meta["P"])]
        assert len(k) == 1 and np.array_equal(v[k[0] + 1], sc.meta["A"]) and np.array_equal(v[k[0] + 2], sc.meta["b"])


def test_clean_up_of_a_straight_raw_path(ms):
    for dev in scene_all_modes(ms, pe.straight_raw_scene(), max_points=160):
        assert dev[1][0] == 2


# ---- d. the A* open list beyond its first chunks --------------------------------------------------------------------------------------------------
def test_open_list_chains_and_releases_chunks():
    """pe.comb_scene: one sub-list of the open list grows to three chained chunks and drains to empty again (the instrument
    astar_open_profile proves it on the CPU); the device expands exactly the cells the instrument and the host do, finds no path, and
    answers the reachable query of the same batch."""
    sc = pe.comb_scene()
    prof = pm.astar_open_profile(sc.occ, sc.cell(sc.starts[0]), sc.cell(sc.goals[0]), sc.m_free)
    assert max(prof["peak"]) > 128
    vmap = capi.Map(0)
    try:
        vmap.set_sched(waves_per_cu=1)   # (3.5 M cells: a cell record per cell and wavefront)
        read(vmap, sc, "astar", 0)
        assert np.array_equal(vmap.occupancy(), sc.occ)
        dev = plan(vmap, sc.starts, sc.goals)
        print("comb: n_points %s expansions %s, the instrument %d" % (dev[1], dev[2], prof["pops"]))
        assert_p5(dev, host(sc, "astar", max_points=16), "comb")
        far = pm.astar_open_profile(sc.occ, sc.cell(sc.starts[1]), sc.cell(sc.goals[1]), sc.m_free)
        assert dev[1][0] == 0 and dev[2][0] == prof["pops"] and far["found"] and dev[1][1] >= 2 and dev[2][1] == far["pops"]   # P1, by the instrument
    finally:
        vmap.close()


# ---- e. limits at their boundary -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["end", "middle"])
def test_key_range_at_its_boundary(ms, which):
    """A* ends a query with -2 as soon as a cell with f >= 2040 cells is opened (include/fasterhip.h) — f = 2040.0 exactly included — and
    the host restatement answers 0 there; below the limit both give the path.  The jump point search has no such limit."""
    sc = pe.key_range_scene(which)
    limit = np.array(sc.meta["limit"])
    read(ms, sc, "astar", 0)
    dev = plan(ms, sc.starts, sc.goals)
    hst = host(sc, "astar", max_points=16)
    print("%s: device n_points %s expansions %s, host n_points %s" % (sc.name, dev[1], dev[2], hst[1]))
    assert np.array_equal(dev[1], np.where(limit, -2, 2)) and np.array_equal(hst[1], np.where(limit, 0, 2))
    assert np.array_equal(dev[2], hst[2])
    assert_p5(dev, hst, sc.name, skip=np.nonzero(limit)[0])
    model_checks(sc, dev, np.nonzero(~limit)[0], "device astar")
    other_entry_points(ms, sc, "astar", dev, sc.name + " astar", skip=np.nonzero(limit)[0])   # (-2 comes out of plan_views_kernel as well)
    for dev in scene_all_modes(ms, sc, modes=(1, 2)):
        assert (dev[1] == 2).all()


@pytest.mark.parametrize("records", [0, 16384])
def test_raw_path_limit_at_its_boundary(ms, records):
    """MAXRAW = 4096 entries of the parent chain (pe.raw_limit_scene: a corridor in which every cell is a jump point): the goal with a
    chain of exactly 4096 entries gets the host's path, the one with 4097 gets -2 (the host restatement has no such limit and returns
    a path); the short queries on either side of them keep their answers.  A* cannot get there — 4095 moves cost more than the 2040
    cells of its key range — so for A* both are -2 already (host: 0)."""
    sc = pe.raw_limit_scene()
    read(ms, sc, "jps", records)
    dev = plan(ms, sc.starts, sc.goals)
    hst = host(sc, "jps", max_points=16)
    print("raw limit, jps, records %d: device n_points %s expansions %s, host n_points %s" % (records, dev[1], dev[2], hst[1]))
    assert list(dev[2]) == sc.meta["chain"]
    assert dev[1][2] == -2 and hst[1][2] >= 2
    assert_p5(dev, hst, "raw limit", skip=[2])
    model_checks(sc, dev, (0, 1, 3), "device jps")
    other_entry_points(ms, sc, "jps", dev, "raw limit, records %d" % records)   # (the empty lattice has no jump points: no limit there)
    if records == 0:
        read(ms, sc, "astar", 0)
        dev = plan(ms, sc.starts, sc.goals)
        hst = host(sc, "astar", max_points=16)
        assert list(dev[1][1:3]) == [-2, -2] and list(hst[1][1:3]) == [0, 0]
        assert_p5(dev, hst, "raw limit astar", skip=[1, 2])
        other_entry_points(ms, sc, "astar", dev, "raw limit astar", skip=[1, 2])


@pytest.mark.parametrize("mode", range(3), ids=MODE_IDS)
def test_max_points_at_its_boundary(ms, mode):
    """A list of exactly max_points vertices is returned, one more gives -1; the clip to max_poly + 1 comes first and may bring an
    over-long list back under max_points; start = goal needs max_points = 2 (with a spacing its goal is a duplicate by the 1e-9 rule: one
    vertex), and max_points = 1 is an argument error."""
    search, records = MODES[mode]
    sc = pe.max_points_scene()
    read(ms, sc, search, records)
    for kw, want in ((dict(max_points=16, max_vertex_dist=0.25), [7, 1, 3]), (dict(max_points=7, max_vertex_dist=0.25), [7, 1, 3]),
                     (dict(max_points=6, max_vertex_dist=0.25), [-1, 1, 3]), (dict(max_points=6, max_vertex_dist=0.25, max_poly=4), [5, 1, 3]),
                     (dict(max_points=2, max_vertex_dist=0.25, max_poly=4), [-1, 1, -1]), (dict(max_points=2), [2, 2, 2])):
        dev = plan(ms, sc.starts, sc.goals, **kw)
        assert list(dev[1]) == want, (kw, dev[1])
        assert_p5(dev, host(sc, search, **kw), str(kw))
        other_entry_points(ms, sc, search, dev, "max points %s" % kw, **kw)
    with pytest.raises(capi.FasterHipError):
        plan(ms, sc.starts, sc.goals, max_points=1)


# ---- f. the vertex epilogue -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1], ids=MODE_IDS[:2])
@pytest.mark.parametrize("name", ["wall/m1", "random/m2"])
def test_vertex_epilogue(ms, name, mode):
    """createMoreVertexes with spacings of which legs are exact multiples (the 1e-9 duplicate rule), of which none is, and larger than
    every leg; the clip to max_poly + 1: the model more_vertexes and the host restatement, bit for bit."""
    search, records = MODES[mode]
    sc = pe.tiny_scene(name)
    idx = pe.tiny_sample(name)[:400]
    read(ms, sc, search, records)
    plain = plan(ms, sc.starts[idx], sc.goals[idx])
    sub = pe.Scene(sc.name + " sample", sc.pattern, sc.starts[idx], sc.goals[idx], inflation=sc.inflation)
    for spacing, _ in pe.SPACINGS:
        for max_poly in (0, 3):
            kw = dict(max_points=64, max_vertex_dist=spacing, max_poly=max_poly)
            dev = plan(ms, sc.starts[idx], sc.goals[idx], **kw)
            assert_p5(dev, host(sc, search, idx=idx, key=name, **kw), "%s spacing %g max_poly %d" % (name, spacing, max_poly))
            other_entry_points(ms, sub, search, dev, "%s spacing %g max_poly %d" % (name, spacing, max_poly), **kw)
            for q in range(len(idx)):
                if plain[1][q] > 0:
                    want = pm.more_vertexes(plain[0][q, :plain[1][q]], spacing, max_poly)
                    assert dev[1][q] == len(want) and np.array_equal(dev[0][q, :dev[1][q]], want), (name, spacing, max_poly, idx[q])


def test_sphere_clip(ms):
    """fh_map_plan_batch_radius_device with a radius that puts vertex 1 exactly on the sphere (strict >: it stays, the crossing lies on a
    later leg), a sphere inside the first leg, the goal inside the sphere (no crossing point): the model clip_to_sphere bit for bit.
    fh_map_set_sphere with |goal - start| of 0.0005 m and of exactly 0 — the radius min(d - 0.001, Ra) is negative, the start itself lies
    outside: the path stays whole and finite, as in the host restatement."""
    sc = pe.tiny_scene("wall/m1")
    idx = pe.tiny_sample("wall/m1")[:400]
    read(ms, sc, "jps", 0)
    plain = plan(ms, sc.starts[idx], sc.goals[idx])
    qs, radius = [], []
    for q in range(len(idx)):
        if plain[1][q] >= 3 and len(qs) < 150:
            v = plain[0][q, :plain[1][q]]
            d, r1 = pm._dist(v[-1], v[0]), pm._dist(v[1], v[0])
            for r in ((r1,) if r1 < d else ()) + (0.5 * r1, d - 0.001, d + 1.0):   # (the radius as it is: this entry point takes no minimum)
                qs.append(q)
                radius.append(r)
    assert len(qs) >= 100
    qs = np.array(qs)
    dev = plan(ms, sc.starts[idx][qs], sc.goals[idx][qs], entry="radius", radius=radius)
    sub = pe.Scene(sc.name + " clipped", sc.pattern, sc.starts[idx][qs], sc.goals[idx][qs], inflation=sc.inflation)
    other_entry_points(ms, sub, "jps", dev, "sphere clip", radius=radius)   # (the same radii through plan_views_kernel)
    on_sphere = 0
    for k, q in enumerate(qs):
        v = plain[0][q, :plain[1][q]]
        want = np.array(pm.clip_to_sphere(v, radius[k]))
        assert dev[1][k] == len(want) and np.array_equal(dev[0][k, :dev[1][k]], want), (idx[q], radius[k], dev[0][k, :dev[1][k]], want)
        if radius[k] == pm._dist(v[1], v[0]):
            on_sphere += 1
            assert np.array_equal(dev[0][k, 1], v[1])
    assert on_sphere >= 20
    c = sc.centre((6, 3, 2))
    starts, goals = np.array([c, c, c]), np.array([c + [0.0005, 0.0, 0.0], c, c + [0.0, 0.5, 0.0]])
    for search in ("astar", "jps"):
        read(ms, sc, search, 0)
        ms.set_sphere(1.0)
        try:
            dev = plan(ms, starts, goals)
        finally:
            ms.set_sphere(0.0)
        with frontend.host_settings(search, 1.0):
            hst = frontend.plan_batch(*sc.map_args(), starts, goals, max_points=16)
        print("negative radius: device %s host %s" % (dev[0][:2, :2].tolist(), hst[0][:2, :2].tolist()))
        assert_p5(dev, hst, "negative radius " + search)
        assert list(dev[1]) == [2, 2, 2] and np.isfinite(dev[0][:, :2]).all()
        assert np.array_equal(dev[0][0, :2], [starts[0], goals[0]]) and np.array_equal(dev[0][1, :2], [starts[1], goals[1]])


# ---- g. the lattice faces and bad numbers -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", range(3), ids=MODE_IDS)
def test_lattice_faces_and_bad_numbers(ms, mode):
    """Starts and goals on the faces of the lattice, one ulp inside and outside, on cell borders, below z = 0, with NaN and +-inf: the
    cell is the model's, the answer the host restatement's; a query that is outside, not finite or not active answers 0 vertices and 0
    expansions and leaves its row alone — also through the view entry point."""
    search, records = MODES[mode]
    sc = pe.lattice_scene()
    want = np.array([pm.inside(sc.cell(a), sc.dims) and pm.inside(sc.cell(b), sc.dims) for a, b in zip(sc.starts, sc.goals)])
    read(ms, sc, search, records)
    n = len(want)
    keep = read_views(ms, sc)
    for entry in ("plain", "radius", "views"):
        dev = plan(ms, sc.starts, sc.goals, entry=entry, view_of=np.zeros(n), n_views=2)
        assert np.array_equal(dev[1] > 0, want), (entry, np.nonzero((dev[1] > 0) != want)[0])
        assert_p5(dev, host(sc, search, max_points=16), "lattice " + entry)
        assert not dev[1][~want].any() and not dev[2][~want].any() and dev[3][~want].all()
        model_checks(sc, dev, np.nonzero(want)[0], "device " + MODE_IDS[mode])
    active = (np.arange(n) % 3 != 0).astype(np.int32)
    off = plan(ms, sc.starts, sc.goals, entry="radius", active=active)
    assert not off[1][active == 0].any() and not off[2][active == 0].any() and off[3][active == 0].all()
    on = active == 1
    assert np.array_equal(off[1][on], dev[1][on]) and np.array_equal(off[0][on].view(np.int64), dev[0][on].view(np.int64))
    del keep


# ---- i. launch order --------------------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_launch_order():
    """plan_order_hist_kernel / plan_order_scatter_kernel run when a batch has more queries than wavefronts hold a workspace: with one
    wavefront per CU a batch of waves + 1 queries is ordered.  Duplicates, zero distance, all queries in one class, distances beyond class
    63 (starts far outside the map) and non-finite queries: the same bytes as with launch_order = 0 and with the default scheduling;
    also for n = waves (not ordered) and n = 1."""
    sc = pe.tiny_scene("wall/m1")
    lat = pe.lattice_scene()
    waves = torch.cuda.get_device_properties(0).multi_processor_count
    n = waves + 1
    rng = np.random.default_rng(3)
    pick = rng.choice(len(sc.starts), n, replace=True)
    batches = {}
    s, g = sc.starts[pick].copy(), sc.goals[pick].copy()
    s[5:25], g[5:25] = s[5], g[5]                      # duplicates
    g[25:35] = s[25:35]                                # zero distance
    s[35:45] += [-400.0, 0.0, 0.0]                     # beyond class 63 (outside the map: no path)
    bad = [i for i, k in enumerate(lat.meta["kinds"]) if k == "nonfinite"]
    k = min(len(bad), n - 45)
    s[45:45 + k], g[45:45 + k] = lat.starts[bad[:k]], lat.goals[bad[:k]]
    batches["mixed"] = (s, g)
    batches["one class"] = (np.tile(sc.starts[pick[0]], (n, 1)) + rng.uniform(-0.01, 0.01, (n, 3)), np.tile(sc.goals[pick[0]], (n, 1)))
    for search in ("astar", "jps"):
        got = {}
        for sched in ((1, 1), (1, 0), (0, 1)):
            vmap = capi.Map(0)
            try:
                vmap.set_sched(*sched)
                read(vmap, sc, search, 0)
                got[sched] = {name: [plan(vmap, b[0][:k], b[1][:k]) for k in (n, waves, 1)] for name, b in batches.items()}
            finally:
                vmap.close()
        for name in batches:
            for j in range(3):
                for sched in ((1, 0), (0, 1)):
                    assert_same_bytes(got[sched][name][j], got[(1, 1)][name][j], (search, name, j, sched))
                    assert np.array_equal(got[sched][name][j][3], got[(1, 1)][name][j][3])
        with frontend.host_settings(search, 0.0):
            hst = frontend.plan_batch(*sc.map_args(), batches["mixed"][0], batches["mixed"][1], max_points=16)
        assert_p5(got[(1, 1)]["mixed"][0], hst, "ordered batch " + search)
        assert (got[(1, 1)]["mixed"][0][1] > 0).sum() > n // 2


# ---- j. state carried between calls ------------------------------------------------------------------------------------------------------------
def test_state_carried_between_calls():
    """One Map: a grid, a smaller one, a larger one, the first again, with the search and the records switched in between — the serial
    stamps, the workspace re-sizing and the jump tables after a re-read: every answer is the host restatement's and that of a fresh Map."""
    tiny, small, big = pe.tiny_scene("wall/m1"), pe.max_points_scene(), pe.jump_scene(1, "hole", 65, True)
    sub = pe.tiny_sample("wall/m1")
    steps = [(tiny, "jps", 0), (small, "jps", 0), (big, "jps", 1024), (tiny, "astar", 0), (big, "astar", 0), (small, "jps", 1024), (tiny, "jps", 1024),
             (tiny, "jps", 0)]
    vmap = capi.Map(0)
    try:
        for i, (sc, search, records) in enumerate(steps):
            idx = sub if sc is tiny else np.arange(len(sc.starts))
            read(vmap, sc, search, records)
            dev = plan(vmap, sc.starts[idx], sc.goals[idx])
            assert_p5(dev, host(sc, search, idx=idx, key="carried", max_points=16), "step %d %s %s" % (i, sc.name, search))
            if i in (2, 3):
                fresh = capi.Map(0)
                try:
                    read(fresh, sc, search, records)
                    assert_same_bytes(plan(fresh, sc.starts[idx], sc.goals[idx]), dev, "fresh map, step %d" % i)
                finally:
                    fresh.close()
    finally:
        vmap.close()
