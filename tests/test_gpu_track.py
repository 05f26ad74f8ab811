"""GPU tests of the tracker of moving obstacles (fh_fleet_obstacle_track_device, Fleet.enable_tracking / track;
include/fasterhip_track.h): every byte of the tracks, the records, the seers and the info equals the model (tests/track_model.py, brute
force over all pairs and all samples of a ray) — on every hand case of tests/track_cases.py step by step, on the two cases found by
seeded searches, on shapes at the edges of a chunk of vehicles and of a grid of obstacles, on rays of every number of rounds, with the
seer in the second and third chunk behind chunks that are all in range and all blocked and at lanes 0 and 63, on an empty map against
no map, with m = 0, and the two argument rules that need a map.  Then the fleet: one that tracks equals one that is told, an obstacle
behind a wall has no bit until somebody has a clear ray to it, and the closed loop of the crossing scene, printed."""
import numpy as np
import pytest

from faster_amd import abi, capi

import link_los_cases as lc
import track_cases as tc
import track_model as tmod

pytestmark = pytest.mark.gpu
GUARD, POISON = 64, 0xA5
SCENE_Z = (1.0, -1.0, 0.5)    # right of the wall, away from the door
DOOR_Z = (1.0, 0.9, 0.5)      # right of the wall, on the line through the middle of the door


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch  # noqa: F401  (torch before the HIP library: one HIP runtime in the process)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def maps():
    """world name -> Map or None; the device's grids are what tests/track_cases.py hands to the model."""
    made = {None: None}
    for name, cloud in (("scene", lc.cloud()), ("empty", np.zeros((0, 3)))):
        m = capi.Map(0)
        m.read(cloud, lc.READ["cells"], lc.READ["res"], lc.READ["center"], lc.READ["z_ground"], lc.READ["z_max"], lc.READ["inflation"])
        dims, origin = m.dims()
        assert tuple(int(d) for d in dims) == lc.DIMS and origin.tolist() == list(lc.ORIGIN)
        assert np.array_equal(m.occupancy(), tc.world(name)[0])
        made[name] = m
    yield made
    for m in made.values():
        if m is not None:
            m.close()


def vehicles_at(pos):
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    v = np.zeros(len(pos), dtype=abi.vehicle_dtype)
    v["state"]["pos"] = pos
    v["state"]["vel"], v["plan_head"], v["status"] = 7.0, -3, 9      # (nothing of a record but the position is read)
    return v


def guarded(a, nbytes=None):
    """Device bytes with poisoned guards on both sides: (whole tensor, pointer to the payload); a = None: a poisoned payload."""
    import torch

    n = len(a.tobytes()) if a is not None else nbytes
    t = torch.full((n + 2 * GUARD,), POISON, dtype=torch.uint8, device="cuda:0")
    if a is not None and n:
        t[GUARD:GUARD + n] = torch.from_numpy(np.frombuffer(a.tobytes(), dtype=np.uint8).copy()).to("cuda:0")
    return t, t.data_ptr() + GUARD


def payload(t, dtype):
    raw = t.cpu().numpy()
    assert (raw[:GUARD] == POISON).all() and (raw[-GUARD:] == POISON).all()
    return raw[GUARD:-GUARD].view(dtype).copy()


def device_track(c, vmap, par, truth, t0, tick, pos, tracks):
    """(tracks, est, seer, info) of one call on device copies, every output poisoned before and guarded on both sides."""
    import torch

    m, v = len(truth), vehicles_at(pos)
    d_truth, d_veh, d_tracks = guarded(truth), guarded(v), guarded(tracks)
    d_est, d_seer, d_info = guarded(None, 64 * m), guarded(None, 4 * m), guarded(None, 32)
    torch.cuda.synchronize()
    c.fleet_obstacle_track_device(vmap, par, d_truth[1], m, t0, tick, d_veh[1] if len(v) else None, len(v), d_tracks[1], d_est[1], d_seer[1], d_info[1])
    c.sync()
    assert payload(d_truth[0], abi.obstacle_dtype).tobytes() == truth.tobytes() and payload(d_veh[0], abi.vehicle_dtype).tobytes() == v.tobytes()
    return (payload(d_tracks[0], abi.obstacle_track_dtype), payload(d_est[0], abi.obstacle_dtype), payload(d_seer[0], np.int32),
            payload(d_info[0], np.int64))


def assert_same(got, want, what):
    for name, g, w in zip(("tracks", "est", "seer", "info"), got, want):
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero([x.tobytes() != y.tobytes() for x, y in zip(g, w)])
            raise AssertionError("%s: %s differs at %s: got %s, want %s" % (what, name, bad[:8], g[bad[:2]], w[bad[:2]]))


def check_case(c, maps, case, what):
    """Every step of the case on the device against the model, the device fed with its own tracks."""
    want = tc.play(tmod, case)
    tracks = np.zeros(len(case["steps"][0][0]), dtype=abi.obstacle_track_dtype)
    for step, ((truth, t0, tick, pos), w) in enumerate(zip(case["steps"], want)):
        got = device_track(c, maps[case["world"]], case["par"], truth, t0, tick, pos, tracks)
        assert_same(got, w, "%s step %d" % (what, step))
        tracks = got[0]
    return want


# ---- 1. the hand cases, step by step (sequences of 1 .. 10 calls, gaps and max_age, the jump through the gate, a repeated tick, n = 0) ----
@pytest.mark.parametrize("name", sorted(tc.CASES))
def test_hand_case(ctx, maps, name):
    check_case(ctx, maps, tc.CASES[name], name)


def test_the_cases_of_the_two_seeded_searches(ctx, maps):
    want = check_case(ctx, maps, tc.orientation_case(tmod), "orientation")
    assert want[0][2].tolist() == [0]                                   # (the ray from the vehicle is free; from the obstacle it is blocked)
    check_case(ctx, maps, tc.summation_case(tmod), "summation order")


def test_an_empty_map_gives_the_bytes_of_no_map(ctx, maps):
    rng = np.random.default_rng(3)
    pos = rng.uniform((-2.1, -2.1, 0.1), (2.1, 2.1, 1.9), size=(70, 3))
    truth = abi.make_obstacles(rng.uniform((-2.5, -2.5, -0.2), (2.5, 2.5, 2.3), size=(9, 3)), None, 0.1)
    tracks = np.zeros(9, dtype=abi.obstacle_track_dtype)
    a = device_track(ctx, None, tc.par(1.0, min_obs=1), truth, 0, 4, pos, tracks)
    b = device_track(ctx, maps["empty"], tc.par(1.0, min_obs=1), truth, 0, 4, pos, tracks)
    assert_same(a, b, "empty map against no map")
    assert 0 < int(a[3][0]) < 9


# ---- 2. shapes: n = 1, 63, 64, 65, 129, 1025 and m = 1, 2, 65, 1025; four calls on one set of tracks ----------------------------------------
def random_world(rng, n, m):
    """Vehicles and obstacles all over the scene and a little outside it, half of the vehicles on a 0.1 m grid (samples on cell
    boundaries, obstacles exactly at r_detect); vehicles with NaN and infinite positions; truth records that are off, not finite and
    with a negative radius; obstacles above and beside the map."""
    pos = rng.uniform((-2.1, -2.1, 0.1), (2.1, 2.1, 1.9), size=(n, 3))
    pos[:n // 2] = np.round(pos[:n // 2] * 10.0) / 10.0
    for k in range(2, n, 7):
        pos[k, k % 3] = (np.nan, np.inf, -np.inf)[k % 3]
    p0 = np.round(rng.uniform((-2.4, -2.4, -0.2), (2.4, 2.4, 2.3), size=(m, 3)) * 10.0) / 10.0
    truth = abi.make_obstacles(p0, rng.uniform(-1.0, 1.0, size=(m, 3)), rng.uniform(0.0, 0.5, size=m))
    for o in range(3, m, 11):
        truth["flags"][o] = 0
    for o in range(5, m, 13):
        truth["p0"][o, 1] = np.nan
    for o in range(7, m, 17):
        truth["radius"][o] = -0.25
    for o in range(9, m, 19):
        truth["v"][o, 2] = np.inf
    return pos, truth


SHAPES = [(1, 1), (63, 2), (64, 65), (65, 1), (129, 2), (1025, 65), (3, 1025), (129, 65)]


@pytest.mark.parametrize("n,m", SHAPES)
def test_shapes_equal_the_model(ctx, maps, n, m):
    rng = np.random.default_rng(100 * n + m)
    pos, truth = random_world(rng, n, m)
    r = 0.6 if n > 200 else 1.0 if n > 64 else 1.5
    case = dict(par=tc.par(r, fit=3, min_obs=2, max_age=6, gate=0.2, grow=0.25), world="scene",
                steps=[(truth, t, t, pos + 0.01 * t) for t in (0, 2, 5, 9)])
    want = check_case(ctx, maps, case, "n %d m %d" % (n, m))
    seen = int(want[0][3][0])
    assert (0 < seen < m) if m > 2 and n > 2 else True
    if m >= 65 and n >= 64:
        flags = np.bitwise_or.reduce(np.concatenate([w[0]["flags"] for w in want]))
        assert any(int(w[3][1]) > 0 for w in want) and flags == abi.FH_TRACK_SEEN | abi.FH_TRACK_LOST | abi.FH_TRACK_RESET   # (what the steps reach)
    if m >= 65 and n > 64:
        assert (want[0][2] >= 64).any()                                              # a seer beyond the first chunk


# ---- 3. rays of K - 1 = 0, 1, 63, 64, 65 and 129 samples: none, one round, the edge of a round, two and three rounds ------------------------
@pytest.mark.parametrize("samples", [0, 1, 63, 64, 65, 129])
def test_ray_lengths(ctx, maps, samples):
    """The vehicle `dist` left of the obstacle on the line through the door (free, however long: the far samples are outside the map)
    and on the line through the wall (blocked as soon as the ray is longer than the obstacle's side of the wall: the hit is in the
    LAST round of the ray)."""
    dist = (samples + 0.5) * 0.5 * lc.RES
    for z, free in ((DOOR_Z, True), (SCENE_Z, dist < 0.6)):
        pos = [(z[0] - dist, z[1], z[2])]
        p = [float(x) for x in pos[0]]
        dd = [z[a] - p[a] for a in range(3)]
        assert max(1, int(np.ceil(np.sqrt(dd[0] * dd[0] + dd[1] * dd[1] + dd[2] * dd[2]) / (0.5 * lc.RES)))) == samples + 1
        want = check_case(ctx, maps, tc.los_case(z, pos, r_detect=13.5), "%d samples to %s" % (samples, z))
        assert want[0][2].tolist() == [0 if free else -1]


# ---- 4. where the seer stands: behind whole chunks that are in range and blocked, and at the two ends of a chunk --------------------------
@pytest.mark.parametrize("seer", [0, 63, 64, 127, 128, 191])
def test_the_seer_behind_blocked_chunks_and_at_lanes_0_and_63(ctx, maps, seer):
    """Every vehicle in front of the seer stands left of the wall, in range and blocked; the seer and every vehicle behind it stand on
    the obstacle's side: the smallest of them is named."""
    rng = np.random.default_rng(seer)
    n = 200
    pos = rng.uniform((-1.1, -1.9, 0.2), (-0.3, 0.6, 1.8), size=(n, 3))
    pos[seer:] = rng.uniform((0.5, -1.9, 0.2), (1.9, 0.0, 1.8), size=(n - seer, 3))
    want = check_case(ctx, maps, tc.los_case(SCENE_Z, pos, r_detect=3.0), "seer %d" % seer)
    assert want[0][2].tolist() == [seer]
    assert tmod.sees(tc.par(3.0), list(SCENE_Z), pos[:seer], None, None, None).all()       # (all of them in range)


# ---- 5. m = 0, and the two argument rules that need a map -----------------------------------------------------------------------------------
def test_no_obstacle_writes_nothing(ctx):
    import torch

    d_veh = guarded(vehicles_at(tc.NEAR))
    outs = [guarded(None, 64) for _ in range(4)]
    torch.cuda.synchronize()
    ctx.fleet_obstacle_track_device(None, tc.par(), None, 0, 0, 0, d_veh[1], 1, outs[0][1], outs[1][1], outs[2][1], outs[3][1])
    ctx.fleet_obstacle_track_device(None, tc.par(), None, 0, 0, 0, None, 0, None, None, None, None)
    ctx.sync()
    assert all((t.cpu().numpy() == POISON).all() for t, _ in outs)
    with pytest.raises(capi.FasterHipError):                                       # (with m > 0 the pointers are looked at)
        ctx.fleet_obstacle_track_device(None, tc.par(), None, 1, 0, 0, d_veh[1], 1, outs[0][1], outs[1][1], outs[2][1], outs[3][1])
    with pytest.raises(capi.FasterHipError):
        ctx.fleet_obstacle_track_device(None, tc.par(), outs[0][1], 1, 0, 0, None, 1, outs[0][1], outs[1][1], outs[2][1], outs[3][1])


def test_the_two_argument_rules_that_need_a_map(ctx, maps):
    d = guarded(None, 512)
    args = (d[1], 1, 0, 0, d[1], 1, d[1], d[1], d[1], d[1])
    fresh = capi.Map(0)
    try:
        with pytest.raises(capi.FasterHipError):                                   # 12. a map that holds no grid
            ctx.fleet_obstacle_track_device(fresh, tc.par(), *args)
    finally:
        fresh.close()
    with pytest.raises(capi.FasterHipError):                                       # 13. more than 4096 cells of the map
        ctx.fleet_obstacle_track_device(maps["scene"], tc.par(4096 * lc.RES + 0.5), *args)
    ctx.sync()
    assert (d[0].cpu().numpy() == POISON).all()


# ---- 6. the fleet ---------------------------------------------------------------------------------------------------------------------------
FLEET_DC = 1.0 / 128.0      # a dyadic dc: with dyadic positions and velocities every sum of the fit is exact
TICKS = 5


def dyadic_fleet(sc):
    """tests/test_gpu_traffic.py's views_fleet with a dyadic dc."""
    from faster_amd.fleet import Fleet
    from test_gpu_fleet import P, fleet_params

    B = len(sc["states"])
    fl = Fleet(B, fleet_params(), n_seg=P["N"], max_poly=P["max_poly"], dc=FLEET_DC, v_max=P["v_max"], a_max=P["a_max"], j_max=P["j_max"],
               decomp_radius=P["decomp_radius"], dist_max_vertexes=P["dist_max_vertexes"])
    fl.set_map(sc["cloud"], sc["cells"], P["res"], sc["center"], P["z_max"], P["inflation"])
    fl.init(sc["states"], sc["goals"])
    fl.set_unknown_views(np.zeros((B, int(np.prod(sc["dims"]))), dtype=np.uint8), origin=sc["origin"], res=P["res"], dims=sc["dims"])
    fl.set_point_views(np.full((B, abi.point_mask_words(len(sc["cloud"]))), 0xFFFFFFFF, dtype=np.uint32))
    return fl


def dyadic_truth(sc, k=6):
    """k obstacles 1.5 m beside the starts of the first k vehicles (rounded to 1 / 64 m), flying towards them at 0.5 m/s."""
    starts = np.round(sc["states"]["pos"][:k] * 64.0) / 64.0
    return abi.make_obstacles(starts + (1.5, 0.0, 0.0), np.tile((-0.5, 0.0, 0.25), (k, 1)), 0.25)


def truth_now(truth, tick, dc):
    """The records a fleet is told at `tick`: where the truth is now, its velocity, the clock at 0."""
    now = truth.copy()
    now["p0"] = truth["p0"] + truth["v"] * (float(tick) * dc)
    return now


def test_a_fleet_that_tracks_equals_a_fleet_that_is_told():
    """Fleet A: enable_obstacles and enable_tracking(truth, r_detect = 6 m, no walls between, fit 4, min_obs 2), then five times
    track() -> obstacles() -> replan() -> next_goals.  Fleet B has no tracker: before obstacles() it is told through set_obstacles where
    the truth is now, from cycle min_obs on (before that the tracker's records are off, and so are those B is told: nobody can know a
    velocity from one sighting).  Positions, velocities and dc are dyadic, so the fit gives the truth back bit for bit, and vehicles(),
    plans() and results() of the two fleets are equal in every byte, cycle by cycle."""
    import test_gpu_traffic as gt

    sc = gt.crossing_scene()
    truth = dyadic_truth(sc)
    a, b = dyadic_fleet(sc), dyadic_fleet(sc)
    try:
        kw = dict(samples=6, stride=25, range=6.0, window=1)
        a.enable_obstacles(truth, **kw)
        a.enable_tracking(truth, 6.0, los=False, fit=4, min_obs=2)
        off = truth.copy()
        off["flags"] = 0
        b.enable_obstacles(off, **kw)
        tick, bits = 0, False
        for cycle in range(5):
            assert (a.track_tick, a.truth_tick) == (tick, tick)
            a.track()
            assert a.obstacle_tick == 0
            tracks, est, seer, info = a.track_records()
            told = truth_now(truth, tick, FLEET_DC)
            if cycle + 1 >= 2:
                assert est.tobytes() == told.tobytes(), cycle                      # the estimate IS the truth, in every bit
                b.set_obstacles(told)
            else:
                assert est.tobytes() == bytes(64 * len(truth)) and (tracks["count"] == 1).all()
                b.set_obstacles(off)
            assert (seer >= 0).all() and info.tolist() == [len(truth), len(truth) if cycle else 0, 0, 0]
            audit = a.obstacle_audit(obstacles=truth, tick0=a.truth_tick)          # ground truth, on the truth's own clock
            assert audit.tobytes() == a.obstacle_audit(obstacles=told, tick0=0).tobytes()
            a.obstacles()
            b.obstacles()
            first = int(a.obstacle_par["first_point"]) // 32
            assert a.point_masks().tobytes() == b.point_masks().tobytes()
            bits = bits or bool(a.point_masks()[:, first:].any())
            a.replan()
            b.replan()
            assert a.vehicles().tobytes() == b.vehicles().tobytes(), cycle
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a.plans(), b.plans())), cycle
            ra, rb = a.results(), b.results()
            for k in ra:
                assert np.ascontiguousarray(ra[k]).tobytes() == np.ascontiguousarray(rb[k]).tobytes(), (cycle, k)
            a.next_goals(TICKS, follow=True)
            b.next_goals(TICKS, follow=True)
            tick += TICKS
        assert bits                                                                # (the obstacles were shown: the equality is of something)
        with pytest.raises(capi.FasterHipError):
            a.set_truth(truth[:2])
        a.set_truth(truth)
        assert a.truth_tick == 0 and a.track_tick == tick
        with pytest.raises(capi.FasterHipError):
            b.track()
    finally:
        a.close()
        b.close()


def hidden_flight(fl, sc, r_detect, cycles, ticks):
    """Seeded search for one obstacle flight that, from where the vehicles START, is in range of somebody and hidden from everybody at
    cycle 0 and seen by somebody at a later cycle: (truth record, world of the fleet's map)."""
    from test_gpu_fleet import P

    fl.sync()
    dims, origin = fl.map.dims()
    occ = fl.map.occupancy()
    pos = sc["states"]["pos"]
    rng = np.random.default_rng(17)
    par = abi.default_track_params(r_detect, FLEET_DC)
    for _ in range(400):
        i = int(rng.integers(len(pos)))
        z0 = np.round((pos[i] + rng.uniform(-1.5, 1.5, size=3) * (1.0, 1.0, 0.2)) * 16.0) / 16.0
        v = rng.integers(-8, 9, size=3) * (0.5, 0.5, 0.0)
        at = lambda c: [float(x) for x in z0 + v * (c * ticks * FLEET_DC)]  # noqa: E731
        if not tmod.sees(par, at(0), pos, None, None, None).any() or tmod.sees(par, at(0), pos, occ, origin, P["res"]).any():
            continue
        if any(tmod.sees(par, at(c), pos, occ, origin, P["res"]).any() for c in range(2, cycles)):
            return abi.make_obstacles([z0], [v], 0.25), (occ, np.asarray(origin, dtype=np.float64), P["res"])
    raise AssertionError("no hidden flight found")


@pytest.mark.parametrize("los", [True, False])
def test_an_obstacle_behind_a_wall_has_no_bit_until_somebody_has_a_clear_ray_to_it(los):
    """One obstacle that starts in range of a vehicle and behind an occupied cell of the fleet's map from everybody, and flies into the
    open.  Per cycle track() -> obstacles(): with los=True no mask row has a bit of it while the model, on the fleet's own positions and
    map, says nobody has a clear ray; from the cycle on in which somebody has, rows have bits (min_obs = 1: one sighting shows it, and
    it is never forgotten).  With los=False it has bits from the first cycle.  The plans come near by construction (a range of 50 m, any
    sampled instant), so a bit tells only whether the record is on."""
    import test_gpu_traffic as gt

    sc = gt.crossing_scene()
    fl = dyadic_fleet(sc)
    cycles, ticks, r_detect = 6, 25, 2.0
    try:
        truth, (occ, origin, res) = hidden_flight(fl, sc, r_detect, cycles, ticks)
        fl.replan()                                                                # (plans to come near to)
        fl.enable_obstacles(truth, samples=4, stride=10, range=50.0, points=1, window=3)
        fl.enable_tracking(truth, r_detect, los=los, fit=1, min_obs=1)
        first = int(fl.obstacle_par["first_point"]) // 32
        known, history = False, []
        for cycle in range(cycles):
            pos = fl.vehicles()["state"]["pos"]
            z = tmod.measurement(truth[0], fl.truth_tick, FLEET_DC)[1]
            sees = tmod.sees(fl.track_par, z, pos, occ if los else None, origin, res)
            fl.track()
            fl.obstacles()
            seer = fl.track_records()[2]
            assert seer.tolist() == [int(np.flatnonzero(sees)[0]) if sees.any() else -1], cycle
            known = known or bool(sees.any())
            bits = bool(fl.point_masks()[:, first:].any())
            assert bits == known, (cycle, los)
            history.append(bits)
            fl.replan()
            fl.next_goals(ticks, follow=True)
        assert history[-1] and history[0] == (not los)                             # hidden at first under los, shown at once without
    finally:
        fl.close()


def test_closed_loop_counts_as_observed():
    """Printed, not asserted: vehicle-cycles with FH_OBSTACLE_HIT against the TRUE obstacles in tests/test_gpu_obstacles.py's
    crossing scene (16 vehicles, 8 obstacles of 0.3 m crossing at 1 m/s), in the first delta_t states / in every state, for three runs:
    the fleet never hears of obstacles; it tracks them (r_detect 6 m, walls hide, fit 4, min_obs 2); it is told the truth (K26)."""
    import test_gpu_obstacles as go
    import test_gpu_traffic as gt

    for name in ("off", "tracking", "perfect knowledge"):
        sc = gt.crossing_scene()
        truth = go.crossing_obstacles(sc)
        fl = gt.views_fleet(sc)
        fixed = every = seen = 0
        try:
            if name != "off":
                fl.enable_obstacles(truth, samples=64, stride=5, range=6.0, window=2)
            if name == "tracking":
                fl.enable_tracking(truth, 6.0, los=True, fit=4, min_obs=2)
            tick = 0
            for c in range(go.C):
                if name == "tracking":
                    fl.track()
                    seen += int(fl.track_records()[3][1])
                if name != "off":
                    fl.obstacles()
                fl.replan()
                for count in (int(fl.params["delta_t"]), 0):
                    hit = int(((fl.obstacle_audit(count=count, obstacles=truth, tick0=tick)["flags"] & abi.FH_OBSTACLE_HIT) != 0).sum())
                    fixed, every = (fixed + hit, every) if count else (fixed, every + hit)
                fl.next_goals(int(sc["ticks"][c]), follow=True)
                tick += int(sc["ticks"][c])
        finally:
            fl.close()
        print("closed loop %-18s FH_OBSTACLE_HIT in the first delta_t states %2d of %d, in every state %2d; records on per cycle %.1f of %d"
              % (name, fixed, go.B * go.C, every, seen / go.C, len(truth)))
