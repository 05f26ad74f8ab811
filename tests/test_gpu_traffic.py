"""GPU tests of the traffic stage (fh_fleet_traffic_device, Fleet.enable_traffic, Fleet.traffic; include/fasterhip_traffic.h): every byte of
the cloud and of the masks equals the numpy model (tests/traffic_model.py, brute force over all (i, k, s)) — at the chunk, word and
group edges of the kernels, on the hand cases of tests/test_traffic_model.py, with words and points that traffic does not own left as
they were and stale bits gone; a fleet with traffic equals a fleet without that is handed the same points and bits; and the closed loop
of the 16-vehicle crossing scene of tests/test_gpu_separation.py."""
import numpy as np
import pytest

from faster_amd import abi, capi

import test_traffic_model as hand
import traffic_model as tm

pytestmark = pytest.mark.gpu
KEEP = 0xA5A5A5A5     # words that traffic does not own
STALE = 0xFFFFFFFF    # traffic words before a call
MAX_STATES = 64


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch  # noqa: F401  (torch before the HIP library: one HIP runtime in the process)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


class Device:
    """Cloud and masks on the device across several calls."""

    def __init__(self, cloud, mask):
        import torch

        self.cloud = torch.from_numpy(np.ascontiguousarray(cloud, dtype=np.float64)).to("cuda:0")
        self.mask = torch.from_numpy(np.ascontiguousarray(mask, dtype=np.uint32).view(np.int32)).to("cuda:0")

    def call(self, c, par, v, pl):
        import torch

        def dev(a):
            return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")

        n, max_states = len(v), pl.shape[1]
        d_veh, d_plans = dev(v), dev(pl)
        torch.cuda.synchronize()
        c.fleet_traffic_device(par, d_veh.data_ptr(), d_plans.data_ptr(), n, max_states, self.cloud.data_ptr(), self.cloud.shape[0],
                               self.mask.data_ptr(), self.mask.shape[1])
        c.sync()
        return self.cloud.cpu().numpy(), self.mask.cpu().numpy().view(np.uint32)


def arrays(par, n, n_static, words_behind=2, points_behind=3):
    """Cloud and masks before a call: static points with a pattern, traffic points poisoned, static words and words behind the traffic
    KEEP, traffic words all ones."""
    first = int(par["first_point"])
    total = first + n * int(par["samples"]) * abi.traffic_points_per_sample(par["hull"])
    assert n_static <= first
    cloud = np.full((total + points_behind, 3), 7e7)
    cloud[:first] = np.arange(3 * first).reshape(first, 3) * 0.5 - 11.0
    cloud[total:] = -3e3
    w0, w1 = first // 32, abi.point_mask_words(total)
    mask = np.full((max(n, 1), w1 + words_behind), KEEP, dtype=np.uint32)
    mask[:, w0:w1] = STALE
    return cloud, mask


def check(c, par, v, pl, what, n_static=40):
    cloud, mask = arrays(par, len(v), n_static)
    want_cloud, want_mask = tm.traffic(par, v, pl, pl.shape[1], cloud, mask)
    got_cloud, got_mask = Device(cloud, mask).call(c, par, v, pl)
    tm.assert_equal(got_cloud, got_mask, want_cloud, want_mask, what)
    first, w0 = int(par["first_point"]), int(par["first_point"]) // 32
    w1 = mask.shape[1] - 2
    assert (got_mask[:, :w0] == KEEP).all() and (got_mask[:, w1:] == KEEP).all(), what           # ownership, stated again
    assert got_cloud[:first].tobytes() == cloud[:first].tobytes() and (got_cloud[-3:] == -3e3).all(), what
    return want_cloud, want_mask


def random_fleet(rng, n, far_from=None, box=2.0):
    """n vehicles on a lattice of 1/64 in a box, each with a straight plan of a random size <= MAX_STATES at a random head; the vehicles
    from `far_from` on stand 100 m away, where no chunk of the others reaches them.  A few flagged records among them."""
    pos = np.round(rng.uniform(0.0, box, size=(n, 3)) * 64) / 64
    if far_from is not None:
        pos[far_from:] += (100.0, 0.0, 0.0)
    sizes = rng.integers(1, MAX_STATES + 1, size=n)
    heads = [int(rng.integers(0, MAX_STATES - s + 1)) for s in sizes]
    step = np.round(rng.normal(size=(n, 3)) * 2) / 64
    v, pl = tm.fleet([p + np.arange(s)[:, None] * d for p, s, d in zip(pos, sizes, step)], pos, max_states=MAX_STATES, heads=heads)
    for k in range(3, n, 11):
        v["plan_size"][k] = 0                       # an empty plan
    for k in range(5, n, 13):
        v["plan_head"][k] = MAX_STATES - int(v["plan_size"][k]) + 1   # head + size > max_states
    for k in range(7, n, 17):
        pl["pos"][k, min(int(v["plan_head"][k]), MAX_STATES - 1), 1] = np.nan    # the first sample is not finite
    return v, pl


# ---- 1. shapes: chunks of 64 samples, words straddled by vehicles, a partial last word, whole chunks of 14 words, two groups, two passes ---
SHAPES = [(1, 1, 0.0), (1, 3, 0.25), (2, 1, 0.0), (2, 2, 0.25), (65, 1, 0.0), (65, 1, 0.25), (5, 3, 0.25), (13, 5, 0.0), (10, 64, 0.25),
          (70, 64, 0.0),     # 4480 samples: 70 chunks, a second group of 64 chunks
          (1030, 1, 0.0)]    # more rows than the mask kernel's grid is high: rows 0 .. 5 are a wavefront's second turn


@pytest.mark.parametrize("n,S,hull", SHAPES)
def test_shapes_equal_the_model(ctx, n, S, hull):
    rng = np.random.default_rng(1000 * n + S)
    v, pl = random_fleet(rng, n, far_from=None if n < 10 else (2 * n) // 3, box=0.5 if n < 10 else 2.0 if n < 200 else 6.0)
    for rule in (abi.FH_TRAFFIC_ALL, abi.FH_TRAFFIC_YIELD_TO_LOWER):
        par = tm.params(S, 3 if S > 1 else 1, 1.0, hull=hull, rule=rule, first_point=64)
        _, mask = check(ctx, par, v, pl, "n %d S %d hull %g rule %d" % (n, S, hull, rule))
        w0, w1 = 2, mask.shape[1] - 2
        if n == 1:
            assert not mask[:, w0:w1].any()      # nothing is set: a vehicle never sees itself
        else:
            assert mask[:, w0:w1].any() and (mask[:, w0:w1] != STALE).any()
        if n >= 10 and rule == abi.FH_TRAFFIC_ALL:   # the far cluster and the near one see nothing of each other, and each sees its own
            far = (2 * n) // 3
            pps = abi.traffic_points_per_sample(hull)
            bits = np.unpackbits(mask[:, w0:w1].view(np.uint8), axis=1, bitorder="little")[:, :n * S * pps]
            assert not bits[:far, far * S * pps:].any() and not bits[far:, :far * S * pps].any()
            assert bits[:far, :far * S * pps].any() and bits[far:, far * S * pps:].any()


# ---- 2. the hand cases: strict range, exact hull adds, the plan end, flagged records, NaN in state_i, yield to lower ---------------------------
@pytest.mark.parametrize("name", sorted(hand.CASES))
def test_hand_cases(ctx, name):
    c = hand.CASES[name]
    _, cloud, mask = hand.inputs(c)
    want_cloud, want_mask = tm.traffic(c["par"], c["v"], c["pl"], c["pl"].shape[1], cloud, mask)
    got_cloud, got_mask = Device(cloud, mask).call(ctx, c["par"], c["v"], c["pl"])
    tm.assert_equal(got_cloud, got_mask, want_cloud, want_mask, name)
    hand.check(c, got_cloud, got_mask, name)


def test_a_bad_extent_with_a_negative_head_and_positions_that_overflow(ctx):
    """Heads and sizes at the ends of int32 (their sum is taken in 64 bits), a centre at 1.7e308 whose hull overflows to infinity, and
    one at 1e300: the prefilter compares in double and the bits follow d2 alone."""
    v, pl = tm.fleet([[(0, 0, 0)] * 4, [(0.5, 0, 0)] * 4, [(0.25, 0, 0)] * 4, [(1.7e308, 0, 0)] * 4, [(1e300, -1e300, 0.5)] * 4, [(0, 0.5, 0)] * 4],
                     [(0, 0, 0), (0.5, 0, 0), (0.25, 0, 0), (1.7e308, 0, 0), (np.inf, 0, 0), (0, 0.5, 0)], max_states=8)
    v["plan_head"][1], v["plan_size"][1] = 2147483647, 2147483647
    v["plan_head"][2], v["plan_size"][2] = -2147483648, 4
    for hull in (0.0, 0.25, 1e308):
        par = tm.params(2, 2147483647, 1.0, hull=hull, first_point=32)
        cloud, mask = check(ctx, par, v, pl, "overflow, hull %g" % hull, n_static=32)
        pps = abi.traffic_points_per_sample(hull)
        assert not cloud[32 + 2 * pps:32 + 6 * pps].any()                       # vehicles 1 and 2 are shown to nobody
        assert tm.bit(mask, 0, 32 + 5 * 2 * pps) and tm.bit(mask, 5, 32) and not mask[4, 1:-2].any()


# ---- 3. ownership over two calls: plans move, stale bits go --------------------------------------------------------------------------------
@pytest.mark.parametrize("S,hull", [(4, 0.0), (3, 0.25)])
def test_two_calls_with_moved_plans(ctx, S, hull):
    rng = np.random.default_rng(5)
    n = 40
    v, pl = random_fleet(rng, n, far_from=30)
    par = tm.params(S, 2, 1.0, hull=hull, first_point=96)
    cloud, mask = arrays(par, n, 90)
    dev = Device(cloud, mask)
    c1, m1 = tm.traffic(par, v, pl, MAX_STATES, cloud, mask)
    tm.assert_equal(*dev.call(ctx, par, v, pl), c1, m1, "first call")
    v2, pl2 = v.copy(), pl.copy()
    pl2["pos"] += (0.75, -0.5, 0.25)                       # the plans move, the vehicles do not: other bits
    v2["state"]["pos"][::2] += (0.5, 0.0, 0.0)
    c2, m2 = tm.traffic(par, v2, pl2, MAX_STATES, c1, m1)
    assert (m2 != m1).any() and ((m1 & ~m2) != 0).any()    # bits of the first call that the second has to clear
    tm.assert_equal(*dev.call(ctx, par, v2, pl2), c2, m2, "second call")
    fresh_c, fresh_m = tm.traffic(par, v2, pl2, MAX_STATES, cloud, mask)
    assert m2.tobytes() == fresh_m.tobytes() and c2.tobytes() == fresh_c.tobytes()   # nothing of the first call is left


# ---- 4. the fleet -----------------------------------------------------------------------------------------------------------------------------
B, C = 16, 4


def crossing_scene():
    """The scene of tests/test_gpu_separation.py's closed loop: 16 vehicles of the forest of tests/test_gpu_fleet.py, each sent to the
    start of the vehicle opposite in the list, at rest."""
    from test_gpu_fleet import scenario

    sc = dict(scenario(B, C, 31))
    starts = sc["states"]["pos"].copy()
    sc["goals"] = starts[(np.arange(B) + B // 2) % B].copy()
    sc["states"] = sc["states"].copy()
    sc["states"]["vel"] = 0.0
    return sc


def views_fleet(sc, cloud=None, mask=None):
    """A fleet of the scene with a view per vehicle in which everything is known: no unknown voxel, every static point in every row."""
    from test_gpu_fleet import P
    from test_gpu_fleet_occupancy import new_fleet

    if cloud is not None:
        sc = dict(sc, cloud=cloud)
    fl = new_fleet(sc, B, P["inflation"])
    fl.set_unknown_views(np.zeros((B, int(np.prod(sc["dims"]))), dtype=np.uint8), origin=sc["origin"], res=P["res"], dims=sc["dims"])
    fl.set_point_views(np.full((B, abi.point_mask_words(len(sc["cloud"]))), 0xFFFFFFFF, dtype=np.uint32) if mask is None else mask)
    return fl


def model_of(fl, par, cloud_before, mask_before):
    return tm.traffic(par, fl.vehicles(), fl._host(fl.d_plans, abi.state_dtype).reshape(fl.n, fl.max_states), fl.max_states, cloud_before,
                      mask_before)


def test_a_fleet_with_traffic_equals_one_that_is_given_its_points_and_bits():
    """Fleet A: enable_traffic, then twice traffic() -> replan() (the first traffic() sees empty plans).  Fleet B never hears of
    traffic: before each replan it gets A's extended cloud through set_map and A's masks through set_point_views.  vehicles(), plans()
    and results() are equal in every byte: the feature adds points and bits and nothing else."""
    from test_gpu_fleet import P

    sc = crossing_scene()
    a, b = views_fleet(sc), None
    try:
        n_static = a.n_cloud
        a.enable_traffic(samples=6, stride=25, range=6.0)
        assert a.n_cloud == n_static and a.n_cloud_all == abi.point_mask_words(n_static) * 32 + B * 6 * 7
        assert a.cloud.shape[0] == a.n_cloud_all and a.point_mask.shape[1] == abi.point_mask_words(a.n_cloud_all)
        for turn in range(2):
            a.traffic()
            a.sync()
            cloud, mask = a.cloud.cpu().numpy().copy(), a.point_masks()
            if b is None:
                b = views_fleet(sc, cloud, mask)
            else:
                b.set_map(cloud, sc["cells"], P["res"], sc["center"], P["z_max"], P["inflation"])
                b.set_point_views(mask)
            assert [name for name, _ in a.stages()] == [name for name, _ in b.stages()]
            a.replan()
            b.replan()
            assert a.vehicles().tobytes() == b.vehicles().tobytes(), turn
            pa, pb = a.plans(), b.plans()
            assert all(x.tobytes() == y.tobytes() for x, y in zip(pa, pb)), turn
            ra, rb = a.results(), b.results()
            for k in ra:
                assert np.ascontiguousarray(ra[k]).tobytes() == np.ascontiguousarray(rb[k]).tobytes(), (turn, k)
            if turn == 1:
                assert mask[:, abi.point_mask_words(n_static):].any()   # the second turn plans around the plans of the first
            a.next_goals(5, follow=True)
            b.next_goals(5, follow=True)
        assert b.traffic_par is None and b.n_cloud == a.n_cloud_all
    finally:
        a.close()
        if b is not None:
            b.close()


def run_loop(rule, count_only=False):
    """C cycles of traffic -> replan -> separation -> next_goals on the crossing scene (rule None: enable_traffic is never called).
    Returns (vehicle-cycles with FH_SEP_NEAR, per cycle: vehicles and plans as bytes)."""
    from test_gpu_fleet import P

    sc = crossing_scene()
    fl = views_fleet(sc)
    near, trace = 0, []
    try:
        n_static = fl.n_cloud
        w0 = abi.point_mask_words(n_static)
        if rule is not None:
            static_mask = fl.point_masks()
            fl.enable_traffic(samples=64, stride=5, range=6.0, rule=rule)
            par = fl.traffic_par
            assert float(par["hull"]) == P["drone_radius"] and int(par["first_point"]) == 32 * w0
        for c in range(C):
            if rule is not None:
                fl.sync()
                cloud_before, mask_before = fl.cloud.cpu().numpy().copy(), fl.point_masks()
                fl.traffic()
                want_cloud, want_mask = model_of(fl, par, cloud_before, mask_before)
                tm.assert_equal(fl.cloud.cpu().numpy(), fl.point_masks(), want_cloud, want_mask, "rule %s, cycle %d" % (rule, c))
                assert want_mask[:, :w0 - 1].tobytes() == static_mask[:, :w0 - 1].tobytes()
                assert want_cloud[:n_static].tobytes() == np.ascontiguousarray(sc["cloud"], dtype=np.float64).tobytes()
                if c == 0:
                    pass                                                  # (a plan is one state: the vehicles stand at their starts)
                elif rule == "all":
                    assert want_mask[:, w0:].any(axis=1).all(), c         # every vehicle has another one within 6 m (DESIGN K8)
                else:
                    assert want_mask[1:, w0:].any() and not want_mask[0, w0:].any()   # vehicle 0 yields to nobody
            fl.replan()
            near += int(((fl.separation()["flags"] & abi.FH_SEP_NEAR) != 0).sum())
            trace.append((fl.vehicles().tobytes(), b"".join(p.tobytes() for p in fl.plans())))
            fl.next_goals(int(sc["ticks"][c]), follow=True)
    finally:
        fl.close()
    return near, trace


def test_closed_loop_equals_the_model_and_without_traffic_today():
    """4 cycles with rule "all" and with "yield": every cycle's cloud tail and masks equal the model, and from cycle 1 on every row has a
    bit.  A fleet that never calls enable_traffic flies what today's shared-map fleet of tests/test_gpu_separation.py flies, byte for
    byte.  How many vehicle-cycles have FH_SEP_NEAR (another vehicle within 0.6 m at one instant of the plan) is printed, not asserted.
    Observed on an MI355X: traffic off 28, rule all 23, rule yield 28 of 64."""
    from test_gpu_fleet import P
    from test_gpu_fleet_occupancy import new_fleet

    near_off, off = run_loop(None)
    sc = crossing_scene()
    fl = new_fleet(sc, B, P["inflation"])
    try:
        fl.set_unknown(np.zeros(int(np.prod(sc["dims"])), dtype=np.uint8), sc["origin"], P["res"], sc["dims"])   # everything is known
        for c in range(C):
            fl.replan()
            assert (fl.vehicles().tobytes(), b"".join(p.tobytes() for p in fl.plans())) == off[c], c
            fl.next_goals(int(sc["ticks"][c]), follow=True)
    finally:
        fl.close()
    near_all, with_all = run_loop("all")
    near_yield, _ = run_loop("yield")
    assert any(x != y for x, y in zip(with_all, off))   # the vehicles plan differently when they see each other
    print("closed loop, %d vehicle-cycles with crossing goals, FH_SEP_NEAR (r = %.2f m): traffic off %d, rule all %d, rule yield %d"
          % (B * C, 2.0 * P["drone_radius"], near_off, near_all, near_yield))


def test_enable_traffic_refuses_what_it_cannot_serve():
    from test_gpu_fleet import P
    from test_gpu_fleet_occupancy import new_fleet

    sc = crossing_scene()
    fl = new_fleet(sc, B, P["inflation"])
    try:
        with pytest.raises(capi.FasterHipError):
            fl.traffic()
        with pytest.raises(capi.FasterHipError):
            fl.enable_traffic(4, 10, 6.0)                     # no views, no masks
        fl.set_unknown_views(view_of=np.zeros(B, dtype=np.int32), n_views=1, origin=sc["origin"], res=P["res"], dims=sc["dims"])
        fl.set_point_views()
        with pytest.raises(capi.FasterHipError):
            fl.enable_traffic(4, 10, 6.0)                     # a team view
        fl.set_point_views(False)
        fl.set_unknown_views(origin=sc["origin"], res=P["res"], dims=sc["dims"])
        fl.set_point_views()
        with pytest.raises(capi.FasterHipError):
            fl.enable_traffic(4, 10, 6.0, rule="left")
        names = [n for n, _ in fl.stages()]
        fl.enable_traffic(4, 10, 6.0, hull=0.0)
        assert [n for n, _ in fl.stages()] == names and fl.n_cloud_all == abi.point_mask_words(fl.n_cloud) * 32 + B * 4
        fl.set_map(sc["cloud"], sc["cells"], P["res"], sc["center"], P["z_max"], P["inflation"])   # again: the tail stays
        assert fl.cloud.shape[0] == fl.n_cloud_all and fl.n_cloud == len(sc["cloud"])
        fl.traffic()
        fl.replan()
        fl.sync()
        fl.set_point_views()                                   # new masks: traffic is off again
        assert fl.traffic_par is None and fl.cloud.shape[0] == fl.n_cloud
    finally:
        fl.close()
