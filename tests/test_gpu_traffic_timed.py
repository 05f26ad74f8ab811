"""GPU tests of time-aware traffic (fh_fleet_traffic_timed_device, Fleet.enable_traffic(timed=True); include/fasterhip_traffic_timed.h):
every byte of the cloud and of the masks equals the numpy model (tests/traffic_timed_model.py, brute force over all (i, k, s, s')) — at
the chunk, word, group and LDS edges of the kernels, on the hand cases of tests/test_traffic_timed_model.py, with words and points that
traffic does not own left as they were and stale bits gone; the two properties of the header on the device; timed and untimed calls
sharing the buffers of one context; and the fleet: the closed loop of the crossing scene of tests/test_gpu_traffic.py against the
model, a timed fleet against one that is handed its points and bits, an untimed fleet against today's signature.  The harness (upload,
poisoned points, STALE and KEEP words) is that of tests/test_gpu_traffic.py."""
import numpy as np
import pytest

from faster_amd import abi, capi

import test_gpu_traffic as gt
import test_traffic_timed_model as hand
import traffic_model as tm
import traffic_timed_model as ttm

pytestmark = pytest.mark.gpu
KEEP, STALE, MAX_STATES, B, C = gt.KEEP, gt.STALE, gt.MAX_STATES, gt.B, gt.C
ALL, YIELD = abi.FH_TRAFFIC_ALL, abi.FH_TRAFFIC_YIELD_TO_LOWER
BEYOND = MAX_STATES + 5   # an instant beyond the end of every plan


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch  # noqa: F401  (torch before the HIP library: one HIP runtime in the process)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def upload(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


def launch(c, par, d_veh, d_plans, n, max_states, dev):
    """One call, timed or untimed by the record's dtype, without a wait."""
    f = c.fleet_traffic_timed_device if par.dtype == abi.traffic_timed_params_dtype else c.fleet_traffic_device
    f(par, d_veh.data_ptr(), d_plans.data_ptr(), n, max_states, dev.cloud.data_ptr(), dev.cloud.shape[0], dev.mask.data_ptr(), dev.mask.shape[1])


def call(dev, c, par, v, pl):
    import torch

    d_veh, d_plans = upload(v), upload(pl)
    torch.cuda.synchronize()
    launch(c, par, d_veh, d_plans, len(v), pl.shape[1], dev)
    c.sync()
    return dev.cloud.cpu().numpy(), dev.mask.cpu().numpy().view(np.uint32)


def model(par, v, pl, cloud, mask):
    f = ttm.traffic_timed if par.dtype == abi.traffic_timed_params_dtype else tm.traffic
    return f(par, v, pl, pl.shape[1], cloud, mask)


def check(c, par, v, pl, what, n_static=40):
    cloud, mask = gt.arrays(par, len(v), n_static)
    want_cloud, want_mask = model(par, v, pl, cloud, mask)
    got_cloud, got_mask = call(gt.Device(cloud, mask), c, par, v, pl)
    tm.assert_equal(got_cloud, got_mask, want_cloud, want_mask, what)
    first, w0 = int(par["first_point"]), int(par["first_point"]) // 32
    w1 = mask.shape[1] - 2
    assert (got_mask[:, :w0] == KEEP).all() and (got_mask[:, w1:] == KEEP).all(), what           # ownership, stated again
    assert got_cloud[:first].tobytes() == cloud[:first].tobytes() and (got_cloud[-3:] == -3e3).all(), what
    return want_cloud, want_mask


def moving_fleet(rng, n, far_from=None, box=2.0):
    """gt.random_fleet with steps of about 1/8 m per state, so that a vehicle travels several ranges along its plan and the instant
    matters: n vehicles on a lattice of 1/64 in a box, straight plans of a random size <= MAX_STATES at a random head; the vehicles from
    `far_from` on fly 100 m away, where no chunk box of the others reaches them.  The flagged records of that fleet among them."""
    pos = np.round(rng.uniform(0.0, box, size=(n, 3)) * 64) / 64
    if far_from is not None:
        pos[far_from:] += (100.0, 0.0, 0.0)
    sizes = rng.integers(1, MAX_STATES + 1, size=n)
    heads = [int(rng.integers(0, MAX_STATES - s + 1)) for s in sizes]
    step = np.round(rng.normal(size=(n, 3)) * 8) / 64
    v, pl = tm.fleet([p + np.arange(s)[:, None] * d for p, s, d in zip(pos, sizes, step)], pos, max_states=MAX_STATES, heads=heads)
    for k in range(3, n, 11):
        v["plan_size"][k] = 0                       # an empty plan
    for k in range(5, n, 13):
        v["plan_head"][k] = MAX_STATES - int(v["plan_size"][k]) + 1   # head + size > max_states
    for k in range(7, n, 17):
        pl["pos"][k, min(int(v["plan_head"][k]), MAX_STATES - 1), 1] = np.nan    # the first state is not finite
    return v, pl


# ---- 1. shapes: the smallest fleets, words straddled by vehicles, chunk ends inside / on / beyond a vehicle's samples with the window
# across them, two chunks, two groups, two turns of a wavefront, the LDS staging at its cap, the window at S - 1 and far beyond ---------------
SHAPES = [(1, 1, 0.0, 0), (2, 1, 0.0, 0), (2, 2, 0.25, 1), (5, 3, 0.25, 1), (3, 63, 0.0, 2), (3, 64, 0.25, 2), (3, 65, 0.0, 2), (65, 1, 0.25, 0),
          (70, 64, 0.0, 3), (1030, 1, 0.0, 0), (3, 512, 0.0, 5), (4, 10, 0.25, 0), (4, 10, 0.25, 9), (4, 10, 0.25, 10 ** 6)]


@pytest.mark.parametrize("n,S,hull,window", SHAPES)
def test_shapes_equal_the_model(ctx, n, S, hull, window):
    rng = np.random.default_rng(1000 * n + S)
    far = None if n < 10 else (2 * n) // 3
    v, pl = moving_fleet(rng, n, far_from=far, box=0.4 if n < 10 else 2.0 if n < 200 else 6.0)
    stride = 1 if S >= 10 else 3 if S > 1 else 1
    for first_instant, rule in ((0, ALL), (0, YIELD), (3, ALL), (3, YIELD), (BEYOND, ALL), (BEYOND, YIELD)):
        par = ttm.params(S, stride, 0.75, hull=hull, rule=rule, first_point=64, first_instant=first_instant, window=window)
        _, mask = check(ctx, par, v, pl, "n %d S %d hull %g window %d first_instant %d rule %d" % (n, S, hull, window, first_instant, rule))
        bits = ttm.traffic_bits(par, n, mask)
        if n == 1:
            assert not bits.any()                # nothing is set: a vehicle never sees itself
        elif first_instant == 0:
            assert bits.any() and not bits.all()
        if far is not None:                      # the far cluster and the near one see nothing of each other, and each sees its own
            pps = abi.traffic_points_per_sample(hull)
            assert not bits[:far, far * S * pps:].any() and not bits[far:, :far * S * pps].any()
            if first_instant == 0:
                assert bits[:far, :far * S * pps].any() and bits[far:, far * S * pps:].any()


# ---- 2. the hand cases ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(hand.CASES))
def test_hand_cases(ctx, name):
    c = hand.CASES[name]
    _, cloud, mask = hand.inputs(c)
    want_cloud, want_mask = model(c["par"], c["v"], c["pl"], cloud, mask)
    got_cloud, got_mask = call(gt.Device(cloud, mask), ctx, c["par"], c["v"], c["pl"])
    tm.assert_equal(got_cloud, got_mask, want_cloud, want_mask, name)
    hand.check(c, got_cloud, got_mask, name)


# ---- 3. ownership over two calls: plans move, stale bits go ---------------------------------------------------------------------------
@pytest.mark.parametrize("S,hull", [(4, 0.0), (3, 0.25)])
def test_two_calls_with_moved_plans(ctx, S, hull):
    rng = np.random.default_rng(5)
    n = 40
    v, pl = moving_fleet(rng, n, far_from=30)
    par = ttm.params(S, 2, 0.75, hull=hull, first_point=96, first_instant=1, window=1)
    cloud, mask = gt.arrays(par, n, 90)
    dev = gt.Device(cloud, mask)
    c1, m1 = model(par, v, pl, cloud, mask)
    tm.assert_equal(*call(dev, ctx, par, v, pl), c1, m1, "first call")
    v2, pl2 = v.copy(), pl.copy()
    pl2["pos"][::2] += (0.75, -0.5, 0.25)                  # every other plan moves: other bits
    c2, m2 = model(par, v2, pl2, c1, m1)
    assert (m2 != m1).any() and ((m1 & ~m2) != 0).any()    # bits of the first call that the second has to clear
    tm.assert_equal(*call(dev, ctx, par, v2, pl2), c2, m2, "second call")
    fresh_c, fresh_m = model(par, v2, pl2, cloud, mask)
    assert m2.tobytes() == fresh_m.tobytes() and c2.tobytes() == fresh_c.tobytes()   # nothing of the first call is left


# ---- 4. the two properties of the header, on the device -----------------------------------------------------------------------------------
def test_bits_are_monotone_in_the_window(ctx):
    rng = np.random.default_rng(11)
    n, S = 9, 7
    v, pl = hand.random_plans(rng, n)
    rows = []
    for w in list(range(S + 2)) + [10 ** 6, 2 ** 31 - 1]:
        par = ttm.params(S, 2, 0.75, hull=0.25, first_point=32, first_instant=1, window=w)
        cloud, mask = gt.arrays(par, n, 30)
        got_cloud, got_mask = call(gt.Device(cloud, mask), ctx, par, v, pl)
        rows.append((ttm.traffic_bits(par, n, got_mask), got_cloud))
    for (lo, c0), (hi, c1) in zip(rows, rows[1:]):
        assert not (lo & ~hi).any() and c0.tobytes() == c1.tobytes()
    assert (rows[0][0] != rows[S - 1][0]).any()
    for bits, _ in rows[S:]:
        assert (bits == rows[S - 1][0]).all()


@pytest.mark.parametrize("n,hull,rule", [(12, 0.0, ALL), (70, 0.25, YIELD)])
def test_one_sample_at_instant_0_is_the_untimed_entry_point(ctx, n, hull, rule):
    """S = 1, first_instant = 0, good non-empty plans, state.pos bitwise the first plan state: fh_fleet_traffic_device on the same
    context writes the same bytes."""
    rng = np.random.default_rng(n)
    v, pl = hand.random_plans(rng, n, good=True)
    par = ttm.params(1, 5, 0.75, hull=hull, rule=rule, first_point=64, window=2)
    cloud, mask = gt.arrays(par, n, 50)
    timed = call(gt.Device(cloud, mask), ctx, par, v, pl)
    untimed = call(gt.Device(cloud, mask), ctx, ttm.untimed(par), v, pl)
    tm.assert_equal(*timed, *untimed, "S = 1")
    assert ttm.traffic_bits(par, n, timed[1]).any()


# ---- 4b. one points kernel and one host prologue under both entry points -------------------------------------------------------------------
ONE_STAGE_SHAPES = [(5, 3, 0.25), (3, 65, 0.0)]   # (the second: a chunk ends inside a vehicle's samples)


@pytest.mark.parametrize("n,S,hull", ONE_STAGE_SHAPES)
def test_both_entry_points_write_the_same_points(ctx, n, S, hull):
    """first_instant = 0 and the same first six fields: the cloud from first_point on is the same in every byte after either call, and it
    is the model's points.  The masks follow different rules and are not compared."""
    v, pl = moving_fleet(np.random.default_rng(1000 * n + S), n, box=0.4)
    par = ttm.params(S, 1 if S >= 10 else 3, 0.75, hull=hull, first_point=64, first_instant=0, window=1)
    cloud, mask = gt.arrays(par, n, 40)
    timed, _ = call(gt.Device(cloud, mask), ctx, par, v, pl)
    untimed, _ = call(gt.Device(cloud, mask), ctx, ttm.untimed(par), v, pl)
    first = int(par["first_point"])
    assert timed[first:].tobytes() == untimed[first:].tobytes()
    want = tm.points(par, *tm.samples(par, v, pl, pl.shape[1])).reshape(-1, 3)
    assert want.any() and timed[first:first + len(want)].tobytes() == want.tobytes()
    assert (timed[first + len(want):] == -3e3).all()


@pytest.mark.parametrize("n,S,hull", ONE_STAGE_SHAPES)
def test_untimed_entry_ignores_its_reserved_words(ctx, n, S, hull):
    """reserved[0..1] of fh_traffic_params lie where fh_traffic_timed_params has first_instant and window: the untimed entry point reads
    neither, so a record with (7, 3, -1, 1 << 30) there gives the cloud and the masks of one with zeros, which are the model's."""
    v, pl = moving_fleet(np.random.default_rng(1000 * n + S), n, box=0.4)
    zeros = tm.params(S, 1 if S >= 10 else 3, 0.75, hull=hull, first_point=64)
    marked = zeros.copy()
    marked["reserved"] = (7, 3, -1, 1 << 30)
    cloud, mask = gt.arrays(zeros, n, 40)
    got_zeros = call(gt.Device(cloud, mask), ctx, zeros, v, pl)
    got_marked = call(gt.Device(cloud, mask), ctx, marked, v, pl)
    assert got_marked[0].tobytes() == got_zeros[0].tobytes() and got_marked[1].tobytes() == got_zeros[1].tobytes()
    tm.assert_equal(*got_marked, *tm.traffic(zeros, v, pl, pl.shape[1], cloud, mask), "reserved words set")
    assert ttm.traffic_bits(zeros, n, got_marked[1]).any()


# ---- 5. timed and untimed calls alternate on one context without a wait: they share TRAFFIC_SAMPLES and TRAFFIC_BOXES ---------------------
def test_timed_and_untimed_calls_alternate_on_one_context(ctx):
    import torch

    rng = np.random.default_rng(23)
    jobs = []
    for n, par in ((40, ttm.params(8, 2, 0.75, hull=0.25, first_point=64, first_instant=2, window=2)),
                   (70, tm.params(64, 1, 1.0, first_point=64)),                      # (larger: both buffers grow between two launches)
                   (40, ttm.params(8, 2, 0.75, rule=YIELD, first_point=64, window=1)),
                   (12, tm.params(3, 2, 1.0, hull=0.25, first_point=64))):
        v, pl = moving_fleet(rng, n, far_from=(2 * n) // 3)
        cloud, mask = gt.arrays(par, n, 40)
        jobs.append((par, v, pl, upload(v), upload(pl), gt.Device(cloud, mask), cloud, mask))
    torch.cuda.synchronize()
    for par, v, pl, d_veh, d_plans, dev, _, _ in jobs:
        launch(ctx, par, d_veh, d_plans, len(v), pl.shape[1], dev)
    ctx.sync()
    for turn, (par, v, pl, _, _, dev, cloud, mask) in enumerate(jobs):
        got = dev.cloud.cpu().numpy(), dev.mask.cpu().numpy().view(np.uint32)
        fresh = capi.Context(0)
        try:
            want = call(gt.Device(cloud, mask), fresh, par, v, pl)
        finally:
            fresh.close()
        tm.assert_equal(*got, *want, "turn %d against a fresh context" % turn)
        tm.assert_equal(*got, *model(par, v, pl, cloud, mask), "turn %d against the model" % turn)


# ---- 6. the fleet ------------------------------------------------------------------------------------------------------------------------
def run_loop(traffic, check_model=False, with_check=False):
    """C cycles of traffic -> replan -> separation -> next_goals on the crossing scene.  traffic: None, or the keyword arguments of
    enable_traffic.  Returns (vehicle-cycles with FH_SEP_NEAR, traffic bits per row and cycle, withheld commits per cycle, per cycle:
    vehicles and plans as bytes)."""
    from test_gpu_fleet import P

    sc = gt.crossing_scene()
    fl = gt.views_fleet(sc)
    near, bits, withheld, trace = 0, [], [], []
    try:
        w0 = abi.point_mask_words(fl.n_cloud)
        if traffic is not None:
            fl.enable_traffic(**traffic)
            par = fl.traffic_par
            assert int(par["first_point"]) == 32 * w0 and float(par["hull"]) == P["drone_radius"]
        if with_check:
            fl.enable_check()
        for c in range(C):
            if traffic is not None:
                if check_model:
                    fl.sync()
                    cloud_before, mask_before = fl.cloud.cpu().numpy().copy(), fl.point_masks()
                fl.traffic()
                got_mask = fl.point_masks()
                if check_model:
                    want = model(par, fl.vehicles(), fl._host(fl.d_plans, abi.state_dtype).reshape(fl.n, fl.max_states), cloud_before, mask_before)
                    tm.assert_equal(fl.cloud.cpu().numpy(), got_mask, *want, "cycle %d" % c)
                    assert want[1][:, :w0 - 1].tobytes() == mask_before[:, :w0 - 1].tobytes()
                bits.append(ttm.traffic_bits(par, B, got_mask).sum(axis=1))
            fl.replan()
            if with_check:
                withheld.append(int(((fl.check_records()["flags"] & abi.FH_CHECK_CONFLICT) != 0).sum()))
            near += int(((fl.separation()["flags"] & abi.FH_SEP_NEAR) != 0).sum())
            trace.append((fl.vehicles().tobytes(), b"".join(p.tobytes() for p in fl.plans())))
            fl.next_goals(int(sc["ticks"][c]), follow=True)
    finally:
        fl.close()
    return near, bits, withheld, trace


TIMED = dict(samples=64, stride=5, range=6.0, timed=True, window=2)


def test_closed_loop_equals_the_model():
    """enable_traffic(64, 5, 6.0, timed=True, window=2), 4 cycles of traffic -> replan -> separation -> next_goals: every cycle's cloud
    tail and masks equal the model on the arrays read back, and the vehicles do see each other (in cycle 0 every plan is one state,
    the start, and every vehicle has another one within 6 m: DESIGN.md K8)."""
    near, bits, _, _ = run_loop(TIMED, check_model=True)
    assert len(bits) == C and bits[0].all()
    print("closed loop, timed window 2: FH_SEP_NEAR %d of %d; traffic bits per row, mean per cycle %s"
          % (near, B * C, [round(float(b.mean()), 1) for b in bits]))


def test_closed_loop_counts_as_observed():
    """Printed, not asserted (time-aware traffic): vehicle-cycles with FH_SEP_NEAR of 64 for traffic off, the untimed rule and
    the timed one with windows 0, 2 and 8 (and window 2 with a range of 2 m), and the same with enable_check and the withheld commits
    per cycle.  Observed on an MI355X: off 28 (withheld 6, 6, 13, 15), untimed 23 (6, 5, 10, 12), timed with range 6 m 23 for every
    window (6, 5, 10, 11), timed with range 2 m 26 (6, 6, 13, 15); with the check 8 of 64 in every row."""
    rows = [("off", None), ("untimed", dict(samples=64, stride=5, range=6.0))] + [("timed w=%d" % w, dict(TIMED, window=w)) for w in (0, 2, 8)]
    rows.append(("timed w=2, range 2 m", dict(TIMED, range=2.0)))   # (a range of the size of what is to be avoided, not of the neighbourhood)
    for name, traffic in rows:
        near, bits, _, _ = run_loop(traffic)
        near_c, _, withheld, _ = run_loop(traffic, with_check=True)
        print("closed loop %-20s FH_SEP_NEAR %2d of %d, bits per row (mean per cycle) %s; with the check %2d, withheld per cycle %s"
              % (name, near, B * C, [round(float(b.mean()), 1) for b in bits], near_c, withheld))


def test_a_timed_fleet_equals_one_that_is_given_its_points_and_bits():
    """Fleet A: enable_traffic(timed=True), then three times traffic() -> replan().  Fleet B never hears of traffic: before each replan it
    gets A's extended cloud through set_map and A's masks through set_point_views.  vehicles(), plans() and results() are equal in
    every byte: the feature adds points and bits and nothing else."""
    from test_gpu_fleet import P

    sc = gt.crossing_scene()
    a, b = gt.views_fleet(sc), None
    try:
        n_static = a.n_cloud
        a.enable_traffic(samples=6, stride=25, range=6.0, timed=True, window=1)
        assert a.traffic_par.dtype == abi.traffic_timed_params_dtype and int(a.traffic_par["window"]) == 1
        assert int(a.traffic_par["first_instant"]) == int(a.params["delta_t"]) - 1
        assert a.n_cloud == n_static and a.n_cloud_all == abi.point_mask_words(n_static) * 32 + B * 6 * 7
        seen = False
        for turn in range(3):
            a.traffic()
            a.sync()
            cloud, mask = a.cloud.cpu().numpy().copy(), a.point_masks()
            seen = seen or bool(mask[:, abi.point_mask_words(n_static):].any())
            if b is None:
                b = gt.views_fleet(sc, cloud, mask)
            else:
                b.set_map(cloud, sc["cells"], P["res"], sc["center"], P["z_max"], P["inflation"])
                b.set_point_views(mask)
            assert [name for name, _ in a.stages()] == [name for name, _ in b.stages()]
            a.replan()
            b.replan()
            assert a.vehicles().tobytes() == b.vehicles().tobytes(), turn
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a.plans(), b.plans())), turn
            ra, rb = a.results(), b.results()
            for k in ra:
                assert np.ascontiguousarray(ra[k]).tobytes() == np.ascontiguousarray(rb[k]).tobytes(), (turn, k)
            a.next_goals(5, follow=True)
            b.next_goals(5, follow=True)
        assert seen and b.traffic_par is None and b.n_cloud == a.n_cloud_all
    finally:
        a.close()
        if b is not None:
            b.close()


def test_an_untimed_fleet_flies_the_bytes_of_todays_signature():
    """timed=False: window and first_instant are ignored, the record is fh_traffic_params, and the fleet flies what a fleet built with
    the positional arguments of before flies."""
    sc = gt.crossing_scene()
    traces = []
    for kw in (dict(), dict(timed=False, window=7, first_instant=3)):
        fl = gt.views_fleet(sc)
        try:
            fl.enable_traffic(8, 25, 6.0, None, "all", **kw)
            assert fl.traffic_par.dtype == abi.traffic_params_dtype
            trace = []
            for c in range(2):
                fl.traffic()
                fl.replan()
                trace.append((fl.vehicles().tobytes(), b"".join(p.tobytes() for p in fl.plans()), fl.point_masks().tobytes()))
                fl.next_goals(int(sc["ticks"][c]), follow=True)
            traces.append(trace)
        finally:
            fl.close()
    assert traces[0] == traces[1]


def test_enable_traffic_refuses_more_samples_than_the_cap_when_timed():
    sc = gt.crossing_scene()
    fl = gt.views_fleet(sc)
    try:
        with pytest.raises(capi.FasterHipError):
            fl.enable_traffic(abi.FH_TRAFFIC_TIMED_MAX_SAMPLES + 1, 1, 6.0, hull=0.0, timed=True)
        assert fl.traffic_par is None
        fl.enable_traffic(abi.FH_TRAFFIC_TIMED_MAX_SAMPLES + 1, 1, 6.0, hull=0.0)                 # (the untimed rule has no cap)
        fl.set_point_views(np.full((B, abi.point_mask_words(fl.n_cloud)), 0xFFFFFFFF, dtype=np.uint32))
        fl.enable_traffic(abi.FH_TRAFFIC_TIMED_MAX_SAMPLES, 1, 6.0, hull=0.0, timed=True, window=3, first_instant=0)
        assert int(fl.traffic_par["first_instant"]) == 0 and int(fl.traffic_par["samples"]) == 512
        fl.traffic()
        fl.sync()
    finally:
        fl.close()
