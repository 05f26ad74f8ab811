"""GPU tests of the separation of committed plans (fh_fleet_separation_device, Fleet.separation; include/fasterhip_separation.h): every
byte of every record equals the numpy model (tests/separation_model.py, brute force over all pairs) — at the wavefront, stride and count
edges of the plans, with the LDS vehicle list below, at and above its capacity, where the broad phase's cells, the clamping and the
fleet-wide half-extent H decide what is looked at, on the hand cases of tests/test_separation_model.py, in a closed loop of the fleet;
no field depends on the cell grid, two runs give the same bytes, and a measurement writes nothing of the fleet."""
import numpy as np
import pytest

from faster_amd import abi, capi

import separation_model as sm
import test_separation_model as hand

pytestmark = pytest.mark.gpu
L = abi.FH_SEP_LIST_VEHICLES
ONE_CELL = ((0.0, 0.0, 0.0), 1.0, (1, 1, 1))
FINE = ((-0.37, -0.21, -0.55), 0.25, (24, 24, 8))   # 6 m x 6 m x 2 m, an origin that is not round


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch  # noqa: F401  (torch before the HIP library: one HIP runtime in the process)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def device_separation(c, par, vehicles, plans, max_states, cells):
    """fh_fleet_separation_device on device copies of the arrays, into a poisoned output."""
    import torch

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")

    n = len(vehicles)
    d_veh, d_plans = dev(vehicles), dev(np.asarray(plans).reshape(n, max_states))
    d_out = torch.full((max(n, 1) * abi.plan_separation_dtype.itemsize,), 0xEE, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    c.fleet_separation_device(par, d_veh.data_ptr(), d_plans.data_ptr(), n, max_states, cells, d_out.data_ptr())
    c.sync()
    out = d_out.cpu().numpy()
    if n == 0:
        assert (out == 0xEE).all()
    return out[:n * abi.plan_separation_dtype.itemsize].view(abi.plan_separation_dtype).copy()


def check(c, par, v, pl, grids, what, want=None):
    """The device on every grid against the model; returns the model's records."""
    want = sm.separation(par, v, pl, pl.shape[1]) if want is None else want
    for g in grids:
        sm.assert_equal_records(device_separation(c, par, v, pl, pl.shape[1], g), want, "%s, grid %s" % (what, g[2]))
    return want


# ---- 1. plan lengths, strides and counts at the borders of the rounds of 64 states ------------------------------------------------------
SIZES = [0, 1, 2, 63, 64, 65, 127, 128, 129, 200, 64, 129, 1, 65]
MAX_STATES = 256


@pytest.fixture(scope="module")
def edge_fleet():
    """Plans of the sizes above at random heads, drifting through a box of 1.5 m so that most pairs come within cap; three bad records
    and a plan with positions that are not finite among them."""
    rng = np.random.default_rng(21)
    n = len(SIZES) + 3
    v = np.zeros(n, dtype=abi.vehicle_dtype)
    pl = np.zeros((n, MAX_STATES), dtype=abi.state_dtype)
    pl["pos"] = rng.uniform(0.0, 1.5, size=(n, MAX_STATES, 3))   # (what lies outside a plan is NEAR everything: reading it shows)
    for i, s in enumerate(SIZES):
        head = int(rng.integers(0, MAX_STATES - s + 1))
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        v["plan_head"][i], v["plan_size"][i] = head, s
        pl["pos"][i, head:head + s] = rng.uniform(0.0, 1.5, size=3) * (1, 1, 0.3) + 0.01 * np.arange(s)[:, None] * d
    pl["pos"][4, v["plan_head"][4] + 3] = (np.nan, 0.5, 0.5)
    pl["pos"][5, v["plan_head"][5] + 64] = (0.5, np.inf, 0.5)       # the last state, where it stands for the others
    v["plan_head"][-3], v["plan_size"][-3] = -1, 5
    v["plan_head"][-2], v["plan_size"][-2] = 10, -1
    v["plan_head"][-1], v["plan_size"][-1] = MAX_STATES - 4, 5
    return v, pl


@pytest.mark.parametrize("stride,count", [(1, 0), (3, 0), (64, 0), (1, 63), (1, 64), (1, 65), (3, 128), (64, 129), (1, 1000), (7, 1)])
def test_plan_sizes_strides_and_counts(ctx, edge_fleet, stride, count):
    v, pl = edge_fleet
    par = sm.params(0.3, 0.9, stride, count)
    want = check(ctx, par, v, pl, (FINE, ONE_CELL), "stride %d count %d" % (stride, count))
    assert (want["flags"][-3:] == abi.FH_SEP_BAD_PLAN).all() and (want["n_tested"][-3:] == 0).all()
    m = np.minimum(SIZES, count) if count else np.array(SIZES)
    assert (want["n_tested"][:len(SIZES)] == -(-m // stride)).all() and want["n_tested"][0] == 0
    assert np.isfinite(want["min_d2"][1:len(SIZES)]).sum() >= 10 and (want["n_near"] > 1).any()
    assert not np.isin(want["worst_other"], [0, len(v) - 3, len(v) - 2, len(v) - 1]).any()   # the empty plan and the bad records are nobody's other
    assert (((want["flags"] & abi.FH_SEP_NEAR) != 0) == (want["first"] >= 0)).all()
    if (stride, count) == (1, 0):
        assert want["flags"][4] & abi.FH_SEP_NOT_FINITE and want["flags"][5] & abi.FH_SEP_NOT_FINITE


@pytest.mark.parametrize("n", [0, 1, 2])
def test_no_vehicle_one_and_two(ctx, n):
    rng = np.random.default_rng(3)
    v, pl = hand.random_fleet(rng, max(n, 1), 70, box=0.5, sizes=[70, 33][:max(n, 1)])
    v, pl = v[:n], pl[:n]
    want = check(ctx, sm.params(0.3, 2.0), v, pl, (FINE, ONE_CELL), "n = %d" % n)
    if n == 1:
        assert want["min_d2"][0] == np.inf and want["n_tested"][0] == 70 and want["flags"][0] == 0
    if n == 2:
        assert np.isfinite(want["min_d2"]).all() and list(want["n_tested"]) == [70, 33]


# ---- 2. the hand cases: exact ties, strict bounds, hovering, bad records, empty plans, NaN and infinity on either side ---------------------
@pytest.mark.parametrize("name", sorted(hand.CASES))
def test_hand_cases(ctx, name):
    par, v, pl, expected = hand.CASES[name]
    want = check(ctx, par, v, pl, (ONE_CELL, ((-2.0, -2.0, -1.0), 0.5, (10, 10, 4))), name)
    hand.check(want, expected, name)


def test_a_shorter_subject_and_others_that_end_in_the_middle(ctx):
    """Vehicle 0 (100 states) passes vehicle 1 of size 1 and vehicle 2, which ends at j = 40 of it; vehicle 3 (30 states) is shorter than
    all it meets.  Rounds of 64: the hover branch is taken in the first round for some lanes and in the second for all."""
    line = np.stack([0.02 * np.arange(100), np.zeros(100), np.zeros(100)], axis=1)
    v, pl = sm.fleet([line, [(1.5, 0.1, 0)], line[:41] + (0, 0.2, 0.1), line[:30] + (0.05, -0.2, 0)])
    want = check(ctx, sm.params(0.25, 0.6), v, pl, (ONE_CELL, FINE), "hover")
    assert want["worst"][0] > 64 and want["n_near"][0] == 3 and want["n_tested"][3] == 30 and want["worst_other"][1] == -1


# ---- 3. the LDS list below, at and above its capacity; no field depends on the grid --------------------------------------------------------
@pytest.mark.parametrize("others", [L - 1, L, L + 1, int(2.2 * L)])
def test_list_capacity_and_grid_independence(ctx, others):
    """`others` vehicles and the subject within 0.4 m, cap 1 m: every one passes the box test of every other, so the list of a vehicle
    holds `others` candidates.  One cell (the flush at L - 64 and the lists after it), and a fine grid that spreads them over 8 cells."""
    rng = np.random.default_rng(others)
    pos = np.round(rng.uniform(0.0, 0.4, size=(others + 1, 3)) * 64) / 64    # (a lattice of 1/64: ties between vehicles happen)
    v, pl = sm.fleet([p[None, :] + 0.01 * np.arange(1 + i % 3)[:, None] for i, p in enumerate(pos)])
    par = sm.params(0.125, 1.0)
    want = sm.separation(par, v, pl, pl.shape[1])
    one = device_separation(ctx, par, v, pl, pl.shape[1], ONE_CELL)
    fine = device_separation(ctx, par, v, pl, pl.shape[1], ((0.0, 0.0, 0.0), 0.2, (2, 2, 2)))
    assert one.tobytes() == fine.tobytes()
    sm.assert_equal_records(one, want, "%d others in one cell" % others)
    assert np.isfinite(want["min_d2"]).all() and want["n_near"].max() > 8


@pytest.mark.parametrize("in_cell", [65, 129])
def test_few_of_many_in_one_cell_pass_the_box_test(ctx, in_cell):
    """One cell of 100 m with vehicles 3 m apart, cap 1 m: of the 65 (129) a wavefront loads in two (three) rounds only the planted
    neighbours pass the box test, and the compaction crosses the rounds."""
    rng = np.random.default_rng(in_cell)
    pos = np.array([(3.0 * (i % 12), 3.0 * (i // 12), 1.0) for i in range(in_cell)])
    for a, b in ((0, 40), (63, 41), (64, 42), (in_cell - 1 if in_cell > 65 else 30, 43)):      # b moves next to a
        pos[b] = pos[a] + (0.25, 0.0, 0.25)
    v, pl = sm.fleet([p[None, :] + 0.001 * rng.normal(size=(5, 3)) for p in pos])
    want = check(ctx, sm.params(0.5, 1.0), v, pl, (((-1.0, -1.0, -1.0), 100.0, (1, 1, 1)), ((-1.0, -1.0, -1.0), 100.0, (2, 1, 1))), "few of many")
    assert (np.isfinite(want["min_d2"]).sum(), int((want["n_near"] == 1).sum())) == (8, 8)


# ---- 4. cells: the half-extent H, centres on borders, vehicles outside the grid ------------------------------------------------------------
@pytest.mark.parametrize("apart", [1, 2, 3])
def test_a_long_box_is_found_from_cells_away(ctx, apart):
    """Vehicle 0 flies 2 `apart` metres along x through cells of 1 m: its centre lies `apart` cells from its end, where vehicle 1 stands
    (size 1) and vehicle 2 waits all the time.  Only H, the largest half-extent of the fleet, makes them look that far."""
    T = 129
    x = np.linspace(0.25, 0.25 + 2.0 * apart, T)
    long_plan = np.stack([x, np.full(T, 3.5), np.full(T, 0.5)], axis=1)
    end = long_plan[-1]
    v, pl = sm.fleet([long_plan, [end + (0.1, 0.25, 0)], np.repeat((end + (0.0, -0.25, 0.1))[None, :], T, axis=0), [(0.5, 0.5, 0.5)]])
    want = check(ctx, sm.params(0.5, 1.0), v, pl, (((0.0, 0.0, 0.0), 1.0, (8, 8, 2)), ONE_CELL), "%d cells apart" % apart)
    assert want["n_near"][0] == 2 and want["worst"][0] == T - 1 and want["worst_other"][2] == 0 and want["first"][2] > 64
    assert want["worst_other"][1] == 2   # (vehicle 1 tests j = 0 only, where vehicle 0 is 2 `apart` metres away: its side of the pair)


def test_centres_on_cell_borders_and_vehicles_outside_the_grid(ctx):
    """A grid of 3 x 3 x 2 cells of 1 m from the origin.  Standing vehicles exactly on borders and corners of cells with a neighbour
    0.25 m away in the next cell, and pairs outside the grid on each of its six sides, which are clamped into the border cells."""
    pts = []
    for p in ((1.0, 1.0, 1.0), (2.0, 0.5, 0.5), (0.5, 2.0, 1.0), (0.0, 0.0, 0.0), (3.0, 3.0, 2.0)):          # on borders and corners
        pts += [p, (p[0] - 0.25, p[1], p[2]), (p[0], p[1] + 0.25, p[2] - 0.25)]
    for p in ((-5.0, 1.5, 1.0), (8.0, 1.5, 1.0), (1.5, -7.0, 1.0), (1.5, 9.0, 1.0), (1.5, 1.5, -4.0), (1.5, 1.5, 6.0), (-1e6, -1e6, 1e6)):
        pts += [p, (p[0] + 0.25, p[1] - 0.25, p[2])]
    pts += [(-0.125, 1.5, 0.5), (0.125, 1.5, 0.5)]                                                            # one outside, one inside
    v, pl = sm.fleet([[p, p] for p in pts])
    want = check(ctx, sm.params(0.5, 1.0), v, pl, (((0.0, 0.0, 0.0), 1.0, (3, 3, 2)), ((0.0, 0.0, 0.0), 0.5, (6, 6, 4)), ONE_CELL), "borders")
    assert (want["flags"] == abi.FH_SEP_NEAR).all() and (want["n_near"] >= 1).all()


def test_not_finite_positions_and_a_box_that_overflows(ctx):
    """40 random plans with NaN and infinities sprinkled on them, one vehicle at +-1.7e308 (its half-extent, and so H, is infinite: every
    vehicle looks at every cell) and one at 1e300."""
    rng = np.random.default_rng(8)
    v, pl = hand.random_fleet(rng, 40, 80, box=1.5, sizes=rng.integers(2, 81, size=40))
    for i in range(0, 36, 3):
        s = int(v["plan_size"][i])
        pl["pos"][i, rng.integers(0, s), rng.integers(0, 3)] = (np.nan, np.inf, -np.inf)[i % 3]
    pl["pos"][36, 0] = (1.7e308, 0.5, 0.5)
    pl["pos"][36, 1] = (-1.7e308, 0.5, 0.5)
    pl["pos"][37, 0] = (1e300, -1e300, 0.5)
    pl["pos"][38, :int(v["plan_size"][38])] = np.nan                                              # no finite position at all
    par = sm.params(0.3, 0.9)
    want = check(ctx, par, v, pl, (FINE, ONE_CELL), "not finite")
    assert ((want["flags"] & abi.FH_SEP_NOT_FINITE) != 0).sum() == 13 and want["min_d2"][38] == np.inf and np.isfinite(want["min_d2"]).sum() > 20
    check(ctx, sm.params(0.3, 0.9, 5, 17), v, pl, (FINE,), "not finite, stride 5 count 17")


# ---- 5. 512 random vehicles, twice ------------------------------------------------------------------------------------------------------
def test_a_random_fleet_twice_gives_the_same_bytes(ctx):
    """The order of the vehicles inside a cell is whatever the atomics gave and may differ between the runs; the records may not."""
    rng = np.random.default_rng(77)
    v, pl = hand.random_fleet(rng, 512, 48, box=6.0)
    par = sm.params(0.3, 0.8)
    a = device_separation(ctx, par, v, pl, 48, FINE)
    b = device_separation(ctx, par, v, pl, 48, FINE)
    assert a.tobytes() == b.tobytes()
    sm.assert_equal_records(a, sm.separation(par, v, pl, 48), "512 random vehicles")
    assert np.isfinite(a["min_d2"]).sum() > 100 and (a["flags"] & abi.FH_SEP_NEAR).any()


# ---- 6. the closed loop -----------------------------------------------------------------------------------------------------------------
def test_closed_loop_with_crossing_goals_equals_the_model_and_writes_nothing():
    """16 vehicles of the forest of tests/test_gpu_fleet.py, each sent to the start of the vehicle opposite in the list, so that their
    plans cross; 4 cycles of replan -> separation -> next_goals.  Fleet.separation() equals the model on Fleet.plans() and
    Fleet.vehicles() read back, and vehicles() and plans() have the bytes they had before it.  The counts are printed as observed."""
    from test_gpu_fleet import P, scenario
    from test_gpu_fleet_occupancy import new_fleet

    B, C = 16, 4
    sc = dict(scenario(B, C, 31))
    starts = sc["states"]["pos"].copy()
    sc["goals"] = starts[(np.arange(B) + B // 2) % B].copy()
    sc["states"] = sc["states"].copy()
    sc["states"]["vel"] = 0.0
    fl = new_fleet(sc, B, P["inflation"])
    near = within = 0
    try:
        fl.set_unknown(np.zeros(int(np.prod(sc["dims"])), dtype=np.uint8), sc["origin"], P["res"], sc["dims"])   # everything is known
        for c in range(C):
            fl.replan()
            veh, plans = fl.vehicles(), fl.plans()
            raw = fl._host(fl.d_plans, abi.state_dtype).tobytes()
            mv, mpl = sm.fleet([p["pos"] for p in plans], max_states=fl.max_states)
            for kw in ({}, dict(cap=6.0, stride=3), dict(r=1.0, cap=3.0, count=P["delta_t"]), dict(cap=6.0, cells=ONE_CELL)):
                got = fl.separation(**kw)
                r = kw.get("r", 2.0 * P["drone_radius"])
                par = sm.params(r, kw.get("cap", 2.0 * r), kw.get("stride", 1), kw.get("count", 0))
                sm.assert_equal_records(got, sm.separation(par, mv, mpl, fl.max_states), "cycle %d, %s" % (c, kw))
            assert fl.vehicles().tobytes() == veh.tobytes() and fl._host(fl.d_plans, abi.state_dtype).tobytes() == raw
            assert (got["n_tested"] == veh["plan_size"]).all()
            near += int(((fl.separation()["flags"] & abi.FH_SEP_NEAR) != 0).sum())
            within += int(np.isfinite(got["min_d2"]).sum())
            fl.next_goals(int(sc["ticks"][c]), follow=True)
    finally:
        fl.close()
    assert within > 0   # (the cases above mean something: some plans come within 6 m of another)
    print("closed loop, %d vehicle-cycles with crossing goals: plans with another vehicle nearer than 2 drone_radius = %.2f m at one instant: %d; "
          "within 6 m: %d" % (B * C, 2.0 * P["drone_radius"], near, within))
