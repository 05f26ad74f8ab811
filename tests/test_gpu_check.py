"""GPU tests of the commit check (fh_fleet_backup_device, fh_fleet_check_device, fh_fleet_revert_device, Fleet.enable_check;
include/fasterhip_check.h): every byte of every record equals the numpy model (tests/check_model.py, brute force over all pairs and
instants) — at the wavefront, kept, stride and count edges of the plans, with the LDS list of others below, at and above its flush mark
and its capacity, where the broad phase's cells, the clamping and the fleet-wide half-extent H decide what is looked at, on the hand cases
of tests/test_check_model.py; no field depends on the cell grid, two runs give the same bytes, the check writes nothing but its records;
backup and revert against the model on poisoned buffers; and the closed loop of a fleet: with the check the set of near pairs never grows,
without it it does."""
import numpy as np
import pytest

from faster_amd import abi, capi

import check_model as cm
import test_check_model as hand

pytestmark = pytest.mark.gpu
L = abi.FH_CHECK_LIST_OTHERS
C, X, NF, BAD = abi.FH_CHECK_CANDIDATE, abi.FH_CHECK_CONFLICT, abi.FH_CHECK_NOT_FINITE, abi.FH_CHECK_BAD_PLAN
ONE_CELL = ((0.0, 0.0, 0.0), 1.0, (1, 1, 1))
FINE = ((-0.37, -0.21, -0.55), 0.25, (24, 24, 8))   # 6 m x 6 m x 2 m, an origin that is not round
GUARD = 64


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch  # noqa: F401  (torch before the HIP library: one HIP runtime in the process)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


def device_check(c, par, v, pl, ov, opl, max_states, cells):
    """fh_fleet_check_device on device copies of the four arrays, into a poisoned output with guard bytes on both sides.  The check is a
    measurement: the four arrays and the guards must have the bytes they had."""
    import torch

    n = len(v)
    host = [np.ascontiguousarray(a).view(np.uint8).reshape(-1) for a in (v, np.asarray(pl).reshape(n, max_states), ov, np.asarray(opl).reshape(n, max_states))]
    d = [dev(a) for a in host]
    nb = n * abi.plan_check_dtype.itemsize
    d_out = torch.full((nb + 2 * GUARD,), 0xEE, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    c.fleet_check_device(par, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), n, max_states, cells, d_out.data_ptr() + GUARD)
    c.sync()
    out = d_out.cpu().numpy()
    assert (out[:GUARD] == 0xEE).all() and (out[GUARD + nb:] == 0xEE).all()
    for a, t in zip(host, d):
        assert t.cpu().numpy().tobytes() == a.tobytes()
    return out[GUARD:GUARD + nb].view(abi.plan_check_dtype).copy()


def check(c, par, cycle, grids, what):
    """The device on every grid against the model; returns the model's records."""
    v, pl, ov, opl = cycle
    ms = pl.shape[1]
    want = cm.check(par, v, pl, ov, opl, ms)
    for g in grids:
        cm.assert_equal_records(device_check(c, par, v, pl, ov, opl, ms, g), want, "%s, grid %s" % (what, g[2]))
    return want


def random_cycle(rng, n, max_states, box, commit=0.7, speed=0.01):
    """n vehicles drifting through a box: old plans of random sizes at random heads; `commit` of them keep a random number of states
    and append a new drift from there (laid out at head 0, as fh_fleet_commit_device does)."""
    half = max_states // 2
    old, heads, commits = [], [], {}

    def drift(start, m):
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        return start[None, :] + speed * np.arange(m)[:, None] * d

    for i in range(n):
        s = int(rng.integers(1, half + 1))
        heads.append(int(rng.integers(0, max_states - s + 1)))
        old.append(drift(rng.uniform(0.0, box, size=3) * (1, 1, 0.3), s))
        if rng.random() < commit:
            kept = int(rng.integers(0, s))
            commits[i] = (s - kept - 1, drift(old[i][kept], int(rng.integers(1, half + 1))))
    return cm.scene(old, commits, max_states=max_states, heads=heads)


# ---- 1. plan lengths, kept states, strides and counts at the borders of the rounds of 64 instants ------------------------------------------
KEPT = [0, 1, 63, 64, 65, 128, 129]
NEW = [1, 63, 64, 65, 128, 129]
MAX_STATES = 320


@pytest.fixture(scope="module")
def edge_cycle():
    """One candidate per (kept, new states) pair — 42 of them, so that the tested instants of a plan number 1, 63, 64, 65, 128 and 129
    behind every kept — in a box of 1.5 m where most pairs come close; others that did not commit of sizes 0, 1, 64, 65 and 300 (longer
    than every candidate: instants behind the candidates' plans); three records with bad extents; positions that are not finite."""
    rng = np.random.default_rng(42)

    def drift(start, m, speed=0.004):
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        return np.asarray(start)[None, :] + speed * np.arange(m)[:, None] * d

    old, heads, commits = [], [], {}
    for kept in KEPT:
        for new in NEW:
            i = len(old)
            s = kept + int(rng.integers(1, 20))
            heads.append(int(rng.integers(0, MAX_STATES - s + 1)))
            old.append(drift(rng.uniform(0.0, 1.5, size=3) * (1, 1, 0.3), s))
            commits[i] = (s - kept - 1, drift(old[i][kept], new))
    for s in (0, 1, 64, 65, 300, 5, 5, 5):
        heads.append(int(rng.integers(0, MAX_STATES - s + 1)))
        old.append(drift(rng.uniform(0.0, 1.5, size=3) * (1, 1, 0.3), s))
    v, pl, ov, opl = cm.scene(old, commits, max_states=MAX_STATES, heads=heads)
    pl["pos"][3, 64, 1] = np.nan                                # candidate (kept 0, 65 new states): state 64, the one lane of its second round
    pl["pos"][8, int(v["plan_size"][8]) - 1, 0] = np.inf        # the last state of a candidate, where it stands for longer others
    opl["pos"][20, heads[20] + 2, 2] = -np.inf                  # an old state: no flag of anyone
    ov["plan_head"][-3], v["plan_head"][-3] = -1, -1
    ov["plan_size"][-2], v["plan_size"][-2] = -1, -1
    ov["plan_head"][-1], v["plan_head"][-1] = MAX_STATES - 4, MAX_STATES - 4
    return v, pl, ov, opl


@pytest.mark.parametrize("stride,count", [(1, 0), (3, 0), (64, 0), (1, 63), (1, 64), (1, 65), (3, 128), (64, 129), (1, 1000), (7, 1)])
def test_plan_sizes_kept_strides_and_counts(ctx, edge_cycle, stride, count):
    want = check(ctx, cm.params(0.3, stride, count), edge_cycle, (FINE, ONE_CELL), "stride %d count %d" % (stride, count))
    nc = len(KEPT) * len(NEW)
    assert ((want["flags"][:nc] & C) != 0).all() and (want["flags"][nc:] == 0).all() and (want["n_tested"][nc:] == 0).all()
    size, kept = np.array([k + m for k in KEPT for m in NEW]), np.repeat(KEPT, len(NEW))
    m = np.minimum(size, count) if count else size
    assert (want["n_tested"][:nc] == np.maximum(-(-(m - kept) // stride), 0)).all()
    assert (((want["flags"] & X) != 0) == (want["first"] >= 0)).all() and (want["first"][want["first"] >= 0] >= kept[want["first"][:nc] >= 0]).all()
    assert not np.isin(want["first_other"], [len(want) - 3, len(want) - 2, len(want) - 1, nc]).any()   # bad records and the empty plan are nobody's other
    if (stride, count) == (1, 0):
        assert want["flags"][3] & NF and want["flags"][8] & NF and not want["flags"][20] & NF
        hit = want[want["first"] >= 0]
        assert 5 < len(hit) < nc and set(hit["first_kind"]) == {0, 1} and (hit["first"] > 128).any()


@pytest.mark.parametrize("n", [0, 1, 2, 65])
def test_no_vehicle_one_two_and_sixty_five(ctx, n):
    rng = np.random.default_rng(3 + n)
    cycle = random_cycle(rng, max(n, 1), 70, box=0.5 if n < 65 else 4.0, commit=1.0)
    cycle = tuple(a[:n] for a in cycle)
    want = check(ctx, cm.params(0.3), cycle, (FINE, ONE_CELL), "n = %d" % n)
    if n == 1:
        assert want["flags"][0] == C and want["first"][0] == -1 and want["d2"][0] == np.inf and want["n_tested"][0] >= 1
    if n == 65:
        assert (want["flags"] & X).any() and ((want["flags"] & (C | X)) == C).any()


# ---- 2. the hand cases ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(hand.CASES))
def test_hand_cases(ctx, name):
    par, cycle, expected, _ = hand.CASES[name]
    want = check(ctx, par, cycle, (ONE_CELL, ((-12.0, -12.0, -12.0), 1.5, (16, 16, 16))), name)
    hand.check(want, expected, name)


# ---- 3. the LDS list around its flush mark and its capacity; no field depends on the grid ------------------------------------------------------
@pytest.mark.parametrize("others,committed", [(L - 129, 0), (L - 128, 0), (L - 127, 0), (L - 1, 0), (L, 0), (L + 1, 0), (L // 2 - 1, 1), (L // 2, 1),
                                              (int(1.1 * L), 1)])
def test_list_capacity_and_grid_independence(ctx, others, committed):
    """`others` vehicles and the subject, the last one, within 0.4 m, r = 0.125 m on a lattice of 1/64 m (ties happen).  committed = 0:
    only the subject commits and its list holds `others` entries; the list is tested and emptied when it holds more than L - 128.
    committed = 1: every vehicle commits, so the subject lists each other twice (2 `others` entries) and the candidates below it fewer.
    One cell, and a fine grid that spreads them over 8 cells."""
    rng = np.random.default_rng(others + committed)
    pos = np.round(rng.uniform(0.0, 0.4, size=(others + 1, 3)) * 64) / 64
    old = [p[None, :] + np.round(rng.uniform(-2, 3, size=(1 + i % 3, 3))) / 64 for i, p in enumerate(pos)]
    new = lambda i: old[i][:1] + np.round(rng.uniform(-2, 3, size=(2 + i % 4, 3))) / 64   # noqa: E731
    commits = {i: (len(old[i]) - 1, new(i)) for i in (range(others + 1) if committed else [others])}
    cycle = cm.scene(old, commits)
    v, pl, ov, opl = cycle
    par = cm.params(0.125)
    want = cm.check(par, v, pl, ov, opl, pl.shape[1])
    one = device_check(ctx, par, v, pl, ov, opl, pl.shape[1], ONE_CELL)
    fine = device_check(ctx, par, v, pl, ov, opl, pl.shape[1], ((0.0, 0.0, 0.0), 0.2, (2, 2, 2)))
    assert one.tobytes() == fine.tobytes()
    cm.assert_equal_records(one, want, "%d others in one cell" % others)
    assert want["flags"][-1] & X and (not committed or set(want["first_kind"][want["first"] >= 0]) == {0, 1})


@pytest.mark.parametrize("in_cell", [65, 129])
def test_few_of_many_in_one_cell_pass_the_box_test(ctx, in_cell):
    """One cell of 100 m with vehicles 3 m apart, r = 0.5 m: of the 65 (129) a wavefront loads in two (three) turns only the planted
    neighbours pass the box test, and the compaction crosses the turns."""
    rng = np.random.default_rng(in_cell)
    pos = np.array([(3.0 * (i % 12), 3.0 * (i // 12), 1.0) for i in range(in_cell)])
    for a, b in ((0, 40), (63, 41), (64, 42), (in_cell - 1 if in_cell > 65 else 30, 43)):      # b moves next to a
        pos[b] = pos[a] + (0.25, 0.0, 0.25)
    old = [p[None, :] + 0.001 * rng.normal(size=(5, 3)) for p in pos]
    commits = {i: (2, old[i][2][None, :] + 0.001 * rng.normal(size=(4, 3))) for i in range(in_cell) if i % 3 != 1}
    want = check(ctx, cm.params(0.5), cm.scene(old, commits), (((-1.0, -1.0, -1.0), 100.0, (1, 1, 1)), ((-1.0, -1.0, -1.0), 100.0, (2, 1, 1))), "few of many")
    assert 4 <= int(((want["flags"] & X) != 0).sum()) <= 8


# ---- 4. cells: the half-extent H, centres on borders, vehicles outside the grid, a box that overflows -------------------------------------
@pytest.mark.parametrize("apart", [1, 2, 3])
def test_a_long_box_is_found_from_cells_away(ctx, apart):
    """Vehicle 3 stands at (0.25, 3.5, 0.5) and commits a flight of 2 `apart` metres along x through cells of 1 m; vehicle 1 stands at
    its end (one state) and vehicle 2 waits next to it all the time.  The centres of their boxes lie `apart` cells from the centre of
    vehicle 3's: only H, the largest half-extent of the fleet, makes it look that far.  Vehicle 0 is far away."""
    T = 129
    x = np.linspace(0.25, 0.25 + 2.0 * apart, T)
    flight = np.stack([x, np.full(T, 3.5), np.full(T, 0.5)], axis=1)
    end = flight[-1]
    cycle = cm.scene([[(0.5, 0.5, 0.5)], [end + (0.1, 0.25, 0)], np.repeat((end + (0.0, -0.25, 0.1))[None, :], T, axis=0), flight[:1]], {3: (0, flight)})
    want = check(ctx, cm.params(0.5), cycle, (((0.0, 0.0, 0.0), 1.0, (8, 8, 2)), ONE_CELL), "%d cells apart" % apart)
    assert want["flags"][3] == C | X and want["first"][3] > 64 and want["first_other"][3] in (1, 2)


def test_centres_on_cell_borders_and_vehicles_outside_the_grid(ctx):
    """A grid of 3 x 3 x 2 cells of 1 m from the origin.  Standing vehicles exactly on borders and corners of cells, each with a
    vehicle that commits a hop to 0.25 m from it out of the next cell, and such pairs outside the grid on each of its six sides, which
    are clamped into the border cells."""
    old, commits = [], {}
    spots = [(1.0, 1.0, 1.0), (2.0, 0.5, 0.5), (0.5, 2.0, 1.0), (0.0, 0.0, 0.0), (3.0, 3.0, 2.0), (-5.0, 1.5, 1.0), (8.0, 1.5, 1.0), (1.5, -7.0, 1.0),
             (1.5, 9.0, 1.0), (1.5, 1.5, -4.0), (1.5, 1.5, 6.0), (-1e6, -1e6, 1e6), (-0.125, 1.5, 0.5)]
    for p in spots:
        p = np.array(p)
        old += [[p], [p + (1.25, 0.0, 0.0)]]
        commits[len(old) - 1] = (0, [p + (1.25, 0.0, 0.0), p + (0.25, 0.0, 0.0)])
    want = check(ctx, cm.params(0.5), cm.scene(old, commits),
                 (((0.0, 0.0, 0.0), 1.0, (3, 3, 2)), ((0.0, 0.0, 0.0), 0.5, (6, 6, 4)), ONE_CELL), "borders")
    assert (want["flags"][1::2] == C | X).all() and (want["first"][1::2] == 1).all() and (want["flags"][0::2] == 0).all()


def test_not_finite_positions_and_a_box_that_overflows(ctx):
    """40 random vehicles with NaN and infinities sprinkled on old and new plans, one new plan from +1.7e308 to -1.7e308 (its
    half-extent, and so H, is infinite: every candidate looks at every cell), one at 1e300 and one with no finite position at all."""
    rng = np.random.default_rng(8)
    v, pl, ov, opl = random_cycle(rng, 40, 80, box=1.5, commit=0.8)
    cand = np.nonzero(v["stage"] == abi.FH_FLEET_STAGE_COMMITTED)[0]
    for i in range(0, 36, 3):   # the last state of a new plan (always tested), any state of an old one
        side_v, side_pl = (v, pl) if i % 2 == 0 else (ov, opl)
        h, s = int(side_v["plan_head"][i]), int(side_v["plan_size"][i])
        side_pl["pos"][i, h + (s - 1 if i % 2 == 0 else rng.integers(0, s)), rng.integers(0, 3)] = (np.nan, np.inf, -np.inf)[i % 3]
    a, b, c3 = cand[-1], cand[-2], cand[-3]
    pl["pos"][a, int(v["plan_size"][a]) - 1] = (1.7e308, 0.5, 0.5)
    pl["pos"][a, int(v["plan_size"][a]) - 2] = (-1.7e308, 0.5, 0.5) if v["plan_size"][a] >= 2 else pl["pos"][a, 0]
    pl["pos"][b, int(v["plan_size"][b]) - 1] = (1e300, -1e300, 0.5)
    pl["pos"][c3, :int(v["plan_size"][c3])] = np.nan
    want = check(ctx, cm.params(0.3), (v, pl, ov, opl), (FINE, ONE_CELL), "not finite")
    tested = [i for i in range(0, 36, 6) if i in cand]
    assert want["flags"][c3] & NF and want["first"][c3] == -1 and all(want["flags"][i] & NF for i in tested) and (want["flags"] & X).any()
    assert ((want["flags"] & NF) != 0).sum() <= len(tested) + 1   # a NaN of an old plan, or of a vehicle that did not commit, is no flag
    check(ctx, cm.params(0.3, 5, 17), (v, pl, ov, opl), (FINE,), "not finite, stride 5 count 17")


# ---- 5. 512 random vehicles, twice -----------------------------------------------------------------------------------------------------------
def test_a_random_fleet_twice_gives_the_same_bytes(ctx):
    """The order of the vehicles inside a cell is whatever the atomics gave and may differ between the runs; the records may not."""
    rng = np.random.default_rng(77)
    v, pl, ov, opl = random_cycle(rng, 512, 48, box=6.0)
    par = cm.params(0.3)
    a = device_check(ctx, par, v, pl, ov, opl, 48, FINE)
    b = device_check(ctx, par, v, pl, ov, opl, 48, FINE)
    assert a.tobytes() == b.tobytes()
    cm.assert_equal_records(a, cm.check(par, v, pl, ov, opl, 48), "512 random vehicles")
    hit = a[a["first"] >= 0]
    assert len(hit) > 20 and set(hit["first_kind"]) == {0, 1} and ((a["flags"] & (C | X)) == C).sum() > 100


# ---- 5b. the separation and the check share the working buffers of a context ------------------------------------------------------------------
def test_separation_and_check_back_to_back_on_shared_buffers(ctx):
    """Both stages sort their boxes into the same five working buffers of a context.  Four calls on one context with no wait between
    them: separation of 65 vehicles in one cell; check of 200 on 4 x 4 x 2 cells (every shared buffer grows, the box records go from 64 to
    80 bytes); separation of 200 on 3 x 3 x 1 cells; check of 65 in one cell.  Each output equals the same call alone on a fresh
    context, byte for byte, and its model."""
    import torch

    import separation_model as sm

    MS = 48
    small, large = random_cycle(np.random.default_rng(91), 65, MS, box=2.0), random_cycle(np.random.default_rng(92), 200, MS, box=6.0)
    spar, cpar = sm.params(0.3, 0.6), cm.params(0.3)
    calls = [("separation", small, ONE_CELL), ("check", large, ((0.0, 0.0, 0.0), 1.5, (4, 4, 2))),
             ("separation", large, ((0.0, 0.0, 0.0), 2.0, (3, 3, 1))), ("check", small, ONE_CELL)]
    dtype = {"separation": abi.plan_separation_dtype, "check": abi.plan_check_dtype}

    def launch(c, kind, cycle, cells, d_out):
        d, n = inputs[id(cycle)], len(cycle[0])
        if kind == "separation":
            c.fleet_separation_device(spar, d[0].data_ptr(), d[1].data_ptr(), n, MS, cells, d_out.data_ptr())
        else:
            c.fleet_check_device(cpar, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), n, MS, cells, d_out.data_ptr())

    def outputs():
        return [torch.full((len(cy[0]) * dtype[kind].itemsize,), 0xEE, dtype=torch.uint8, device="cuda:0") for kind, cy, _ in calls]

    inputs = {id(cy): [dev(a) for a in cy] for cy in (small, large)}
    outs, alone = outputs(), outputs()
    torch.cuda.synchronize()
    for (kind, cy, cells), d_out in zip(calls, outs):   # back to back: nothing here waits for the stream
        launch(ctx, kind, cy, cells, d_out)
    ctx.sync()
    for (kind, cy, cells), d_out, d_alone in zip(calls, outs, alone):
        fresh = capi.Context(0)
        try:
            launch(fresh, kind, cy, cells, d_alone)
            fresh.sync()
        finally:
            fresh.close()
        got = d_out.cpu().numpy().view(dtype[kind]).copy()
        what = "%s of %d vehicles on %s cells" % (kind, len(cy[0]), cells[2])
        assert got.tobytes() == d_alone.cpu().numpy().tobytes(), what + ": not what the call gives alone on a fresh context"
        if kind == "separation":
            sm.assert_equal_records(got, sm.separation(spar, cy[0], cy[1], MS), what)
        else:
            cm.assert_equal_records(got, cm.check(cpar, cy[0], cy[1], cy[2], cy[3], MS), what)
    # (the scene shows something: vehicles near each other and commits in conflict, in both fleets)
    for (kind, _, _), d_out in zip(calls, outs):
        rec = d_out.cpu().numpy().view(dtype[kind])
        assert (rec["flags"] & (abi.FH_SEP_NEAR if kind == "separation" else X)).any()


# ---- 6. backup and revert on poisoned buffers ----------------------------------------------------------------------------------------------
def copy_fleet(rng):
    """Vehicle records of random bytes with extents at the borders that matter: heads of zero and not, sizes whose 6 s chunks of 16
    bytes end below, at and above a turn of 64 lanes (10, 11, 32), the rounds of 64 states, empty, and the three kinds of bad extent."""
    ms = 160
    ext = [(0, 0), (0, 1), (7, 1), (0, 10), (3, 11), (0, 32), (5, 32), (0, 63), (9, 64), (0, 65), (31, 129), (0, ms), (ms, 0), (ms - 1, 1),
           (-1, 5), (10, -1), (ms - 4, 5), (2 ** 31 - 1, 2 ** 31 - 1)]
    n = len(ext)
    v = np.frombuffer(rng.bytes(n * abi.vehicle_dtype.itemsize), dtype=abi.vehicle_dtype).copy()
    pl = np.frombuffer(rng.bytes(n * ms * abi.state_dtype.itemsize), dtype=abi.state_dtype).reshape(n, ms).copy()
    for k, (h, s) in enumerate(ext):
        v["plan_head"][k], v["plan_size"][k] = h, s
    return v, pl, ms


def test_backup_against_the_model_on_poisoned_buffers(ctx):
    import torch

    v, pl, ms = copy_fleet(np.random.default_rng(5))
    n = len(v)
    want_v = np.frombuffer(bytes([cm.POISON]) * v.nbytes, dtype=abi.vehicle_dtype).copy()
    want_pl = np.frombuffer(bytes([cm.POISON]) * pl.nbytes, dtype=abi.state_dtype).reshape(n, ms).copy()
    cm.backup(v, pl, ms, want_v, want_pl)
    d_v, d_pl = dev(v), dev(pl)
    d_bv = torch.full((v.nbytes + 2 * GUARD,), cm.POISON, dtype=torch.uint8, device="cuda:0")
    d_bpl = torch.full((pl.nbytes + 2 * GUARD,), cm.POISON, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.fleet_backup_device(d_v.data_ptr(), d_pl.data_ptr(), n, ms, d_bv.data_ptr() + GUARD, d_bpl.data_ptr() + GUARD)
    ctx.sync()
    assert d_v.cpu().numpy().tobytes() == v.tobytes() and d_pl.cpu().numpy().tobytes() == pl.tobytes()
    for got, want in ((d_bv.cpu().numpy(), want_v), (d_bpl.cpu().numpy(), want_pl)):
        assert (got[:GUARD] == cm.POISON).all() and (got[-GUARD:] == cm.POISON).all()
        assert got[GUARD:-GUARD].tobytes() == want.tobytes()   # the records, the live extents, and poison everywhere else


def test_revert_against_the_model_on_poisoned_buffers(ctx):
    import torch

    rng = np.random.default_rng(6)
    bv, bpl, ms = copy_fleet(rng)
    n = len(bv)
    v = np.frombuffer(bytes([cm.POISON]) * bv.nbytes, dtype=abi.vehicle_dtype).copy()
    pl = np.frombuffer(bytes([cm.POISON]) * bpl.nbytes, dtype=abi.state_dtype).reshape(n, ms).copy()
    rec = np.frombuffer(rng.bytes(n * abi.plan_check_dtype.itemsize), dtype=abi.plan_check_dtype).copy()   # (only one bit of a record matters)
    rec["flags"] = np.where(np.arange(n) % 3 != 2, rec["flags"] | X, rec["flags"] & ~X)
    want_v, want_pl = v.copy(), pl.copy()
    loose = cm.revert(rec, bv, bpl, ms, want_v, want_pl)
    assert loose.any() and ((rec["flags"] & X) != 0).sum() == 12
    d_rec, d_bv, d_bpl = dev(rec), dev(bv), dev(bpl)
    d_v = torch.full((v.nbytes + 2 * GUARD,), cm.POISON, dtype=torch.uint8, device="cuda:0")
    d_pl = torch.full((pl.nbytes + 2 * GUARD,), cm.POISON, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.fleet_revert_device(d_rec.data_ptr(), d_bv.data_ptr(), d_bpl.data_ptr(), n, ms, d_v.data_ptr() + GUARD, d_pl.data_ptr() + GUARD)
    ctx.sync()
    for t, a in ((d_rec, rec), (d_bv, bv), (d_bpl, bpl)):
        assert t.cpu().numpy().tobytes() == a.tobytes()
    got_v, got_pl = d_v.cpu().numpy(), d_pl.cpu().numpy()
    for got in (got_v, got_pl):
        assert (got[:GUARD] == cm.POISON).all() and (got[-GUARD:] == cm.POISON).all()
    got_v = got_v[GUARD:-GUARD].view(abi.vehicle_dtype)
    got_pl = got_pl[GUARD:-GUARD].view(abi.state_dtype).reshape(n, ms)
    assert got_v.tobytes() == want_v.tobytes()
    assert (got_v["stage"][(rec["flags"] & X) != 0] == abi.FH_FLEET_STAGE_CONFLICT).all()
    # every state but those of a reverted plan outside its restored extent, which the header leaves unspecified
    assert got_pl[~loose].tobytes() == want_pl[~loose].tobytes()


# ---- 7. the closed loop ------------------------------------------------------------------------------------------------------------------------
def crossing(B, C_):
    from test_gpu_fleet import scenario

    sc = dict(scenario(B, C_, 31))
    starts = sc["states"]["pos"].copy()
    sc["goals"] = starts[(np.arange(B) + B // 2) % B].copy()
    sc["states"] = sc["states"].copy()
    sc["states"]["vel"] = 0.0
    return sc


def crossing_fleet(sc, B):
    from test_gpu_fleet import P
    from test_gpu_fleet_occupancy import new_fleet

    fl = new_fleet(sc, B, P["inflation"])
    fl.set_unknown(np.zeros(int(np.prod(sc["dims"])), dtype=np.uint8), sc["origin"], P["res"], sc["dims"])   # everything is known
    return fl


def whole_plans(fl):
    return fl.vehicles(), fl._host(fl.d_plans, abi.state_dtype).reshape(fl.n, fl.max_states)


def near_pairs(fl, c, r):
    """The near pairs of the fleet's plans as they stand, Fleet.separation(stride = 1, count = 0) the judge: it names the vehicles that
    are near somebody, the same entry point on the two plans of a pair alone says whether that pair is near; the model agrees."""
    v, pl = whole_plans(fl)

    def on_device(par, veh, plans, ms):
        n = len(veh)
        if n == fl.n:
            return fl.separation(r=float(par["r"]), cap=float(par["cap"]), stride=1, count=0)
        import torch

        d_v, d_pl = dev(veh), dev(plans)
        d_out = torch.empty(n * abi.plan_separation_dtype.itemsize, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        c.fleet_separation_device(par, d_v.data_ptr(), d_pl.data_ptr(), n, ms, ONE_CELL, d_out.data_ptr())
        c.sync()
        return d_out.cpu().numpy().view(abi.plan_separation_dtype).copy()

    pairs = cm.near_pairs(r, v, pl, fl.max_states, separation=on_device)
    assert pairs == cm.near_pairs(r, v, pl, fl.max_states)
    return pairs


def test_closed_loop_near_pairs_never_grow_with_the_check_and_do_without_it(ctx):
    """16 vehicles of the forest of tests/test_gpu_fleet.py, each sent to the start of the vehicle opposite in the list, so that their
    plans cross; 4 cycles of replan -> next_goals.  First without enable_check: a replan creates a near pair that was not there (the
    test that fails without the feature is the second half: the same scene must not).  Then with enable_check(stride = 1, count = 0),
    the stages run one by one: the backup equals the model's, every cycle's records equal the model on the arrays read back, the revert
    equals the model, and the set of near pairs after every replan and after every next_goals is a subset of the set before it.  How
    many commits are withheld and who arrives is printed as observed."""
    from test_gpu_fleet import P

    B, CY = 16, 4
    r = 2.0 * P["drone_radius"]
    sc = crossing(B, CY)
    # without the check
    fl = crossing_fleet(sc, B)
    try:
        assert [name for name, _ in fl.stages()] == ["begin", "path_search", "corridors", "corridor_problems", "whole_solve", "safe_corridor",
                                                     "safe_solve", "commit"]
        start = near_pairs(fl, ctx, r)
        before, grew = start, []
        for cyc in range(CY):
            fl.replan()
            after = near_pairs(fl, ctx, r)
            grew.append(sorted(after - before))
            fl.next_goals(int(sc["ticks"][cyc]), follow=True)
            before = near_pairs(fl, ctx, r)
        free_arrived = int((fl.vehicles()["status"] != abi.FH_VEHICLE_TRAVELING).sum())
    finally:
        fl.close()
    print("closed loop without the check: near pairs at the start %s; new near pairs per replan %s" % (sorted(start), grew))
    assert any(grew), "no replan of the unchecked fleet created a near pair: the scene shows nothing"
    # with it
    fl = crossing_fleet(sc, B)
    withheld, committed = [], []
    try:
        fl.enable_check(stride=1, count=0)
        assert [name for name, _ in fl.stages()][-5:] == ["safe_solve", "backup", "commit", "check", "revert"]
        par = cm.params(r)
        before = near_pairs(fl, ctx, r)
        assert before == start
        for cyc in range(CY):
            fl._follow_current()
            for name, launch in fl.stages():
                launch()
                if name == "safe_solve":
                    v0, pl0 = whole_plans(fl)
                elif name == "backup":
                    ov = fl._host(fl.d_backup_vehicles, abi.vehicle_dtype)
                    opl = fl._host(fl.d_backup_plans, abi.state_dtype).reshape(B, fl.max_states)
                    assert ov.tobytes() == v0.tobytes()
                    for k in range(B):
                        h, s = int(ov["plan_head"][k]), int(ov["plan_size"][k])
                        assert opl[k, h:h + s].tobytes() == pl0[k, h:h + s].tobytes()
                elif name == "commit":
                    v1, pl1 = whole_plans(fl)
                elif name == "check":
                    rec = fl.check_records()
                    cm.assert_equal_records(rec, cm.check(par, v1, pl1, ov, opl, fl.max_states), "cycle %d" % cyc)
                    assert whole_plans(fl)[0].tobytes() == v1.tobytes() and whole_plans(fl)[1].tobytes() == pl1.tobytes()
                elif name == "revert":
                    v2, pl2 = whole_plans(fl)
                    want_v, want_pl = v1.copy(), pl1.copy()
                    loose = cm.revert(rec, ov, opl, fl.max_states, want_v, want_pl)
                    assert v2.tobytes() == want_v.tobytes() and pl2[~loose].tobytes() == want_pl[~loose].tobytes()
            committed.append(int(((rec["flags"] & C) != 0).sum()))
            withheld.append(int(((rec["flags"] & X) != 0).sum()))
            assert (v2["stage"][(rec["flags"] & X) != 0] == abi.FH_FLEET_STAGE_CONFLICT).all()
            after = near_pairs(fl, ctx, r)
            assert after <= before, "cycle %d: the replan created the near pairs %s" % (cyc, sorted(after - before))
            fl.next_goals(int(sc["ticks"][cyc]), follow=True)
            before = near_pairs(fl, ctx, r)
            assert before <= after, "cycle %d: next_goals created the near pairs %s" % (cyc, sorted(before - after))
        arrived = int((fl.vehicles()["status"] != abi.FH_VEHICLE_TRAVELING).sum())
    finally:
        fl.close()
    print("closed loop with the check, r = %.2f m: committed per cycle %s, of them withheld %s; vehicles no longer TRAVELING after %d cycles: %d "
          "(without the check: %d); near pairs at the end %s" % (r, committed, withheld, CY, arrived, free_arrived, sorted(before)))


def test_a_check_that_never_fires_leaves_the_fleet_as_it_is_without_enable_check():
    """The same scene twice, 3 cycles: a fleet that never calls enable_check launches the chain it always launched, and a fleet with
    enable_check(r = 0), whose check can find nothing, ends every cycle with the same bytes in vehicles() and in the plans: backup,
    check and revert change nothing of a fleet that has no conflict."""
    B, CY = 16, 3
    sc = crossing(B, CY)
    got = []
    for checked in (False, True):
        fl = crossing_fleet(sc, B)
        try:
            if checked:
                fl.enable_check(r=0.0)
            assert len(fl.stages()) == (11 if checked else 8)
            cycles = []
            for cyc in range(CY):
                fl.replan()
                cycles.append([a.tobytes() for a in (fl.vehicles(),) + tuple(fl.plans())])
                if checked:
                    rec = fl.check_records()
                    assert not (rec["flags"] & X).any() and (rec["flags"] & C).any()
                fl.next_goals(int(sc["ticks"][cyc]), follow=True)
            got.append(cycles)
        finally:
            fl.close()
    assert got[0] == got[1]
