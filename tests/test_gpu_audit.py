"""GPU tests of the plan audit (fh_fleet_audit_device, Fleet.audit; include/fasterhip_audit.h): every field of every record equals the
numpy model (tests/audit_model.py) bit for bit — on hand-built vehicle records and plans at the wavefront, stride and count edges, with
the hand cases of tests/test_audit_model.py among them; with the LDS point list at its capacity; on a fine lattice whose box takes several
slabs; in a closed loop of the fleet; and a measurement changes nothing."""
import numpy as np
import pytest

from faster_amd import abi, capi

import audit_model as am
import test_audit_model as hand

pytestmark = pytest.mark.gpu
L, SLAB = abi.FH_AUDIT_LIST_POINTS, abi.FH_AUDIT_SLAB_CELLS
MAX_STATES = 1024
GRID = ((0.37, -0.21, 0.05), 0.25, (40, 36, 12))   # 10 m x 9 m x 3 m, an origin that is not round
CELLS = 40 * 36 * 12


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch  # noqa: F401  (torch before the HIP library: one HIP runtime in the process)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def device_audit(c, par, vehicles, plans, max_states, grid=None, flags=None, view_stride=None, view_of=None, n_views=0, cloud=None, point_mask=None):
    """fh_fleet_audit_device on device copies of the arrays; flags [n_views][cells] are laid out with view_stride bytes per view."""
    import torch

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")

    n = len(vehicles)
    keep = [dev(vehicles), dev(np.asarray(plans).reshape(n, max_states))]
    kw = {}
    if flags is not None:
        flags = np.asarray(flags, dtype=np.uint8).reshape(len(flags), -1)
        stride = flags.shape[1] if view_stride is None else view_stride
        if stride:
            laid = np.full((len(flags), stride), 1, dtype=np.uint8)   # (what lies between two views is unknown: it must never be read)
            laid[:, :flags.shape[1]] = flags
        else:
            laid = flags[:1]
        keep.append(dev(laid))
        kw.update(grid=grid, d_flags=keep[-1].data_ptr(), view_stride=stride)
    if view_of is not None:
        keep.append(dev(np.asarray(view_of, dtype=np.int32)))
        kw.update(d_view_of=keep[-1].data_ptr())
    if cloud is not None and len(cloud):
        keep.append(dev(np.asarray(cloud, dtype=np.float64).reshape(-1, 3)))
        kw.update(d_cloud=keep[-1].data_ptr(), n_cloud=len(cloud))
    if point_mask is not None:
        point_mask = np.asarray(point_mask, dtype=np.uint32)
        keep.append(dev(point_mask))
        kw.update(d_point_mask=keep[-1].data_ptr(), mask_words=point_mask.shape[1])
    d_out = torch.full((n * abi.plan_audit_dtype.itemsize,), 0xEE, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    c.fleet_audit_device(par, keep[0].data_ptr(), keep[1].data_ptr(), n, max_states, d_out.data_ptr(), n_views=n_views, **kw)
    c.sync()
    return d_out.cpu().numpy().view(abi.plan_audit_dtype).copy()


# ---- 1. hand-built plans ---------------------------------------------------------------------------------------------------------------------
SIZES = [0, 1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024]


def hand_built_fleet():
    """27 vehicles: every size of SIZES twice (the second with a head that is not zero where the plan leaves room), two more long plans, and
    three bad records.  Plans are gentle random curves that start inside or beside the lattice; the long ones cross its border and run
    more than 3 m outside.  Six views: random with 20 % unknown, all known, all unknown, one shared by two vehicles, random again."""
    rng = np.random.default_rng(2024)
    sizes = SIZES + SIZES + [700, 900]
    n = len(sizes) + 3
    veh = np.zeros(n, dtype=abi.vehicle_dtype)
    plans = np.zeros((n, MAX_STATES), dtype=abi.state_dtype)
    plans["pos"] = 1e6   # (states outside a plan lie nowhere near anything: reading one would show)
    for i, size in enumerate(sizes):
        head = 0 if i < len(SIZES) else int(rng.integers(0, MAX_STATES - size + 1))
        start = rng.uniform([-1.0, -1.0, 0.2], [11.0, 9.5, 2.8])
        u = rng.normal(size=3) * [1.0, 1.0, 0.15]
        u /= np.linalg.norm(u)
        step = rng.uniform(0.01, 0.03)
        k = np.arange(size)[:, None]
        pos = start + k * step * u + 0.2 * np.sin(k * 0.01 + rng.uniform(0, 6, size=3))
        veh["plan_head"][i], veh["plan_size"][i] = head, size
        plans["pos"][i, head:head + size] = pos
    # positions that are not finite, and one that is finite and absurd
    for i, j, v in ((9, 5, np.nan), (9, 1000, np.inf), (10, 64, -np.inf), (20, 0, np.nan), (21, 1023, 1e300), (5, 10, 1e300), (3, 62, np.nan)):
        plans["pos"][i, veh["plan_head"][i] + j, i % 3] = v
    plans["pos"][2, veh["plan_head"][2]:veh["plan_head"][2] + 2] = np.nan          # a plan with no finite state at all
    for i, (head, size) in zip(range(len(sizes), n), ((-1, 10), (0, -1), (MAX_STATES - 9, 10))):
        veh["plan_head"][i], veh["plan_size"][i] = head, size
    views = np.zeros((6, CELLS), dtype=np.uint8)
    views[0] = rng.random(CELLS) < 0.2
    views[2] = 1
    views[3] = rng.random(CELLS) < 0.2
    views[4] = rng.random(CELLS) < 0.2
    views[5] = (rng.random(CELLS) < 0.2) * 7                                        # (any non-zero byte is unknown)
    view_of = np.array([0, 1, 2, 3, 4, 5] * 5, dtype=np.int32)[:n]
    view_of[7], view_of[8] = 3, 3                                                   # two more vehicles share view 3
    view_of[12], view_of[13] = 6, -1                                                # out of range
    cloud = rng.uniform([-2.0, -2.0, 0.0], [12.0, 11.0, 3.0], size=(3001, 3))
    cloud[::97, 1] = np.nan
    mask = rng.integers(0, 2 ** 32, size=(6, abi.point_mask_words(len(cloud))), dtype=np.uint64).astype(np.uint32)
    return veh, plans, views, view_of, cloud, mask


@pytest.fixture(scope="module")
def fleet27():
    return hand_built_fleet()


@pytest.mark.parametrize("stride,count", [(1, 0), (2, 65), (10, 0), (64, 5000), (65, 64), (2000, 0), (1, 1), (1, 64), (3, 65)])
def test_hand_built_plans_equal_the_model(ctx, fleet27, stride, count):
    veh, plans, views, view_of, cloud, mask = fleet27
    par = am.params(0.3, 0.35, 0.6, stride, count)
    common = dict(grid=GRID, flags=views, view_of=view_of, n_views=6, cloud=cloud, point_mask=mask)
    want = am.audit(par, veh, plans, MAX_STATES, **common)
    got = device_audit(ctx, par, veh, plans, MAX_STATES, view_stride=CELLS + 13, **common)
    am.assert_equal_records(got, want, "stride %d count %d" % (stride, count))
    assert (got["flags"][-3:] == abi.FH_AUDIT_BAD_PLAN).all() and not got["n_tested"][-3:].any() and (got["view"][-3:] == -1).all()
    assert (got["flags"][:-3] & abi.FH_AUDIT_BAD_PLAN == 0).all()
    assert got["flags"][12] & abi.FH_AUDIT_NO_VIEW and got["flags"][13] & abi.FH_AUDIT_NO_VIEW and got["view"][12] == 6 and got["view"][13] == -1
    if (stride, count) == (1, 0):   # the case does exercise what it is built for
        assert (got["flags"] & abi.FH_AUDIT_UNKNOWN).any() and (got["flags"] & abi.FH_AUDIT_OCCUPIED).any()
        assert ((got["flags"] & abi.FH_AUDIT_NOT_FINITE) != 0).sum() >= 5 and np.isinf(got["min_unknown_d2"][[1, 12]]).all()
        assert (got["n_tested"][:len(SIZES)] == SIZES).all() and got["worst_unknown"].max() > 64


def test_one_grid_for_the_fleet_no_masks_and_single_sides(ctx, fleet27):
    """view_stride == 0 with n_views == 1: every vehicle reads view 0, whatever view_of says; without masks every point counts; each side
    alone; neither side."""
    veh, plans, views, view_of, cloud, mask = fleet27
    par = am.params(0.3, 0.35, 0.6, 2, 0)
    for kw, dkw in ((dict(grid=GRID, flags=views[:1], n_views=1, shared_grid=True, cloud=cloud), dict(view_stride=0)),
                    (dict(grid=GRID, flags=views[:1], n_views=1, shared_grid=True, view_of=view_of), dict(view_stride=0)),
                    (dict(cloud=cloud, point_mask=mask, view_of=view_of, n_views=6), {}),
                    (dict(cloud=cloud), {}),
                    (dict(grid=GRID, flags=views, n_views=6, view_of=view_of), {}),
                    ({}, {})):
        want = am.audit(par, veh, plans, MAX_STATES, **kw)
        mkw = {k: v for k, v in kw.items() if k != "shared_grid"}
        got = device_audit(ctx, par, veh, plans, MAX_STATES, **mkw, **dkw)
        am.assert_equal_records(got, want, str(sorted(kw)))
    assert (got["view"] == -1).all() and (got["flags"] & ~(abi.FH_AUDIT_BAD_PLAN | abi.FH_AUDIT_NOT_FINITE) == 0).all()


@pytest.mark.parametrize("name", sorted(hand.hand_cases()))
def test_the_hand_cases_on_the_device(ctx, name):
    """The cases of tests/test_audit_model.py, each surrounded by other vehicles of the same launch: the answers worked out by hand."""
    positions, par, want = hand.hand_cases()[name]
    v1, p1 = am.one_plan(positions, max_states=8, head=2)
    filler_v, filler_p = am.one_plan([hand.FAR, hand.at(0.3), hand.C], max_states=8)
    veh, plans = np.concatenate([filler_v, v1, filler_v]), np.concatenate([filler_p, p1, filler_p])
    if name == "mask":
        cloud, mask = hand.mask_case_inputs()
        kw = dict(cloud=cloud, point_mask=mask, n_views=1, view_of=[0, 0, 0])
    else:
        kw = dict(grid=hand.GRID, flags=hand.one_voxel_view(), n_views=1, view_of=[0, 0, 0])
    got = device_audit(ctx, par, veh, plans, 8, **kw)
    am.assert_equal_records(got, am.audit(par, veh, plans, 8, **kw), name)
    assert not hand.differs(got[1], want), (name, got[1], want)


# ---- 2. the point list at its capacity -----------------------------------------------------------------------------------------------------
CAP_LIST = 0.5
LINE = np.array([5.0, 5.0, 1.5]) + np.arange(70)[:, None] * np.array([0.01, 0.0, 0.0])   # one plan of 70 states along x


def edge_points(e=1e-6):
    """(six points e beyond cap from the nearest state, one on each side of the grown box; one point e inside cap of state 0)."""
    lo, hi, cap = LINE.min(axis=0), LINE.max(axis=0), CAP_LIST
    outside = [(lo[0] - cap - e, 5.0, 1.5), (hi[0] + cap + e, 5.0, 1.5), (5.3, lo[1] - cap - e, 1.5), (5.3, hi[1] + cap + e, 1.5),
               (5.3, 5.0, lo[2] - cap - e), (5.3, 5.0, hi[2] + cap + e)]
    return np.array(outside), np.array([lo[0] - cap + e, 5.0, 1.5])


def list_case(n_cloud, inside, masked, seed):
    """`inside` finite points that the vehicle knows lie in the box of LINE grown by cap (well inside it, two pairs of duplicates, the
    first one 0.15 m from state 10); every other point lies 2 m outside, or just outside a side of the box, or is not finite, or lies
    inside and is unknown to the view.  The known points include k = 31, 32, 63, 64 and the last one."""
    rng = np.random.default_rng(seed)
    cap, pos = CAP_LIST, LINE
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    cloud = rng.uniform(lo - 3.0, lo - 2.0, size=(n_cloud, 3))                      # far outside
    special = list(dict.fromkeys(k for k in (31, 32, 63, 64, n_cloud - 1) if 0 <= k < n_cloud))[:inside]
    order = [int(k) for k in rng.permutation(n_cloud) if int(k) not in set(special)]
    pick = np.array(special + order[:inside - len(special)], dtype=np.int64)
    rest = np.array(order[inside - len(special):], dtype=np.int64)                 # every point that is not inside and known
    assert len(pick) == inside and len(pick) + len(rest) == n_cloud
    cloud[pick] = rng.uniform(lo - 0.9 * cap, hi + 0.9 * cap, size=(len(pick), 3))
    cloud[pick[0]] = pos[10] + [0.05, 0.1, -0.1]
    if len(pick) > 3:
        cloud[pick[1]], cloud[pick[3]] = cloud[pick[0]], cloud[pick[2]]             # duplicates
    if len(rest) >= 9:
        cloud[rest[0], 0], cloud[rest[1], 1], cloud[rest[2], 2] = np.nan, np.inf, -np.inf
        cloud[rest[3:9]] = edge_points()[0]
    mask = None
    if masked:
        known = np.zeros(n_cloud, dtype=bool)
        known[pick] = True
        known[rest[::2]] = True                                                      # points outside the box that the view knows
        decoys = rest[9:][1::2][:20]                                                 # inside the box and NOT known
        cloud[decoys] = rng.uniform(lo - 0.5 * cap, hi + 0.5 * cap, size=(len(decoys), 3))
        mask = np.zeros((1, abi.point_mask_words(n_cloud) + 1), dtype=np.uint32)
        k = np.nonzero(known)[0]
        np.bitwise_or.at(mask[0], k >> 5, (np.uint32(1) << (k & 31).astype(np.uint32)))
    v, pl = am.one_plan(pos, max_states=80, head=3)
    return am.params(0.1, 0.45, cap), v, pl, cloud, mask


@pytest.mark.parametrize("n_cloud,inside,masked", [(19993, L - 1, False), (19993, L, False), (19993, L + 1, False), (19993, 2 * L + 1, False),
                                                   (19993, L, True), (19993, 2 * L + 1, True), (1, 1, False), (1, 1, True), (63, 63, True),
                                                   (64, 64, False), (64, 40, True), (65, 65, True), (65, 65, False)])
def test_the_point_list_at_its_capacity(ctx, n_cloud, inside, masked):
    par, v, pl, cloud, mask = list_case(n_cloud, inside, masked, 7 + n_cloud + inside)
    kw = dict(cloud=cloud, point_mask=mask, n_views=1 if masked else 0)
    want = am.audit(par, v, pl, 80, **kw)
    got = device_audit(ctx, par, v, pl, 80, **kw)
    am.assert_equal_records(got, want, "%d points, %d inside, masked %s" % (n_cloud, inside, masked))
    assert got["flags"][0] == abi.FH_AUDIT_OCCUPIED and got["n_tested"][0] == 70 and got["view"][0] == (0 if masked else -1)
    assert got["first_occupied"][0] >= 0 and got["min_occupied_d2"][0] <= 0.0225


def test_points_just_outside_and_just_inside_the_grown_box(ctx):
    """Alone with the plan, a point 1e-6 beyond cap on each side of the box is not seen; the one 1e-6 inside is, at (cap - 1e-6)^2."""
    par = am.params(0.1, 0.45, CAP_LIST)
    v, pl = am.one_plan(LINE, max_states=80, head=3)
    outside, inside_point = edge_points()
    got = device_audit(ctx, par, v, pl, 80, cloud=outside)
    am.assert_equal_records(got, am.audit(par, v, pl, 80, cloud=outside), "points outside only")
    assert got["flags"][0] == 0 and np.isinf(got["min_occupied_d2"][0]) and got["worst_occupied"][0] == -1
    both = np.concatenate([outside, inside_point[None]])
    got = device_audit(ctx, par, v, pl, 80, cloud=both)
    am.assert_equal_records(got, am.audit(par, v, pl, 80, cloud=both), "one point inside")
    d = inside_point[0] - LINE[0, 0]
    assert got["min_occupied_d2"][0] == d * d and got["worst_occupied"][0] == 0 and got["first_occupied"][0] == -1   # (0.45 < 0.5 - 1e-6)


# ---- 3. slabs ----------------------------------------------------------------------------------------------------------------------------------
FINE = ((-0.013, 0.007, 0.011), 0.02, (200, 150, 70))   # 4 m x 3 m x 1.4 m in cells of 2 cm: 2.1 M cells a view
FINE_CELLS = 200 * 150 * 70
CAP_FINE = 0.1


def box_cells(pos):
    b = am.device_box(pos.min(axis=0), pos.max(axis=0), CAP_FINE, FINE)
    return [hi - lo + 1 for lo, hi in b], b


def rows_per_slab(bx):
    return (SLAB // 64) // ((bx + 63) // 64)


def diagonal(lo, hi, n):
    p = lo + (np.arange(n) / max(n - 1, 1))[:, None] * (np.asarray(hi) - lo)
    p[-1] = hi
    return p


def extent_for(cells, axis, axis_lo):
    """hi so that positions in [axis_lo, hi] give a box of `cells` cells on this axis of FINE (searched with the restated formula)."""
    lo3 = np.array([1.0, 1.0, 0.3])
    lo3[axis] = axis_lo
    for k in range(2000):
        hi3 = lo3.copy()
        hi3[axis] = axis_lo + 0.005 * k
        b = am.device_box(lo3, hi3, CAP_FINE, FINE)
        if b[axis][1] - b[axis][0] + 1 == cells:
            return hi3[axis]
    raise AssertionError(cells)


def test_slabs_equal_the_model(ctx):
    """Vehicle 0 and 1: long plans on the fine lattice whose boxes take several slabs, 20 % unknown.  Vehicle 2: a box of exactly
    FH_AUDIT_SLAB_CELLS cells (64 x 32 x 32, one slab); vehicle 3: one row of cells more (64 x 33 x 32 needs a second slab).  Vehicle 4:
    everything known but ONE voxel in the first row of the second slab of its box, and the only state near it has its own cell in the
    last row of the first slab."""
    rng = np.random.default_rng(77)
    n = 5
    pos = [diagonal(np.array([0.5, 0.4, 0.2]), [3.2, 2.5, 1.1], 400) + 0.05 * np.sin(np.arange(400)[:, None] * 0.05),
           diagonal(np.array([3.6, 0.3, 1.2]), [0.4, 2.8, 0.15], 257)]
    lo = np.array([1.0, 1.0, 0.3])
    for by in (32, 33):
        hi = [extent_for(64, 0, lo[0]), extent_for(by, 1, lo[1]), extent_for(32, 2, lo[2])]
        pos.append(diagonal(lo, hi, 90))
    dims2, _ = box_cells(pos[2])
    dims3, _ = box_cells(pos[3])
    assert dims2 == [64, 32, 32] and dims2[0] * dims2[1] * dims2[2] == SLAB and dims3 == [64, 33, 32], (dims2, dims3)
    assert rows_per_slab(64) == dims2[1] * dims2[2] and dims3[1] * dims3[2] > rows_per_slab(64)
    # vehicle 4: a plan along x, and states that step in y across the border between the two slabs of its box
    base = diagonal(np.array([0.8, 1.2, 0.5]), [2.6, 2.2, 0.9], 120)
    dims4, b4 = box_cells(base)
    rps = rows_per_slab(dims4[0])
    assert dims4[1] * dims4[2] > rps and dims4[0] > 64
    r_border = rps                                       # the first row of the second slab
    z_b, y_b = b4[2][0] + r_border // dims4[1], b4[1][0] + r_border % dims4[1]
    assert r_border % dims4[1] > 0                       # (the row before it is the same z, one cell lower in y)
    x_b = (b4[0][0] + b4[0][1]) // 2
    centre = (np.array([x_b, y_b, z_b]) + 0.5) * FINE[1] + np.array(FINE[0])
    probe = centre - [0.0, FINE[1], 0.0]                 # the centre of the cell in the row before: 2 cm from the voxel
    plan4 = np.concatenate([base[:60], probe[None], base[60:]])
    assert box_cells(plan4)[1] == b4                     # (the probe lies inside the base plan's box: the rows are where they were)
    pos.append(plan4)
    veh = np.zeros(n, dtype=abi.vehicle_dtype)
    plans = np.zeros((n, 512), dtype=abi.state_dtype)
    for i, p in enumerate(pos):
        veh["plan_size"][i] = len(p)
        plans["pos"][i, :len(p)] = p
    views = (rng.random((3, FINE_CELLS)) < 0.2).astype(np.uint8)
    views[2] = 0
    views[2, (z_b * FINE[2][1] + y_b) * FINE[2][0] + x_b] = 1
    view_of = np.array([0, 1, 0, 1, 2], dtype=np.int32)
    for i in (0, 1):
        d, _ = box_cells(pos[i])
        assert d[1] * d[2] > 2 * rows_per_slab(d[0]), d  # several slabs
    par = am.params(0.05, 0.05, CAP_FINE)
    kw = dict(grid=FINE, flags=views, view_of=view_of, n_views=3)
    want = am.audit(par, veh, plans, 512, **kw)
    got = device_audit(ctx, par, veh, plans, 512, **kw)
    am.assert_equal_records(got, want, "slabs")
    assert (got["flags"][:4] == abi.FH_AUDIT_UNKNOWN).all()
    assert got["worst_unknown"][4] == 60 and got["first_unknown"][4] == 60 and got["min_unknown_d2"][4] == want["min_unknown_d2"][4] < 0.021 ** 2


# ---- 4. the closed loop ----------------------------------------------------------------------------------------------------------------------
def fleet_par(fl, stride=1, count=0):
    r = float(fl.params["rule"]["drone_radius"])
    return am.params(r, r, 2.0 * r, stride, count)


def model_of_fleet(fl, par, truth=False):
    veh = fl.vehicles()
    plans = fl._host(fl.d_plans, abi.state_dtype).reshape(fl.n, fl.max_states)
    cloud = fl.cloud.cpu().numpy()
    if truth:
        return am.audit(par, veh, plans, fl.max_states, cloud=cloud)
    origin, res, dims = fl.grid
    return am.audit(par, veh, plans, fl.max_states, grid=(origin, res, dims), flags=fl.views().reshape(fl.n_views, -1), n_views=fl.n_views,
                    cloud=cloud, point_mask=None if fl.point_mask is None else fl.point_masks())


def test_closed_loop_equals_the_model():
    """16 vehicles x 6 cycles of sense -> observe -> replan -> audit -> next_goals in the forest of tests/test_gpu_fleet_occupancy.py.  Three
    audits per cycle, each equal to the model: against what the vehicle knows at stride 3, the delta_t states the next replan cannot
    change, and against every point of the cloud.  What is counted at the end is printed as observed, not asserted."""
    from test_gpu_fleet import P, scenario
    from test_gpu_fleet_occupancy import ONE_CELL, R_SENSE, new_fleet

    B, C = 16, 6
    sc = scenario(B, C, 31)
    probe = capi.Map(0)
    probe.read(sc["cloud"], sc["cells"], P["res"], sc["center"], 0.0, P["z_max"], ONE_CELL)
    dims, origin = probe.dims()
    probe.close()
    dims, origin = [int(d) for d in dims], np.array(origin, dtype=np.float64)
    iz, iy, ix = np.meshgrid(np.arange(dims[2]), np.arange(dims[1]), np.arange(dims[0]), indexing="ij")
    centres = np.stack([(ix + 0.5) * P["res"] + origin[0], (iy + 0.5) * P["res"] + origin[1], (iz + 0.5) * P["res"] + origin[2]], axis=-1)
    start_views = np.ones((B, dims[2], dims[1], dims[0]), dtype=np.uint8)
    for i in range(B):
        start_views[i][np.linalg.norm(centres - sc["states"]["pos"][i], axis=-1) < 1.5] = 0
    fl = new_fleet(sc, B, ONE_CELL)
    near_unknown = near_known = near_truth = near_unknown_committed = cycles = 0
    try:
        fl.set_unknown_views(start_views.reshape(B, -1), origin=origin, res=P["res"], dims=dims)
        fl.set_point_views()
        for c in range(C):
            fl.sense(R_SENSE)
            fl.observe()
            fl.replan()
            view = fl.audit(stride=3)
            am.assert_equal_records(view, model_of_fleet(fl, fleet_par(fl, 3, 0)), "cycle %d, stride 3" % c)
            head = fl.audit(count=P["delta_t"])
            am.assert_equal_records(head, model_of_fleet(fl, fleet_par(fl, 1, P["delta_t"])), "cycle %d, count delta_t" % c)
            truth = fl.audit(truth=True)
            am.assert_equal_records(truth, model_of_fleet(fl, fleet_par(fl), truth=True), "cycle %d, truth" % c)
            full = fl.audit()
            am.assert_equal_records(full, model_of_fleet(fl, fleet_par(fl)), "cycle %d, every state" % c)
            size = fl.vehicles()["plan_size"]
            assert (truth["min_occupied_d2"] <= full["min_occupied_d2"]).all()
            for a, m, s in ((view, size, 3), (head, np.minimum(size, P["delta_t"]), 1), (truth, size, 1)):
                assert (a["n_tested"] == -(-m // s)).all()
                assert (((a["flags"] & abi.FH_AUDIT_UNKNOWN) != 0) == (a["first_unknown"] >= 0)).all()
                assert (((a["flags"] & abi.FH_AUDIT_OCCUPIED) != 0) == (a["first_occupied"] >= 0)).all()
            assert (truth["view"] == -1).all() and (truth["first_unknown"] == -1).all() and (view["view"] == np.arange(B)).all()
            near_unknown += int(((full["flags"] & abi.FH_AUDIT_UNKNOWN) != 0).sum())
            near_known += int(((full["flags"] & abi.FH_AUDIT_OCCUPIED) != 0).sum())
            near_truth += int(((truth["flags"] & abi.FH_AUDIT_OCCUPIED) != 0).sum())
            near_unknown_committed += int(((head["flags"] & abi.FH_AUDIT_UNKNOWN) != 0).sum())
            cycles += B
            fl.next_goals(int(sc["ticks"][c]), follow=True)
    finally:
        fl.close()
    print("closed loop, %d vehicle-cycles, drone_radius %.2f m, forest of %d points, lattice %.2f m: plans nearer than drone_radius to an unknown "
          "voxel centre %d (in their first delta_t states %d), to a point the vehicle knows %d, to any point of the cloud %d"
          % (cycles, P["drone_radius"], len(sc["cloud"]), P["res"], near_unknown, near_unknown_committed, near_known, near_truth))


# ---- 5. a measurement changes nothing -------------------------------------------------------------------------------------------------------
def test_an_audit_changes_nothing_of_the_fleet():
    from test_gpu_fleet import P, scenario
    from test_gpu_fleet_occupancy import ONE_CELL, R_SENSE, new_fleet

    B = 8
    sc = scenario(B, 2, 31)
    fl = new_fleet(sc, B, ONE_CELL)
    try:
        fl.set_unknown(sc["flags"][0].reshape(-1), sc["origin"], P["res"], sc["dims"])
        assert [name for name, _ in fl.stages()] == ["begin", "path_search", "corridors", "corridor_problems", "whole_solve", "safe_corridor",
                                                     "safe_solve", "commit"]
        fl.replan()
        shared = fl.audit()                                            # one grid for the whole fleet
        assert (shared["view"] == 0).all() and not (shared["flags"] & abi.FH_AUDIT_NO_VIEW).any()
        veh, plans = fl.vehicles(), fl._host(fl.d_plans, abi.state_dtype).reshape(B, fl.max_states)
        am.assert_equal_records(shared, am.audit(fleet_par(fl), veh, plans, fl.max_states, grid=fl.grid, flags=sc["flags"][0].reshape(1, -1),
                                                 n_views=1, shared_grid=True, cloud=sc["cloud"]), "one grid")
        fl.set_unknown_views(origin=sc["origin"], res=P["res"], dims=sc["dims"])
        fl.set_point_views()
        fl.sense(R_SENSE)
        fl.observe()
        fl.replan()

        def snapshot():
            fl.sync()
            return [t.cpu().numpy().tobytes() for t in (fl.d_vehicles, fl.d_plans, fl.view_flags, fl.point_mask, fl.cloud, fl.d_wr, fl.d_sr)]

        before, stages = snapshot(), [name for name, _ in fl.stages()]
        for kw in ({}, dict(stride=3), dict(count=P["delta_t"]), dict(truth=True), dict(r_unknown=0.1, r_occupied=0.2, cap=1.0)):
            rec = fl.audit(**kw)
            assert rec.dtype == abi.plan_audit_dtype and rec.shape == (B,)
        assert snapshot() == before
        assert [name for name, _ in fl.stages()] == stages == ["begin", "map_views", "path_search", "corridors", "corridor_problems", "whole_solve",
                                                               "safe_corridor", "safe_solve", "commit"]
    finally:
        fl.close()
