"""GPU tests of the radio link with a line of sight (fh_fleet_link_groups_los_device, Fleet.link(los=True);
include/fasterhip_link_los.h): every byte of labels and info equals the numpy model (tests/link_los_model.py, brute force over all pairs)
— on every hand case of tests/link_los_cases.py, on 96 vehicles in 24 views in a small random forest at three ranges and three numbers of
passes, on one cell and on a fine grid, with more neighbours in line of sight than a row of the lists holds, on an empty map against
fh_fleet_link_groups_device, twice in a row on one context; the two argument rules that need a map; and a fleet of eight vehicles in two
rooms that is one group without and two with los, until a ninth stands in the doorway."""
import numpy as np
import pytest

from faster_amd import capi

import link_los_cases as lc
import link_los_model as ll
import link_model as lm
import map_read_model as mr
import sense_model
from test_gpu_fleet import P, fleet_params
from test_gpu_link import GUARD, POISON, dev, device_groups

pytestmark = pytest.mark.gpu
ONE_CELL = ((0.0, 0.0, 0.0), 1.0, (1, 1, 1))
FINE = ((-2.13, -2.21, -0.05), 0.25, (18, 18, 9))    # over the whole scene, an origin that is not round
COARSE = ((-1.0, -1.0, 0.0), 1.5, (2, 3, 1))         # vehicles outside the grid are clamped into it
GRIDS = (ONE_CELL, FINE, COARSE)


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch  # noqa: F401  (torch before the HIP library: one HIP runtime in the process)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def read_map(cloud):
    """(Map, occ, origin): the scene's lattice with this cloud; the device's grid is the host model's."""
    m = capi.Map(0)
    m.read(cloud, lc.READ["cells"], lc.READ["res"], lc.READ["center"], lc.READ["z_ground"], lc.READ["z_max"], lc.READ["inflation"])
    dims, origin = m.dims()
    occ = m.occupancy()
    want, _, want_origin = mr.occupancy(cloud, **lc.READ)
    assert tuple(int(d) for d in dims) == lc.DIMS and origin.tolist() == list(lc.ORIGIN) == np.asarray(want_origin).tolist()
    assert np.array_equal(occ, want)
    return m, occ, np.asarray(origin, dtype=np.float64)


@pytest.fixture(scope="module")
def scene():
    m, occ, origin = read_map(lc.cloud())
    assert np.array_equal(occ, lc.expected_occupancy())
    yield m, occ, origin
    m.close()


@pytest.fixture(scope="module")
def forest():
    m, occ, origin = read_map(lc.forest_cloud())
    yield m, occ, origin
    m.close()


@pytest.fixture(scope="module")
def empty():
    m, occ, origin = read_map(np.zeros((0, 3)))
    assert not occ.any()
    yield m, occ, origin
    m.close()


def device_groups_los(c, vmap, par, v, view_of, n_views, cells):
    """fh_fleet_link_groups_los_device on device copies, into poisoned outputs with guard bytes on both sides.  A measurement: the inputs
    and the guards must have the bytes they had."""
    import torch

    n = len(v)
    d_v = dev(v) if n else torch.zeros(16, dtype=torch.uint8, device="cuda:0")
    d_vo = None if view_of is None else dev(view_of)
    nb = 4 * n_views
    d_lab = torch.full((nb + 2 * GUARD,), POISON, dtype=torch.uint8, device="cuda:0")
    d_info = torch.full((32 + 2 * GUARD,), POISON, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    c.fleet_link_groups_los_device(vmap, par, d_v.data_ptr(), n, None if d_vo is None else d_vo.data_ptr(), n_views, cells,
                                   d_lab.data_ptr() + GUARD, d_info.data_ptr() + GUARD)
    c.sync()
    lab, info = d_lab.cpu().numpy(), d_info.cpu().numpy()
    for out, size in ((lab, nb), (info, 32)):
        assert (out[:GUARD] == POISON).all() and (out[GUARD + size:] == POISON).all()
    if n:
        assert d_v.cpu().numpy().tobytes() == np.ascontiguousarray(v).tobytes()
    if d_vo is not None:
        assert d_vo.cpu().numpy().tobytes() == np.ascontiguousarray(view_of).tobytes()
    return lab[GUARD:GUARD + nb].view(np.int32).copy(), info[GUARD:GUARD + 32].view(np.int64).copy()


def compare(c, world, par, v, view_of, n_views, what, grids=GRIDS, want=None):
    """The device on every grid against the model; returns the model's (labels, info)."""
    vmap, occ, origin = world
    want_l, want_i = ll.groups_los(par, v, view_of, n_views, occ, origin, lc.RES) if want is None else want
    for g in grids:
        got_l, got_i = device_groups_los(c, vmap, par, v, view_of, n_views, g)
        assert np.array_equal(got_i, want_i), (what, g[2], got_i.tolist(), want_i.tolist())
        assert np.array_equal(got_l, want_l), (what, g[2], np.nonzero(got_l != want_l)[0][:8].tolist())
    return want_l, want_i


# ---- 1. the hand cases -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_hand_case(ctx, scene, name):
    par, v, vo, n_views, want_l, want_i = lc.case(name)
    got_l, got_i = compare(ctx, scene, par, v, vo, n_views, name)
    assert got_l.tolist() == want_l.tolist() and got_i.tolist() == want_i.tolist()   # (the model gives what is written next to the case)


def test_the_pair_whose_answer_depends_on_the_orientation(ctx, scene):
    """The same two positions are linked in one index order and blocked in the other (tests/test_link_los_model.py): the device casts the
    ray from the vehicle with the smaller index, whichever of the two asks."""
    _, occ, origin = scene
    p, q, _ = lc.orientation_pair(occ, origin, lc.RES, ll.blocked)
    par = lm.params(3.0, 2)
    v, _ = lm.fleet([p, q])
    want = compare(ctx, scene, par, v, None, 2, "free from the smaller index")
    assert want[0].tolist() == [0, 0] and want[1].tolist() == [0, 1, 1, 0]
    v, _ = lm.fleet([q, p])
    want = compare(ctx, scene, par, v, None, 2, "blocked from the smaller index")
    assert want[0].tolist() == [0, 1] and want[1].tolist() == [0, 2, 0, 1]


# ---- 2. random fleets --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("range_", (0.8, 1.5, 3.0))
def test_96_vehicles_in_24_views_in_a_forest_on_every_grid(ctx, forest, range_):
    pos, view_of = lc.forest_fleet()
    v, vo = lm.fleet(pos, view_of)
    _, occ, origin = forest
    adj, blk = ll.linked_los(lm.params(range_), v, vo, 24, occ, origin, lc.RES)
    assert blk.any() and adj.any()
    for passes in (1, 2, 32):
        want_l, want_i = compare(ctx, forest, lm.params(range_, passes), v, vo, 24, "forest, range %g, %d passes" % (range_, passes))
        assert want_i[2] == np.triu(adj, 1).sum() and want_i[3] == np.triu(blk, 1).sum() > 0
        plain_l, plain_i = device_groups(ctx, lm.params(range_, passes), v, vo, 24, FINE)
        assert want_i[2] + want_i[3] == plain_i[2] and plain_i[3] == 0
    assert want_i[0] == 0
    for g in np.unique(want_l):   # settled: every group inside one plain group
        assert len(set(plain_l[want_l == g].tolist())) == 1
    # the same vehicles with a view each: many groups instead of the two or three that 24 shared views leave
    want_l, want_i = compare(ctx, forest, lm.params(range_, 32), v, None, 96, "forest, range %g, a view each" % range_, grids=(ONE_CELL, FINE))
    assert want_i[1] > 3 or range_ > 1.0


def test_80_vehicles_in_two_rooms_are_above_the_capacity_of_a_row(ctx, scene):
    """Every vehicle of the left room has more than FH_LINK_LIST = 64 neighbours in line of sight: the hook walks the cells again and casts
    the rays again in every pass."""
    pos = lc.room_fleet()
    v, _ = lm.fleet(pos)
    _, occ, origin = scene
    adj, blk = ll.linked_los(lm.params(8.0), v, None, 80, occ, origin, lc.RES)
    assert (adj.sum(axis=1) > 64).sum() >= 40 and 0 < (adj.sum(axis=1) <= 64).sum() and blk.any()
    assert np.array_equal(adj | blk, ~np.eye(80, dtype=bool))   # all within range
    for passes in (1, 2, 8):
        want_l, want_i = compare(ctx, scene, lm.params(8.0, passes), v, None, 80, "rooms, %d passes" % passes, grids=(ONE_CELL, FINE))
    assert want_i[0] == 0 and want_i[2] + want_i[3] == 80 * 79 // 2


def test_an_empty_map_gives_the_bytes_of_the_plain_link(ctx, empty):
    pos, view_of = lc.forest_fleet(4)
    view_of[[3, 40]] = (-1, 24)
    pos[5] = (np.nan, 1.0, 1.0)
    pos[50] = (1.0, np.inf, 1.0)
    pos[91] = (1e300, -1e300, 1e300)   # finite and far away: d2 overflows, never in range, no ray
    v, vo = lm.fleet(pos, view_of)
    vmap = empty[0]
    for passes in (1, 32):
        par = lm.params(1.5, passes)
        for g in GRIDS:
            plain_l, plain_i = device_groups(ctx, par, v, vo, 24, g)
            los_l, los_i = device_groups_los(ctx, vmap, par, v, vo, 24, g)
            assert los_l.tobytes() == plain_l.tobytes() and los_i.tobytes() == plain_i.tobytes() and los_i[3] == 0 and los_i[2] > 0
        want_l, want_i = lm.groups(par, v, vo, 24)
        assert np.array_equal(los_l, want_l) and np.array_equal(los_i, want_i)
    # no vehicle at all: the identity
    v0, _ = lm.fleet(np.zeros((0, 3)))
    got_l, got_i = device_groups_los(ctx, vmap, lm.params(1.0, 3), v0, None, 5, ONE_CELL)
    assert got_l.tolist() == [0, 1, 2, 3, 4] and got_i.tolist() == [0, 5, 0, 0]


def test_two_calls_in_a_row_on_one_context(ctx, scene, forest):
    pos, view_of = lc.forest_fleet(5)
    v, vo = lm.fleet(pos, view_of)
    a = device_groups_los(ctx, forest[0], lm.params(1.5, 4), v, vo, 24, FINE)
    b = device_groups_los(ctx, scene[0], lm.params(3.0, 4), v, vo, 24, COARSE)
    c = device_groups_los(ctx, forest[0], lm.params(1.5, 4), v, vo, 24, FINE)
    p = device_groups(ctx, lm.params(1.5, 4), v, vo, 24, FINE)
    d = device_groups_los(ctx, forest[0], lm.params(1.5, 4), v, vo, 24, FINE)
    assert all(np.array_equal(a[k], c[k]) and np.array_equal(a[k], d[k]) for k in (0, 1)) and not np.array_equal(a[1], b[1])
    assert p[1][2] == a[1][2] + a[1][3]


def test_the_two_argument_rules_that_need_a_map(ctx, scene):
    """A map that holds no grid, then a range of more than 4096 cells of the map: FH_ERR_ARG, in that order, before anything is launched."""
    import torch

    v, _ = lm.fleet([[-1.0, 0.0, 0.5], [-0.5, 0.0, 0.5]])   # (both in the left room)
    d_v, d_lab, d_info = dev(v), torch.zeros(2, dtype=torch.int32, device="cuda:0"), torch.full((4,), 7, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    fresh = capi.Map(0)
    try:
        for par in (lm.params(1.0), lm.params(1e9)):
            with pytest.raises(capi.FasterHipError, match="no grid"):
                ctx.fleet_link_groups_los_device(fresh, par, d_v.data_ptr(), 2, None, 2, ONE_CELL, d_lab.data_ptr(), d_info.data_ptr())
        with pytest.raises(capi.FasterHipError):
            ctx.fleet_link_groups_los_device(None, lm.params(1.0), d_v.data_ptr(), 2, None, 2, ONE_CELL, d_lab.data_ptr(), d_info.data_ptr())
    finally:
        fresh.close()
    top = 4096 * lc.RES   # (a power of two times res_map: the quotient is exactly 4096)
    with pytest.raises(capi.FasterHipError, match="4096 cells"):
        ctx.fleet_link_groups_los_device(scene[0], lm.params(float(np.nextafter(top, np.inf))), d_v.data_ptr(), 2, None, 2, ONE_CELL,
                                         d_lab.data_ptr(), d_info.data_ptr())
    with pytest.raises(capi.FasterHipError):   # an earlier clause comes first: passes
        ctx.fleet_link_groups_los_device(scene[0], lm.params(1e9, 0), d_v.data_ptr(), 2, None, 2, ONE_CELL, d_lab.data_ptr(), d_info.data_ptr())
    ctx.sync()
    assert d_info.cpu().tolist() == [7, 7, 7, 7]   # nothing was written
    ctx.fleet_link_groups_los_device(scene[0], lm.params(top, 2), d_v.data_ptr(), 2, None, 2, ONE_CELL, d_lab.data_ptr(), d_info.data_ptr())
    ctx.sync()
    assert d_lab.cpu().tolist() == [0, 0] and d_info.cpu().tolist() == [0, 1, 1, 0]


# ---- 3. Fleet.link(los=True) -------------------------------------------------------------------------------------------------------------------
LEFT = [(-1.0, 0.6, 0.5), (-1.4, -0.4, 0.7), (-0.6, 0.2, 0.9), (-1.2, 1.4, 0.5)]
RIGHT = [(1.0, 0.6, 0.5), (1.4, -0.4, 0.7), (0.8, 0.2, 0.9), (1.2, 1.4, 0.5)]
DOORWAY = (0.1, 0.9, 0.5)


def room_fleet(cloud, positions):
    from faster_amd.fleet import Fleet

    B = len(positions)
    fl = Fleet(B, fleet_params(), n_seg=P["N"], max_poly=P["max_poly"], dc=P["dc"], v_max=P["v_max"], a_max=P["a_max"], j_max=P["j_max"],
               decomp_radius=P["decomp_radius"], dist_max_vertexes=P["dist_max_vertexes"])
    fl.set_map(cloud, lc.READ["cells"], lc.RES, lc.READ["center"], lc.READ["z_max"], lc.READ["inflation"])
    fl.init(np.array(positions, dtype=np.float64), np.array(positions, dtype=np.float64))
    return fl


def sensed_and_linked(cloud, positions, los):
    """One period of sense -> link on a fleet with a view per vehicle that starts all unknown: (labels, info, views after the merge) and
    what the models give for them."""
    B = len(positions)
    cells = int(np.prod(lc.DIMS))
    fl = room_fleet(cloud, positions)
    try:
        dims, origin = fl.map.dims()
        occ = fl.map.occupancy()
        assert tuple(int(d) for d in dims) == lc.DIMS and origin.tolist() == list(lc.ORIGIN)   # (z_ground = 0 gives the scene's lattice too)
        fl.set_unknown_views(np.ones((B, cells), dtype=np.uint8), origin=origin, res=lc.RES, dims=list(lc.DIMS))
        fl.sense(1.0)
        assert [name for name, _ in fl.link_stages(8.0, los=los)] == ["link_groups_los" if los else "link_groups", "link_merge"]
        fl.link(8.0, los=los)
        labels, info = fl.link_records()
        views = fl.views().reshape(B, -1)
        veh = fl.vehicles()
    finally:
        fl.close()
    want_v = np.ones((B, lc.DIMS[2], lc.DIMS[1], lc.DIMS[0]), dtype=np.uint8)
    sense_model.sense(want_v, None, veh["state"]["pos"], 1.0, origin, lc.RES, occ, origin, lc.RES)
    par = lm.params(8.0)
    want_l, want_i = ll.groups_los(par, veh, None, B, occ, origin, lc.RES) if los else lm.groups(par, veh, None, B)
    assert np.array_equal(labels, want_l) and np.array_equal(info, want_i)
    want_f, _ = lm.merge(want_l, want_v.reshape(-1), cells, cells, None, 0)
    assert np.array_equal(views.reshape(-1), want_f)
    return labels, info, views, want_v.reshape(B, -1)


def test_eight_vehicles_in_two_rooms_and_a_ninth_in_the_doorway():
    plugged = np.concatenate([lc.cloud(), np.array([lc.centre(10, iy, iz) for iy in (13, 14, 15) for iz in range(10)])])   # no door
    # a voxel that only room A senses: the one vehicle 0 stands in, 1.8 m and more from every vehicle of room B
    ix, iy, iz = (int(np.floor((LEFT[0][a] - lc.ORIGIN[a]) / lc.RES)) for a in range(3))
    cell = (iz * lc.DIMS[1] + iy) * lc.DIMS[0] + ix
    labels, info, views, sensed = sensed_and_linked(plugged, LEFT + RIGHT, los=False)
    assert labels.tolist() == [0] * 8 and info.tolist() == [0, 1, 28, 0]
    assert (sensed[:4, cell] == 0).any() and (sensed[4:, cell] == 1).all() and (views[:, cell] == 0).all()
    labels, info, views, sensed = sensed_and_linked(plugged, LEFT + RIGHT, los=True)
    assert labels.tolist() == [0, 0, 0, 0, 4, 4, 4, 4] and info.tolist() == [0, 2, 12, 16]
    assert (views[:4, cell] == 0).all() and (views[4:, cell] == 1).all()   # still unknown in every view of room B
    assert all(np.array_equal(views[i], views[0]) for i in range(4)) and all(np.array_equal(views[i], views[4]) for i in range(4, 8))
    # with the door open and a ninth vehicle in the doorway it is one group again
    labels, info, views, sensed = sensed_and_linked(lc.cloud(), LEFT + RIGHT + [DOORWAY], los=True)
    assert labels.tolist() == [0] * 9 and info[1] == 1 and info[3] > 0 and info[2] + info[3] == 36
    assert (views[:, cell] == 0).all()
    # ... and without it the door alone links whom it lets see each other
    labels, info, views, sensed = sensed_and_linked(lc.cloud(), LEFT + RIGHT, los=True)
    assert info[2] + info[3] == 28 and info[3] > 0


def test_los_needs_a_map():
    from faster_amd.fleet import Fleet

    fl = Fleet(2, fleet_params(), n_seg=P["N"], max_poly=P["max_poly"])
    try:
        fl.init(np.zeros((2, 3)), np.zeros((2, 3)))
        fl.set_unknown_views(np.ones((2, 8), dtype=np.uint8), origin=(0.0, 0.0, 0.0), res=1.0, dims=[2, 2, 2])
        with pytest.raises(capi.FasterHipError, match="set_map"):
            fl.link(1.0, los=True)
    finally:
        fl.close()
