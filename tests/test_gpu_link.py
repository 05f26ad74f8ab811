"""GPU tests of the radio link (fh_fleet_link_groups_device, fh_fleet_link_merge_device, Fleet.link; include/fasterhip_link.h): every
byte equals the numpy model (tests/link_model.py, brute force over all pairs) — labels and info on one cell and on a fine grid, with
more linked neighbours than a row of the lists holds, with fewer passes than a chain needs, with vehicles that do not speak; the merge
on unaligned rows with poisoned padding and poisoned traffic words, one table at a time, twice in a row; Fleet.link against the two
calls made by hand; and a fleet of eight linked vehicles with a view each against the same vehicles as one team, cycle by cycle."""
import numpy as np
import pytest

from faster_amd import abi, capi

import link_model as lm
from test_gpu_fleet import P, fleet_params, scenario

pytestmark = pytest.mark.gpu
ONE_CELL = ((0.0, 0.0, 0.0), 1.0, (1, 1, 1))
FINE = ((-0.37, -0.21, -0.55), 0.25, (24, 24, 24))   # 6 m x 6 m x 6 m, an origin that is not round
COARSE = ((-1.0, -1.0, -1.0), 2.5, (3, 4, 2))        # vehicles outside the grid are clamped into it
GRIDS = (ONE_CELL, FINE, COARSE)
GUARD = 64
POISON = 0xA5


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


def device_groups(c, par, v, view_of, n_views, cells):
    """fh_fleet_link_groups_device on device copies, into poisoned outputs with guard bytes on both sides.  A measurement: the inputs and
    the guards must have the bytes they had."""
    import torch

    n = len(v)
    d_v = dev(v) if n else torch.zeros(16, dtype=torch.uint8, device="cuda:0")
    d_vo = None if view_of is None else dev(view_of)
    nb = 4 * n_views
    d_lab = torch.full((nb + 2 * GUARD,), POISON, dtype=torch.uint8, device="cuda:0")
    d_info = torch.full((32 + 2 * GUARD,), POISON, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    c.fleet_link_groups_device(par, d_v.data_ptr(), n, None if d_vo is None else d_vo.data_ptr(), n_views, cells, d_lab.data_ptr() + GUARD,
                               d_info.data_ptr() + GUARD)
    c.sync()
    lab, info = d_lab.cpu().numpy(), d_info.cpu().numpy()
    for out, size in ((lab, nb), (info, 32)):
        assert (out[:GUARD] == POISON).all() and (out[GUARD + size:] == POISON).all()
    if n:
        assert d_v.cpu().numpy().tobytes() == np.ascontiguousarray(v).tobytes()
    if d_vo is not None:
        assert d_vo.cpu().numpy().tobytes() == np.ascontiguousarray(view_of).tobytes()
    return lab[GUARD:GUARD + nb].view(np.int32).copy(), info[GUARD:GUARD + 32].view(np.int64).copy()


def compare(c, par, v, view_of, n_views, what, grids=GRIDS):
    """The device on every grid against the model; returns the model's (labels, info)."""
    want_l, want_i = lm.groups(par, v, view_of, n_views)
    for g in grids:
        got_l, got_i = device_groups(c, par, v, view_of, n_views, g)
        assert np.array_equal(got_i, want_i), (what, g[2], got_i.tolist(), want_i.tolist())
        assert np.array_equal(got_l, want_l), (what, g[2], np.nonzero(got_l != want_l)[0][:8].tolist())
    return want_l, want_i


# ---- 1. the groups ---------------------------------------------------------------------------------------------------------------------------
def box_fleet(seed=11):
    """96 vehicles, 64 views through view_of, in a 6 m box; half of them on a lattice of 0.25 m, where pairs stand exactly at range."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0.0, 6.0, size=(96, 3))
    pos[:48] = np.round(pos[:48] * 4.0) / 4.0
    pos[0], pos[1], pos[2] = (2.0, 2.0, 2.0), (3.0, 2.0, 2.0), (2.0, 2.0, np.nextafter(3.0, 0.0))   # exactly at range of 0, and just inside
    view_of = rng.integers(0, 64, size=96).astype(np.int32)
    return pos, view_of


@pytest.mark.parametrize("passes", (1, 2, 3, 32))
def test_a_box_of_96_vehicles_and_64_views_on_every_grid(ctx, passes):
    pos, view_of = box_fleet()
    v, vo = lm.fleet(pos, view_of)
    want_l, want_i = compare(ctx, lm.params(1.0, passes), v, vo, 64, "box, %d passes" % passes)
    assert want_i[2] > 40 and 1 < want_i[1] < 64
    d = pos[:, None, :] - pos[None, :, :]
    assert ((d * d).sum(axis=2) == 1.0).sum() >= 2            # some pair stands exactly at range: strictness is exercised
    if passes == 32:
        assert want_i[0] == 0
        assert np.array_equal(want_l, lm.components(64, lm.edges(lm.linked(lm.params(1.0), v, vo, 64), lm.views_of(96, vo))))
    if passes == 1:
        assert want_i[0] > 0


def test_vehicles_that_do_not_speak(ctx):
    pos, view_of = box_fleet(12)
    view_of[[3, 40, 77]] = (-1, 64, 1 << 30)
    pos[5] = (np.nan, 1.0, 1.0)
    pos[50] = (1.0, np.inf, 1.0)
    pos[90] = (1.0, 1.0, -np.inf)
    pos[91] = (1e300, -1e300, 1e300)          # finite and far outside every grid: d2 overflows to infinity
    pos[92] = (-50.0, 2.0, 2.0)
    v, vo = lm.fleet(pos, view_of)
    compare(ctx, lm.params(1.0, 8), v, vo, 64, "silent vehicles")
    # without view_of a vehicle is its own view; the vehicles from n_views on have none
    compare(ctx, lm.params(1.0, 8), v, None, 70, "no view_of, 70 views for 96 vehicles")
    compare(ctx, lm.params(1.0, 8), v, None, 300, "no view_of, 300 views: more than one workgroup of views")


def test_no_vehicle_and_one_vehicle(ctx):
    v, _ = lm.fleet(np.zeros((0, 3)))
    want_l, want_i = compare(ctx, lm.params(1.0, 3), v, None, 5, "n = 0", grids=(ONE_CELL,))
    assert want_l.tolist() == [0, 1, 2, 3, 4] and want_i.tolist() == [0, 5, 0, 0]
    v, _ = lm.fleet([[1.0, 2.0, 3.0]])
    compare(ctx, lm.params(1.0, 1), v, None, 1, "n = 1")


def test_a_cluster_of_80_inside_one_range_is_above_the_capacity_of_a_row(ctx):
    """Every vehicle of the cluster has 79 linked neighbours, FH_LINK_LIST is 64: the hook walks the cells again.  A tail of vehicles
    hangs on the cluster in descending view order, so that the labels need the passes and the overflowed vehicles matter in each."""
    rng = np.random.default_rng(5)
    cluster = rng.uniform(0.0, 0.5, size=(80, 3))
    tail = np.array([[0.5 + 0.8 * (j + 1), 0.25, 0.25] for j in range(12)])
    pos = np.concatenate([tail[::-1], cluster])           # views 0 .. 11: the tail, its far end first
    v, _ = lm.fleet(pos)
    for passes in (1, 2, 4, 16):
        want_l, want_i = compare(ctx, lm.params(1.0, passes), v, None, 92, "cluster, %d passes" % passes)
    assert want_i[2] >= 80 * 79 // 2 and want_i[0] == 0 and want_l.tolist() == [0] * 92
    adj = lm.linked(lm.params(1.0), v, None, 92)
    assert adj.sum(axis=1).max() > 64 and (adj.sum(axis=1) > 64).sum() >= 80


@pytest.mark.parametrize("passes", (1, 2, 8))
def test_a_chain_of_40_in_descending_index_order(ctx, passes):
    pos = [[0.9 * (39 - i), 0.0, 0.0] for i in range(40)]
    v, _ = lm.fleet(pos)
    want_l, want_i = compare(ctx, lm.params(1.0, passes), v, None, 40, "chain, %d passes" % passes)
    if passes == 1:
        assert want_l.tolist() == [0, 0] + list(range(0, 38)) and want_i[0] == 39
    if passes == 2:
        assert want_i[0] > 0 and want_l.max() > 0
    if passes == 8:
        assert want_l.tolist() == [0] * 40 and want_i.tolist() == [0, 1, 39, 0]


def test_two_runs_give_the_same_bytes_and_the_stage_shares_the_cell_buffers(ctx):
    pos, view_of = box_fleet(13)
    v, vo = lm.fleet(pos, view_of)
    a = device_groups(ctx, lm.params(1.0, 4), v, vo, 64, FINE)
    b = device_groups(ctx, lm.params(2.0, 4), v, vo, 64, COARSE)
    c = device_groups(ctx, lm.params(1.0, 4), v, vo, 64, FINE)
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1]) and not np.array_equal(a[1], b[1])


# ---- 2. the merge ----------------------------------------------------------------------------------------------------------------------------
MERGE_LABELS = np.array([0, 0, 1, -1, 99, 5, 0, 7, 7, 7, 10, 3], dtype=np.int32)
# {0, 1, 6} and {7, 8, 9} are groups; 2: its label 1 is no root; 3: negative; 4: >= n_views; 5, 10: roots alone; 11: its label 3 is no root


def device_merge(c, labels, flags, stride, view_bytes, mask, shared, skew=0):
    """fh_fleet_link_merge_device on device copies with guard bytes around both tables; `skew` moves the flags off their alignment."""
    import torch

    d_lab = dev(labels)
    d_f = d_m = None
    if flags is not None:
        d_f = torch.full((len(flags) + 2 * GUARD + 16,), POISON, dtype=torch.uint8, device="cuda:0")
        d_f[GUARD + skew:GUARD + skew + len(flags)] = torch.from_numpy(flags).to("cuda:0")
    if mask is not None:
        d_m = torch.full((mask.size * 4 + 2 * GUARD,), POISON, dtype=torch.uint8, device="cuda:0")
        d_m[GUARD:GUARD + mask.size * 4] = dev(mask)
    torch.cuda.synchronize()
    words = 0 if mask is None else mask.shape[1]
    outs = []
    for _ in range(2):
        c.fleet_link_merge_device(d_lab.data_ptr(), len(labels), None if d_f is None else d_f.data_ptr() + GUARD + skew, stride, view_bytes,
                                  None if d_m is None else d_m.data_ptr() + GUARD, words, shared)
        c.sync()
        f = m = None
        if d_f is not None:
            raw = d_f.cpu().numpy()
            assert (raw[:GUARD + skew] == POISON).all() and (raw[GUARD + skew + len(flags):] == POISON).all()
            f = raw[GUARD + skew:GUARD + skew + len(flags)].copy()
        if d_m is not None:
            raw = d_m.cpu().numpy()
            assert (raw[:GUARD] == POISON).all() and (raw[GUARD + mask.size * 4:] == POISON).all()
            m = raw[GUARD:GUARD + mask.size * 4].view(np.uint32).reshape(mask.shape).copy()
        outs.append((f, m))
    assert d_lab.cpu().numpy().tobytes() == labels.tobytes()
    return outs


def merge_tables(rng, n_views, stride, view_bytes, words, shared):
    """Flags with about a third of the bytes clear and the padding poisoned, masks with the words from `shared` on poisoned per row."""
    flags = rng.integers(0, 3, size=(n_views, stride)).astype(np.uint8) * rng.integers(1, 120, size=(n_views, stride)).astype(np.uint8)
    flags[:, view_bytes:] = 0xC0 + np.arange(n_views, dtype=np.uint8)[:, None]
    mask = (rng.integers(0, 1 << 32, size=(n_views, words), dtype=np.uint64) & rng.integers(0, 1 << 32, size=(n_views, words), dtype=np.uint64)
            ).astype(np.uint32)
    mask[:, shared:] = 0xDEAD0000 + np.arange(n_views, dtype=np.uint32)[:, None]
    return flags.reshape(-1), mask


@pytest.mark.parametrize("view_bytes,stride", ((105, 105), (105, 107), (2048, 2048)))
@pytest.mark.parametrize("shared", (0, 2, 5))
def test_merge_equals_the_model_on_poisoned_tables(ctx, view_bytes, stride, shared):
    rng = np.random.default_rng(view_bytes + stride + shared)
    n_views, words = len(MERGE_LABELS), 5
    flags, mask = merge_tables(rng, n_views, stride, view_bytes, words, shared)
    want_f, want_m = lm.merge(MERGE_LABELS, flags, stride, view_bytes, mask, shared)
    assert not np.array_equal(want_f, flags) and (shared == 0) == np.array_equal(want_m, mask)
    for skew in (0, 1, 6):   # the first row at any alignment, rows of 105 and 107 bytes at every one
        first, second = device_merge(ctx, MERGE_LABELS, flags, stride, view_bytes, mask, shared, skew)
        for f, m in (first, second):   # (run twice in a row, the second call changes nothing)
            assert np.array_equal(f, want_f), (skew, np.nonzero(f != want_f)[0][:8].tolist())
            assert np.array_equal(m, want_m), (skew, np.nonzero(m != want_m))
        rows = first[0].reshape(n_views, stride)
        assert np.array_equal(rows[:, view_bytes:], flags.reshape(n_views, stride)[:, view_bytes:])   # the padding
        assert np.array_equal(first[1][:, shared:], mask[:, shared:])                                # the words from shared_words on
    # one table at a time
    (f, m), _ = device_merge(ctx, MERGE_LABELS, flags, stride, view_bytes, None, 0, 3)
    assert m is None and np.array_equal(f, want_f)
    (f, m), _ = device_merge(ctx, MERGE_LABELS, None, 0, 0, mask, shared)
    assert f is None and np.array_equal(m, want_m)


def test_merge_of_many_senders_into_one_root_and_of_no_group(ctx):
    """40 views send to view 3 (every word of the root is met by many senders); with identity labels nothing is written."""
    rng = np.random.default_rng(9)
    n_views, stride, vb, words = 41, 333, 331, 9
    labels = np.full(n_views, 3, dtype=np.int32)
    flags, mask = merge_tables(rng, n_views, stride, vb, words, 7)
    flags = np.where(rng.uniform(size=flags.shape) < 0.97, np.maximum(flags, 1), 0).astype(np.uint8)   # few zeros: most bytes survive the AND
    flags.reshape(n_views, stride)[:, vb:] = 0xEE
    want_f, want_m = lm.merge(labels, flags, stride, vb, mask, 7)
    (f, m), (f2, m2) = device_merge(ctx, labels, flags, stride, vb, mask, 7, 5)
    assert np.array_equal(f, want_f) and np.array_equal(m, want_m) and np.array_equal(f2, want_f) and np.array_equal(m2, want_m)
    assert 0 < (want_f.reshape(n_views, stride)[3, :vb] != 0).sum() < vb
    ident = np.arange(n_views, dtype=np.int32)
    (f, m), _ = device_merge(ctx, ident, flags, stride, vb, mask, 7, 5)
    assert np.array_equal(f, flags) and np.array_equal(m, mask)


# ---- 3. Fleet.link ---------------------------------------------------------------------------------------------------------------------------
def forest(B, C, seed=31):
    sc = scenario(B, C, seed)
    probe = capi.Map(0)
    probe.read(sc["cloud"], sc["cells"], P["res"], sc["center"], 0.0, P["z_max"], 0.1)
    dims, origin = probe.dims()
    probe.close()
    sc["dims"], sc["origin"] = [int(d) for d in dims], np.array(origin, dtype=np.float64)
    return sc


def start_views(sc, B):
    dims, origin = sc["dims"], sc["origin"]
    iz, iy, ix = np.meshgrid(np.arange(dims[2]), np.arange(dims[1]), np.arange(dims[0]), indexing="ij")
    centres = np.stack([(ix + 0.5) * P["res"] + origin[0], (iy + 0.5) * P["res"] + origin[1], (iz + 0.5) * P["res"] + origin[2]], axis=-1)
    views = np.ones((B, dims[2], dims[1], dims[0]), dtype=np.uint8)
    for i in range(B):
        views[i][np.linalg.norm(centres - sc["states"]["pos"][i], axis=-1) < 1.5] = 0
    return views.reshape(B, -1)


def new_fleet(sc, B):
    from faster_amd.fleet import Fleet

    fl = Fleet(B, fleet_params(), n_seg=P["N"], max_poly=P["max_poly"], dc=P["dc"], v_max=P["v_max"], a_max=P["a_max"], j_max=P["j_max"],
               decomp_radius=P["decomp_radius"], dist_max_vertexes=P["dist_max_vertexes"])
    fl.set_map(sc["cloud"], sc["cells"], P["res"], sc["center"], P["z_max"], 0.1)   # (inflation below one cell, as in the occupancy tests)
    fl.init(sc["states"], sc["goals"])
    return fl


def test_fleet_link_equals_the_two_calls_made_by_hand():
    """16 vehicles, a view each, a range that makes several groups: Fleet.link against the model, and against groups and merge called
    through the context on copies of the same tables."""
    import torch

    B = 16
    sc = forest(B, 1)
    fl = new_fleet(sc, B)
    try:
        fl.set_unknown_views(start_views(sc, B), origin=sc["origin"], res=P["res"], dims=sc["dims"])
        fl.set_point_views()
        fl.sense(3.0)
        fl.observe()
        veh = fl.vehicles()                                   # (synchronises: the copies below see what sense and observe wrote)
        before_f, before_m = fl.view_flags.clone(), fl.point_mask.clone()
        pos = veh["state"]["pos"]
        d = np.sort(np.linalg.norm(pos[:, None] - pos[None], axis=2)[np.triu_indices(B, 1)])
        rng_link = float(d[B])                                # the B shortest distances are links: groups, and vehicles alone
        fl.link(rng_link, passes=B - 1)
        labels, info = fl.link_records()
        got_f, got_m = fl.views().reshape(B, -1), fl.point_masks()
        want_l, want_i = lm.groups(lm.params(rng_link, B - 1), veh, None, B)
        assert np.array_equal(labels, want_l) and np.array_equal(info, want_i) and 1 < info[1] < B
        cells = before_f.shape[1]
        want_f, want_m = lm.merge(want_l, before_f.cpu().numpy().reshape(-1), cells, cells, before_m.cpu().numpy().view(np.uint32),
                                  before_m.shape[1])
        assert np.array_equal(got_f.reshape(-1), want_f) and np.array_equal(got_m, want_m)
        assert not np.array_equal(want_f, before_f.cpu().numpy().reshape(-1)) and not np.array_equal(want_m, before_m.cpu().numpy().view(np.uint32))
        # by hand, on copies
        fl.sync()
        d_lab, d_info = torch.zeros(B, dtype=torch.int32, device="cuda:0"), torch.zeros(4, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        fl.ctx.fleet_link_groups_device(lm.params(rng_link, B - 1), fl.d_vehicles.data_ptr(), B, None, B, fl.separation_cells(rng_link),
                                        d_lab.data_ptr(), d_info.data_ptr())
        fl.ctx.fleet_link_merge_device(d_lab.data_ptr(), B, before_f.data_ptr(), cells, cells, before_m.data_ptr(), before_m.shape[1],
                                       before_m.shape[1])
        fl.sync()
        assert np.array_equal(d_lab.cpu().numpy(), labels) and np.array_equal(d_info.cpu().numpy(), info)
        assert np.array_equal(before_f.cpu().numpy(), got_f) and np.array_equal(before_m.cpu().numpy().view(np.uint32), got_m)
    finally:
        fl.close()


def test_a_fleet_that_never_links_makes_todays_calls():
    sc = forest(4, 1)
    fl = new_fleet(sc, 4)
    try:
        fl.set_unknown_views(start_views(sc, 4), origin=sc["origin"], res=P["res"], dims=sc["dims"])
        assert [name for name, _ in fl.stages()] == ["begin", "path_search", "corridors", "corridor_problems", "whole_solve", "safe_corridor",
                                                     "safe_solve", "commit"]
        with pytest.raises(capi.FasterHipError):
            fl.link_records()
        fl.link(100.0)
        assert [name for name, _ in fl.stages()] == ["begin", "path_search", "corridors", "corridor_problems", "whole_solve", "safe_corridor",
                                                     "safe_solve", "commit"]
        assert fl.link_records()[0].tolist() == [0, 0, 0, 0]
    finally:
        fl.close()
    fl = new_fleet(sc, 4)
    try:
        with pytest.raises(capi.FasterHipError):
            fl.link(1.0)                                          # needs set_unknown_views
    finally:
        fl.close()


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------------------------
def test_eight_linked_vehicles_with_a_view_each_fly_what_one_team_flies():
    """Fleet X: 8 vehicles, a view each, a range that links everybody.  Fleet Y: the same vehicles as one team (view_of = 0).  6 cycles
    of sense -> observe -> link -> replan -> next goals in the small forest of the occupancy tests: after every cycle every view and
    mask row of X is Y's, and the vehicle records and plans are equal byte for byte (the OR of observed rows is the observation of the
    AND of the views)."""
    B, C = 8, 6
    sc = forest(B, C)
    sv = start_views(sc, B)
    X, Y = new_fleet(sc, B), new_fleet(sc, B)
    try:
        X.set_unknown_views(sv, origin=sc["origin"], res=P["res"], dims=sc["dims"])
        Y.set_unknown_views(sv.min(axis=0)[None, :], view_of=np.zeros(B, dtype=np.int32), n_views=1, origin=sc["origin"], res=P["res"],
                            dims=sc["dims"])
        X.set_point_views()
        Y.set_point_views()
        known, stages = [], []
        for c in range(C):
            for fl in (X, Y):
                fl.sense(3.0)
                fl.observe()
            X.link(1000.0)
            labels, info = X.link_records()
            assert labels.tolist() == [0] * B and info.tolist() == [0, 1, B * (B - 1) // 2, 0], c
            vx, vy, mx, my = X.views().reshape(B, -1), Y.views().reshape(1, -1), X.point_masks(), Y.point_masks()
            assert all(np.array_equal(vx[i], vy[0]) for i in range(B)), ("views", c)
            assert all(np.array_equal(mx[i], my[0]) for i in range(B)), ("masks", c)
            known.append(int(np.unpackbits(my[0].view(np.uint8)).sum()))
            for fl in (X, Y):
                fl.replan()
            assert X.vehicles().tobytes() == Y.vehicles().tobytes(), ("after replan", c)
            stages.append(X.vehicles()["stage"])
            for fl in (X, Y):
                fl.next_goals(int(sc["ticks"][c]), follow=True)
            assert X.vehicles().tobytes() == Y.vehicles().tobytes() and X.goals().tobytes() == Y.goals().tobytes(), ("after next_goals", c)
            px, py = X.plans(), Y.plans()
            assert all(a.tobytes() == b.tobytes() for a, b in zip(px, py)), ("plans", c)
        stages = np.concatenate(stages)
        print("linked fleet == team: points known per cycle %s, stages %s" % (known, np.bincount(stages)))
        assert known[-1] >= known[0] > 0 and (stages == abi.FH_FLEET_STAGE_COMMITTED).any()
    finally:
        X.close()
        Y.close()


def test_with_traffic_the_traffic_words_are_those_of_a_run_without_link():
    """The same fleet X with enable_traffic: sense -> observe -> traffic -> link -> replan -> next goals.  W is the same fleet that
    never links; every cycle it is given X's vehicles and plans and runs the traffic stage.  The traffic words of every row of X after
    link are W's, and what the traffic stage had written into X; the words below them are the OR over the group."""
    B, C = 8, 3
    sc = forest(B, C)
    sv = start_views(sc, B)
    X, W = new_fleet(sc, B), new_fleet(sc, B)
    try:
        for fl in (X, W):
            fl.set_unknown_views(sv.copy(), origin=sc["origin"], res=P["res"], dims=sc["dims"])
            fl.set_point_views()
            fl.enable_traffic(samples=4, stride=20, range=50.0)
        first = int(X.traffic_par["first_point"]) // 32
        assert 0 < first < X.point_mask.shape[1]
        seen = 0
        for c in range(C):
            X.sense(3.0)
            X.observe()
            X.traffic()
            before = X.point_masks()
            X.link(1000.0)
            after = X.point_masks()
            X.sync()
            W.d_vehicles.copy_(X.d_vehicles)
            W.d_plans.copy_(X.d_plans)
            W.torch.cuda.synchronize()
            W.traffic()
            lone = W.point_masks()
            assert np.array_equal(after[:, first:], before[:, first:]) and np.array_equal(after[:, first:], lone[:, first:]), c
            both = np.bitwise_or.reduce(before[:, :first], axis=0)
            assert all(np.array_equal(after[i, :first], both) for i in range(B)), c
            seen += int((after[:, first:] != 0).sum())
            # the rows differ in their traffic words (a vehicle does not see its own plan), so ORing them would have changed them
            if c:
                assert not all(np.array_equal(after[i, first:], after[0, first:]) for i in range(B)), c
            X.replan()
            X.next_goals(int(sc["ticks"][c]), follow=True)
        assert seen > 0
    finally:
        X.close()
        W.close()
