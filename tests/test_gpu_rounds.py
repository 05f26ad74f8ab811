"""GPU tests of the priority rounds (fh_fleet_round_classes_device, fh_fleet_round_gate_device, Fleet.enable_rounds;
include/fasterhip_rounds.h): every byte of every record equals the numpy model (tests/rounds_model.py, brute force over all pairs and
instants) — at the wavefront edges of the fleet, with more lower neighbours than a row of the lists holds, for every `rounds`, with fewer
passes than a chain needs, at the stride and count edges of the plans, with positions that are not finite and bad extents, where the
cells decide what is looked at; no field depends on the cell grid, two runs give the same bytes, the stage shares the cell buffers with
separation and check; the gate against the model on poisoned buffers; and the orchestration of a fleet byte for byte: all vehicles in
the last round fly what a plain fleet flies, two rounds equal a fleet gated by hand through today's public stages, device classes equal
the model, and in the closed loop with the check the set of near pairs never grows after any round."""
import numpy as np
import pytest

from faster_amd import abi, capi

import check_model as cm
import rounds_model as rm
import separation_model as sm

pytestmark = pytest.mark.gpu
ONE_CELL = ((0.0, 0.0, 0.0), 1.0, (1, 1, 1))
FINE = ((-0.37, -0.21, -0.55), 0.25, (24, 24, 8))   # 6 m x 6 m x 2 m, an origin that is not round
GRIDS = (ONE_CELL, FINE)
GUARD = 64
OVER, UNSET, NF, BAD = abi.FH_ROUND_OVERFLOW, abi.FH_ROUND_UNSETTLED, abi.FH_ROUND_NOT_FINITE, abi.FH_ROUND_BAD_PLAN


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


def device_classes(c, par, v, pl, max_states, cells):
    """fh_fleet_round_classes_device on device copies of the two arrays, into a poisoned output with guard bytes on both sides.  A
    measurement: the two arrays and the guards must have the bytes they had."""
    import torch

    n = len(v)
    host = [np.ascontiguousarray(a).view(np.uint8).reshape(-1) for a in (v, np.asarray(pl).reshape(n, max_states))]
    d = [dev(a) if n else torch.zeros(16, dtype=torch.uint8, device="cuda:0") for a in host]
    nb = n * abi.plan_round_dtype.itemsize
    d_out = torch.full((nb + 2 * GUARD,), 0xEE, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    c.fleet_round_classes_device(par, d[0].data_ptr(), d[1].data_ptr(), n, max_states, cells, d_out.data_ptr() + GUARD)
    c.sync()
    out = d_out.cpu().numpy()
    assert (out[:GUARD] == 0xEE).all() and (out[GUARD + nb:] == 0xEE).all()
    if n:
        for a, t in zip(host, d):
            assert t.cpu().numpy().tobytes() == a.tobytes()
    return out[GUARD:GUARD + nb].view(abi.plan_round_dtype).copy()


def compare(c, par, v, pl, what, grids=GRIDS):
    """The device on every grid against the model; returns the model's records."""
    ms = pl.shape[1]
    want = rm.classes(par, v, pl, ms)
    for g in grids:
        rm.assert_equal_records(device_classes(c, par, v, pl, ms, g), want, "%s, grid %s" % (what, g[2]))
    return want


SIZES = (1, 2, 63, 64, 65, 128, 129, 130, 200)


def random_fleet(rng, n, max_states, box, speed=0.01):
    """n vehicles drifting through a box: plans with sizes around the rounds of 64 instants at random heads."""
    ps, heads = [], []
    for _ in range(n):
        s = int(rng.choice(SIZES))
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        ps.append((rng.uniform(0.0, box, size=3) * (1, 1, 0.3))[None, :] + speed * np.arange(s)[:, None] * d)
        heads.append(int(rng.integers(0, max_states - s + 1)))
    return rm.fleet(ps, max_states=max_states, heads=heads)


# ---- 1. fleet sizes at the wavefront edges, every `rounds` ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (0, 1, 2, 63, 64, 65))
def test_fleet_sizes_and_rounds(ctx, n):
    rng = np.random.default_rng(100 + n)
    v, pl = random_fleet(rng, n, 256, 3.0)
    seen = set()
    for rounds in (1, 2, 3, 64):
        want = compare(ctx, rm.params(0.8, rounds, passes=n), v, pl, "n %d, rounds %d" % (n, rounds))
        assert not want["flags"].any() and (want["round_class"] < rounds).all()
        seen |= set(want["round_class"].tolist())
        if rounds == 1:
            assert not want["round_class"].any()
    if n >= 63:
        assert len(seen) >= 3 and (want["n_lower"] > 0).sum() > n // 2   # the fleet is dense enough to show something


def test_a_dense_fleet_fills_and_flushes_the_lds_list_more_than_once(ctx):
    """200 vehicles in 1.5 m: up to 199 lower candidates per vehicle pass the boxes (the list holds 128 and is emptied above 64), and the
    numbers of lower neighbours lie on both sides of the row of 64."""
    rng = np.random.default_rng(7)
    v, pl = random_fleet(rng, 200, 256, 1.5)
    want = compare(ctx, rm.params(0.7, 64, passes=64), v, pl, "dense")
    assert want["n_lower"].max() > abi.FH_ROUNDS_LIST + 10 and ((want["n_lower"] > 30) & (want["n_lower"] <= abi.FH_ROUNDS_LIST)).any()
    assert (want["flags"] & OVER).any()


# ---- 2. the capacity of a row ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (66, 67))
def test_more_lower_neighbours_than_a_row_holds(ctx, n):
    v, pl = rm.fleet([[[0.01 * i, 0.0, 0.0]] for i in range(n)])
    want = compare(ctx, rm.params(1.0, 3, passes=2), v, pl, "clump of %d" % n)
    assert want["n_lower"].tolist() == list(range(n))                       # exact above the capacity
    assert np.nonzero(want["flags"] & OVER)[0].tolist() == list(range(65, n))
    want = compare(ctx, rm.params(1.0, 64, passes=64), v, pl, "clump of %d, 64 rounds" % n)
    assert want["round_class"][:65].tolist() == list(range(64)) + [63] and want["decided_pass"][64] == 64


def test_a_vehicle_above_an_overflowed_one_treats_it_as_decided(ctx):
    v, pl = rm.fleet([[[0.01 * i, 0.0, 0.0]] for i in range(66)] + [[[0.65 + 0.995, 0.0, 0.0]]])
    want = compare(ctx, rm.params(1.0, 3, passes=1), v, pl, "above the overflow")
    assert want["flags"][65] == OVER and (int(want["n_lower"][66]), int(want["round_class"][66]), int(want["decided_pass"][66])) == (1, 0, 1)


# ---- 3. fewer passes than the chain needs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("passes", (0, 1, 3, 5))
def test_a_chain_of_six(ctx, passes):
    v, pl = rm.fleet([[[float(i), 0.0, 0.0]] for i in range(6)])
    want = compare(ctx, rm.params(1.5, 4, passes=passes), v, pl, "chain, %d passes" % passes)
    assert np.nonzero(want["flags"] & UNSET)[0].tolist() == list(range(passes + 1, 6))
    assert want["decided_pass"].tolist() == list(range(min(passes, 5) + 1)) + [-1] * (5 - min(passes, 5))


# ---- 4. stride and count ------------------------------------------------------------------------------------------------------------------
def _line(a, b, m):
    return np.linspace(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), m)


def test_stride_and_count_edges(ctx):
    # two plans of 131 states, far apart but for one instant
    def pair(j_hit, m=131):
        a = _line((0, 0, 0), (13, 0, 0), m)
        b = _line((0, 5, 0), (13, 5, 0), m)
        b[j_hit] = a[j_hit] + (0.0, 0.1, 0.0)
        return rm.fleet([a, b], max_states=160, heads=[3, 29])

    v, pl = pair(130)   # the last tested instant: 130 = 65 * 2 = 26 * 5
    for stride, near in ((1, 1), (2, 1), (5, 1), (3, 0), (7, 0)):
        assert compare(ctx, rm.params(0.5, 4, stride=stride), v, pl, "last instant, stride %d" % stride)["n_lower"][1] == near
    v, pl = pair(65)    # an instant that the strides 2 and 64 skip
    for stride, near in ((1, 1), (5, 1), (13, 1), (65, 1), (2, 0), (64, 0)):
        assert compare(ctx, rm.params(0.5, 4, stride=stride), v, pl, "instant 65, stride %d" % stride)["n_lower"][1] == near
    for count, near in ((0, 1), (66, 1), (65, 0), (64, 0), (1, 0)):   # behind count
        assert compare(ctx, rm.params(0.5, 4, count=count), v, pl, "instant 65, count %d" % count)["n_lower"][1] == near
    # a short plan standing inside a long one's path: M is the larger size
    for m_short in (1, 2, 64):
        short = np.tile(np.array([[7.0, 0.2, 0.0]]), (m_short, 1))
        short[:-1, 0] = 30.0   # (until it stands)
        v, pl = rm.fleet([short, _line((0, 0.2, 0), (9, 0.2, 0), 91)], max_states=128, heads=[5, 17])
        want = compare(ctx, rm.params(0.5, 4), v, pl, "short plan of %d" % m_short)
        assert want["n_lower"].tolist() == [0, 1] and want["round_class"].tolist() == [0, 1]
        assert compare(ctx, rm.params(0.5, 4, count=m_short + 1), v, pl, "short plan, counted")["n_lower"][1] == 0


# ---- 5. positions that are not finite, bad extents -----------------------------------------------------------------------------------------------
def test_not_finite_and_bad_extents(ctx):
    rng = np.random.default_rng(5)
    v, pl = random_fleet(rng, 40, 256, 1.0)
    v["plan_head"][3], v["plan_size"][3] = 250, 7          # head + size > max_states
    v["plan_head"][9] = -1
    v["plan_size"][11] = -5
    v["plan_head"][12], v["plan_size"][12] = 0x7fffffff, 0x7fffffff
    v["plan_size"][14] = 0                                  # no state: no neighbours, no flag
    for i, j, val in ((5, 0, np.nan), (17, 1, np.inf), (20, 2, -np.inf), (26, 0, 1e300)):
        s = int(v["plan_size"][i])
        pl["pos"][i, int(v["plan_head"][i]) + (s - 1 if j == 1 else 0), j % 3] = val
    i = next(k for k in range(27, 40) if v["plan_size"][k] >= 63)
    pl["pos"][i, int(v["plan_head"][i]) + 31] = np.nan      # an instant that stride 2 skips and that is not the last state
    for stride, count in ((1, 0), (2, 0), (1, 1), (3, 40)):
        want = compare(ctx, rm.params(0.6, 8, stride=stride, count=count), v, pl, "stride %d, count %d" % (stride, count))
        assert (want["flags"][[3, 9, 11, 12]] == BAD).all() and not want["n_lower"][[3, 9, 11, 12, 14]].any()
        assert want["flags"][5] == NF and want["flags"][26] == 0 and want["flags"][14] == 0
        assert (want["flags"][i] == NF) == (stride == 1 and count == 0)
    assert rm.classes(rm.params(0.6, 8), v, pl, 256)["flags"][[17, 20]].tolist() == [NF, NF]
    # a fleet without a single finite position: nobody is boxed
    pl["pos"] = np.nan
    want = compare(ctx, rm.params(0.6, 8), v, pl, "all NaN")
    assert not want["n_lower"].any() and not want["round_class"].any()


# ---- 6. the cells ---------------------------------------------------------------------------------------------------------------------------
def test_cell_borders_outside_the_grid_and_one_cell(ctx):
    origin, res, dims = FINE
    ps = []
    for ix in range(0, 26, 2):        # on the borders of cells, the last ones on and beyond the upper face of the grid
        for iy in (0, 3, 24):
            ps.append([[origin[0] + ix * res, origin[1] + iy * res, origin[2] + 2 * res]])
    ps += [[[-50.0, -50.0, -50.0]], [[-50.0, -50.3, -50.0]], [[1e6, 2.0, 0.0]], [[1e6, 2.3, 0.0]], [[1e300, 0.0, 0.0]], [[1e300, 0.1, 0.0]]]
    v, pl = rm.fleet(ps)
    coarse = ((-0.37, -0.21, -0.55), 3.0, (2, 2, 1))
    want = compare(ctx, rm.params(0.55, 5, passes=40), v, pl, "borders", grids=(ONE_CELL, FINE, coarse))
    assert want["n_lower"][-5] == 1 and want["n_lower"][-3] == 1 and want["n_lower"][-1] == 1 and (want["n_lower"][:-6] > 0).any()
    want = compare(ctx, rm.params(0.0, 5), v, pl, "reach 0", grids=(ONE_CELL, FINE))
    assert not want["n_lower"].any()


# ---- 7. repetition, and the cell buffers shared with separation and check -----------------------------------------------------------------------
def test_twice_the_same_bytes_and_back_to_back_with_separation_and_check(ctx):
    import torch

    from test_gpu_check import random_cycle

    rng = np.random.default_rng(11)
    v, pl = random_fleet(rng, 130, 256, 2.0)
    par = rm.params(0.7, 6, passes=20)
    first = device_classes(ctx, par, v, pl, 256, FINE)
    rm.assert_equal_records(device_classes(ctx, par, v, pl, 256, FINE), first, "again")
    rm.assert_equal_records(first, rm.classes(par, v, pl, 256), "model")
    # one stream, no synchronisation in between: classes, separation, check, classes on a fleet of another size
    cv, cpl, cov, copl = random_cycle(rng, 70, 128, 1.5)
    d = [dev(a) for a in (v, pl, cv, cpl, cov, copl)]
    outs = [torch.full((n * dt.itemsize,), 0xEE, dtype=torch.uint8, device="cuda:0")
            for n, dt in ((130, abi.plan_round_dtype), (130, abi.plan_separation_dtype), (70, abi.plan_check_dtype), (70, abi.plan_round_dtype))]
    spar, cpar, par2 = sm.params(0.5, 1.0), cm.params(0.4), rm.params(0.5, 3, passes=8)
    torch.cuda.synchronize()
    ctx.fleet_round_classes_device(par, d[0].data_ptr(), d[1].data_ptr(), 130, 256, FINE, outs[0].data_ptr())
    ctx.fleet_separation_device(spar, d[0].data_ptr(), d[1].data_ptr(), 130, 256, ONE_CELL, outs[1].data_ptr())
    ctx.fleet_check_device(cpar, d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(), 70, 128, FINE, outs[2].data_ptr())
    ctx.fleet_round_classes_device(par2, d[2].data_ptr(), d[3].data_ptr(), 70, 128, ONE_CELL, outs[3].data_ptr())
    ctx.sync()
    rm.assert_equal_records(outs[0].cpu().numpy().view(abi.plan_round_dtype), first, "before the others")
    assert outs[1].cpu().numpy().tobytes() == sm.separation(spar, v, pl, 256).tobytes()
    cm.assert_equal_records(outs[2].cpu().numpy().view(abi.plan_check_dtype), cm.check(cpar, cv, cpl, cov, copl, 128), "check between")
    rm.assert_equal_records(outs[3].cpu().numpy().view(abi.plan_round_dtype), rm.classes(par2, cv, cpl, 128), "after the others")


# ---- 8. the gate ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 64, 300))
def test_gate_equals_the_model_and_writes_nothing_else(ctx, n):
    import torch

    rng = np.random.default_rng(n)
    v = np.frombuffer(rng.bytes(n * abi.vehicle_dtype.itemsize), dtype=abi.vehicle_dtype).copy()   # whatever the other fields hold
    v["stage"] = rng.choice([abi.FH_FLEET_STAGE_CONFLICT, abi.FH_FLEET_STAGE_COMMITTED, 0], size=n)
    rec = np.frombuffer(rng.bytes(n * 16), dtype=abi.plan_round_dtype).copy()
    rec["round_class"] = rng.integers(0, 4, size=n)
    begin = rng.choice([0, 1, 1, 7], size=n).astype(np.int32)
    d_rec, d_begin = dev(rec), dev(begin)
    for rnd in (0, 1, 3, 5, 63, abi.FH_ROUND_RETRY, abi.FH_ROUND_RESTORE):
        d_v = torch.full((v.nbytes + 2 * GUARD,), rm.POISON, dtype=torch.uint8, device="cuda:0")
        d_v[GUARD:GUARD + v.nbytes] = dev(v)
        d_act = torch.full((4 * n + 2 * GUARD,), rm.POISON, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        ctx.fleet_round_gate_device(None if rnd < 0 else d_rec.data_ptr(), rnd, d_begin.data_ptr(), n, d_v.data_ptr() + GUARD, d_act.data_ptr() + GUARD)
        ctx.sync()
        want_v, want_act = rm.gate(rec, rnd, begin, v)
        got_v, got_act = d_v.cpu().numpy(), d_act.cpu().numpy()
        for got in (got_v, got_act):
            assert (got[:GUARD] == rm.POISON).all() and (got[-GUARD:] == rm.POISON).all()
        assert got_v[GUARD:-GUARD].tobytes() == want_v.tobytes(), rnd          # `active` as the model, every other byte as it was
        assert got_act[GUARD:-GUARD].view(np.int32).tolist() == want_act.tolist(), rnd
        assert d_rec.cpu().numpy().tobytes() == rec.tobytes() and d_begin.cpu().numpy().tobytes() == begin.tobytes()
        if rnd == 5:
            assert not want_act.any()
        elif rnd == abi.FH_ROUND_RESTORE:
            assert want_act.tolist() == (begin != 0).astype(int).tolist()
    with pytest.raises(capi.FasterHipError):
        ctx.fleet_round_gate_device(d_rec.data_ptr(), 0, d_begin.data_ptr(), n, d_v.data_ptr(), d_begin.data_ptr())   # one array for both
    with pytest.raises(capi.FasterHipError):
        ctx.fleet_round_gate_device(None, 0, d_begin.data_ptr(), n, d_v.data_ptr(), d_act.data_ptr())                  # a class needs records


# ---- 9. the orchestration of a fleet ----------------------------------------------------------------------------------------------------------
B = 16
PLAIN = ["begin", "path_search", "corridors", "corridor_problems", "whole_solve", "safe_corridor", "safe_solve", "commit"]


def _snapshot(fl):
    return fl.vehicles().tobytes(), b"".join(p.tobytes() for p in fl.plans())


def test_a_fleet_that_never_calls_enable_rounds_has_todays_stage_list():
    from test_gpu_check import crossing, crossing_fleet

    fl = crossing_fleet(crossing(B, 1), B)
    try:
        assert [name for name, _ in fl.stages()] == PLAIN
        fl.enable_check()
        assert [name for name, _ in fl.stages()] == PLAIN[:-1] + ["backup", "commit", "check", "revert"]
        with pytest.raises(capi.FasterHipError):
            fl.round_records()
        fl.enable_rounds(2, retries=1)
        body = PLAIN[1:-1] + ["backup", "commit", "check", "revert"]
        assert [name for name, _ in fl.stages()] == (["begin", "round_classes"] + ["gate@0"] + [s + "@0" for s in body] + ["gate@1"]
                                                     + [s + "@1" for s in body] + ["gate@retry 0"] + [s + "@retry 0" for s in body]
                                                     + ["gate_restore"])
        assert float(fl.round_par["reach"]) == 4.0 * float(fl.params["rule"]["drone_radius"])
    finally:
        fl.close()


def test_all_vehicles_in_the_last_of_three_rounds_fly_what_a_plain_fleet_flies():
    """(a) enable_rounds(3, classes = all 2): two empty rounds leave nothing behind, and a gated vehicle replans as an ungated one."""
    from test_gpu_check import crossing, crossing_fleet

    CY = 3
    sc = crossing(B, CY)
    got = []
    for rounds in (False, True):
        fl = crossing_fleet(sc, B)
        try:
            if rounds:
                fl.enable_rounds(3, classes=np.full(B, 2, dtype=np.int32))
                names = [name for name, _ in fl.stages()]
                assert names[:2] == ["begin", "gate@0"] and names[-1] == "gate_restore" and len(names) == 1 + 3 * 8 + 1
                assert "round_classes" not in names
            cycles = []
            for cyc in range(CY):
                fl.replan()
                cycles.append(_snapshot(fl))
                fl.next_goals(int(sc["ticks"][cyc]), follow=True)
            if rounds:
                rec = fl.round_records()
                assert (rec["round_class"] == 2).all() and not rec["decided_pass"].any() and not rec["flags"].any()
            got.append(cycles)
        finally:
            fl.close()
    assert got[0] == got[1]
    assert len(set(got[0])) == CY   # (the fleet moves)


def _timed_fleet(sc):
    from test_gpu_traffic import views_fleet

    fl = views_fleet(sc)
    fl.enable_traffic(samples=64, stride=5, range=6.0, timed=True, window=2)
    fl.enable_check(stride=1, count=0)
    return fl


def test_two_rounds_equal_a_fleet_gated_by_hand_through_todays_stages():
    """(b) Fleet A: timed traffic, check, enable_rounds(2, classes = i % 2).  Fleet B never hears of rounds: the test runs its begin, then
    per round switches the vehicles of the other class off with byte edits of fh_vehicle.active and d_active and calls traffic() and
    the rest of today's stages.  After every round and after the cycle: the same vehicles, plans and check records."""
    import torch

    from test_gpu_traffic import crossing_scene

    CY = 3
    sc = crossing_scene()
    cls = np.arange(B, dtype=np.int32) % 2
    a, b = _timed_fleet(sc), _timed_fleet(sc)
    word = abi.vehicle_dtype.fields["active"][1] // 4
    try:
        a.enable_rounds(2, classes=cls)
        assert "traffic@0" in [n for n, _ in a.stages()] and "traffic@1" in [n for n, _ in a.stages()]

        def set_active(on):
            b.sync()
            t = torch.from_numpy(on.astype(np.int32)).to(b.dev)
            b.d_vehicles.view(torch.int32).reshape(B, -1)[:, word] = t
            b.d_active.copy_(t)
            torch.cuda.synchronize()

        withheld = []
        for cyc in range(CY):
            snaps = {}
            a._follow_current()
            for name, launch in a.stages():
                launch()
                if name.startswith("revert@") or name == "gate_restore":
                    snaps[name] = _snapshot(a)
            by_round = a.check_records_by_round()
            stages_b = b.stages()
            assert [n for n, _ in stages_b][0] == "begin" and "traffic" not in [n for n, _ in stages_b]
            b._follow_current()
            stages_b[0][1]()
            b.sync()
            begin = b.d_active.cpu().numpy().copy()
            for r in range(2):
                set_active((begin != 0) & (cls == r))
                b.traffic()
                for _, launch in stages_b[1:]:
                    launch()
                assert _snapshot(b) == snaps["revert@%d" % r], (cyc, r)
                cm.assert_equal_records(by_round[r], b.check_records(), "cycle %d, round %d" % (cyc, r))
                cand = (by_round[r]["flags"] & abi.FH_CHECK_CANDIDATE) != 0
                assert not (cand & (cls != r)).any()
            set_active(begin != 0)
            assert _snapshot(b) == snaps["gate_restore"], cyc
            assert (a.vehicles()["active"] == (begin != 0)).all()
            last = a.check_records()
            for i in range(B):
                assert last[i].tobytes() == by_round[cls[i] if (by_round[cls[i]]["flags"][i] & abi.FH_CHECK_CANDIDATE) else 1][i].tobytes()
            withheld.append([int(((rec["flags"] & abi.FH_CHECK_CONFLICT) != 0).sum()) for rec in by_round])
            a.next_goals(int(sc["ticks"][cyc]), follow=True)
            b.next_goals(int(sc["ticks"][cyc]), follow=True)
        print("two fixed rounds, withheld per cycle and round: %s" % withheld)
    finally:
        a.close()
        b.close()


def test_device_classes_of_a_fleet_equal_the_model_on_the_plans_read_back():
    """(c) enable_rounds(3) on the crossing scene: every cycle's round records equal the model on the vehicles and plans as they stood
    when the cycle began, and the vehicles of a round are those of its class."""
    from test_gpu_check import crossing, crossing_fleet, whole_plans

    CY = 3
    sc = crossing(B, CY)
    fl = crossing_fleet(sc, B)
    try:
        fl.enable_rounds(3, reach=2.0, passes=16)
        shown = []
        for cyc in range(CY):
            v, pl = whole_plans(fl)
            fl.replan()
            rec = fl.round_records()
            rm.assert_equal_records(rec, rm.classes(fl.round_par, v, pl, fl.max_states), "cycle %d" % cyc)
            shown.append(np.bincount(rec["round_class"], minlength=3).tolist())
            fl.next_goals(int(sc["ticks"][cyc]), follow=True)
        assert any(s[1] > 0 for s in shown)   # somebody has a neighbour: the classes are not all zero
        print("device classes, vehicles per class and cycle: %s" % shown)
    finally:
        fl.close()


def test_closed_loop_near_pairs_never_grow_after_any_round():
    """The crossing scene, 4 cycles, enable_check(stride = 1, count = 0), timed traffic, 2 rounds and 1 retry with device classes.  The
    set of near pairs (judge: Fleet.separation and tests/separation_model.py, as in tests/test_gpu_check.py) never grows after any
    round's revert nor after next_goals; every round's check records equal tests/check_model.py on the arrays read back.  FH_SEP_NEAR
    of 64 vehicle-cycles, the commits withheld per round and the arrivals are printed as observed, not asserted.  Observed on an
    MI355X: FH_SEP_NEAR 8 of 64; withheld per cycle in round 0, round 1 and the retry 2, 2, 4 / 1, 3, 4 / 1, 9, 8 /
    1, 8, 9; one vehicle no longer TRAVELING after the four cycles."""
    from test_gpu_check import near_pairs, whole_plans
    from test_gpu_fleet import P
    from test_gpu_traffic import crossing_scene

    CY = 4
    r = 2.0 * P["drone_radius"]
    sc = crossing_scene()
    fl = _timed_fleet(sc)
    c = capi.Context(0)
    near, withheld, committed = 0, [], []
    try:
        fl.enable_rounds(2, retries=1)
        assert float(fl.round_par["reach"]) == 6.0   # the traffic's range
        par = cm.params(r)
        before = near_pairs(fl, c, r)
        for cyc in range(CY):
            fl._follow_current()
            row = 0
            for name, launch in fl.stages():
                launch()
                stage = name.split("@")[0]
                if stage == "backup":
                    ov = fl._host(fl.d_backup_vehicles, abi.vehicle_dtype)
                    opl = fl._host(fl.d_backup_plans, abi.state_dtype).reshape(B, fl.max_states)
                elif stage == "commit":
                    v1, pl1 = whole_plans(fl)
                elif stage == "check":
                    rec = fl.check_records_by_round()[row]
                    cm.assert_equal_records(rec, cm.check(par, v1, pl1, ov, opl, fl.max_states), "cycle %d, %s" % (cyc, name))
                elif stage == "revert":
                    after = near_pairs(fl, c, r)
                    assert after <= before, "cycle %d, %s: the round created the near pairs %s" % (cyc, name, sorted(after - before))
                    before = after
                    row += 1
            by_round = fl.check_records_by_round()
            committed.append([int(((x["flags"] & abi.FH_CHECK_CANDIDATE) != 0).sum()) for x in by_round])
            withheld.append([int(((x["flags"] & abi.FH_CHECK_CONFLICT) != 0).sum()) for x in by_round])
            near += int(((fl.separation()["flags"] & abi.FH_SEP_NEAR) != 0).sum())
            fl.next_goals(int(sc["ticks"][cyc]), follow=True)
            after = near_pairs(fl, c, r)
            assert after <= before, "cycle %d: next_goals created the near pairs %s" % (cyc, sorted(after - before))
            before = after
        arrived = int((fl.vehicles()["status"] != abi.FH_VEHICLE_TRAVELING).sum())
        print("closed loop, 2 rounds + 1 retry, timed traffic, check r = %.2f m: FH_SEP_NEAR %d of %d; candidates per cycle and round %s, "
              "of them withheld %s; vehicles no longer TRAVELING after %d cycles: %d" % (r, near, B * CY, committed, withheld, CY, arrived))
    finally:
        fl.close()
        c.close()


def test_enable_rounds_refuses_what_it_cannot_serve():
    from test_gpu_check import crossing, crossing_fleet

    fl = crossing_fleet(crossing(B, 1), B)
    try:
        for kw in (dict(rounds=0), dict(rounds=65), dict(rounds=2, retries=1), dict(rounds=2, classes=np.full(B, 2)),
                   dict(rounds=2, classes=np.zeros(B - 1, dtype=np.int32))):
            with pytest.raises(capi.FasterHipError):
                fl.enable_rounds(**kw)
        assert fl.round_par is None and [name for name, _ in fl.stages()] == PLAIN
    finally:
        fl.close()
