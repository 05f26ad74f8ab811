"""GPU tests of the sample clock and of every kernel that hands its samples to a caller — sample_kernel, pair_glue_kernel (clock_at on
the device), plan_append_kernel, fleet_commit_kernel and the two next-goal kernels — against tests/sample_model.py: the reference's clock
as a Python loop, the states evaluated exactly in rationals, a bound derived from the number formats, and a deque.

All inputs are synthetic results written here (nothing is solved): any (DC, dt, N) can be posed, so samples fall ON knots, plan ends fall
on the edges of the sampler's 64-state tiles, capacities cut trajectories short, and the trajectories are discontinuous on purpose — a
sample evaluated in the wrong segment is wrong in every field (tests/test_sample_model.py holds the cases to that, on the CPU).
Everything discrete is compared exactly: counts, k_safe, cursors, the segment of a sample (the bits of its jerk), moved bytes, and the
canary bytes behind what a kernel may write.  No tolerance here is a measured number."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_model as sm  # noqa: E402
from faster_amd import abi, capi  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = sm.cases()
SB = abi.state_dtype.itemsize   # 96
CANARY = 0xA5
GUARD = 10 * SB                 # canary bytes behind every output buffer
SIZED = (2, 64, 65, 128, 129, 200)
_MODEL = {}


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch  # noqa: F401  (torch before the HIP library: one HIP runtime in the process)


def model(key):
    """(problem, result, ref, bound, intervals) of CASES[key] (int) or of the sized trajectory ('sized', n), computed once."""
    if key not in _MODEL:
        if isinstance(key, int):
            pr, rs = sm.case_records(CASES[key], 100 * key)
            pr, rs = pr[0], rs[0]
        else:
            DC, dt, N = sm.sized(key[1])
            pr, rs = sm.synthetic_problem(N, DC), sm.synthetic_result(N, dt, 5000 + key[1])
        _MODEL[key] = (pr, rs) + sm.states(pr, rs)
    return _MODEL[key]


def to_dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(torch.device("cuda", 0))


def canary(nbytes):
    import torch

    return torch.full((int(nbytes),), CANARY, dtype=torch.uint8, device=torch.device("cuda", 0))


def is_canary(b):
    return bool((np.frombuffer(b, dtype=np.uint8) == CANARY).all()) if len(b) else True


def caps(size):
    return sorted({0, 1, 63, 64, 65, size - 1, size, size + 7})


def test_sample_batch_against_the_model():
    """fh_sample_batch_device and fh_sample_batch, every case, max_samples in {0, 1, 63, 64, 65, size - 1, size, size + 7}: counts exact,
    the jerk of every written sample has the model's bits (its segment, and the zeroed tail at sample size - 1 only), pos / vel / accel
    within the model's bound, every byte behind state min(size, max_samples) still the canary (device entry point; the host entry point
    returns zeros there), unsolved / n_seg = 0 / n_seg = 17 records give count 0 and an untouched slot."""
    import torch

    ctx = capi.Context(0)
    launches = []
    try:
        for ci, case in enumerate(CASES):
            pr, rs = sm.case_records(case, 100 * ci)
            size = sm.count(case.N, case.dt, case.DC)
            d_pr, d_rs = to_dev(pr), to_dev(rs)
            for ms in caps(size):
                d_st, d_cnt = canary(4 * ms * SB + GUARD), torch.full((4,), -7, dtype=torch.int32, device=d_pr.device)
                ctx.sample_batch_device(d_pr.data_ptr(), d_rs.data_ptr(), 4, ms, d_st.data_ptr(), d_cnt.data_ptr())
                launches.append((ci, ms, d_st, d_cnt, ctx.sample_batch(pr, rs, ms)))
        ctx.sync()
        launches = [(ci, ms, d_st.cpu().numpy().tobytes(), d_cnt.cpu().numpy(), host) for ci, ms, d_st, d_cnt, host in launches]
    finally:
        ctx.close()
    written = 0
    for ci, ms, raw, cnt, (h_states, h_cnt) in launches:
        _, _, ref, bound, _ = model(ci)
        size, where = len(ref), "%s max_samples %d" % (CASES[ci].name, ms)
        assert cnt.tolist() == [size, 0, 0, 0] == h_cnt.tolist(), (where, cnt, h_cnt)
        nw = min(size, ms)
        got = np.frombuffer(raw, dtype=abi.state_dtype, count=nw)
        sm.check_states(got, ref[:nw], bound[:nw], where)
        assert is_canary(raw[nw * SB:]), where            # the rest of slot 0, the three slots of the bad records, the guard
        sm.check_states(h_states[0, :nw], ref[:nw], bound[:nw], where + " (host)")
        assert not np.frombuffer(h_states.tobytes()[nw * SB:], dtype=np.uint8).any(), where
        assert h_states[0, :nw].tobytes() == got.tobytes(), where   # one kernel behind both entry points
        written += nw
    assert written > 20000


def knot_samples(ivs, closed):
    """The samples at which the model's clock enters a segment, or a clock without the running sum is in another one."""
    return [i for i in range(len(ivs)) if (i > 0 and ivs[i] != ivs[i - 1]) or ivs[i] != closed[i]]


def test_hand_off_state_is_the_clocks_sample_on_the_device():
    """fh_pair_glue_device, rule mode 0, one polytope (a box of +-1e6), shrink 0: x0 of the safe problem is sample k of the whole
    trajectory at the clock's own t and interval — fh::clock_at compiled for the device.  Per case every knot sample and its two
    neighbours, k = 0, k = size - 1 (vel = accel = 0) and 32 random k; r_frac = (k + 0.5) / size.  r_frac is an argument of the launch,
    so every (case, k) is a launch of one pair; all of them are queued on one stream and waited for once."""
    rng = np.random.default_rng(2024)
    pairs = []   # (case, k or None for an unsolved whole result)
    for ci, case in enumerate(CASES):
        _, _, ref, _, ivs = model(ci)
        size = len(ref)
        knots = knot_samples(ivs, sm.closed_form_intervals(size, case.DC, case.dt, case.N))
        ks = {0, size - 1} | {int(k) for k in rng.integers(0, size, 32)}
        for k in knots:
            ks |= {k - 1, k, k + 1}
        pairs += [(ci, k) for k in sorted(ks) if 0 <= k < size] + [(ci, None)]
    P = len(pairs)
    whole, wres = np.zeros(P, dtype=abi.problem_dtype), np.zeros(P, dtype=abi.result_dtype)
    faces = np.zeros(6 * P, dtype=abi.face_dtype)
    tmpl = np.zeros(P, dtype=abi.problem_dtype)
    for p, (ci, k) in enumerate(pairs):
        pr, rs = model(ci)[:2]
        whole[p], wres[p] = pr, rs
        if k is None:
            wres["solved"][p] = 0
        whole["n_poly"][p], whole["face_begin"][p], whole["face_off"][p, 1:] = 1, 6 * p, 6
        for f in range(6):
            faces["a"][6 * p + f, f % 3], faces["b"][6 * p + f] = (1.0 if f < 3 else -1.0), 1e6
    tmpl["n_seg"], tmpl["dc"] = 6, 0.01
    tmpl["x0"] = np.nan
    ctx = capi.Context(0)
    try:
        ctx.set_pair_rule(mode=0)
        ctx.set_pair_margin(-1.0)
        d_w, d_wr, d_f, d_s, d_sf = to_dev(whole), to_dev(wres), to_dev(faces), to_dev(tmpl), to_dev(np.zeros_like(faces))
        for p, (ci, k) in enumerate(pairs):
            size = len(model(ci)[2])
            r_frac = 0.5 if k is None else (k + 0.5) / size
            assert k is None or int(r_frac * float(size)) == k
            ctx.pair_glue_device(d_w.data_ptr() + p * abi.problem_dtype.itemsize, d_wr.data_ptr() + p * abi.result_dtype.itemsize, d_f.data_ptr(),
                                 1, r_frac, 0.0, 1, d_s.data_ptr() + p * abi.problem_dtype.itemsize, d_sf.data_ptr())
        ctx.sync()
        safe = d_s.cpu().numpy().view(abi.problem_dtype)
        sfaces = d_sf.cpu().numpy().view(abi.face_dtype)
    finally:
        ctx.close()
    on_knots = 0
    for p, (ci, k) in enumerate(pairs):
        where = "%s k %s" % (CASES[ci].name, k)
        if k is None:
            assert safe["n_seg"][p] == 0 and np.isnan(safe["x0"][p]).all(), where
            continue
        _, _, ref, bound, ivs = model(ci)
        want = np.concatenate([ref["pos"][k], ref["vel"][k], ref["accel"][k]])
        err = np.abs(safe["x0"][p] - want)
        assert (err <= bound[k, :9]).all(), (where, "segment %d" % ivs[k], safe["x0"][p], want, err, bound[k, :9])
        if k == len(ref) - 1:
            assert not safe["x0"][p, 3:].any(), where
        assert safe["n_seg"][p] == 6 and safe["n_poly"][p] == 1 and safe["face_begin"][p] == 6 * p and safe["face_off"][p, 1] == 6, where
        assert sfaces[6 * p:6 * p + 6].tobytes() == faces[6 * p:6 * p + 6].tobytes(), where   # shrink 0: the box itself
        on_knots += int(k > 0 and ivs[k] != ivs[k - 1])
    print("hand-off: %d pairs, %d of them on the first sample of a segment" % (P, on_knots))
    assert on_knots > 100


def test_append_plans_against_the_model():
    """fh_append_plans_device with synthetic whole AND safe results, mode 0, r_frac such that k_safe + 1 is in {1, 63, 64, 65, 128, size_w},
    safe trajectories of {2, 64, 65, 200} samples, max_states in {k + 1 - 3 (not below 0), k + 1, k + 2, count - 1, count, count + 5}: the plan
    is the model's (jerk bit for bit, the rest within the bound), counts and k_safe exact, canary behind min(count, max_states); a pair
    whose safe result is unsolved commits nothing.  r_frac and max_states are arguments of the launch: one pair per launch, one wait."""
    import torch

    wholes = [ci for ci, c in enumerate(CASES) if c.name.startswith("table") and sm.count(c.N, c.dt, c.DC) >= 129]
    assert len(wholes) >= 6
    pairs = []   # (whole case, k, safe size or None: unsolved safe result)
    for ci in wholes:
        size_w = len(model(ci)[2])
        for k1 in (1, 63, 64, 65, 128, size_w):
            pairs += [(ci, k1 - 1, ns) for ns in (2, 64, 65, 200)]
        pairs.append((ci, 63, None))
    P = len(pairs)
    whole, wres = np.zeros(P, dtype=abi.problem_dtype), np.zeros(P, dtype=abi.result_dtype)
    safe, sres = np.zeros(P, dtype=abi.problem_dtype), np.zeros(P, dtype=abi.result_dtype)
    launches = []   # (pair, max_states, byte offset of its slot)
    total = 0
    for p, (ci, k, ns) in enumerate(pairs):
        whole[p], wres[p] = model(ci)[:2]
        safe[p], sres[p] = model(("sized", ns if ns else 64))[:2]
        if ns is None:
            sres["solved"][p] = 0
        count = k + 1 + (ns or 0)
        for ms in sorted({max(k + 1 - 3, 0), k + 1, k + 2, max(count - 1, 0), count, count + 5}):
            launches.append((p, ms, total))
            total += ms * SB + GUARD
    L = len(launches)
    ctx = capi.Context(0)
    try:
        ctx.set_pair_rule(mode=0)
        d_w, d_wr, d_s, d_sr = to_dev(whole), to_dev(wres), to_dev(safe), to_dev(sres)
        d_pl = canary(total)
        d_cnt, d_k = (torch.full((L,), -7, dtype=torch.int32, device=d_w.device) for _ in range(2))
        ps, rs = abi.problem_dtype.itemsize, abi.result_dtype.itemsize
        for l, (p, ms, off) in enumerate(launches):
            ci, k, ns = pairs[p]
            size_w = len(model(ci)[2])
            r_frac = (k + 0.5) / size_w
            assert int(r_frac * float(size_w)) == k
            ctx.append_plans_device(d_w.data_ptr() + p * ps, d_wr.data_ptr() + p * rs, d_s.data_ptr() + p * ps, d_sr.data_ptr() + p * rs, 1, r_frac, ms,
                                    d_pl.data_ptr() + off, d_cnt.data_ptr() + 4 * l, d_k.data_ptr() + 4 * l)
        ctx.sync()
        raw, counts, ks = d_pl.cpu().numpy().tobytes(), d_cnt.cpu().numpy(), d_k.cpu().numpy()
    finally:
        ctx.close()
    cut = 0
    for l, (p, ms, off) in enumerate(launches):
        ci, k, ns = pairs[p]
        where = "%s k %d safe %s max_states %d" % (CASES[ci].name, k, ns, ms)
        slot = raw[off:off + ms * SB + GUARD]
        if ns is None:
            assert counts[l] == 0 and ks[l] == -1 and is_canary(slot), where
            continue
        _, _, wref, wbound, _ = model(ci)
        _, _, sref, sbound, _ = model(("sized", ns))
        want = sm.append_to_plan(wref[:0], wref, k, sref)
        bound = np.concatenate([wbound[:k + 1], sbound])
        assert counts[l] == len(want) == k + 1 + ns and ks[l] == k, (where, counts[l], ks[l])
        nw = min(len(want), ms)
        sm.check_states(np.frombuffer(slot, dtype=abi.state_dtype, count=nw), want[:nw], bound[:nw], where)
        assert is_canary(slot[nw * SB:]), where
        cut += int(nw < len(want))
    assert cut > L // 3


def commit_params(r_known):
    p = abi.default_fleet_params()
    p["delta_t"], p["goal_radius"] = 200, 0.3
    p["rule"]["mode"], p["rule"]["r_known"], p["rule"]["drone_radius"], p["rule"]["delta_h"], p["rule"]["delta_a"] = 1, r_known, 0.3, 1.0, 0.5
    return p


@pytest.mark.parametrize("need_safe", [True, False], ids=["whole sample 0 + safe trajectory", "whole trajectory alone"])
def test_commit_kernel_moves_a_long_kept_prefix(need_safe):
    """fh_fleet_commit_device with delta_t = 200 on synthetic results: old plans of random states, plan_size in {1, 50, 199, 200, 201, 300}
    (a kept prefix of up to 199 states: four trips of the 64-state move), plan_head in {0, 1, 63, 64, 65, 100} (source and destination
    overlapping inside a chunk, across chunks, not at all).  The committed plan is old[head : head + kept] + whole[0 .. k] + safe[:] — the
    prefix byte for byte, the samples as the model has them —, what lies behind it keeps the old bytes, plan_head is 0 and plan_size
    exact, GOAL_SEEN is decided from the model's last state, which lies on sample 1, 63, 64, 127, 128 or 199 of the last trajectory
    sampled (tile rows 1, 63, 0, 63, 0, 7).  Rule mode 1: r_known = 0 puts unknown space at sample 0 (k_safe = 0, a safe trajectory is
    needed), r_known = 1e12 nowhere (no safe trajectory: k_safe = the last whole sample)."""
    import torch

    rng = np.random.default_rng(11 + int(need_safe))
    params = commit_params(0.0 if need_safe else 1e12)
    combos = [(psz, head, n) for psz in (1, 50, 199, 200, 201, 300) for head in (0, 1, 63, 64, 65, 100) for n in SIZED]
    B, max_states = len(combos), 640
    whole, wres = np.zeros(B, dtype=abi.problem_dtype), np.zeros(B, dtype=abi.result_dtype)
    safe, sres = np.zeros(B, dtype=abi.problem_dtype), np.zeros(B, dtype=abi.result_dtype)
    veh = np.zeros(B, dtype=abi.vehicle_dtype)
    old = np.zeros((B, max_states), dtype=abi.state_dtype)
    for f in ("pos", "vel", "accel", "jerk"):
        old[f] = rng.normal(size=(B, max_states, 3))
    want, bounds, keeps = [], [], []
    for i, (psz, head, n) in enumerate(combos):
        wkey = (3 + i % 5) if need_safe else ("sized", n)     # the whole trajectory: a knot case / the sized one (it ends the plan)
        whole[i], wres[i] = model(wkey)[:2]
        safe[i], sres[i] = model(("sized", n))[:2]
        wref, wbound = model(wkey)[2:4]
        if need_safe:
            k, (sref, sbound) = 0, model(("sized", n))[2:4]
        else:
            k, sref, sbound = len(wref) - 1, wref[:0], wbound[:0]
            sres["solved"][i] = 0
        veh["plan_head"][i], veh["plan_size"][i] = head, psz
        veh["k_end_whole"][i] = max(psz - 200, 0)
        kept = psz - int(veh["k_end_whole"][i]) - 1
        keeps.append((kept, k, len(sref)))
        want.append(sm.append_to_plan(old[i, head:head + kept], wref, k, sref))
        bounds.append(np.concatenate([np.zeros((kept, 12)), wbound[:k + 1], sbound]))
        assert head + psz <= max_states and len(want[i]) <= max_states
    veh["active"], veh["status"] = 1, rng.integers(0, 2, B)
    for f in ("whole_init", "whole_final", "whole_inc", "safe_init", "safe_final", "safe_inc"):
        veh[f] = rng.integers(1, 30, B).astype(np.float64)
    veh["g_term"] = rng.uniform(-50, 50, (B, 3)) + 1e5      # far from every trajectory ...
    for i in range(0, B, 5):                                  # ... except for a fifth of the vehicles: 0.1 m from the end of the new plan
        veh["g_term"][i] = want[i][-1]["pos"] + np.array([0.1, 0.0, 0.0])
    n_points = np.full(B, 5, dtype=np.int32)
    ctx = capi.Context(0)
    try:
        d_veh, d_np = to_dev(veh), torch.from_numpy(n_points).to(torch.device("cuda", 0))
        d_plans = torch.cat([to_dev(old), canary(GUARD)])
        d_w, d_wr, d_s, d_sr = to_dev(whole), to_dev(wres), to_dev(safe), to_dev(sres)
        ctx.fleet_commit_device(params, d_veh.data_ptr(), d_plans.data_ptr(), B, max_states, d_np.data_ptr(), d_w.data_ptr(), d_wr.data_ptr(),
                                d_s.data_ptr(), d_sr.data_ptr())
        ctx.sync()
        got = d_veh.cpu().numpy().view(abi.vehicle_dtype)
        raw = d_plans.cpu().numpy().tobytes()
    finally:
        ctx.close()
    assert is_canary(raw[B * max_states * SB:])
    plans = np.frombuffer(raw, dtype=abi.state_dtype, count=B * max_states).reshape(B, max_states)
    seen = 0
    for i, (psz, head, n) in enumerate(combos):
        kept, k, ns = keeps[i]
        where = "plan_size %d plan_head %d trajectory of %d samples" % (psz, head, n)
        g = got[i]
        assert g["stage"] == abi.FH_FLEET_STAGE_COMMITTED, (where, g["stage"])
        assert (g["needed_safe"], g["k_safe"], g["n_safe"]) == (int(need_safe), k, ns), (where, g["needed_safe"], g["k_safe"], g["n_safe"])
        assert g["n_whole"] == len(model((3 + i % 5) if need_safe else ("sized", n))[2]), where
        assert g["plan_head"] == 0 and g["plan_size"] == len(want[i]) == kept + k + 1 + ns, (where, g["plan_head"], g["plan_size"])
        assert plans[i, :kept].tobytes() == want[i][:kept].tobytes(), (where, "the kept prefix")
        sm.check_states(plans[i, kept:len(want[i])], want[i][kept:], bounds[i][kept:], where)
        assert plans[i, len(want[i]):].tobytes() == old[i, len(want[i]):].tobytes(), (where, "behind the plan")
        d = np.linalg.norm(veh["g_term"][i] - want[i][-1]["pos"])
        assert d < 0.2 or d > 1e3, where   # (nowhere near the goal radius: the model's last state decides)
        assert g["status"] == (abi.FH_VEHICLE_GOAL_SEEN if d < 0.3 else veh["status"][i]), (where, g["status"], d)
        seen += int(d < 0.3)
    assert seen == len(range(0, B, 5))
    rows = {(keeps[i][2] - 1 if need_safe else keeps[i][1]) % 64 for i in range(0, B, 5)}
    assert {0, 63} <= rows, rows   # GOAL_SEEN vehicles whose last state is on the first and on the last row of the sampler's tile


def tick_values(n):
    return {max(1, t) for t in (1, 2, n - 2, n - 1, n, n + 5, 400, 2 ** 31 - 1)}


LENGTHS = (0, 1, 2, 64, 300)
TICKS = sorted(set().union(*(tick_values(n) for n in LENGTHS)))


def clamp(c, n):
    return min(max(c, 0), n - 1)


def test_next_goals_against_the_deque_model():
    """fh_next_goals_device: plans of {0, 1, 2, 64, 300} states, start cursors {0, 1, 5, len - 2, len - 1} (a cursor outside its plan
    counts as the nearest state of it), ticks in {1, 2, len - 2, len - 1, len, len + 5, 400, 2^31 - 1} (at least 1): the goal has the
    bytes of the model's state, the cursor is the model's, an empty plan gives a zero state, ok = 0 and keeps its cursor; then three
    calls in a row with mixed ticks: the model's goals and cursors after each, and no cursor ever moves backwards."""
    import torch

    rng = np.random.default_rng(5)
    entries = [(n, c) for n in LENGTHS for c in sorted({0, 1, 5, n - 2, n - 1})]
    E, max_states = len(entries), 310
    plans = np.zeros((E, max_states), dtype=abi.state_dtype)
    for f in ("pos", "vel", "accel", "jerk"):
        plans[f] = rng.normal(size=(E, max_states, 3))
    counts = np.array([n for n, _ in entries], dtype=np.int32)
    start = np.array([c for _, c in entries], dtype=np.int32)
    dev = torch.device("cuda", 0)
    ctx = capi.Context(0)
    runs = []
    try:
        d_pl = torch.cat([to_dev(plans), canary(GUARD)])
        d_cnt = torch.from_numpy(counts).to(dev)
        for seq in [(t,) for t in TICKS] + [(2, 2 ** 31 - 1, 1), (1, 400, 2 ** 31 - 1), (2 ** 31 - 1, 2 ** 31 - 1, 2), (63, 1, 236), (5, 2, 3)]:
            d_cur = torch.from_numpy(start).to(dev)
            steps = []
            for t in seq:
                d_g, d_ok = canary(E * SB + GUARD), torch.full((E,), -7, dtype=torch.int32, device=dev)
                ctx.next_goals_device(d_pl.data_ptr(), d_cnt.data_ptr(), d_cur.data_ptr(), E, max_states, t, d_g.data_ptr(), d_ok.data_ptr())
                ctx.sync()
                steps.append((t, d_g.cpu().numpy().tobytes(), d_ok.cpu().numpy(), d_cur.cpu().numpy().copy()))
            runs.append(steps)
        assert d_pl.cpu().numpy().tobytes() == plans.tobytes() + bytes([CANARY]) * GUARD
    finally:
        ctx.close()
    zero = np.zeros((), dtype=abi.state_dtype).tobytes()
    for steps in runs:
        cur = start.copy()
        for t, graw, ok, new in steps:
            assert is_canary(graw[E * SB:])
            for e, (n, _) in enumerate(entries):
                where = "plan of %d, cursor %d, ticks %d (of %s)" % (n, cur[e], t, [s[0] for s in steps])
                g = graw[e * SB:(e + 1) * SB]
                if n == 0:
                    assert g == zero and ok[e] == 0 and new[e] == cur[e], where
                    continue
                c0 = clamp(int(cur[e]), n)
                goal, popped = sm.next_goal(range(c0, n), t)
                assert g == plans[e, goal].tobytes() and ok[e] == 1, (where, "state %d of the plan expected" % goal)
                assert new[e] == c0 + popped and new[e] >= c0, (where, new[e], c0 + popped)
            cur = new


@pytest.mark.parametrize("follow", [0, 1])
def test_fleet_next_goals_against_the_deque_model(follow):
    """fh_fleet_next_goals_device, the same plans / offsets / ticks with the plan at [plan_head, plan_head + plan_size): goal, plan_head
    and plan_size are the model's; with follow = 0 fh_vehicle.state keeps its bytes, with follow = 1 it becomes the goal; no other byte
    of the vehicle changes; an empty plan gives a zero state and an untouched vehicle; three calls in a row never move plan_head back."""
    import torch

    rng = np.random.default_rng(6)
    entries = [(n, h) for n in LENGTHS for h in sorted({0, 1, 5, max(n - 2, 0), max(n - 1, 0)})]
    E, max_states = len(entries), 600
    plans = np.zeros((E, max_states), dtype=abi.state_dtype)
    for f in ("pos", "vel", "accel", "jerk"):
        plans[f] = rng.normal(size=(E, max_states, 3))
    veh = np.frombuffer(rng.integers(1, 120, E * abi.vehicle_dtype.itemsize, dtype=np.uint8).tobytes(), dtype=abi.vehicle_dtype).copy()
    veh["plan_size"], veh["plan_head"] = [n for n, _ in entries], [h for _, h in entries]
    assert all(h + n <= max_states for n, h in entries)
    dev = torch.device("cuda", 0)
    ctx = capi.Context(0)
    runs = []
    try:
        d_pl = torch.cat([to_dev(plans), canary(GUARD)])
        for seq in [(t,) for t in TICKS] + [(2, 2 ** 31 - 1, 1), (1, 400, 2 ** 31 - 1), (2 ** 31 - 1, 2 ** 31 - 1, 2), (63, 1, 236), (5, 2, 3)]:
            d_veh = torch.cat([to_dev(veh), canary(GUARD)])
            steps = []
            for t in seq:
                d_g = canary(E * SB + GUARD)
                ctx.fleet_next_goals_device(d_veh.data_ptr(), d_pl.data_ptr(), E, max_states, t, follow, d_g.data_ptr())
                ctx.sync()
                steps.append((t, d_g.cpu().numpy().tobytes(), d_veh.cpu().numpy().tobytes()))
            runs.append(steps)
        assert d_pl.cpu().numpy().tobytes() == plans.tobytes() + bytes([CANARY]) * GUARD
    finally:
        ctx.close()
    zero = np.zeros((), dtype=abi.state_dtype).tobytes()
    for steps in runs:
        cur = veh.copy()
        for t, graw, vraw in steps:
            assert is_canary(graw[E * SB:]) and is_canary(vraw[E * abi.vehicle_dtype.itemsize:])
            new = np.frombuffer(vraw, dtype=abi.vehicle_dtype, count=E)
            for e in range(E):
                n, h = int(cur["plan_size"][e]), int(cur["plan_head"][e])
                where = "plan of %d at %d, ticks %d (of %s)" % (n, h, t, [s[0] for s in steps])
                g = graw[e * SB:(e + 1) * SB]
                want = cur[e].copy()
                if n == 0:
                    assert g == zero, where
                else:
                    goal, popped = sm.next_goal(range(h, h + n), t)
                    assert g == plans[e, goal].tobytes(), (where, "state %d of the slot expected" % goal)
                    want["plan_head"], want["plan_size"] = h + popped, n - popped
                    if follow:
                        want["state"] = plans[e, goal]
                assert new[e]["plan_head"] >= h, where
                assert new[e].tobytes() == want.tobytes(), (where, new[e]["plan_head"], new[e]["plan_size"], want["plan_head"], want["plan_size"])
            cur = new.copy()
