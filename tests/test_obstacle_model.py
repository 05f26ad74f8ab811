"""The numpy model of moving obstacles (tests/obstacle_model.py; include/fasterhip_obstacles.h) against closed forms worked out by hand
on dyadic coordinates (every range, reach and detection boundary is hit exactly), the three properties of the header (the third against
tests/traffic_timed_model.py), and planted mutants: each of obstacle_model.VARIANTS is shown to change a named hand case, so a kernel
that made that mistake would differ from the model there.  CASES, arrays() and inputs() are also what tests/test_gpu_obstacles.py runs
on the device.  No GPU."""
import numpy as np
import pytest

import obstacle_model as om
import traffic_model as tm
import traffic_timed_model as ttm
from faster_amd import abi

KEEP = 0xA5A5A5A5     # words that the stage does not own
STALE = 0xFFFFFFFF    # owned words before a call
INF, NAN = float("inf"), float("nan")


def arrays(par, n, m, words_behind=2, points_behind=3):
    """Cloud and masks before a call: the points below first_point with a pattern, owned points poisoned, the words below and behind
    the owned ones KEEP, owned words all ones."""
    first = int(par["first_point"])
    total = first + m * int(par["samples"]) * int(par["points"])
    cloud = np.full((total + points_behind, 3), 7e7)
    cloud[:first] = np.arange(3 * first).reshape(first, 3) * 0.5 - 11.0
    cloud[total:] = -3e3
    w0, w1 = first // 32, abi.point_mask_words(total)
    mask = np.full((max(n, 1), w1 + words_behind), KEEP, dtype=np.uint32)
    mask[:, w0:w1] = STALE
    return cloud, mask


def rest(pos, states=1):
    """A plan of `states` states, all at pos."""
    return [tuple(pos)] * states


def line(p, d, states):
    return [tuple(np.asarray(p, dtype=np.float64) + j * np.asarray(d, dtype=np.float64)) for j in range(states)]


def case(par, obs, plans, positions=None, tick0=0, max_states=None, heads=None, **expect):
    positions = [p[0] if len(p) else (0.0, 0.0, 0.0) for p in plans] if positions is None else positions
    v, pl = tm.fleet(plans, positions, max_states=max_states, heads=heads)
    return dict(par=par, obs=np.asarray(obs), tick0=tick0, v=v, pl=pl, **expect)


APPROACH = abi.make_obstacles([(4, 0, 0)], [(-1, 0, 0)], 0.5)   # c = 4 - tau on the x axis, a ball of 0.5


def _cases():
    C = {}
    # one vehicle at rest at the origin, one obstacle coming down the x axis: S = 8, dc = 0.5, c[s] = 4 - 0.5 s; reach = 1.5 + 0.5 = 2,
    # so |c| < 2 holds for s = 5, 6, 7 and s = 4 (c = 2 exactly) is outside
    C["approach"] = case(om.params(8, 1, 1.5, dc=0.5, first_point=32), APPROACH, [rest((0, 0, 0))], bits={0: [5, 6, 7]})
    # the clock has run two ticks: c[s] = 3 - 0.5 s, |c| < 2 for s = 3 .. 7 (s = 2: exactly 2); now = 3
    C["approach_tick0_2"] = case(om.params(8, 1, 1.5, dc=0.5, first_point=32), APPROACH, [rest((0, 0, 0))], tick0=2, bits={0: [3, 4, 5, 6, 7]})
    # seven points per sample at the obstacle's own radius: the same decisions, pps bits each
    C["approach_7"] = case(om.params(8, 1, 1.5, dc=0.5, points=7, first_point=32), APPROACH, [rest((0, 0, 0))], bits={0: [5, 6, 7]})
    # radius 0: reach = range; |c| < 1.5 for s = 6, 7 (s = 5: exactly 1.5)
    C["radius_0"] = case(om.params(8, 1, 1.5, dc=0.5, points=7, first_point=32), abi.make_obstacles([(4, 0, 0)], [(-1, 0, 0)], 0.0),
                         [rest((0, 0, 0))], bits={0: [6, 7]})
    # detection: now = 4; r_detect = 4 is exactly there (not detected: strict), 4.5 detects, 3 does not although samples 5 .. 7 are nearer
    C["detect_exact"] = case(om.params(8, 1, 1.5, dc=0.5, r_detect=4.0, first_point=32), APPROACH, [rest((0, 0, 0))], bits={0: []})
    C["detect_beyond"] = case(om.params(8, 1, 1.5, dc=0.5, r_detect=4.5, first_point=32), APPROACH, [rest((0, 0, 0))], bits={0: [5, 6, 7]})
    C["detect_now_not_sample"] = case(om.params(8, 1, 1.5, dc=0.5, r_detect=3.0, first_point=32), APPROACH, [rest((0, 0, 0))], bits={0: []})
    # detection asks state.pos, the match asks the plan: a vehicle that stands at (3.5, 0, 0) but whose plan rests at the origin
    C["detect_from_pos"] = case(om.params(8, 1, 1.5, dc=0.5, r_detect=1.0, first_point=32), APPROACH, [rest((0, 0, 0))], positions=[(3.5, 0, 0)],
                                bits={0: [5, 6, 7]})
    # a NaN in state.pos: with detection on nothing is detected, with detection off state.pos is not read
    C["pos_nan_detect_on"] = case(om.params(8, 1, 1.5, dc=0.5, r_detect=100.0, first_point=32), APPROACH, [rest((0, 0, 0))],
                                  positions=[(0, NAN, 0)], bits={0: []})
    C["pos_nan_detect_off"] = case(om.params(8, 1, 1.5, dc=0.5, first_point=32), APPROACH, [rest((0, 0, 0))], positions=[(0, NAN, 0)],
                                   bits={0: [5, 6, 7]})
    # the window: the observer flies x = 0, 10, 20, 30, an obstacle rests at x = 30.  window 1: sample s sees s' = 3 for s = 2, 3 only;
    # an index that wrapped round would give sample 0 the observer's last sample
    flier = [line((0, 0, 0), (10, 0, 0), 4)]
    resting = abi.make_obstacles([(30, 0, 0)], None, 0.25)
    C["window_1"] = case(om.params(4, 1, 0.5, dc=0.5, first_point=32, window=1), resting, flier, bits={0: [2, 3]})
    C["window_0"] = case(om.params(4, 1, 0.5, dc=0.5, first_point=32, window=0), resting, flier, bits={0: [3]})
    C["window_all"] = case(om.params(4, 1, 0.5, dc=0.5, first_point=32, window=3), resting, flier, bits={0: [0, 1, 2, 3]})
    # first_instant and stride: samples at j = 2, 5, 8; the plan (4 states) has ended at j = 5 and 8 and stands at x = 30
    C["instants"] = case(om.params(3, 3, 0.5, dc=0.5, first_point=32, first_instant=2), resting, flier, bits={0: [1, 2]})
    # records that are shown to nobody: off, NaN / inf in p0, v or radius, a negative radius; and a c that overflows from sample 1 on
    # (p0 = 1e308, v = 1.7e308 per unit: tau = 0 at s = 0, where the obstacle is at 1e308 and far from everybody; 1.85e308 is no double)
    bad = abi.make_obstacles([(1, 0, 0)] * 8 + [(1e308, 0, 0)], [(0, 0, 0)] * 8 + [(1.7e308, 0, 0)], 0.25)
    bad["flags"][0] = 0
    bad["p0"][1, 1], bad["p0"][2, 2], bad["v"][3, 0], bad["v"][4, 1], bad["radius"][5], bad["radius"][6] = NAN, INF, NAN, -INF, NAN, INF
    bad["radius"][7] = -0.25
    C["bad_records"] = case(om.params(2, 1, 2.0, dc=0.5, points=7, first_point=32), bad, [rest((0, 0, 0))], bits={0: []}, shown=[16])
    C["bad_records_and_one_good"] = case(om.params(2, 1, 2.0, dc=0.5, first_point=32), np.concatenate([bad, abi.make_obstacles([(1, 0, 0)])]),
                                         [rest((0, 0, 0))], bits={0: [18, 19]}, shown=[16, 18, 19])
    # observers that show nothing have an all-zero row: a bad extent, an empty plan; vehicle 2 beside them sees the obstacle
    v3 = case(om.params(2, 1, 2.0, dc=0.5, first_point=32), abi.make_obstacles([(1, 0, 0)]), [rest((0, 0, 0), 2)] * 3, max_states=4,
              bits={0: [], 1: [], 2: [0, 1]})
    v3["v"]["plan_head"][0], v3["v"]["plan_size"][1] = 3, 0   # head + size = 5 > max_states; an empty plan
    C["observers_without_samples"] = v3
    # a large clock: the sum tick0 + j is taken in integers and converted once.  tick0 = 2^53 + 1, dc = 2^-52, p0 = -2, v = 1: the
    # instants 2^53 + 1 + s convert (ties to even) to 2^53 + 0, 2, 4, 4, so c = 0, 2^-51, 2^-50, 2^-50, and with range 2^-51 sample 0
    # alone is nearer (sample 1 is exactly at the range).  (double)tick0 + s would put sample 1 at 0 too.
    big = abi.make_obstacles([(-2, 0, 0)], [(1, 0, 0)], 0.0)
    C["tick0_large"] = case(om.params(4, 1, 2.0 ** -51, dc=2.0 ** -52, first_point=32), big, [rest((0, 0, 0))], tick0=2 ** 53 + 1,
                            bits={0: [0]}, shown=[1, 2, 3])
    return C


CASES = _cases()


def inputs(c):
    """(layout, cloud, mask) of a case before the call."""
    n, m = len(c["v"]), len(c["obs"])
    cloud, mask = arrays(c["par"], n, m)
    return om.layout(c["par"], m), cloud, mask


def run(c, variant=None):
    _, cloud, mask = inputs(c)
    return om.obstacles(c["par"], c["obs"], c["tick0"], c["v"], c["pl"], c["pl"].shape[1], cloud, mask, variant)


def check(c, cloud, mask, what=""):
    """The expectations a case states by hand, on a result (the model's or the device's)."""
    n, m, par = len(c["v"]), len(c["obs"]), c["par"]
    S, pps, first = int(par["samples"]), int(par["points"]), int(par["first_point"])
    bits = om.obstacle_bits(par, n, m, mask)
    for i, want in c["bits"].items():
        got = sorted(set(np.nonzero(bits[i])[0] // pps))
        assert got == sorted(want), (what, i, got, want)
        assert bits[i].sum() == len(want) * pps, (what, i)
    if "shown" in c:   # the samples (o S + s) whose centre is written; every other owned point is zero
        pts = np.asarray(cloud).reshape(-1, 3)[first:first + m * S * pps].reshape(m * S, pps, 3)
        assert sorted(np.nonzero(pts.reshape(m * S, -1).any(axis=1))[0]) == sorted(c["shown"]), what


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_cases(name):
    c = CASES[name]
    _, cloud0, mask0 = inputs(c)
    cloud, mask = run(c)
    check(c, cloud, mask, name)
    first, w0 = int(c["par"]["first_point"]), int(c["par"]["first_point"]) // 32
    assert (mask[:, :w0] == KEEP).all() and (mask[:, -2:] == KEEP).all() and not (mask[:, w0:-2] == STALE).all()   # whole words, no others
    assert cloud[:first].tobytes() == cloud0[:first].tobytes() and (cloud[-3:] == -3e3).all() and not (cloud[first:-3] == 7e7).any()


def test_closed_form_points_and_hull():
    """approach_7: sample 6 is at c = 1: the centre and the six points at the obstacle's radius 0.5 in the header's order; tick0 = 2
    moves every centre by v 2 dc = -1."""
    c = CASES["approach_7"]
    cloud, _ = run(c)
    got = cloud[32 + 6 * 7:32 + 7 * 7]
    assert got.tolist() == [[1, 0, 0], [1.5, 0, 0], [0.5, 0, 0], [1, 0.5, 0], [1, -0.5, 0], [1, 0, 0.5], [1, 0, -0.5]]
    moved, _ = run(dict(c, tick0=2))
    assert (moved[32:32 + 56].reshape(8, 7, 3)[:, 0, 0] == 3 - 0.5 * np.arange(8)).all()
    show, cc, now, reach2 = om.samples(c["par"], c["obs"], 2)
    assert show.all() and now.tolist() == [[3, 0, 0]] and reach2.tolist() == [4.0]
    # the large clock: the instants are 2^53 + 1 + s, of which only the even ones are doubles; the conversion rounds to even
    t = om.taus(2 ** 53 + 1, [0, 1, 2, 3], 2.0 ** -52)
    assert (t * 2.0 ** 52 - 2.0 ** 53).tolist() == [0.0, 2.0, 4.0, 4.0]


# ---- the three properties of the header -------------------------------------------------------------------------------------------------
def random_scene(rng, n, m, states=12, box=2.0, moving=True):
    """Dyadic coordinates (1/64 lattice), velocities on 1/8, radii on 1/16; a few vehicles with flagged records."""
    pos = np.round(rng.uniform(0.0, box, size=(n, 3)) * 64) / 64
    step = np.round(rng.normal(size=(n, 3)) * 8) / 64
    sizes = rng.integers(1, states + 1, size=n)
    heads = [int(rng.integers(0, states - s + 1)) for s in sizes]
    v, pl = tm.fleet([p + np.arange(s)[:, None] * d for p, s, d in zip(pos, sizes, step)], pos, max_states=states, heads=heads)
    p0 = np.round(rng.uniform(0.0, box, size=(m, 3)) * 64) / 64
    vel = np.round(rng.normal(size=(m, 3)) * 4) / 8 if moving else None
    obs = abi.make_obstacles(p0, vel, np.round(rng.uniform(0.0, 0.5, size=m) * 16) / 16)
    return v, pl, obs


def test_bits_are_monotone_in_the_window_and_constant_from_S_minus_1():
    rng = np.random.default_rng(3)
    n, m, S = 6, 5, 7
    v, pl, obs = random_scene(rng, n, m)
    rows = []
    for w in list(range(S + 2)) + [10 ** 6, 2 ** 31 - 1]:
        par = om.params(S, 2, 0.5, dc=0.125, first_point=32, first_instant=1, window=w)
        cloud, mask = arrays(par, n, m)
        c, k = om.obstacles(par, obs, 3, v, pl, pl.shape[1], cloud, mask)
        rows.append((om.obstacle_bits(par, n, m, k), c))
    for (lo, c0), (hi, c1) in zip(rows, rows[1:]):
        assert not (lo & ~hi).any() and c0.tobytes() == c1.tobytes()
    assert (rows[0][0] != rows[S - 1][0]).any() and rows[0][0].any()
    for bits, _ in rows[S:]:
        assert (bits == rows[S - 1][0]).all()


def test_bits_are_monotone_in_r_detect():
    rng = np.random.default_rng(4)
    n, m, S = 6, 9, 5
    v, pl, obs = random_scene(rng, n, m)
    rows = []
    for r in (2.0 ** -6, 0.25, 0.5, 1.0, 2.0, 64.0):
        par = om.params(S, 2, 0.75, dc=0.125, r_detect=r, points=7, first_point=32, window=1)
        cloud, mask = arrays(par, n, m)
        _, k = om.obstacles(par, obs, 0, v, pl, pl.shape[1], cloud, mask)
        rows.append(om.obstacle_bits(par, n, m, k))
    for lo, hi in zip(rows, rows[1:]):
        assert not (lo & ~hi).any()
    assert not rows[0].any() and rows[-1].any() and any((a != b).any() for a, b in zip(rows, rows[1:]))
    par = om.params(S, 2, 0.75, dc=0.125, r_detect=0.0, points=7, first_point=32, window=1)   # off: what the largest radius gives here
    _, k = om.obstacles(par, obs, 0, v, pl, pl.shape[1], *arrays(par, n, m))
    assert (om.obstacle_bits(par, n, m, k) == rows[-1]).all()


def resting_as_vehicles(v, pl, obs):
    """The fleet with the obstacles appended as vehicles n .. n + m - 1, each with a plan of one state at p0."""
    n, m, states = len(v), len(obs), pl.shape[1]
    v2, pl2 = np.zeros(n + m, dtype=v.dtype), np.zeros((n + m, states), dtype=pl.dtype)
    v2[:n], pl2[:n] = v, pl
    pl2["pos"][n:] = 1e6
    pl2["pos"][n:, 0] = obs["p0"]
    v2["plan_size"][n:] = 1
    v2["state"]["pos"][n:] = obs["p0"]
    return v2, pl2


@pytest.mark.parametrize("window", [0, 2, 100])
def test_resting_points_equal_timed_traffic_of_appended_vehicles(window):
    """v = 0, radius = 0, r_detect = 0, points = 1, n S a multiple of 32, first_point advanced by n S: words and points equal what
    tests/traffic_timed_model.py writes for rows 0 .. n - 1."""
    rng = np.random.default_rng(5)
    n, m, S, F = 4, 7, 8, 64
    v, pl, obs = random_scene(rng, n, m, moving=False)
    obs["radius"] = 0.0
    tpar = ttm.params(S, 2, 0.75, first_point=F, first_instant=1, window=window)
    opar = om.params(S, 2, 0.75, dc=0.125, first_point=F + n * S, first_instant=1, window=window)
    total = F + (n + m) * S
    cloud = np.full((total, 3), 7e7)
    mask = np.full((n + m, abi.point_mask_words(total)), STALE, dtype=np.uint32)
    v2, pl2 = resting_as_vehicles(v, pl, obs)
    tc, tk = ttm.traffic_timed(tpar, v2, pl2, pl2.shape[1], cloud, mask)
    oc, ok = om.obstacles(opar, obs, 5, v, pl, pl.shape[1], cloud, mask[:n])
    assert oc[F + n * S:].tobytes() == tc[F + n * S:].tobytes()
    w = (F + n * S) // 32
    assert ok[:, w:].tobytes() == np.ascontiguousarray(tk[:n, w:]).tobytes() and ok[:, w:].any() and not (ok[:, w:] == STALE).all()


# ---- the audit: closed forms ----------------------------------------------------------------------------------------------------------
def audit_case(par, obs, plans, tick0=0, **kw):
    v, pl = tm.fleet(plans, [p[0] if len(p) else (0, 0, 0) for p in plans], **kw)
    return dict(par=par, obs=np.asarray(obs), tick0=tick0, v=v, pl=pl)


def _audit_cases():
    A = {}
    # the vehicle flies x = 0.5 j, the obstacle 4 - 0.5 j (dc = 0.5, v = -1): the distance is |4 - j|, zero at j = 4
    meet = [line((0, 0, 0), (0.5, 0, 0), 9)]
    A["meet_hit_1"] = dict(audit_case(abi.default_obstacle_audit_params(0.5, 0.5), abi.make_obstacles([(4, 0, 0)], [(-1, 0, 0)], 0.5), meet),
                           want=dict(flags=abi.FH_OBSTACLE_HIT, n_tested=9, first=4, first_obstacle=0, worst=4, worst_obstacle=0, n_hit=1, min_d2=0.0))
    # r + radius = 1.5: j = 3 (distance 1) hits, j = 2 (distance 2) does not
    A["meet_hit_1_5"] = dict(audit_case(abi.default_obstacle_audit_params(0.5, 0.5), abi.make_obstacles([(4, 0, 0)], [(-1, 0, 0)], 1.0), meet),
                             want=dict(flags=abi.FH_OBSTACLE_HIT, n_tested=9, first=3, first_obstacle=0, worst=4, worst_obstacle=0, n_hit=1, min_d2=0.0))
    # the clock two ticks on: the obstacle is at 3 - 0.5 j, the distance |3 - j|
    A["meet_tick0_2"] = dict(audit_case(abi.default_obstacle_audit_params(0.5, 0.5), abi.make_obstacles([(4, 0, 0)], [(-1, 0, 0)], 0.5), meet, tick0=2),
                             want=dict(flags=abi.FH_OBSTACLE_HIT, n_tested=9, first=3, first_obstacle=0, worst=3, worst_obstacle=0, n_hit=1, min_d2=0.0))
    # stride 3 tests j = 0, 3, 6: the nearest is j = 3 at distance 1, exactly r + radius: no hit
    A["meet_stride_3"] = dict(audit_case(abi.default_obstacle_audit_params(0.5, 0.5, stride=3), abi.make_obstacles([(4, 0, 0)], [(-1, 0, 0)], 0.5), meet),
                              want=dict(flags=0, n_tested=3, first=-1, first_obstacle=-1, worst=3, worst_obstacle=0, n_hit=0, min_d2=1.0))
    # count 3 tests j = 0, 1, 2: min at j = 2, distance 2
    A["meet_count_3"] = dict(audit_case(abi.default_obstacle_audit_params(0.5, 0.5, count=3), abi.make_obstacles([(4, 0, 0)], [(-1, 0, 0)], 0.5), meet),
                             want=dict(flags=0, n_tested=3, first=-1, first_obstacle=-1, worst=2, worst_obstacle=0, n_hit=0, min_d2=4.0))
    # ties: a vehicle at rest for three states between two resting obstacles at distance 1: the smallest j, then the smallest o;
    # r + radius = 1 exactly: not a hit
    twins = abi.make_obstacles([(1, 0, 0), (-1, 0, 0)], None, 0.5)
    A["ties_at_the_bound"] = dict(audit_case(abi.default_obstacle_audit_params(0.5, 0.5), twins, [rest((0, 0, 0), 3)]),
                                  want=dict(flags=0, n_tested=3, first=-1, first_obstacle=-1, worst=0, worst_obstacle=0, n_hit=0, min_d2=1.0))
    A["ties_hit"] = dict(audit_case(abi.default_obstacle_audit_params(0.75, 0.5), twins, [rest((0, 0, 0), 3)]),
                         want=dict(flags=abi.FH_OBSTACLE_HIT, n_tested=3, first=0, first_obstacle=0, worst=0, worst_obstacle=0, n_hit=2, min_d2=1.0))
    # no obstacle, an obstacle that is off, an empty plan
    A["no_obstacle"] = dict(audit_case(abi.default_obstacle_audit_params(0.5, 0.5), abi.make_obstacles(np.zeros((0, 3))), meet),
                            want=dict(flags=0, n_tested=9, first=-1, first_obstacle=-1, worst=-1, worst_obstacle=-1, n_hit=0, min_d2=INF))
    A["obstacle_off"] = dict(audit_case(abi.default_obstacle_audit_params(0.5, 0.5), abi.make_obstacles([(0, 0, 0)], on=False), meet),
                             want=dict(flags=0, n_tested=9, first=-1, first_obstacle=-1, worst=-1, worst_obstacle=-1, n_hit=0, min_d2=INF))
    A["empty_plan"] = dict(audit_case(abi.default_obstacle_audit_params(0.5, 0.5), twins, [[]], max_states=4),
                           want=dict(flags=0, n_tested=0, first=-1, first_obstacle=-1, worst=-1, worst_obstacle=-1, n_hit=0, min_d2=INF))
    # flagged records: a bad extent (alone), a tested position that is not finite (skipped, counted)
    bad = audit_case(abi.default_obstacle_audit_params(0.75, 0.5), twins, [rest((0, 0, 0), 3)], max_states=4)
    bad["v"]["plan_head"][0] = 2
    A["bad_plan"] = dict(bad, want=dict(flags=abi.FH_OBSTACLE_BAD_PLAN, n_tested=0, first=-1, first_obstacle=-1, worst=-1, worst_obstacle=-1,
                                        n_hit=0, min_d2=INF))
    nf = audit_case(abi.default_obstacle_audit_params(0.75, 0.5), twins, [rest((0, 0, 0), 3)])
    nf["pl"]["pos"][0, 0, 2] = NAN
    A["not_finite"] = dict(nf, want=dict(flags=abi.FH_OBSTACLE_NOT_FINITE | abi.FH_OBSTACLE_HIT, n_tested=3, first=1, first_obstacle=0, worst=1,
                                         worst_obstacle=0, n_hit=2, min_d2=1.0))
    return A


AUDIT_CASES = _audit_cases()


def run_audit(c, variant=None):
    return om.audit(c["par"], c["obs"], c["tick0"], c["v"], c["pl"], c["pl"].shape[1], variant)


def check_audit(c, rec, what=""):
    for k, want in c["want"].items():
        assert rec[k][0] == want, (what, k, rec[k][0], want)
    assert rec["reserved"][0] == 0 and not rec["reserved_d"][0].any(), what


@pytest.mark.parametrize("name", sorted(AUDIT_CASES))
def test_audit_hand_cases(name):
    check_audit(AUDIT_CASES[name], run_audit(AUDIT_CASES[name]), name)


# ---- planted mutants: each is shown to fail a named case ----------------------------------------------------------------------------------
MUTANTS = {   # variant -> (a case of the bits that it changes or None, a case of the audit that it changes or None)
    "le": ("approach", "ties_at_the_bound"),
    "no_radius": ("approach", "meet_hit_1_5"),
    "no_tick0": ("approach_tick0_2", "meet_tick0_2"),
    "detect_at_sample": ("detect_now_not_sample", None),
    "window_unclipped": ("window_1", None),
    "sum_first": ("approach", "meet_hit_1"),
    "ties_larger": (None, "ties_hit"),
}


def test_every_variant_is_planted():
    assert sorted(MUTANTS) == sorted(om.VARIANTS)


@pytest.mark.parametrize("variant", sorted(MUTANTS))
def test_planted_mutants_fail_their_named_case(variant):
    bits_case, audit_name = MUTANTS[variant]
    if bits_case is not None:
        c = CASES[bits_case]
        cloud, mask = run(c, variant)
        good = run(c)
        assert mask.tobytes() != good[1].tobytes() or cloud.tobytes() != good[0].tobytes(), bits_case
        with pytest.raises(AssertionError):
            check(c, cloud, mask, bits_case)
    if audit_name is not None:
        c = AUDIT_CASES[audit_name]
        assert run_audit(c, variant).tobytes() != run_audit(c).tobytes(), audit_name
        with pytest.raises(AssertionError):
            check_audit(c, run_audit(c, variant), audit_name)
    # and a variant changes nothing where its mistake cannot show: the resting, undetected-by-nobody scene of the window
    if variant in ("no_tick0", "detect_at_sample", "ties_larger"):
        c = CASES["window_1"]
        assert run(c, variant)[1].tobytes() == run(c)[1].tobytes()
