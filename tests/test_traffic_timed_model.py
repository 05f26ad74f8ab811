"""The numpy model of time-aware traffic (tests/traffic_timed_model.py, the restatement of include/fasterhip_traffic_timed.h) on hand
cases whose answers are worked out by hand, eight wrong variants of the model, each of which changes the case that is named for it,
and the two properties the header states: the bits are monotone in `window`, and S = 1 is fasterhip_traffic.h's rule.
tests/test_gpu_traffic_timed.py runs the same cases on the device.  Coordinates are multiples of 1/64, so every difference, square and
sum below is exact.  Points are numbered k S + s behind first_point (no hull) in the tables of expected bits."""
import numpy as np
import pytest

import traffic_model as tm
import traffic_timed_model as ttm
from faster_amd import abi
from test_traffic_model import STALE, case, check, inputs

ALL, YIELD = abi.FH_TRAFFIC_ALL, abi.FH_TRAFFIC_YIELD_TO_LOWER
FAR = (100.0, 100.0, 0.0)


def crossing(window):
    """Vehicle 0 flies +x through the origin at instant 10, vehicle 1 flies +y through it at instant 30; 0.25 m per state, 41 samples,
    stride 1, range 1 m.  They are never nearer than 5 m at one instant.  Both state.pos lie: they are the origin, which is not read."""
    a = [((j - 10) * 0.25, 0, 0) for j in range(41)]
    b = [(0, (j - 30) * 0.25, 0) for j in range(41)]
    return a, b, ttm.params(41, 1, 1.0, window=window)


def hand_cases():
    c = {}
    # strictness: (3, 4, 0) is exactly 5 from the origin: clear with range 5; one lattice step nearer is set
    c["exactly_range"] = case(ttm.params(1, 1, 5.0), [[(0, 0, 0)], [(3, 4, 0)]], [(0, 0, 0), (3, 4, 0)], {(0, 1): False, (1, 0): False},
                              {0: (0, 0, 0), 1: (3, 4, 0)}, clear_rows=(0, 1))
    c["one_step_nearer"] = case(ttm.params(1, 1, 5.0), [[(0, 0, 0)], [(3, 4 - 1 / 64, 0)]], [(0, 0, 0), (3, 4 - 1 / 64, 0)],
                                {(0, 1): True, (1, 0): True, (0, 0): False, (1, 1): False})
    # the crossing: nothing at the same instant, nothing within 8 samples; a window that spans the 20 instants between the two
    # passages shows the passage: sample 30 of vehicle 1 is the origin, where vehicle 0 is at its sample 10, and the other way round
    for w in (0, 8):
        a, b, par = crossing(w)
        c["crossing_window_%d" % w] = case(par, [a, b], [(0, 0, 0), (0, 0, 0)], {(0, 41 + 30): False, (1, 10): False}, clear_rows=(0, 1))
    a, b, par = crossing(20)
    c["crossing_window_20"] = case(par, [a, b], [(0, 0, 0), (0, 0, 0)],
                                   {(0, 41 + 30): True, (1, 10): True, (0, 41 + 29): True, (0, 41 + 20): False, (0, 10): False, (1, 41 + 30): False,
                                    (0, 41 + 34): False})   # (sample 34 of vehicle 1 is (0, 1, 0): exactly 1 m from the origin, whose sample 10 its window misses)
    # the window is clipped at s = 0 and at s = S - 1 and does not wrap: S = 4, window 2.  Vehicle 0 stands at x = 0, 10, 20, 30.
    # Vehicle 1: sample 0 near 0's sample 3 and sample 3 near 0's sample 0 (three samples apart: clear).  Vehicle 2: sample 0 near 0's
    # sample 2 (set), sample 3 near 0's sample 1 (set, an s' below s)
    c["window_clipped"] = case(ttm.params(4, 1, 1.0, window=2),
                               [[(0, 0, 0), (10, 0, 0), (20, 0, 0), (30, 0, 0)], [(30.5, 0, 0), FAR, FAR, (0.5, 0, 0)],
                                [(20.5, 0, 0), FAR, FAR, (10.5, 0, 0)]], [(0, 0, 0)] * 3,
                               {(0, 4): False, (0, 5): False, (0, 6): False, (0, 7): False, (0, 8): True, (0, 9): False, (0, 10): False, (0, 11): True,
                                (1, 0): False, (1, 3): False, (2, 2): True, (2, 1): True, (2, 0): False, (2, 3): False})
    # first_instant beyond the end of every plan: all samples are the last states, (9, 0, 0) and (20, 0, 0); the first states are near
    c["first_instant_beyond_end"] = case(ttm.params(2, 1, 1.0, first_instant=100), [[(0, 0, 0), (5, 0, 0), (9, 0, 0)], [(0.5, 0, 0), (5.5, 0, 0), (20, 0, 0)]],
                                         [(0, 0, 0), (0.5, 0, 0)], {(0, 2): False, (0, 3): False, (1, 0): False, (1, 1): False},
                                         {0: (9, 0, 0), 1: (9, 0, 0), 2: (20, 0, 0), 3: (20, 0, 0)}, clear_rows=(0, 1))
    # instants 1, 3, 5: vehicle 1 has two states, so all three are its last state (1, 0, 0), inside range 2 of vehicle 0
    c["plan_end"] = case(ttm.params(3, 2, 2.0, first_instant=1), [[(0, 0, 0)] * 6, [(10, 0, 0), (1, 0, 0)]], [(0, 0, 0), (10, 0, 0)],
                         {(0, 3): True, (0, 4): True, (0, 5): True, (1, 0): True, (1, 2): True}, {3: (1, 0, 0), 4: (1, 0, 0), 5: (1, 0, 0)})
    # alone: its own samples lie on its own plan and are never shown to it
    c["alone"] = case(ttm.params(2, 1, 1.0, window=1), [[(0.5, 0, 0), (0.5, 0, 0)]], [(0.5, 0, 0)], {(0, 0): False, (0, 1): False}, clear_rows=(0,))
    # an observer with a NaN at instant 1: with window 0 that s' matches nothing, its neighbours do; with window 1 they match for it
    nan_plans = [[(0, 0, 0), (np.nan, 0, 0), (0, 0, 0)], [(0.5, 0, 0)] * 3]
    c["observer_nan_instant"] = case(ttm.params(3, 1, 1.0), nan_plans, [(0, 0, 0), (0.5, 0, 0)],
                                     {(0, 3): True, (0, 4): False, (0, 5): True, (1, 0): True, (1, 1): False, (1, 2): True}, {1: (0, 0, 0)})
    c["observer_nan_window_1"] = case(ttm.params(3, 1, 1.0, window=1), nan_plans, [(0, 0, 0), (0.5, 0, 0)],
                                      {(0, 3): True, (0, 4): True, (0, 5): True, (1, 0): True, (1, 1): False, (1, 2): True})
    # observers with an empty plan (0) and with head + size > max_states (1): all-zero rows although the words held ones, shown to
    # nobody; 2 and 3 see each other.  The positions of 0 and 1 are where 2 stands: they are not read
    cc = case(ttm.params(2, 1, 1.0, window=1), [[], [(0, 0, 0)] * 2, [(0, 0, 0)] * 2, [(0.5, 0, 0)] * 2], [(0, 0, 0)] * 4, {}, max_states=4)
    cc["v"]["plan_head"][1], cc["v"]["plan_size"][1] = 3, 2
    cc["bits"] = dict([((i, p), False) for i in (0, 1) for p in range(8)]
                      + [((2, p), p in (6, 7)) for p in range(8)] + [((3, p), p in (4, 5)) for p in range(8)])
    cc["clear_rows"], cc["points"] = (0, 1), {0: (0, 0, 0), 1: (0, 0, 0), 2: (0, 0, 0), 3: (0, 0, 0), 6: (0.5, 0, 0)}
    c["observer_without_a_plan"] = cc
    # yield to lower: vehicle i sees k < i only
    c["yield"] = case(ttm.params(1, 1, 2.0, rule=YIELD), [[(0, 0, 0)], [(0.5, 0, 0)], [(1, 0, 0)]], [(0, 0, 0), (0.5, 0, 0), (1, 0, 0)],
                      {(0, 1): False, (0, 2): False, (1, 0): True, (1, 2): False, (2, 0): True, (2, 1): True}, clear_rows=(0,))
    # stride 3, window 1 SAMPLE (three states): vehicle 0 is at x = 0, 6, 12, 18 at the instants 0, 3, 6, 9.  Sample 1 of vehicle 1 is
    # near 0's sample 2 (set); its sample 3 is near 0's sample 0 (three samples apart: clear)
    one = [FAR] * 10
    one[3], one[9] = (12.5, 0, 0), (0.5, 0, 0)
    c["stride_window_in_samples"] = case(ttm.params(4, 3, 1.0, window=1), [[(2 * j, 0, 0) for j in range(10)], one], [(0, 0, 0), FAR],
                                         {(0, 4): False, (0, 5): True, (0, 6): False, (0, 7): False, (1, 2): True, (1, 0): False, (1, 1): False, (1, 3): False},
                                         {5: (12.5, 0, 0), 7: (0.5, 0, 0), 2: (12, 0, 0)})
    return c


CASES = hand_cases()
# the case each wrong variant changes
CHANGED_BY = {"le": "exactly_range", "no_clamp": "plan_end", "self": "alone", "window_instants": "stride_window_in_samples",
              "window_one_sided": "window_clipped", "observer_unshown_matches": "observer_nan_instant",
              "ignores_first_instant": "first_instant_beyond_end", "state_pos": "crossing_window_0"}


def run(c, variant=None):
    _, cloud, mask = inputs(c)
    return ttm.traffic_timed(c["par"], c["v"], c["pl"], c["pl"].shape[1], cloud, mask, variant)


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_cases(name):
    cloud, mask = run(CASES[name])
    check(CASES[name], cloud, mask, name)


@pytest.mark.parametrize("variant", ttm.VARIANTS)
def test_every_wrong_variant_changes_its_case(variant):
    assert set(CHANGED_BY) == set(ttm.VARIANTS)
    name = CHANGED_BY[variant]
    good_cloud, good_mask = run(CASES[name])
    bad_cloud, bad_mask = run(CASES[name], variant)
    assert good_cloud.tobytes() != bad_cloud.tobytes() or good_mask.tobytes() != bad_mask.tobytes(), variant
    with pytest.raises(AssertionError):
        check(CASES[name], bad_cloud, bad_mask, name)


def test_the_crossing_in_numbers():
    """The time-matched rule with range 1 m shows nothing for the windows 0 to 8 and 7 points in each row with window 40 (every sampled
    instant): the samples of the other plan strictly inside 1 m of the origin, where the own plan passes."""
    a, b, _ = crossing(0)
    v, pl = tm.fleet([a, b], [a[0], b[0]])
    cloud, mask = np.zeros((82, 3)), np.full((2, 3), STALE, dtype=np.uint32)
    for w in range(9):
        _, m = ttm.traffic_timed(crossing(w)[2], v, pl, 41, cloud, mask)
        assert not m.any(), w
    _, m = ttm.traffic_timed(crossing(40)[2], v, pl, 41, cloud, mask)
    bits = ttm.traffic_bits(crossing(40)[2], 2, m)
    assert bits.sum(axis=1).tolist() == [7, 7]
    assert np.nonzero(bits[0])[0].tolist() == list(range(41 + 27, 41 + 34)) and np.nonzero(bits[1])[0].tolist() == list(range(7, 14))


def random_plans(rng, n, max_states=24, box=1.5, good=False):
    """n straight plans on the lattice of 1/64 in a small box, state.pos at the first plan state; unless `good`, an empty plan, a bad
    extent and a NaN among them."""
    pos = np.round(rng.uniform(0.0, box, size=(n, 3)) * 64) / 64
    sizes = rng.integers(1, max_states + 1, size=n)
    heads = [int(rng.integers(0, max_states - s + 1)) for s in sizes]
    step = np.round(rng.normal(size=(n, 3)) * 4) / 64
    v, pl = tm.fleet([p + np.arange(s)[:, None] * d for p, s, d in zip(pos, sizes, step)], pos, max_states=max_states, heads=heads)
    if not good:
        v["plan_size"][1] = 0
        v["plan_head"][2] = max_states - int(v["plan_size"][2]) + 1
        pl["pos"][3, min(int(v["plan_head"][3]) + 2, max_states - 1), 2] = np.nan
    return v, pl


@pytest.mark.parametrize("S,stride,hull,rule", [(6, 2, 0.0, ALL), (9, 1, 0.25, YIELD)])
def test_bits_are_monotone_in_the_window_and_constant_from_s_minus_1_on(S, stride, hull, rule):
    rng = np.random.default_rng(S)
    n = 9
    v, pl = random_plans(rng, n)
    rows = []
    for w in list(range(S + 2)) + [10 ** 6, 2 ** 31 - 1]:
        par = ttm.params(S, stride, 0.75, hull=hull, rule=rule, first_point=32, first_instant=1, window=w)
        n_cloud, words = tm.layout(par, n)
        cloud, mask = ttm.traffic_timed(par, v, pl, pl.shape[1], np.zeros((n_cloud, 3)), np.full((n, words), STALE, dtype=np.uint32))
        rows.append((ttm.traffic_bits(par, n, mask), cloud))
    for (lo, c0), (hi, c1) in zip(rows, rows[1:]):
        assert not (lo & ~hi).any() and c0.tobytes() == c1.tobytes()
    assert (rows[0][0] != rows[S - 1][0]).any()                                # (the window matters in this fleet)
    for bits, _ in rows[S:]:
        assert (bits == rows[S - 1][0]).all()


@pytest.mark.parametrize("hull,rule", [(0.0, ALL), (0.25, YIELD)])
def test_one_sample_at_instant_0_is_the_untimed_rule(hull, rule):
    """S = 1, first_instant = 0, good non-empty plans, state.pos bitwise the first plan state: cloud and masks of fasterhip_traffic.h's
    model, byte for byte, whatever the window."""
    rng = np.random.default_rng(7)
    n = 12
    v, pl = random_plans(rng, n, good=True)
    for w in (0, 3):
        par = ttm.params(1, 5, 0.75, hull=hull, rule=rule, first_point=64, window=w)
        n_cloud, words = tm.layout(par, n)
        cloud, mask = np.full((n_cloud, 3), 3.5), np.full((n, words), STALE, dtype=np.uint32)
        got = ttm.traffic_timed(par, v, pl, pl.shape[1], cloud, mask)
        want = tm.traffic(ttm.untimed(par), v, pl, pl.shape[1], cloud, mask)
        tm.assert_equal(*got, *want, "S = 1")
        assert ttm.traffic_bits(par, n, got[1]).any()


def test_params_helpers():
    p = abi.default_traffic_timed_params(4, 5, 6.0, hull=0.3, rule=YIELD, first_point=64, first_instant=9, window=2)
    assert (int(p["samples"]), int(p["stride"]), float(p["range"]), float(p["hull"]), int(p["rule"]), int(p["first_point"]), int(p["first_instant"]),
            int(p["window"])) == (4, 5, 6.0, 0.3, 1, 64, 9, 2)
    assert not p["reserved"].any() and abi.traffic_timed_params_dtype.itemsize == 48 and abi.FH_TRAFFIC_TIMED_MAX_SAMPLES == 512
    assert tm.layout(p, 3) == (64 + 3 * 4 * 7, 5)
    u = ttm.untimed(p)
    assert u.dtype == abi.traffic_params_dtype and all(u[k] == p[k] for k in ("range", "hull", "samples", "stride", "rule", "first_point"))
