"""The model of the tracker of moving obstacles (tests/track_model.py, include/fasterhip_track.h) on the CPU: closed forms on dyadic
coordinates (a constant velocity comes back bit for bit from 2 .. 8 sightings, extrapolation and the growing radius, the ring's wrap,
min_obs, the gate, max_age to the tick, a stale tick), the line of sight in the walled scene of tests/link_los_cases.py, two properties,
and every wrong variant of the model failing the case named for it.  tests/test_gpu_track.py compares the device with this model on the
same cases in every byte."""
import numpy as np
import pytest

from faster_amd import abi

import track_cases as tc
import track_model as tmod

SEEN, LOST, RESET, STALE, BAD = (abi.FH_TRACK_SEEN, abi.FH_TRACK_LOST, abi.FH_TRACK_RESET, abi.FH_TRACK_STALE, abi.FH_TRACK_BAD_FIT)
H = abi.FH_TRACK_HISTORY


def play(name, variant=None):
    return tc.play(tmod, tc.CASES[name], variant)


def on(est):
    return bool(est["flags"] & abi.FH_OBSTACLE_ON)


def assert_estimate(est, tick, radius=tc.RADIUS):
    """The record is on and says, bit for bit, where the flight of tc.P0, tc.V is at `tick`, and its velocity."""
    assert on(est) and est["p0"].tolist() == tc.where(tick) and est["v"].tolist() == list(tc.V) and float(est["radius"]) == radius
    assert int(est["reserved"]) == 0


@pytest.mark.parametrize("k", range(2, 9))
def test_a_constant_velocity_comes_back_bit_for_bit(k):
    outs = play("constant_velocity_%d" % k)
    for step, (tr, est, seer, info) in enumerate(outs):
        assert int(tr["count"][0]) == step + 1 and int(tr["head"][0]) == 0 and int(tr["flags"][0]) == SEEN and seer.tolist() == [0]
        assert tr["tick"][0].tolist() == list(range(step + 1)) + [0] * (H - step - 1)
        assert tr["pos"][0][:step + 1].tolist() == [tc.where(t) for t in range(step + 1)] and not tr["pos"][0][step + 1:].any()
        assert float(tr["radius"][0]) == tc.RADIUS and not tr["reserved"].any()
        if step + 1 >= k:
            assert_estimate(est[0], step)
            assert info.tolist() == [1, 1, 0, 0]
        else:
            assert est.tobytes() == bytes(64) and info.tolist() == [1, 0, 0, 0]


def test_uneven_ticks_and_a_fit_window():
    ticks = [0, 1, 4, 6, 7, 12]
    for step, (tr, est, _, _) in enumerate(play("uneven_ticks")):
        if step >= 1:
            assert_estimate(est[0], ticks[step])
    for step, (tr, est, _, _) in enumerate(play("fit_window_of_three")):
        assert int(tr["count"][0]) == step + 1
        if step >= 1:
            assert_estimate(est[0], step)


def test_extrapolation_and_the_growing_radius_while_unseen():
    outs = play("extrapolation_and_grow")
    for (tr, est, seer, info), tick in zip(outs[3:], (5, 9)):
        assert seer.tolist() == [-1] and int(tr["flags"][0]) == 0 and int(tr["count"][0]) == 3 and info.tolist() == [0, 1, 0, 0]
        assert tr.tobytes()[:-48] == outs[2][0].tobytes()[:-48]                      # (the sightings stay; the flags are this call's)
        assert_estimate(est[0], tick, tc.RADIUS + 0.5 * ((tick - 2) * tc.DC))


def test_the_ring_wraps_at_the_ninth_sighting():
    outs = play("ring_wrap")
    tr8, tr9, tr10 = outs[7][0][0], outs[8][0][0], outs[9][0][0]
    assert (int(tr8["count"]), int(tr8["head"])) == (8, 0) and tr8["tick"].tolist() == list(range(8))
    assert (int(tr9["count"]), int(tr9["head"])) == (8, 1) and tr9["tick"].tolist() == [8, 1, 2, 3, 4, 5, 6, 7]
    assert (int(tr10["count"]), int(tr10["head"])) == (8, 2) and tr10["tick"].tolist() == [8, 9, 2, 3, 4, 5, 6, 7]
    assert tr9["pos"][0].tolist() == tc.where(8) and tr9["pos"][1].tolist() == tc.where(1)
    for step in (8, 9):
        assert_estimate(outs[step][1][0], step)


def test_min_obs_and_a_fit_of_one():
    outs = play("min_obs_three")
    assert [on(o[1][0]) for o in outs] == [False, False, True, True] and [int(o[3][1]) for o in outs] == [0, 0, 1, 1]
    assert all(int(o[0]["flags"][0]) == SEEN for o in outs)                         # (too few sightings is no bad fit)
    for step, (tr, est, _, _) in enumerate(play("fit_one_is_the_last_position")):
        assert on(est[0]) and est["p0"][0].tolist() == tc.where(step) and est["v"][0].tolist() == [0.0, 0.0, 0.0]


def test_the_gate_resets_when_the_truth_jumps():
    outs = play("gate_reset")
    assert [int(o[0]["flags"][0]) for o in outs] == [SEEN, SEEN, SEEN, SEEN | RESET, SEEN]
    assert [int(o[0]["count"][0]) for o in outs] == [1, 2, 3, 1, 2] and [int(o[3][2]) for o in outs] == [0, 0, 0, 1, 0]
    assert [on(o[1][0]) for o in outs] == [False, True, True, False, True]
    assert outs[4][1]["p0"][0].tolist() == tc.where(4, (5.5, -2.25, 0.75)) and outs[4][1]["v"][0].tolist() == list(tc.V)
    assert [int(o[0]["flags"][0]) for o in play("gate_holds_on_the_flight")] == [SEEN] * 5


def test_lost_exactly_one_tick_after_max_age():
    outs = play("lost_after_max_age")
    assert [int(o[0]["flags"][0]) for o in outs] == [SEEN, SEEN, 0, LOST, 0] and [int(o[0]["count"][0]) for o in outs] == [1, 2, 2, 0, 0]
    assert_estimate(outs[2][1][0], 5)
    assert outs[3][0].tobytes()[:-48] == bytes(320 - 48) and outs[3][1].tobytes() == bytes(64) and outs[3][3].tolist() == [0, 0, 0, 1]
    assert outs[4][0].tobytes() == bytes(320) and outs[4][3].tolist() == [0, 0, 0, 0]
    outs = play("lost_and_seen_again_in_one_call")
    assert [int(o[0]["flags"][0]) for o in outs] == [SEEN, SEEN, SEEN | LOST, SEEN] and [int(o[0]["count"][0]) for o in outs] == [1, 2, 1, 2]


def test_a_stale_tick_is_ignored():
    outs = play("stale_tick")
    assert [int(o[0]["flags"][0]) for o in outs] == [SEEN, SEEN, STALE, STALE, SEEN] and [int(o[0]["count"][0]) for o in outs] == [1, 2, 2, 2, 3]
    assert outs[2][2].tolist() == [0] and outs[2][3].tolist() == [1, 1, 0, 0]       # (it was seen, and the record of before stands)
    assert outs[2][0]["tick"].tolist() == outs[1][0]["tick"].tolist() and outs[2][1].tobytes() == outs[1][1].tobytes()
    assert_estimate(outs[4][1][0], 2)


def test_line_of_sight():
    seer = lambda name: play(name)[0][2].tolist()  # noqa: E731
    assert seer("behind_the_wall") == [-1] and play("behind_the_wall")[0][0].tobytes() == bytes(320)
    assert seer("a_second_vehicle_beside_it") == [1]
    assert seer("through_the_door") == [0]
    assert seer("sharing_an_occupied_cell") == [0]
    assert seer("vehicle_inside_an_inflated_cell") == [0]
    assert seer("obstacle_outside_the_map") == [1]
    assert seer("exactly_at_r_detect") == [-1]
    assert seer("two_see_it") == [2]
    assert seer("wall_without_a_map") == [0] and seer("nobody_there") == [-1]
    a, b = play("wall_without_a_map")[0], play("wall_in_an_empty_map")[0]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))                    # an empty map is map = NULL


def test_truth_records_that_are_not_valid_are_seen_by_nobody():
    tr, est, seer, info = play("truth_records_that_are_not_valid")[0]
    assert seer.tolist() == [-1] * 6 + [0] and info.tolist() == [1, 1, 0, 0]
    assert tr[:6].tobytes() == bytes(6 * 320) and est[:6].tobytes() == bytes(6 * 64) and on(est[6]) and float(est["radius"][6]) == 0.0


def test_a_bad_record_reads_as_an_empty_track_and_bad_numbers_are_a_bad_fit():
    case = tc.CASES["constant_velocity_2"]
    good = tc.play(tmod, case)[-1][0]
    for field, value in (("count", 9), ("count", -1), ("head", 8), ("head", -1)):
        bad = good.copy()
        bad[field] = value
        tr = tc.play(tmod, dict(case, steps=case["steps"][:1]), tracks=bad)[0][0]
        assert (int(tr["count"][0]), int(tr["head"][0])) == (1, 0), (field, value)
    bad = good.copy()
    bad["tick"][0, 1] = -5
    assert int(tc.play(tmod, dict(case, steps=case["steps"][:1]), tracks=bad)[0][0]["count"][0]) == 1
    bad = good.copy()
    bad["pos"][0, 0, 1] = np.inf                                                  # a number that is no position: the fit is not usable
    truth, t0, _, _ = case["steps"][0]
    tr, est, seer, info = tmod.track(case["par"], truth, 2, 2, tc.FAR, bad)
    assert int(tr["flags"][0]) == BAD and est.tobytes() == bytes(64) and info.tolist() == [0, 0, 0, 0]
    dirty = good.copy()                                                             # what the record held besides does not show
    dirty["reserved"], dirty["flags"] = 7, 255
    dirty["tick"][0, 5], dirty["pos"][0, 6] = 99, 4.0
    a = tmod.track(case["par"], truth, 2, 2, tc.NEAR, good)
    b = tmod.track(case["par"], truth, 2, 2, tc.NEAR, dirty)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_seen_is_monotone_in_r_detect():
    rng = np.random.default_rng(5)
    occ, origin, res = tc.world("scene")
    pos = rng.uniform((-2.1, -2.1, 0.1), (2.1, 2.1, 1.9), size=(24, 3))
    truth = abi.make_obstacles(rng.uniform((-2.1, -2.1, 0.1), (2.1, 2.1, 1.9), size=(16, 3)), None, 0.1)
    before = np.zeros((16, 24), dtype=bool)
    counts = []
    for r in (0.5, 1.0, 1.5, 2.5, 4.0):
        now = np.array([tmod.sees(tc.par(r), [float(x) for x in t["p0"]], pos, occ, origin, res) for t in truth])
        assert not (before & ~now).any()
        before = now
        counts.append(int(now.sum()))
    assert counts[0] < counts[-1] < 16 * 24                                          # (some are seen, and walls hide some to the end)


@pytest.mark.parametrize("variant", sorted(tc.TELLS))
def test_each_variant_fails_the_case_named_for_it(variant):
    name = tc.TELLS[variant]
    right, wrong = play(name), play(name, variant)
    assert any(x.tobytes() != y.tobytes() for a, b in zip(right, wrong) for x, y in zip(a, b)), (variant, name)


def test_the_two_variants_told_by_a_seeded_search():
    case = tc.orientation_case(tmod)
    assert tc.play(tmod, case)[0][2].tolist() == [0] and tc.play(tmod, case, "ray_from_obstacle")[0][2].tolist() == [-1]
    case = tc.summation_case(tmod)
    assert case is not None
    assert set(tmod.VARIANTS) == set(tc.TELLS) | {"ray_from_obstacle", "newest_first"}
