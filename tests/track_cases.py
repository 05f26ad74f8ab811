"""The hand cases of the tracker of moving obstacles (include/fasterhip_track.h), shared by tests/test_track_model.py (the model on the
CPU) and tests/test_gpu_track.py (every byte of the device against the model).  Not a test file.

A case is a sequence of calls on one set of tracks that start empty: dict(par, world, steps), world None (map = NULL), "scene" (the
walled map of tests/link_los_cases.py: a wall at x in [-0.2, 0.4) with a door at y in [0.8, 1.0), a pillar at x, y in [-1.8, -1.2)) or
"empty" (its lattice without a point); a step is (truth [m] abi.obstacle_dtype, truth_tick0, tick, positions [n][3]).  Coordinates,
velocities and dc are dyadic where a closed form is asserted, so every sum of the fit is exact."""
import numpy as np

from faster_amd import abi

import link_los_cases as lc

DC = 0.125
NAN, INF = float("nan"), float("inf")
P0, V, RADIUS = (1.5, -2.25, 0.75), (0.5, -0.25, 1.0), 0.375
NEAR = [(1.0, -2.0, 1.0)]       # a vehicle that sees the flight of P0, V for its first 16 ticks with r_detect = 8
FAR = [(100.0, 100.0, 100.0)]


def par(r_detect=8.0, **kw):
    return abi.default_track_params(r_detect, DC, **kw)


def flight(tick, p0=P0, v=V, radius=RADIUS):
    """One obstacle on the flight p0 + v t, written as a real system writes it: where it is at `tick`, the truth's clock at 0."""
    at = np.asarray(p0) + np.asarray(v) * (tick * DC)
    return abi.make_obstacles([at], [v], radius)


def where(tick, p0=P0, v=V):
    return (np.asarray(p0) + np.asarray(v) * (tick * DC)).tolist()


def seen_at(ticks, pos=None, **kw):
    """The flight seen by NEAR at each of `ticks`: one truth record at clock 0, the truth's clock = the tick."""
    truth = abi.make_obstacles([P0], [V], RADIUS)
    return dict(par=par(**kw), world=None, steps=[(truth, t, t, NEAR if pos is None else pos) for t in ticks])


def world(name):
    """(occ, origin, res) of a world for the model, or None."""
    if name is None:
        return None
    occ = lc.expected_occupancy() if name == "scene" else np.zeros_like(lc.expected_occupancy())
    return occ, np.array(lc.ORIGIN, dtype=np.float64), lc.RES


def one(z, radius=0.25):
    return abi.make_obstacles([z], None, radius)


def los_case(z, pos, w="scene", r_detect=3.0, **kw):
    return dict(par=par(r_detect, min_obs=1, **kw), world=w, steps=[(one(z), 0, 0, pos)])


CASES = {}
for _k in range(2, 9):   # k sightings one tick apart, fitted all: v and the current position come back bit for bit
    CASES["constant_velocity_%d" % _k] = seen_at(range(_k), fit=8, min_obs=_k)
CASES["uneven_ticks"] = seen_at([0, 1, 4, 6, 7, 12], fit=8)
CASES["fit_window_of_three"] = seen_at(range(6), fit=3)
# three sightings, then the vehicle is gone: ticks 5 and 9 extrapolate, and the radius grows by grow * age
CASES["extrapolation_and_grow"] = dict(seen_at(range(3), grow=0.5), steps=seen_at(range(3))["steps"] + [
    (abi.make_obstacles([P0], [V], RADIUS), t, t, FAR) for t in (5, 9)])
CASES["ring_wrap"] = seen_at(range(10), fit=8)
CASES["min_obs_three"] = seen_at(range(4), min_obs=3)
CASES["fit_one_is_the_last_position"] = seen_at(range(3), fit=1, min_obs=1)
# the truth jumps by (4, 0, 0) at tick 3: with a gate of 1 m the track starts anew there
CASES["gate_reset"] = dict(par=par(gate=1.0), world=None, steps=[(flight(t, P0 if t < 3 else (5.5, -2.25, 0.75)), 0, t, NEAR) for t in range(5)])
CASES["gate_holds_on_the_flight"] = seen_at(range(5), gate=0.25)
# seen at ticks 0 and 1, then nobody near: max_age = 4 keeps the track at tick 5 (age 4) and forgets it at tick 6
CASES["lost_after_max_age"] = dict(seen_at([0, 1], max_age=4), steps=seen_at([0, 1])["steps"] + [
    (abi.make_obstacles([P0], [V], RADIUS), t, t, FAR) for t in (5, 6, 7)])
CASES["lost_and_seen_again_in_one_call"] = seen_at([0, 1, 9, 10], max_age=4)
CASES["stale_tick"] = seen_at([0, 1, 1, 0, 2])
# line of sight in the walled scene: obstacle right of the wall, vehicle left of it
CASES["behind_the_wall"] = los_case((1.0, -1.0, 0.5), [(-1.0, -1.0, 0.5)])
CASES["a_second_vehicle_beside_it"] = los_case((1.0, -1.0, 0.5), [(-1.0, -1.0, 0.5), (1.0, -0.5, 0.5)])
CASES["through_the_door"] = los_case((1.0, 0.9, 0.5), [(-1.0, 0.9, 0.5)])
CASES["sharing_an_occupied_cell"] = los_case((0.18, -1.0, 0.5), [(0.13, -1.0, 0.5)])       # x cell 10 of the wall: K = 1, no sample
CASES["vehicle_inside_an_inflated_cell"] = los_case((-1.0, -1.0, 0.5), [(-0.1, -1.0, 0.5)])
CASES["wall_without_a_map"] = los_case((1.0, -1.0, 0.5), [(-1.0, -1.0, 0.5)], w=None)
CASES["wall_in_an_empty_map"] = los_case((1.0, -1.0, 0.5), [(-1.0, -1.0, 0.5)], w="empty")
# the obstacle above the map: from below the ray goes through the wall inside the map (blocked); at its height every sample is outside (free)
CASES["obstacle_outside_the_map"] = los_case((1.0, -1.0, 2.5), [(-1.0, -1.0, 0.5), (-1.0, -1.0, 2.5)])
CASES["exactly_at_r_detect"] = los_case((-1.0, 0.5, 0.5), [(-1.0, -1.0, 0.5)], r_detect=1.5)
CASES["two_see_it"] = los_case((-1.0, 0.0, 0.5), [(NAN, 0.0, 0.5), (1.0, 0.0, 0.5), (-1.0, -0.5, 0.5), (-1.0, 0.5, 0.5)])
CASES["truth_records_that_are_not_valid"] = dict(par=par(min_obs=1), world=None, steps=[(np.concatenate([
    abi.make_obstacles([P0], [V], RADIUS, on=False), abi.make_obstacles([(NAN, 0.0, 0.0)], [V], RADIUS),
    abi.make_obstacles([P0], [(0.0, INF, 0.0)], RADIUS), abi.make_obstacles([P0], [V], -0.5), abi.make_obstacles([P0], [V], NAN),
    abi.make_obstacles([(1e308, 0.0, 0.0)], [(1e308, 0.0, 0.0)], RADIUS), abi.make_obstacles([P0], [V], 0.0)]), 8, 8, NEAR)])
CASES["nobody_there"] = dict(par=par(min_obs=1), world=None, steps=[(abi.make_obstacles([P0], [V], RADIUS), 0, 0, np.zeros((0, 3)))])

# the case each variant of tests/track_model.py changes ("ray_from_obstacle" and "newest_first" are told by seeded searches)
TELLS = {"le": "exactly_at_r_detect", "end_cells_tested": "vehicle_inside_an_inflated_cell", "seer_largest": "two_see_it", "no_gate": "gate_reset",
         "age_inclusive": "lost_after_max_age", "stale_accepted": "stale_tick"}


def play(model, case, variant=None, tracks=None):
    """The case through tests/track_model.py: [(tracks, est, seer, info)] per step."""
    w = world(case["world"])
    occ, origin, res = w if w is not None else (None, None, None)
    outs = []
    for truth, t0, tick, pos in case["steps"]:
        if tracks is None:
            tracks = np.zeros(len(truth), dtype=abi.obstacle_track_dtype)
        out = model.track(case["par"], truth, t0, tick, pos, tracks, occ, origin, res, variant)
        outs.append(out)
        tracks = out[0]
    return outs


def orientation_case(model):
    """The pair of tests/link_los_cases.py's seeded search as vehicle and obstacle: the ray from the vehicle is free, the ray from the
    obstacle blocked."""
    occ, origin, res = world("scene")
    found = lc.orientation_pair(occ, origin, res, lambda p, q, o, mo, mr: model.blocked([float(x) for x in p], [float(x) for x in q], o, mo, mr))
    assert found is not None
    p, q, _ = found
    return los_case(tuple(q), [tuple(p)], r_detect=4.0)


def summation_case(model):
    """Seeded search: four sightings of a flight on no grid whose fit differs in a bit when the sums run from the newest."""
    rng = np.random.default_rng(11)
    for _ in range(200):
        p0, v = rng.uniform(-3, 3, size=3), rng.uniform(-1, 1, size=3)
        case = dict(par=par(50.0, fit=4), world=None,
                    steps=[(abi.make_obstacles([p0], [v], RADIUS), t, t, NEAR) for t in (0, 1, 3, 4)])
        if play(model, case)[-1][1].tobytes() != play(model, case, "newest_first")[-1][1].tobytes():
            return case
    return None
