"""The numpy model of the traffic stage (tests/traffic_model.py, the restatement of include/fasterhip_traffic.h) on hand cases whose
answers are worked out by hand, and six wrong variants of the model, each of which changes the case that is named for it.
tests/test_gpu_traffic.py runs the same cases on the device.  Coordinates are multiples of 1/8, so every difference, square and sum
below is exact."""
import numpy as np
import pytest

import traffic_model as tm
from faster_amd import abi

ALL, YIELD = abi.FH_TRAFFIC_ALL, abi.FH_TRAFFIC_YIELD_TO_LOWER
STALE = 0xFFFFFFFF


def case(par, plan_positions, positions, bits, points=None, clear_rows=(), **kw):
    """bits: {(row, cloud point): expected bit}; points: {cloud point: xyz}; clear_rows: rows whose traffic words are all zero."""
    v, pl = tm.fleet(plan_positions, positions, **kw)
    return dict(par=par, v=v, pl=pl, bits=bits, points=points or {}, clear_rows=tuple(clear_rows))


def hand_cases():
    c = {}
    # (3, 4, 0) is exactly 5 from the origin: not shown with range 5 (strict), shown with the next double above 5
    c["exactly_range"] = case(tm.params(1, 1, 5.0), [[(0, 0, 0)], [(3, 4, 0)]], [(0, 0, 0), (3, 4, 0)], {(0, 1): False, (1, 0): False},
                              {0: (0, 0, 0), 1: (3, 4, 0)}, clear_rows=(0, 1))
    c["just_above_range"] = case(tm.params(1, 1, 5.000000000000001), [[(0, 0, 0)], [(3, 4, 0)]], [(0, 0, 0), (3, 4, 0)],
                                 {(0, 1): True, (1, 0): True, (0, 0): False, (1, 1): False})
    # S = 3, stride 2: vehicle 1 has two states, so the instants 2 and 4 are its last state (1, 0, 0), inside range 2 of vehicle 0
    c["plan_end"] = case(tm.params(3, 2, 2.0), [[(0, 0, 0)] * 5, [(10, 0, 0), (1, 0, 0)]], [(0, 0, 0), (10, 0, 0)],
                         {(0, 3): False, (0, 4): True, (0, 5): True, (1, 0): False}, {3: (10, 0, 0), 4: (1, 0, 0), 5: (1, 0, 0)}, clear_rows=(1,))
    # alone: its own samples lie on its own position and are never shown to it
    c["alone"] = case(tm.params(2, 1, 1.0), [[(0.5, 0, 0), (0.5, 0, 0)]], [(0.5, 0, 0)], {(0, 0): False, (0, 1): False}, clear_rows=(0,))
    # the traffic words hold ones from the last cycle: they are written whole
    c["stale_bits"] = case(tm.params(1, 1, 1.0, first_point=32), [[(0, 0, 0)], [(0.5, 0, 0)], [(9, 9, 9)]], [(0, 0, 0), (0.5, 0, 0), (9, 9, 9)],
                           {(0, 1): True, (0, 2): False, (0, 0): False, (0, 3): False, (0, 31): False, (1, 0): True, (2, 0): False}, clear_rows=(2,))
    # the hull: centre, +x, -x, +y, -y, +z, -z
    h = 0.25
    c["hull_points"] = case(tm.params(1, 1, 4.0, hull=h), [[(1, 2, 3)], [(-1, 0.5, 0)]], [(1, 2, 3), (-1, 0.5, 0)],
                            {(0, 7): True, (0, 13): True, (0, 0): False, (0, 14): False, (1, 0): True, (1, 6): True, (1, 7): False},
                            {0: (1, 2, 3), 1: (1.25, 2, 3), 2: (0.75, 2, 3), 3: (1, 2.25, 3), 4: (1, 1.75, 3), 5: (1, 2, 3.25), 6: (1, 2, 2.75),
                             7: (-1, 0.5, 0), 8: (-0.75, 0.5, 0), 9: (-1.25, 0.5, 0), 12: (-1, 0.5, 0.25), 13: (-1, 0.5, -0.25)})
    # one decision per sample: the centre at exactly range keeps all seven clear although the -x point is nearer; a centre inside range
    # sets all seven although the +x point is outside
    c["per_sample"] = case(tm.params(1, 1, 1.0, hull=h), [[(0, 0, 0)], [(1, 0, 0)], [(0, 0.875, 0)]], [(0, 0, 0), (1, 0, 0), (0, 0.875, 0)],
                           dict([((0, 7 + o), False) for o in range(7)] + [((0, 14 + o), True) for o in range(7)] + [((1, 0), False), ((2, 0), True)]))
    # yield to lower: vehicle i sees k < i only
    c["yield"] = case(tm.params(1, 1, 2.0, rule=YIELD), [[(0, 0, 0)], [(0.5, 0, 0)], [(1, 0, 0)]], [(0, 0, 0), (0.5, 0, 0), (1, 0, 0)],
                      {(0, 1): False, (0, 2): False, (1, 0): True, (1, 2): False, (2, 0): True, (2, 1): True}, clear_rows=(0,))
    # an empty plan, a negative head, head + size > max_states, a NaN and an infinity in a sampled position: zeros, shown to nobody;
    # vehicle 6 has a NaN in its own position: its row is clear, and it is still shown to the others
    n = 7
    plans = [[(0, 0, 0)] * 2, [], [(0.125, 0, 0)] * 2, [(0.25, 0, 0)] * 2, [(np.nan, 0, 0), (0.375, 0, 0)], [(0.5, 0, 0), (0, np.inf, 0)], [(0.625, 0, 0)] * 2]
    pos = [(0, 0, 0), (0, 0, 0), (0.125, 0, 0), (0.25, 0, 0), (0.375, 0, 0), (0.5, 0, 0), (0.625, np.nan, 0)]
    cc = case(tm.params(2, 1, 3.0), plans, pos, {}, max_states=4, heads=[0, 0, 0, 0, 0, 0, 0])
    cc["v"]["plan_head"][2] = -1
    cc["v"]["plan_head"][3], cc["v"]["plan_size"][3] = 3, 2
    bits = {}
    shown = {0: (1, 1), 1: (0, 0), 2: (0, 0), 3: (0, 0), 4: (0, 1), 5: (1, 0), 6: (1, 1)}
    for i in range(n):
        for k in range(n):
            for s in range(2):
                bits[(i, 2 * k + s)] = bool(shown[k][s]) and k != i and i != 6
    cc["bits"], cc["clear_rows"] = bits, (6,)
    cc["points"] = {2: (0, 0, 0), 3: (0, 0, 0), 4: (0, 0, 0), 5: (0, 0, 0), 6: (0, 0, 0), 7: (0, 0, 0), 8: (0, 0, 0), 9: (0.375, 0, 0), 10: (0.5, 0, 0),
                    11: (0, 0, 0), 12: (0.625, 0, 0)}
    c["flagged"] = cc
    return c


CASES = hand_cases()
# the case each wrong variant changes
CHANGED_BY = {"le": "exactly_range", "no_clamp": "plan_end", "self": "alone", "or": "stale_bits", "hull_order": "hull_points",
              "per_point": "per_sample"}


def inputs(c):
    """(n_cloud, cloud, mask) before the call: static points with a pattern, traffic points poisoned, traffic words all ones."""
    n = len(c["v"])
    n_cloud, words = tm.layout(c["par"], n)
    cloud = np.arange(3 * n_cloud, dtype=np.float64).reshape(n_cloud, 3) + 0.5
    mask = np.full((n, words), STALE, dtype=np.uint32)
    return n_cloud, cloud, mask


def run(c, variant=None):
    _, cloud, mask = inputs(c)
    return tm.traffic(c["par"], c["v"], c["pl"], c["pl"].shape[1], cloud, mask, variant)


def check(c, cloud, mask, name):
    first = int(c["par"]["first_point"])
    n = len(c["v"])
    total = n * int(c["par"]["samples"]) * abi.traffic_points_per_sample(c["par"]["hull"])
    for (i, point), want in c["bits"].items():
        assert tm.bit(mask, i, first + point) == want, (name, i, point)
    for point, xyz in c["points"].items():
        assert cloud[first + point].tolist() == [float(x) for x in xyz], (name, point, cloud[first + point])
    w0, w1 = first // 32, -(-(first + total) // 32)
    for i in c["clear_rows"]:
        assert not mask[i, w0:w1].any(), (name, i)
    assert (mask[:, :w0] == STALE).all() and (mask[:, w1:] == STALE).all()
    if (first + total) % 32:
        assert not (mask[:, w1 - 1] >> np.uint32((first + total) % 32)).any(), name   # bits past the last traffic point
    _, before, _ = inputs(c)
    assert cloud[:first].tobytes() == before[:first].tobytes()


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_cases(name):
    cloud, mask = run(CASES[name])
    check(CASES[name], cloud, mask, name)


@pytest.mark.parametrize("variant", tm.VARIANTS)
def test_every_wrong_variant_changes_its_case(variant):
    assert set(CHANGED_BY) == set(tm.VARIANTS)
    name = CHANGED_BY[variant]
    good_cloud, good_mask = run(CASES[name])
    bad_cloud, bad_mask = run(CASES[name], variant)
    assert good_cloud.tobytes() != bad_cloud.tobytes() or good_mask.tobytes() != bad_mask.tobytes(), variant
    with pytest.raises(AssertionError):
        check(CASES[name], bad_cloud, bad_mask, name)


def test_words_straddled_by_sample_groups_and_a_partial_last_word():
    """n = 5, S = 3, hull: 21 bits per vehicle, 105 bits in 4 words; vehicle 0 sees everyone, so its row is ones except its own 21 bits
    and the 23 bits past the end."""
    line = [(0.125 * j, 0, 0) for j in range(3)]
    v, pl = tm.fleet([[(x + k, 0, 0) for x, _, _ in line] for k in range(5)], [(k, 0, 0) for k in range(5)])
    par = tm.params(3, 1, 100.0, hull=0.25)
    n_cloud, words = tm.layout(par, 5)
    assert (n_cloud, words) == (105, 4)
    cloud, mask = tm.traffic(par, v, pl, 3, np.zeros((n_cloud, 3)), np.full((5, words), STALE, dtype=np.uint32))
    stream = sum(int(mask[0, w]) << (32 * w) for w in range(4))
    assert stream == ((1 << 105) - 1) & ~((1 << 21) - 1)
    stream = sum(int(mask[2, w]) << (32 * w) for w in range(4))
    assert stream == ((1 << 105) - 1) & ~(((1 << 21) - 1) << 42)


def test_params_and_layout_helpers():
    p = abi.default_traffic_params(4, 5, 6.0, hull=0.3, rule=YIELD, first_point=64)
    assert (int(p["samples"]), int(p["stride"]), float(p["range"]), float(p["hull"]), int(p["rule"]), int(p["first_point"])) == (4, 5, 6.0, 0.3, 1, 64)
    assert not p["reserved"].any() and abi.traffic_params_dtype.itemsize == 48
    assert abi.traffic_points_per_sample(0.0) == 1 and abi.traffic_points_per_sample(0.3) == 7
    assert tm.layout(p, 3) == (64 + 3 * 4 * 7, 5)
