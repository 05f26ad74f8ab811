"""The model of the commit check (tests/check_model.py, the numpy restatement of include/fasterhip_check.h) on hand cases whose answers
are written down, every deliberate mistake of `check_model.VARIANTS` changing one of them at least; the invariant the header promises,
on random small fleets with the separation's model (tests/separation_model.py) as the judge; and the revert on byte arrays.  No GPU;
tests/test_gpu_check.py runs the same cases on the device."""
import numpy as np

from faster_amd import abi

import check_model as cm

INF = float("inf")
C, X, NF, BAD = abi.FH_CHECK_CANDIDATE, abi.FH_CHECK_CONFLICT, abi.FH_CHECK_NOT_FINITE, abi.FH_CHECK_BAD_PLAN
NONE = (0, 0, -1, -1, -1, INF)   # the record of a vehicle that is no candidate


def line(a, b, n):
    """n positions from a to b inclusive (n >= 2), or n copies of a when b is None."""
    a = np.asarray(a, dtype=np.float64)
    if b is None:
        return np.repeat(a[None, :], n, axis=0)
    return a[None, :] + (np.asarray(b, dtype=np.float64) - a)[None, :] * (np.arange(n) / (n - 1.0))[:, None]


def _cases():
    """name -> (par, (v, pl, ov, opl), {vehicle: (flags, n_tested, first, first_other, first_kind, d2)}, the variants that change it)."""
    cases = {}
    O = (0.0, 0.0, 0.0)
    # 3-4-5: an other at exactly r = 5 is no conflict; (3, 3.75, 0) is at d2 = 23.0625
    cases["exactly_r_is_no_conflict"] = (cm.params(5.0), cm.scene([[O], line((3, 4, 0), None, 3)], {0: (0, line(O, None, 2))}),
                                         {0: (C, 2, -1, -1, -1, INF), 1: NONE}, {"le"})
    cases["just_inside_r"] = (cm.params(5.0), cm.scene([[O], line((3, 3.75, 0), None, 3)], {0: (0, line(O, None, 2))}),
                              {0: (C | X, 2, 0, 1, 0, 23.0625)}, set())
    # ties: vehicle 2 flies (0,0,0) -> (4,0,0) in 5 states; at j = 1 it is at (1,0,0)
    fly = line(O, (4, 0, 0), 5)
    near1 = [(9, 9, 9), (1, 3, 0), (9, 9, 9), (9, 9, 9), (9, 9, 9)]    # d2 = 9 at j = 1 only
    near2 = [(9, 9, 9), (9, 9, 9), (2, 0, 3), (9, 9, 9), (9, 9, 9)]    # d2 = 9 at j = 2 only
    cases["tie_in_j_goes_to_the_smaller_k"] = (cm.params(3.5), cm.scene([near1, near1, [O]], {2: (0, fly)}),
                                               {2: (C | X, 5, 1, 0, 0, 9.0)}, {"larger_k_on_ties"})
    cases["smaller_j_beats_smaller_k"] = (cm.params(3.5), cm.scene([near2, near1, [O]], {2: (0, fly)}), {2: (C | X, 5, 1, 1, 0, 9.0)}, set())
    # vehicle 0 stood far away and commits into `near1`: its old plan is clear, its new one is not: kind 1 of the smaller k wins over kind 0 of k = 1
    far = line((-9, -9, -9), None, 1)
    near1b = [(-9, -9, -9), (1, -3, 0), (-9, -9, -9), (-9, -9, -9), (-9, -9, -9)]
    cases["tie_in_k_kind_1_of_a_lower_candidate"] = (cm.params(3.125), cm.scene([far, near1, [O]], {0: (0, near1b), 2: (0, fly)}),   # (0 passes 10 from where 2 stood)
                                                     {0: (C, 5, -1, -1, -1, INF), 2: (C | X, 5, 1, 0, 1, 9.0)}, {"no_kind1"})
    # the same vehicle old AND new at the same place: kind 0 before kind 1
    cases["tie_in_kind_goes_to_0"] = (cm.params(3.125), cm.scene([near1, [O]], {0: (4, near1), 1: (0, fly)}),
                                      {0: (C, 5, -1, -1, -1, INF), 1: (C | X, 5, 1, 0, 0, 9.0)}, set())
    # kept: vehicle 0 has 6 old states along x and replans from kept = 3 (k_end_whole = 2); vehicle 1 stands next to its state 1
    old6 = line(O, (5, 0, 0), 6)
    by1 = line((1, 1, 0), None, 8)
    cases["a_conflict_below_kept_is_not_this_commits"] = (cm.params(1.5), cm.scene([old6, by1], {0: (2, line((3, 5, 0), (5, 5, 0), 3))}),
                                                         {0: (C, 3, -1, -1, -1, INF)}, {"from_zero"})
    cases["kept_zero_tests_everything"] = (cm.params(1.5), cm.scene([old6, by1], {0: (5, line(O, (5, 0, 0), 6))}),
                                           {0: (C | X, 6, 0, 1, 0, 2.0)}, set())
    # kept = the whole new plan (nothing new: cur size = kept = 3): no instant of its own, but it stands at (2,0,0) and vehicle 1 comes by at j = 5
    pass_by = np.array([(9, 9, 9)] * 5 + [(2, 1, 0)] + [(9, 9, 9)] * 2, dtype=np.float64)
    cases["kept_is_the_whole_plan_and_it_is_flown_through_later"] = (cm.params(1.5), cm.scene([old6, pass_by], {0: (2, np.zeros((0, 3)))}),
                                                                    {0: (C | X, 0, 5, 1, 0, 1.0)}, {"own_size_only"})
    # an other that ended before kept_i stands at its last state
    cases["an_other_that_ended_before_kept"] = (cm.params(1.5), cm.scene([old6, [(9, 9, 9), (4, 1, 0)]], {0: (2, line((3, 0, 0), (5, 0, 0), 3))}),
                                                {0: (C | X, 3, 3, 1, 0, 2.0)}, set())
    # a candidate that ends (3 states) and is flown through at j = 7
    through = np.array([(9, 9, 9)] * 7 + [(2, 0, 1)] + [(9, 9, 9)] * 2, dtype=np.float64)
    cases["a_candidate_that_ends_is_flown_through_later"] = (cm.params(1.5), cm.scene([[O], through], {0: (0, line(O, (2, 0, 0), 3))}),
                                                            {0: (C | X, 3, 7, 1, 0, 1.0)}, {"own_size_only"})
    # lower indexes have priority: 0 and 1 cross at j = 2 and are sqrt 2 apart at j = 1 already; 0 passes, 1 is withheld by cur_0
    a, b = line((0, 0, 0), (4, 0, 0), 5), line((2, -2, 0), (2, 2, 0), 5)
    cases["the_lower_index_has_priority"] = (cm.params(1.5), cm.scene([[(0, 0, 0)], [(2, -2, 0)]], {0: (0, a), 1: (0, b)}),
                                             {0: (C, 5, -1, -1, -1, INF), 1: (C | X, 5, 1, 0, 1, 2.0)}, {"no_kind1", "kind1_of_higher"})
    # a kind-1 other that is itself in conflict still counts: 0 runs into the standing 2 and is withheld, 1 is withheld by cur_0 all the same
    cases["a_withheld_lower_candidate_still_counts"] = (cm.params(1.5), cm.scene([[(0, 0, 0)], [(2, -2, 0)], line((4, 1, 0), None, 2)],
                                                                               {0: (0, a), 1: (0, b)}),
                                                        {0: (C | X, 5, 3, 2, 0, 2.0), 1: (C | X, 5, 1, 0, 1, 2.0), 2: NONE}, {"no_kind1"})
    # bad extents: on the candidate's side (old or new) it is no candidate; an other with a bad old extent is nobody's other
    v, pl, ov, opl = cm.scene([[O], line((1, 0, 0), None, 2), [(50, 0, 0)], [(0, 50, 0)]],
                              {0: (0, line(O, None, 2)), 2: (0, line((50, 0, 0), None, 2)), 3: (0, line((0, 50, 0), None, 2))})
    ov["plan_head"][1] = -1                # the only near other: its old extent is bad
    ov["plan_size"][2] = pl.shape[1] + 1   # candidate 2: bad old extent
    v["plan_head"][3] = pl.shape[1]        # candidate 3: bad new extent (head + size > max_states)
    cases["bad_extents_on_either_side"] = (cm.params(1.5), (v, pl, ov, opl), {0: (C, 2, -1, -1, -1, INF), 1: NONE, 2: NONE, 3: NONE}, {"bad_as_other"})
    # kept outside [0, min(old size, new size)] is clamped and flagged
    v, pl, ov, opl = cm.scene([old6, by1, old6 + (0, 50, 0)], {0: (2, line((3, 5, 0), (5, 5, 0), 3)), 2: (2, line((3, 55, 0), (5, 55, 0), 3))})
    ov["k_end_whole"][0] = 9     # kept = -4 -> 0: the conflict at j = 0 .. 2 below the real kept shows
    ov["k_end_whole"][2] = -9    # kept = 14 -> 6
    cases["kept_is_clamped_and_flagged"] = (cm.params(1.5), (v, pl, ov, opl), {0: (C | X | BAD, 6, 0, 1, 0, 2.0), 2: (C | BAD, 0, -1, -1, -1, INF)}, set())
    # not finite: a NaN of the candidate at the instant of the only conflict, an infinity of the other at another one; inf - inf
    v, pl, ov, opl = cm.scene([[O], near1, near2], {0: (0, fly)})
    pl["pos"][0, 1, 2] = np.nan
    opl["pos"][2, 2, 0] = np.inf
    cases["nan_and_infinity_fail_the_comparison"] = (cm.params(3.5), (v, pl, ov, opl), {0: (C | NF, 5, -1, -1, -1, INF)}, set())
    v, pl, ov, opl = cm.scene([[O], near1], {0: (0, fly)})
    pl["pos"][0, 1, 0], opl["pos"][1, 1, 0] = np.inf, np.inf
    pl["pos"][0, 3] = (9, 9, 9)   # (and one real conflict behind it: the flag does not end the test)
    cases["inf_minus_inf"] = (cm.params(3.5), (v, pl, ov, opl), {0: (C | NF | X, 5, 3, 1, 0, 0.0)}, set())
    v, pl, ov, opl = cm.scene([[O], near1], {0: (0, fly)})
    opl["pos"][1, 1, 1] = np.nan   # the other's NaN: no flag of anyone
    cases["nan_of_the_other_is_no_flag"] = (cm.params(3.5), (v, pl, ov, opl), {0: (C, 5, -1, -1, -1, INF)}, set())
    # stride and count: the only conflict is at j = 5 of 8 new states
    fly8 = line(O, (7, 0, 0), 8)
    at5 = np.array([(9, 9, 9)] * 5 + [(5, 1, 0)] + [(9, 9, 9)] * 2, dtype=np.float64)
    sc = cm.scene([[O], at5], {0: (0, fly8)})
    cases["stride_1"] = (cm.params(1.5), sc, {0: (C | X, 8, 5, 1, 0, 1.0)}, set())
    cases["stride_2_steps_over_it"] = (cm.params(1.5, 2), sc, {0: (C, 4, -1, -1, -1, INF)}, set())
    cases["stride_5_lands_on_it"] = (cm.params(1.5, 5), sc, {0: (C | X, 2, 5, 1, 0, 1.0)}, set())
    cases["count_5_ends_before_it"] = (cm.params(1.5, 1, 5), sc, {0: (C, 5, -1, -1, -1, INF)}, set())
    cases["count_6_reaches_it"] = (cm.params(1.5, 1, 6), sc, {0: (C | X, 6, 5, 1, 0, 1.0)}, set())
    cases["count_caps_the_instants_behind_the_plan"] = (cm.params(1.5, 1, 5), cm.scene([[O], through], {0: (0, line(O, (2, 0, 0), 3))}),
                                                       {0: (C, 3, -1, -1, -1, INF)}, set())
    # who is a candidate: committed AND active
    v, pl, ov, opl = cm.scene([[O], [O], line((0, 1, 0), None, 3)], {0: (0, line(O, None, 2)), 1: (0, line(O, None, 2))})
    v["stage"][0] = abi.FH_FLEET_STAGE_NO_SAFE
    v["active"][1] = 0
    cases["not_committed_or_not_active_is_no_candidate"] = (cm.params(1.5), (v, pl, ov, opl), {0: NONE, 1: NONE, 2: NONE}, set())
    return cases


CASES = _cases()


def check(records, expected, name):
    for i, want in expected.items():
        got = tuple(records[k][i] for k in ("flags", "n_tested", "first", "first_other", "first_kind", "d2"))
        assert got == want, "%s, vehicle %d: model %s, written down %s" % (name, i, got, want)
    assert (records["reserved"] == 0).all()


def run(name, variant=None):
    par, (v, pl, ov, opl), _, _ = CASES[name]
    return cm.check(par, v, pl, ov, opl, pl.shape[1], variant)


def test_hand_cases():
    for name, (_, _, expected, _) in CASES.items():
        check(run(name), expected, name)


def test_every_variant_changes_the_cases_that_name_it_and_only_those():
    seen = set()
    for name, (_, _, _, variants) in CASES.items():
        want = run(name).tobytes()
        for var in cm.VARIANTS:
            changed = run(name, var).tobytes() != want
            if var in variants:
                assert changed, (name, var)
                seen.add(var)
    assert seen == set(cm.VARIANTS), set(cm.VARIANTS) - seen


# ---- the invariant -----------------------------------------------------------------------------------------------------------------------
def random_cycle(rng, n, box=4, longest=8):
    """n vehicles on the integer lattice of a small box, plans of 1 .. `longest` states that walk one lattice step per state; each
    vehicle commits with probability 2/3 a new walk behind a random number of kept states."""
    def walk(start, steps):
        p = [np.asarray(start, dtype=np.float64)]
        for _ in range(steps):
            p.append(np.clip(p[-1] + rng.integers(-1, 2, size=3), 0, box))
        return np.array(p)

    old = [walk(rng.integers(0, box + 1, size=3), int(rng.integers(0, longest))) for _ in range(n)]
    commits = {}
    for i in range(n):
        if rng.random() < 2.0 / 3.0:
            kept = int(rng.integers(0, len(old[i])))   # 0 .. size - 1: the start state A is old[kept]
            commits[i] = (len(old[i]) - kept - 1, walk(old[i][kept], int(rng.integers(0, longest))))
    return cm.scene(old, commits, max_states=2 * longest + 2)


def tick(v, pl, ticks):
    """fh_fleet_next_goals_device on host arrays: `ticks` states go from the front of every plan while more than one is left."""
    v = v.copy()
    pops = np.minimum(ticks, np.maximum(v["plan_size"] - 1, 0))
    v["plan_head"] += pops
    v["plan_size"] -= pops
    return v, pl


def test_near_pairs_never_grow_with_the_check_and_do_grow_without_it():
    rng = np.random.default_rng(2024)
    r, grew_without, withheld, committed = 1.5, 0, 0, 0   # lattice neighbours at 1 and sqrt 2 are near, at sqrt 3 and 2 they are not
    for _ in range(150):
        n = int(rng.integers(2, 6))
        v, pl, ov, opl = random_cycle(rng, n)
        ms = pl.shape[1]
        before = cm.near_pairs(r, ov, opl, ms)
        grew_without += bool(cm.near_pairs(r, v, pl, ms) - before)
        rec = cm.check(cm.params(r), v, pl, ov, opl, ms)
        committed += int(((rec["flags"] & C) != 0).sum())
        withheld += int(((rec["flags"] & X) != 0).sum())
        cm.revert(rec, ov, opl, ms, v, pl)
        after = cm.near_pairs(r, v, pl, ms)
        assert after <= before, (after - before, rec)
        v2, pl2 = tick(v, pl, int(rng.integers(1, 6)))
        assert cm.near_pairs(r, v2, pl2, ms) <= after
    assert grew_without >= 30, grew_without          # the property means something: unchecked commits do create near pairs
    assert 0 < withheld < committed, (withheld, committed)   # and the check lets commits through


# ---- backup and revert on byte arrays ----------------------------------------------------------------------------------------------------
def test_backup_and_revert_on_byte_arrays():
    par, (v, pl, ov, opl), _, _ = CASES["a_withheld_lower_candidate_still_counts"]
    v, pl = v.copy(), pl.copy()
    ms = pl.shape[1]
    # the backup of the old side into poisoned arrays holds the records and the live extents, and nothing else is written
    bv = np.frombuffer(bytes([cm.POISON]) * ov.nbytes, dtype=abi.vehicle_dtype).copy()
    bpl = np.frombuffer(bytes([cm.POISON]) * opl.nbytes, dtype=abi.state_dtype).reshape(opl.shape).copy()
    ov2 = ov.copy()
    ov2["plan_head"][2], ov2["plan_size"][2] = 1, 1     # a head that is not zero
    cm.backup(ov2, opl, ms, bv, bpl)
    assert bv.tobytes() == ov2.tobytes()
    live = np.zeros(opl.shape, dtype=bool)
    for k in range(len(ov2)):
        live[k, ov2["plan_head"][k]:ov2["plan_head"][k] + ov2["plan_size"][k]] = True
    assert bpl[live].tobytes() == opl[live].tobytes() and (bpl[~live].view(np.uint8) == cm.POISON).all()
    # the revert: 0 and 1 are withheld, 2 is not touched
    rec = cm.check(par, v, pl, ov, opl, ms)
    assert [int(f) & X for f in rec["flags"]] == [X, X, 0]
    v0, pl0 = v.copy(), pl.copy()
    loose = cm.revert(rec, ov, opl, ms, v, pl)
    for k in (0, 1):
        want = ov[k].copy()
        want["stage"] = abi.FH_FLEET_STAGE_CONFLICT
        assert v[k].tobytes() == want.tobytes() and abi.FH_FLEET_STAGE_CONFLICT == 7
        h, s = int(ov["plan_head"][k]), int(ov["plan_size"][k])
        assert pl[k, h:h + s].tobytes() == opl[k, h:h + s].tobytes() and not loose[k, h:h + s].any() and loose[k, h + s:].all()
    assert v[2].tobytes() == v0[2].tobytes() and pl[2].tobytes() == pl0[2].tobytes() and not loose[2].any()
    # a record without FH_CHECK_CONFLICT reverts nothing, whatever else it holds
    rec["flags"] = C | NF | BAD
    v1, pl1 = v0.copy(), pl0.copy()
    assert not cm.revert(rec, ov, opl, ms, v1, pl1).any() and v1.tobytes() == v0.tobytes() and pl1.tobytes() == pl0.tobytes()
