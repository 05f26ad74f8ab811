"""The numpy model of the plan audit (tests/audit_model.py, the restatement of include/fasterhip_audit.h) on hand cases whose answers are
worked out by hand, and five wrong variants of the model, each of which changes the case that is named for it.  tests/test_gpu_audit.py
embeds the same cases among its plans and compares the device with the model."""
import numpy as np
import pytest

from faster_amd import abi

import audit_model as am

INF = float("inf")
# a lattice of 8 x 8 x 8 cells of 0.5 m from the origin: centres at 0.25, 0.75, ...; the one unknown voxel (2, 2, 2) has its centre at
# (1.25, 1.25, 1.25).  All numbers below are binary fractions: every d2 is exact.
GRID = ((0.0, 0.0, 0.0), 0.5, (8, 8, 8))
C = (1.25, 1.25, 1.25)


def one_voxel_view():
    f = np.zeros((1, 8 * 8 * 8), dtype=np.uint8)
    f[0, (2 * 8 + 2) * 8 + 2] = 1
    return f


def at(dx):
    return (C[0] - dx, C[1], C[2])


FAR = (3.75, 3.75, 3.75)   # d2 = 3 * 2.5^2: outside every cap used here


def hand_cases():
    """name -> (positions, params, expected fields).  Unknown side only, except "mask", which has a cloud and masks instead."""
    U, O = abi.FH_AUDIT_UNKNOWN, abi.FH_AUDIT_OCCUPIED
    none = dict(flags=0, first_unknown=-1, worst_unknown=-1, min_unknown_d2=INF)
    return {
        # dx = 0.5, d2 = 0.25 = r r: the comparison is strict, the voxel is seen and the state is not near
        "strict": ([at(0.5)], am.params(0.5, 0.5, 1.0), dict(flags=0, n_tested=1, first_unknown=-1, worst_unknown=0, min_unknown_d2=0.25)),
        # the same voxel one ulp closer: dx = 1.25 - nextafter(0.75, 1) = 0.5 - 2^-53 exactly, dx dx rounds below 0.25
        "one_ulp": ([(np.nextafter(0.75, 1.0), C[1], C[2])], am.params(0.5, 0.5, 1.0),
                    dict(flags=U, n_tested=1, first_unknown=0, worst_unknown=0, min_unknown_d2=(0.5 - 2.0 ** -53) * (0.5 - 2.0 ** -53))),
        "on_centre": ([FAR, C], am.params(0.5, 0.5, 1.0), dict(flags=U, n_tested=2, first_unknown=1, worst_unknown=1, min_unknown_d2=0.0)),
        # dx = 1 = cap: d2 = cap cap is not below it, nothing is looked at
        "at_cap": ([at(1.0)], am.params(0.5, 0.5, 1.0), dict(n_tested=1, **none)),
        # two states at dx = -0.5 and +0.5: the smaller index is the worst one
        "tie": ([FAR, at(0.5), at(-0.5)], am.params(0.75, 0.5, 1.0), dict(flags=U, n_tested=3, first_unknown=1, worst_unknown=1, min_unknown_d2=0.25)),
        # stride 5 on a plan of 3: index 0 is tested and nothing else (the near state is index 2)
        "stride_past_plan": ([FAR, FAR, C], am.params(0.5, 0.5, 1.0, stride=5), dict(n_tested=1, **none)),
        # count 3 cuts the plan of 4 in front of the near state; with stride 2 the tested indexes are 0 and 2
        "count_cuts": ([FAR, FAR, FAR, C], am.params(0.5, 0.5, 1.0, stride=2, count=3), dict(n_tested=2, **none)),
        "empty": ([], am.params(0.5, 0.5, 1.0), dict(n_tested=0, **none)),
        # 40 points, all at FAR but point 33 at dx = 0.25 of the state; the view knows point 33 alone (bit 1 of word 1)
        "mask": ([C], am.params(0.5, 0.5, 1.0), dict(flags=O, n_tested=1, first_occupied=0, worst_occupied=0, min_occupied_d2=0.0625, view=0,
                                                     first_unknown=-1, worst_unknown=-1, min_unknown_d2=INF)),
    }


def mask_case_inputs():
    cloud = np.tile(np.array(C) + 0.25 * np.arange(3), (40, 1)) + 20.0
    cloud[33] = at(0.25)
    mask = np.zeros((1, 2), dtype=np.uint32)
    mask[0, 1] = 1 << 1
    return cloud, mask


def run_case(name, variant=None):
    positions, par, _ = hand_cases()[name]
    v, pl = am.one_plan(positions)
    if name == "mask":
        cloud, mask = mask_case_inputs()
        return am.audit(par, v, pl, pl.shape[1], n_views=1, cloud=cloud, point_mask=mask, variant=variant)[0]
    return am.audit(par, v, pl, pl.shape[1], grid=GRID, flags=one_voxel_view(), n_views=1, variant=variant)[0]


def differs(rec, want):
    return [k for k, w in want.items() if not (rec[k] == w)]


@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_hand_cases(name):
    rec, want = run_case(name), hand_cases()[name][2]
    assert not differs(rec, want), (name, rec, want)
    if name != "mask":
        assert rec["view"] == 0 and rec["first_occupied"] == -1 and rec["worst_occupied"] == -1 and rec["min_occupied_d2"] == INF
    assert rec["reserved"] == 0 and not rec["reserved_d"].any()


def test_structure_flags_and_defaults():
    par = am.params(0.5, 0.5, 1.0)
    for head, size in ((-1, 2), (0, -1), (3, 2)):   # max_states = 4
        v, pl = am.one_plan([C, C], max_states=4)
        v["plan_head"], v["plan_size"] = head, size
        rec = am.audit(par, v, pl, 4, grid=GRID, flags=one_voxel_view(), n_views=1)[0]
        assert rec["flags"] == abi.FH_AUDIT_BAD_PLAN and rec["n_tested"] == 0 and rec["view"] == -1 and rec["min_unknown_d2"] == INF
    v, pl = am.one_plan([C, (np.nan, 0, 0), (np.inf, 0, 0), at(0.25)])
    rec = am.audit(par, v, pl, 4, grid=GRID, flags=one_voxel_view(), view_of=[5], n_views=1)[0]   # a view out of range: no unknown side
    assert rec["flags"] == abi.FH_AUDIT_NO_VIEW | abi.FH_AUDIT_NOT_FINITE and rec["view"] == 5 and rec["n_tested"] == 4 and rec["worst_unknown"] == -1
    rec = am.audit(par, v, pl, 4, grid=GRID, flags=one_voxel_view(), n_views=1)[0]
    assert rec["flags"] == abi.FH_AUDIT_UNKNOWN | abi.FH_AUDIT_NOT_FINITE and (rec["first_unknown"], rec["worst_unknown"]) == (0, 0)
    rec = am.audit(par, v, pl, 4)[0]   # neither side
    assert rec["flags"] == abi.FH_AUDIT_NOT_FINITE and rec["view"] == -1 and rec["n_tested"] == 4
    un, oc = abi.audit_distances(am.audit(par, *am.one_plan([at(0.5)]), 1, grid=GRID, flags=one_voxel_view(), n_views=1))
    assert un[0] == 0.5 and oc[0] == INF
    d = abi.default_audit_params(0.42)
    assert (d["r_unknown"], d["r_occupied"], d["cap"], d["stride"], d["count"]) == (0.42, 0.42, 0.84, 1, 0)


@pytest.mark.parametrize("variant,case", [("le", "strict"), ("corner", "on_centre"), ("last_on_ties", "tie"), ("floor_n_tested", "stride_past_plan"),
                                          ("mask_word_64", "mask")])
def test_a_wrong_variant_changes_its_case(variant, case):
    assert variant in am.VARIANTS
    want = hand_cases()[case][2]
    assert not differs(run_case(case), want)
    assert differs(run_case(case, variant), want), (variant, case)


def test_every_variant_is_shown_wrong():
    assert sorted(am.VARIANTS) == sorted(["le", "corner", "last_on_ties", "floor_n_tested", "mask_word_64"])
