"""The numpy restatement of the certificate (tests/certify_model.py, the model of include/fasterhip_certify.h) is worth comparing a kernel
with: the CPU oracle's results pass it at the project's own feas_tol with orders of magnitude to spare, spoiling one thing in a result
raises the number and the flag that belong to it and nothing else, and cases small enough to work out by hand give the numbers worked out."""
import numpy as np
import pytest

from faster_amd import abi, corridor

import certify_model as cm

FEAS_TOL = 1e-9   # fh_params.feas_tol
TOL = abi.certify_tol(FEAS_TOL)
C = {k: getattr(abi, "FH_CERT_" + k) for k in ("CORRIDOR", "ASSIGNMENT", "X0", "XF", "CONTINUITY", "BOX", "COST")}


@pytest.fixture(scope="module")
def solved(oracle):
    out = {}
    for name, (pr, faces, _) in (("whole", corridor.whole_batch(512, 7)), ("safe", corridor.safe_batch(512, 8)),
                                 ("n15", corridor.whole_batch(128, 9, n_seg=15, p_choices=(4, 6, 8)))):
        out[name] = (pr, faces, oracle.solve_batch(pr, faces))
    return out


def test_oracle_results_pass_at_feas_tol(solved):
    """All 1152 oracle results are solved and no defect comes near feas_tol = 1e-9: every number is below 1e-12 (relative for the cost)."""
    for name, (pr, faces, res) in solved.items():
        assert res["solved"].all(), name
        c = cm.certify(pr, faces, res, TOL)
        assert not c["flags"].any(), (name, np.nonzero(c["flags"])[0][:8])
        worst = {k: float(c[k].max()) for k in ("corridor_assigned", "corridor_best", "x0_defect", "xf_defect", "continuity_defect", "v_excess",
                                                "a_excess", "j_excess")}
        worst["cost_rel"] = float((c["cost_defect"] / np.maximum(1.0, np.abs(res["cost"]))).max())
        print(name, {k: "%.1e" % v for k, v in worst.items()})
        assert all(v < 1e-12 for v in worst.values()), (name, worst)
        assert (c["corridor_best"] <= c["corridor_assigned"]).all() and (c["worst_seg"] >= 0).all() and (c["worst_seg"] < pr["n_seg"]).all()
        assert (c["v_peak"] >= pr["v_max"] + c["v_excess"] - 1e-12).all() and (c["a_peak"] >= pr["a_max"] + c["a_excess"] - 1e-12).all()


def dense_corridor(p, faces, r):
    """corridor_assigned and corridor_best by another route: all control points against all rows as one matrix product per polytope."""
    N, Q, fb, off = int(p["n_seg"]), int(p["n_poly"]), int(p["face_begin"]), p["face_off"]
    cp = cm.control_points(np.array(r["coeff"][:N]), float(r["dt"]))
    e = np.array([[(faces["a"][fb + off[q]:fb + off[q + 1]] @ cp[t].T - faces["b"][fb + off[q]:fb + off[q + 1], None]).max() for q in range(Q)]
                  for t in range(N)])
    return max(e[t, int(r["assign"][t])] for t in range(N)), e.min(axis=1).max()


def test_one_thing_spoilt_raises_its_number_and_its_flag(solved):
    """Result 318 of the whole batch lies 0.9 m inside its corridor, 2.5 m/s below v_max and 0.05 below j_max: nothing that moves it by a
    millimetre touches a row it was not aimed at."""
    pr, faces, res = solved["whole"]
    i = 318
    p, r = pr[i], res[i]
    base = cm.certify_one(p, faces, r, TOL)
    N, dt = int(p["n_seg"]), float(r["dt"])
    assert base["flags"] == 0 and base["corridor_best"] < -0.5 and base["v_excess"] < -1.0 and int(p["n_poly"]) == 2

    def spoilt(change, own_faces=None):
        rr = r.copy()
        ff = faces if own_faces is None else own_faces
        change(rr)
        return cm.certify_one(p, ff, rr, TOL)

    def coeff(t, j, delta):
        def change(rr):
            rr["coeff"][t][j] += delta
        return change

    # a d coefficient of an inner segment: the position jumps by 1e-3 at both of its knots, nothing else moves
    c = spoilt(coeff(4, 9, 1e-3))
    assert c["flags"] == C["CONTINUITY"] and abs(c["continuity_defect"] - 1e-3) < 1e-12
    assert c["x0_defect"] == base["x0_defect"] and c["xf_defect"] == base["xf_defect"] and c["cost"] == base["cost"]
    # the c of the last segment: its velocity moves by 1e-3 at both ends (the knot before it and xf), its end position by 1e-3 dt
    c = spoilt(coeff(N - 1, 7, 1e-3))
    assert c["flags"] == C["XF"] | C["CONTINUITY"]
    assert abs(c["xf_defect"] - max(1e-3, 1e-3 * dt)) < 1e-12 and abs(c["continuity_defect"] - 1e-3) < 1e-12
    # the d of the first segment: x0 and the first knot
    c = spoilt(coeff(0, 11, -1e-3))
    assert c["flags"] == C["X0"] | C["CONTINUITY"] and abs(c["x0_defect"] - 1e-3) < 1e-12
    # the cost
    def scale(rr):
        rr["cost"] *= 1 + 1e-6
    c = spoilt(scale)
    assert c["flags"] == C["COST"] and abs(c["cost_defect"] - 1e-6 * float(r["cost"])) < 1e-9 * float(r["cost"]) and c["cost"] == base["cost"]
    # a segment assigned to the polytope it is not in: the MIQP's own feasibility does not change, the assignment's does
    rr = r.copy()
    rr["assign"][N - 1] = 0   # (the last segment ends 0.34 m outside the first polytope)
    c = cm.certify_one(p, faces, rr, TOL)
    want_assigned, want_best = dense_corridor(p, faces, rr)
    assert c["flags"] == C["ASSIGNMENT"] and c["corridor_assigned"] > 0.3 and abs(c["corridor_assigned"] - want_assigned) < 1e-12
    assert c["corridor_best"].tobytes() == base["corridor_best"].tobytes() and abs(want_best - base["corridor_best"]) < 1e-12
    # a face of polytope 1 moved inward until the end of the last segment, which lies in no other polytope, is 0.01 outside it: both
    # corridor numbers, and the worst segment is one of those assigned to that polytope
    f = int(p["face_begin"]) + int(p["face_off"][1])
    cp = cm.control_points(np.array(r["coeff"][:N]), dt)[N - 1, 3]
    moved = faces.copy()
    moved["b"][f] = float(moved["a"][f] @ cp) - 0.01
    c = spoilt(lambda rr: None, moved)
    want_assigned, want_best = dense_corridor(p, moved, r)
    assert c["flags"] == C["CORRIDOR"] | C["ASSIGNMENT"] and c["corridor_best"] >= 0.01 - 1e-12
    assert abs(c["corridor_assigned"] - want_assigned) < 1e-12 and abs(c["corridor_best"] - want_best) < 1e-12 and 5 <= c["worst_seg"] <= 9
    for k in ("x0_defect", "xf_defect", "continuity_defect", "v_excess", "a_excess", "j_excess", "v_peak", "a_peak", "cost", "cost_defect"):
        assert c[k].tobytes() == base[k].tobytes(), k
    # the bounds: each of the three rows alone
    for k, flag in (("v_max", "v_excess"), ("a_max", "a_excess"), ("j_max", "j_excess")):
        q = p.copy()
        q[k] = float(p[k] + base[flag]) - 1e-3     # 1e-3 below the largest |.| at the knots
        c = cm.certify_one(q, faces, r, TOL)
        assert c["flags"] == C["BOX"] and abs(c[flag] - 1e-3) < 1e-12, k


def one_segment(x, y, z, dt, box=(-1.0, 2.0), cost=0.0):
    pr, res = abi.make_problems(1), np.zeros(1, dtype=abi.result_dtype)
    A = np.concatenate([np.eye(3), -np.eye(3)])
    faces, off = abi.pack_faces([(A, np.concatenate([np.full(3, box[1]), -np.full(3, box[0])]))])
    pr["n_seg"], pr["n_poly"], pr["force_final_pos"] = 1, 1, 1
    pr["face_off"][0][:] = 6
    pr["face_off"][0][0] = 0
    pr["v_max"], pr["a_max"], pr["j_max"] = 1.5, 5.0, 8.0
    res["solved"], res["dt"], res["cost"] = 1, dt, cost
    res["coeff"][0][0] = np.array([x, y, z]).T.reshape(-1)   # [a b c d] per axis -> ax ay az bx by bz ...
    res["assign"][0] = -1
    res["assign"][0][0] = 0
    return pr, faces, res


def test_one_segment_worked_out_by_hand():
    """dt = 2, box [-1, 2]^3, v_max 1.5, a_max 5, j_max 8, cost reported 44, force_final_pos.  Per axis (a, b, c, d):
      x ( 1, -3,  2, 0.5 ): pos 0.5 -> 0.5, vel 2 -> 2, acc -6 -> 6, jerk 6;  cp = 0.5, (4 + 1.5)/3 = 11/6, (-12 + 8 + 1.5)/3 = -5/6, 0.5;
                            tau* = 3/3 = 1 lies inside (0, 2) and vel(1) = 3 - 6 + 2 = -1: |.| = 1 does not beat 2
      y ( 0, .5, -1, 1   ): pos 1 -> 1, vel -1 -> 1, acc 1 -> 1, jerk 0;      cp = 1, 1/3, 1/3, 1;  a = 0: no tau*
      z (-.5, 0,  0, 0.25): pos 0.25 -> -3.75, vel 0 -> -6, acc 0 -> -6, jerk -3;  cp = 0.25, 0.25, 0.25, -3.75;  tau* = -0 / -1.5 = 0: excluded
    corridor: the worst row is -z <= 1 at cp3: 3.75 - 1 = 2.75 (x: 11/6 - 2 and 5/6 - 1 = -1/6; y: -1).
    x0 = the start except pos x = 0.25 -> 0.25.  xf = the end except vel y = 0.5 -> 0.5.  N = 1 -> continuity 0.
    v_excess = 2 - 1.5, a_excess = 6 - 5, j_excess = 6 - 8.  v_peak = 6 (z at dt), a_peak = 6.  cost = 36 + 0 + 9 = 45 -> defect 1."""
    pr, faces, res = one_segment((1, -3, 2, 0.5), (0, 0.5, -1, 1), (-0.5, 0, 0, 0.25), 2.0, cost=44.0)
    pr["x0"][0] = [0.25, 1, 0.25, 2, -1, 0, -6, 1, 0]
    pr["xf"][0] = [0.5, 1, -3.75, 2, 0.5, -6, 6, 1, -6]
    c = cm.certify_one(pr[0], faces, res[0], abi.certify_tol(2.75, 0.25, 1.0, 0.03125))
    want = dict(corridor_assigned=2.75, corridor_best=2.75, x0_defect=0.25, xf_defect=0.5, continuity_defect=0.0, v_excess=0.5, a_excess=1.0,
                j_excess=-2.0, v_peak=6.0, a_peak=6.0, cost=45.0, cost_defect=1.0)
    assert {k: float(c[k]) for k in cm.NUMBERS} == want and c["worst_seg"] == 0
    assert c["flags"] == C["XF"]          # corridor, x0 and a_excess EQUAL their tolerances: `>` is strict; 1 < 0.03125 * 44
    c = cm.certify_one(pr[0], faces, res[0], abi.certify_tol(2.7, 0.2, 0.9, 0.02))
    assert c["flags"] == sum(C.values()) - C["CONTINUITY"]
    pr["force_final_pos"], pr["xf"][0][2] = 0, 100.0   # the final position is not a row of the safe trajectory
    assert cm.certify_one(pr[0], faces, res[0])["xf_defect"] == 0.5
    pr["n_poly"] = 0
    c = cm.certify_one(pr[0], faces, res[0], TOL)
    assert np.isneginf(c["corridor_best"]) and np.isneginf(c["corridor_assigned"]) and c["worst_seg"] == -1 and not c["flags"] & (C["CORRIDOR"] | C["ASSIGNMENT"])


def test_velocity_peaks_inside_the_segment_and_the_strict_ends():
    """vel = -3 tau^2 + 6 tau on (0, 2): zero at both ends, 3 at tau* = 1.  With tau* exactly 0 (b = 0) or exactly dt (a = 1, b = -3,
    dt = 1) the stationary point is an end point, excluded by 0 < tau* < dt, and v_peak is the larger end value."""
    pr, faces, res = one_segment((-1, 3, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0), 2.0)
    c = cm.certify_one(pr[0], faces, res[0])
    assert c["v_peak"] == 3.0 and c["v_excess"] == -1.5 and c["a_peak"] == 6.0
    pr, faces, res = one_segment((1, 0, -5, 0), (0, 0, 0, 0), (0, 0, 0, 0), 1.0)      # vel = 3 tau^2 - 5: -5 at tau* = 0, -2 at 1
    assert cm.certify_one(pr[0], faces, res[0])["v_peak"] == 5.0
    pr, faces, res = one_segment((1, -3, 0.5, 0), (0, 0, 0, 0), (0, 0, 0, 0), 1.0)    # vel = 3 tau^2 - 6 tau + 0.5: 0.5 at 0, -2.5 at tau* = dt = 1
    assert cm.certify_one(pr[0], faces, res[0])["v_peak"] == 2.5
    pr, faces, res = one_segment((1, -3, 0.5, 0), (0, 0, 0, 0), (0, 0, 0, 0), 1.0 + 2.0 ** -40)   # ... and a hair later it is inside
    assert cm.certify_one(pr[0], faces, res[0])["v_peak"] == 2.5 and 0 < 3.0 / 3.0 < 1.0 + 2.0 ** -40


def test_structural_flags_of_the_model():
    pr, faces, res = one_segment((1, -3, 2, 0.5), (0, 0.5, -1, 1), (-0.5, 0, 0, 0.25), 2.0)
    zero = np.zeros((), dtype=abi.certificate_dtype)

    def only(flag, p=pr[0], r=res[0], f=faces):
        c = cm.certify_one(p, f, r, TOL)
        zero["flags"] = flag
        return c.tobytes() == zero.tobytes()

    for field, v, flag in (("solved", 0, abi.FH_CERT_UNSOLVED), ("dt", 0.0, abi.FH_CERT_NOT_FINITE), ("dt", np.nan, abi.FH_CERT_NOT_FINITE)):
        r = res[0].copy()
        r[field] = v
        assert only(flag, r=r), (field, v)
    r = res[0].copy()
    r["coeff"][0][5] = np.inf
    assert only(abi.FH_CERT_NOT_FINITE, r=r)
    r = res[0].copy()
    r["coeff"][1][0] = np.nan      # a dead row
    assert cm.certify_one(pr[0], faces, r).tobytes() == cm.certify_one(pr[0], faces, res[0]).tobytes()
    r["assign"][0] = 1
    assert only(abi.FH_CERT_BAD_INPUT, r=r)
    for field, v in (("n_seg", 0), ("n_seg", 17), ("n_poly", -1), ("n_poly", 9), ("face_begin", -1), ("face_begin", 1)):
        p = pr[0].copy()
        p[field] = v
        assert only(abi.FH_CERT_BAD_INPUT, p=p), (field, v)
    p = pr[0].copy()
    p["face_off"][0] = 1
    assert only(abi.FH_CERT_BAD_INPUT, p=p)
    p = pr[0].copy()
    p["n_poly"], p["face_off"][1], p["face_off"][2] = 2, 6, 5
    assert only(abi.FH_CERT_BAD_INPUT, p=p)
