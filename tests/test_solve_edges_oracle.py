"""The inputs of tests/test_gpu_solve_edges.py (tests/solve_edge_cases.py), proved on the CPU oracle alone: each record of the table of
unusable records is what it claims to be — a restatement of the rule of include/fasterhip.h agrees with the oracle on every row —, the
factor window of exactly FH_MAX_TRIALS steps is accepted and the next ulp refused, and the batches at the borders of the kernel builds
and at the face caps are mostly solvable, so that what the kernels are compared on is trajectories and not a column of INFEASIBLE."""
import time

import numpy as np

import solve_edge_cases as sec
from faster_amd import abi

RESULT_FIELDS = ("solved", "trials", "status", "factor", "dt", "cost", "coeff", "assign")  # everything but the work counters


def compare(got, ref, cost_rtol=1e-7, coeff_atol=1e-6):
    """the bars of the suite (tests/test_gpu_parity.py::compare; that module is GPU-only, hence restated)"""
    for f in ("status", "solved", "trials", "factor", "dt"):
        assert np.array_equal(got[f], ref[f]), f
    ok = ref["solved"] == 1
    np.testing.assert_allclose(got["cost"][ok], ref["cost"][ok], rtol=cost_rtol, atol=1e-9)
    np.testing.assert_allclose(got["coeff"][ok], ref["coeff"][ok], rtol=0, atol=coeff_atol)


def test_table_rule_of_the_header_equals_the_oracle_on_every_record(oracle):
    pr, faces, rows = sec.bad_record_table()
    ref = oracle.solve_batch(pr, faces)
    names = [r["name"] for r in rows]
    for i, r in enumerate(rows):
        assert sec.header_says_bad(pr[i]) == r["bad"], r["name"]
        assert (ref["status"][i] == abi.FH_ST_BAD_INPUT) == r["bad"], r["name"]
    # every clause is there (the count per kind: three n_seg, two n_poly, ... eighteen NaN words and one inf)
    bad = [r["name"] for r in rows if r["bad"]]
    assert len(bad) == len(set(bad)) == 3 + 2 + 1 + 1 + 1 + 1 + 1 + 3 + 3 + 2 + 1 + 12 + 18 + 1 + 2
    # an unusable record is reported as zeros, status BAD_INPUT, no assignment
    blank = np.zeros(1, dtype=abi.result_dtype)
    blank["status"], blank["assign"] = abi.FH_ST_BAD_INPUT, -1
    for i in np.flatnonzero([r["bad"] for r in rows]):
        assert ref[i: i + 1].tobytes() == blank.tobytes(), names[i]
        assert not rows[i - 1]["bad"] and not rows[i + 1]["bad"], names[i]
    # rows of its own for every record, inside the array (the kernel cannot see n_faces) — except the clause face_begin < 0 itself
    for i, r in enumerate(rows):
        p = pr[i]
        if r["name"] == "face_begin = -1":
            assert p["face_begin"] == -1
            continue
        claimed = max([int(v) for v in p["face_off"][: int(np.clip(p["n_poly"], 0, abi.FH_MAX_POLY)) + 1]] + [0])
        assert 0 <= p["face_begin"] and p["face_begin"] + claimed <= len(faces), r["name"]
    # the good clones: the base problems are solved, by an early factor (so that a longer window changes nothing)
    assert ref["solved"][0] == 1 and ref["solved"][1] == 1 and ref["trials"][0] < 10 and ref["nodes"][1] > 10
    seen = set()
    for i, r in enumerate(rows):
        if r["bad"]:
            continue
        seen.add(r["name"].split(" (")[0])
        assert ref["solved"][i] == 1, r["name"]
        if r["twin"] is None:
            continue
        # a good clone gives its base's result bit for bit (solve_edge_cases.bad_record_table says why `assign` is left out of two)
        for f in RESULT_FIELDS:
            if f not in r["skip"]:
                assert ref[f][i].tobytes() == ref[f][r["twin"]].tobytes(), (r["name"], f)
        if r["name"].startswith(("garbage", "window", "base")):  # nothing a solve reads has changed: the same work, too
            assert ref[i: i + 1].tobytes() == ref[r["twin"]: r["twin"] + 1].tobytes(), r["name"]
    assert sum(1 for r in rows if r["skip"]) == 4 and all(r["skip"] == ("assign",) for r in rows if r["skip"])  # (each of the two, twice)
    assert {"garbage in unused fields", "window of exactly 4096 steps", "polytope 0 with 64 rows", "256 rows as 4 x 64", "256 rows as 8 x 32",
            "v_max = inf", "a zero-row polytope inside the corridor"} <= seen
    i = names.index("256 rows as 8 x 32")
    assert pr["n_poly"][i] == 8 and list(np.diff(pr["face_off"][i])) == [32] * 8
    i = names.index("256 rows as 4 x 64")
    assert pr["n_poly"][i] == 4 and list(np.diff(pr["face_off"][i])[:4]) == [64] * 4
    i = names.index("a zero-row polytope inside the corridor")
    assert pr["n_poly"][i] == 5 and pr["face_off"][i][2] == pr["face_off"][i][3]
    i = names.index("257 rows")
    assert pr["face_off"][i][8] == 257 and np.diff(pr["face_off"][i]).max() <= abi.FH_MAX_FACES_POLY
    i = names.index("garbage in unused fields (0)")
    assert pr["reserved"][i] in (sec.INT32_MIN, sec.INT32_MAX, -1) and set(pr["face_off"][i][5:]) <= {sec.INT32_MIN, sec.INT32_MAX, -1}


def test_window_of_4096_steps_is_accepted_and_the_next_ulp_refused(oracle):
    pr, faces = sec.window_boundary_problems()
    assert (pr["f_final"][0] - pr["f_init"][0]) / pr["f_inc"][0] == 4096.0 < (pr["f_final"][1] - pr["f_init"][1]) / pr["f_inc"][1]
    t0 = time.time()
    ref = oracle.solve_batch(pr, faces)
    print("4097 trials on the oracle: %.3f s" % (time.time() - t0))  # (milliseconds; what proves "refuted at the root" is asserted below)
    assert ref["trials"][0] == 4097 and ref["status"][0] == abi.FH_ST_INFEASIBLE and ref["solved"][0] == 0
    assert ref["nodes"][0] <= 4097 and ref["qp_iters"][0] == 0  # every trial refuted at its root, without an iteration
    assert ref["status"][1] == abi.FH_ST_BAD_INPUT and ref["trials"][1] == 0
    assert not sec.header_says_bad(pr[0]) and sec.header_says_bad(pr[1])


def test_border_batches_are_mostly_solvable(oracle):
    groups = sec.border_batches()
    assert {(n, f) for n, f, _, _, _ in groups} == {(n, f) for n in sec.BORDER_N for f in (0, 1)}
    for n, force, P, pr, faces in groups:
        assert 32 <= len(pr) <= 64 and (pr["n_seg"] == n).all() and (pr["n_poly"] == P).all() and (pr["force_final_pos"] == force).all()
        ref = oracle.solve_batch(pr, faces)
        assert not (ref["status"] == abi.FH_ST_BAD_INPUT).any()
        if sec.border_cannot_be_half_solved(n, force, P):
            assert ref["solved"].mean() < 0.5, (n, force, P)  # (named because it cannot hold — not because it was convenient)
        else:
            assert ref["solved"].mean() >= 0.5, (n, force, P, ref["solved"].mean())
    assert not any(sec.border_cannot_be_half_solved(n, f, P) for n in sec.BORDER_N for f in (0, 1) for P in range(9) if n >= 5 or (n >= 2 and f == 0))
    assert len(groups) == len(sec.BORDER_N) * 2 * (abi.FH_MAX_POLY + 1)
    assert [sec.build_of(n) for n in sec.BORDER_N] == [6, 6, 6, 6, 6, 10, 10, 10, 15, 15, 15, 16]


def test_face_cap_batches_have_exact_rows_and_equal_their_unpadded_twins(oracle):
    for rows in sec.FACE_ROWS:
        for n_seg in (6, 10, 15, 16):
            pr, faces, pr0, faces0 = sec.face_cap_group(rows, n_seg)
            assert len(pr) == sec.FACE_SIZE and (sec.rows_of(pr) == rows).all() and (sec.rows_of(pr0) < rows).all()
            assert np.diff(pr["face_off"], axis=1).max() <= abi.FH_MAX_FACES_POLY
            assert not any(sec.header_says_bad(p) for p in pr)
            ref, ref0 = oracle.solve_batch(pr, faces), oracle.solve_batch(pr0, faces0)
            assert ref["solved"].mean() >= 0.5, (rows, n_seg)
            compare(ref, ref0)
