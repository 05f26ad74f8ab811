"""Inputs for the tests of a solve launch at its edges (tests/test_solve_edges_oracle.py proves them on the CPU oracle,
tests/test_gpu_solve_edges.py sends them to the kernels): the table of unusable records, the factor-window boundary, batches at the
borders of the 6 / 10 / 15 / 16 kernel builds and batches with an exact number of face rows.  numpy only; every seed is a constant."""
import numpy as np

from faster_amd import abi, corridor

INT32_MIN, INT32_MAX = -(2**31), 2**31 - 1
FH_MAX_TRIALS = 4096  # faster_amd/csrc/fh_solve.hip.hpp; the oracle's bad_input() carries the same number


# ---- the header's rule, restated (include/fasterhip.h: field comments of fh_problem, FH_MAX_*, FH_ST_BAD_INPUT) --------------------
def header_says_bad(p):
    """Is record p unusable by what include/fasterhip.h says about its fields?  n_seg in 1..FH_MAX_SEG, n_poly in 0..FH_MAX_POLY,
    polytope q owns the rows [face_begin + face_off[q], face_begin + face_off[q + 1]) of the batch face array — so face_off[0] = 0,
    face_begin >= 0, no polytope has a negative number of rows or more than FH_MAX_FACES_POLY, the problem no more than FH_MAX_FACES —,
    a factor window `for (f = f_init; f <= f_final; f += f_inc)` that ends (f_inc > 0, finite ends) after at most FH_MAX_TRIALS steps,
    positive dc and bounds (+inf is a bound), finite x0 and xf, and pins that name a segment and a polytope of the problem.  Fields that
    the record does not use (face_off beyond n_poly, reserved) say nothing."""
    n_seg, n_poly = int(p["n_seg"]), int(p["n_poly"])
    if not 1 <= n_seg <= abi.FH_MAX_SEG or not 0 <= n_poly <= abi.FH_MAX_POLY:
        return True
    off = [int(v) for v in p["face_off"]]
    if off[0] != 0 or int(p["face_begin"]) < 0:
        return True
    counts = [off[q + 1] - off[q] for q in range(n_poly)]
    if any(c < 0 or c > abi.FH_MAX_FACES_POLY for c in counts) or (n_poly and off[n_poly] > abi.FH_MAX_FACES):
        return True
    f_init, f_final, f_inc = float(p["f_init"]), float(p["f_final"]), float(p["f_inc"])
    if not f_inc > 0 or not np.isfinite(f_init) or not np.isfinite(f_final):
        return True
    if (f_final - f_init) / f_inc > FH_MAX_TRIALS:
        return True
    if any(not float(p[k]) > 0 for k in ("dc", "v_max", "a_max", "j_max")):
        return True
    if not np.isfinite(p["x0"]).all() or not np.isfinite(p["xf"]).all():
        return True
    pins = int(p["pin"][0]) | (int(p["pin"][1]) << 32)
    for t in range(abi.FH_MAX_SEG):
        v = (pins >> (4 * t)) & 15
        if v and (t >= n_seg or v > n_poly):
            return True
    return False


# ---- rows ----------------------------------------------------------------------------------------------------------------------------
def polys_of(p, faces):
    fb = int(p["face_begin"])
    return [(faces["a"][fb + p["face_off"][q]: fb + p["face_off"][q + 1]].copy(), faces["b"][fb + p["face_off"][q]: fb + p["face_off"][q + 1]].copy())
            for q in range(int(p["n_poly"]))]


def pad_poly(A, b, rows, rng):
    """The polytope (A, b) with `rows` rows: scaled copies of its own rows, moved outwards by up to 0.5 m — the same set
    (tests/test_gpu_parity.py::test_many_faces_and_degenerate_rows pads this way)."""
    extra = rows - len(b)
    assert extra >= 0
    if extra == 0:
        return A, b
    idx = rng.integers(0, len(b), size=extra)
    s = rng.uniform(0.5, 2.0, size=extra)
    return np.vstack([A, A[idx] * s[:, None]]), np.concatenate([b, b[idx] * s + rng.uniform(0, 0.5, size=extra)])


def with_polys(p, polys):
    """(record, rows): a copy of record p whose corridor is `polys`, rows from 0."""
    f, off = abi.pack_faces(polys)
    q = np.array([p], dtype=abi.problem_dtype)
    q["n_poly"] = len(polys)
    q["face_begin"] = 0
    q["face_off"][0, : len(off)] = off
    q["face_off"][0, len(off):] = off[-1]
    return q, f


def padded_to(p, faces, total, rng):
    """Record p with exactly `total` rows: every polytope padded, none beyond FH_MAX_FACES_POLY; None if the corridor cannot have that
    many (or has more already)."""
    polys = polys_of(p, faces)
    have = [len(b) for _, b in polys]
    if not polys or sum(have) > total or total > abi.FH_MAX_FACES_POLY * len(polys):
        return None
    want = list(have)
    k = 0
    while sum(want) < total:  # round robin, so that no polytope exceeds its cap before the others are full
        if want[k % len(want)] < abi.FH_MAX_FACES_POLY:
            want[k % len(want)] += 1
        k += 1
    return with_polys(p, [pad_poly(A, b, w, rng) for (A, b), w in zip(polys, want)])


# ---- the table of unusable records -----------------------------------------------------------------------------------------------------
TABLE_SEED = 20241
BASE_SEEDS = (911, 918)  # corridor.whole_batch seeds of the two base problems (4 and 8 polytopes, N = 10); record 0 of each


def bad_record_table(seed=TABLE_SEED):
    """(problems, faces, rows) — rows[i] is a dict: name, bad (the expected class), twin (index of the record whose result a good clone
    must repeat BIT FOR BIT, or None for the two base records) and skip (result fields left out of that comparison, with the reason
    below; the work counters nodes / qp_iters / kflops are never part of it outside the oracle, they count who did what).

    Two good base problems (N = 10; 4 and 8 polytopes — 4 x 64 and 8 x 32 rows need corridors of those sizes), each clause of
    bad_scalars / bad_corridor violated in exactly one clone of the first, and clones that must stay good and give their base's result:
      * garbage in unused fields, a window of exactly FH_MAX_TRIALS steps (the base is solved by an early factor): nothing a solve reads
        has changed;
      * padded corridors: the same sets, the extra rows strictly outside them — never active, so the iterates are the base's.  `assign`
        is left out for polytope 0 padded to 64 rows: where two polytopes overlap a segment may sit in either, and more rows change which
        one the branching tries first (the oracle itself answers with another, equally valid, assignment);
      * v_max = +inf: the base's speed bound is not active at its optimum and does not decide its time allocation;
      * an empty polytope (zero rows: all of space) inserted into the corridor: the optimum of the base stays optimal — the base's cost
        is reached again —, but the polytopes behind the empty one are renumbered and a segment may sit in the empty one: `assign` is
        left out (tests/test_gpu_parity.check_assignment_valid holds it instead).
    Every record has rows of its own inside the face array (face_begin >= 0, all of its claimed rows exist) except the one whose clause
    is face_begin < 0.  Bad and good records alternate: every bad record has good neighbours."""
    rng = np.random.default_rng(seed)
    b4p, b4f, _ = corridor.whole_batch(1, seed=BASE_SEEDS[0], n_seg=10, p_choices=(4,))
    b8p, b8f, _ = corridor.whole_batch(1, seed=BASE_SEEDS[1], n_seg=10, p_choices=(8,))
    base, base8 = with_polys(b4p[0], polys_of(b4p[0], b4f)), with_polys(b8p[0], polys_of(b8p[0], b8f))
    P = int(base[0]["n_poly"][0])

    def clone(src=base, **fields):
        q, f = src[0].copy(), src[1].copy()
        for k, v in fields.items():
            q[k][0] = v
        return q, f

    def at(field, i, v, src=base):
        q, f = clone(src)
        q[field][0, i] = v
        return q, f

    bad = []
    for v in (0, -1, abi.FH_MAX_SEG + 1):
        bad.append(("n_seg = %d" % v, clone(n_seg=v)))
    for v in (-1, abi.FH_MAX_POLY + 1):
        bad.append(("n_poly = %d" % v, clone(n_poly=v)))
    bad.append(("face_off[0] = 1", at("face_off", 0, 1)))
    bad.append(("face_begin = -1", clone(face_begin=-1)))
    bad.append(("polytope 1 with -1 rows", at("face_off", 2, int(base[0]["face_off"][0, 1]) - 1)))
    polys = polys_of(base[0][0], base[1])
    bad.append(("polytope 0 with 65 rows", with_polys(base[0][0], [pad_poly(*polys[0], abi.FH_MAX_FACES_POLY + 1, rng)] + polys[1:])))
    polys8 = polys_of(base8[0][0], base8[1])
    bad.append(("257 rows", with_polys(base8[0][0], [pad_poly(A, b, w, rng) for (A, b), w in zip(polys8, [32] * 7 + [33])])))
    for v in (0.0, -1.0, np.nan):
        bad.append(("f_inc = %r" % v, clone(f_inc=v)))
    for v in (np.inf, -np.inf, np.nan):
        bad.append(("f_init = %r" % v, clone(f_init=v)))
    for v in (np.nan, np.inf):
        bad.append(("f_final = %r" % v, clone(f_final=v)))
    bad.append(("window of one ulp more than 4096 steps", clone(f_init=1.0, f_inc=1.0, f_final=float(np.nextafter(4097.0, np.inf)))))
    for k in ("dc", "v_max", "a_max", "j_max"):
        for v in (0.0, -1.0, np.nan):
            bad.append(("%s = %r" % (k, v), clone(**{k: v})))
    for k in ("x0", "xf"):
        for i in range(9):
            bad.append(("%s[%d] = nan" % (k, i), at(k, i, np.nan)))
    bad.append(("x0[2] = inf", at("x0", 2, np.inf)))
    q, f = clone()
    abi.set_pins(q[0], [-1] * 10 + [0])
    bad.append(("pin on segment 10 of 10", (q, f)))
    q, f = clone()
    abi.set_pins(q[0], [P])
    bad.append(("pin to polytope %d of %d" % (P, P), (q, f)))

    good = []  # (name, (record, rows), twin: 0 = base, 1 = base8; skip)
    for k in range(4):
        q, f = clone()
        q["face_off"][0, P + 1:] = rng.choice([INT32_MIN, INT32_MAX, -1], size=abi.FH_MAX_POLY - P)
        q["reserved"][0] = rng.choice([INT32_MIN, INT32_MAX, -1])
        good.append(("garbage in unused fields (%d)" % k, (q, f), 0, ()))
    good.append(("window of exactly 4096 steps", clone(f_init=1.0, f_inc=1.0, f_final=4097.0), 0, ()))
    good.append(("polytope 0 with 64 rows", with_polys(base[0][0], [pad_poly(*polys[0], abi.FH_MAX_FACES_POLY, rng)] + polys[1:]), 0, ("assign",)))
    good.append(("256 rows as 4 x 64", with_polys(base[0][0], [pad_poly(A, b, 64, rng) for A, b in polys]), 0, ()))
    good.append(("256 rows as 8 x 32", with_polys(base8[0][0], [pad_poly(A, b, 32, rng) for A, b in polys8]), 1, ()))
    good.append(("v_max = inf", clone(v_max=np.inf), 0, ()))
    empty = (np.zeros((0, 3)), np.zeros(0))
    good.append(("a zero-row polytope inside the corridor", with_polys(base[0][0], polys[:2] + [empty] + polys[2:]), 0, ("assign",)))

    recs = [("base", base, False, None, ()), ("base, 8 polytopes", base8, False, None, ())]
    for k, (name, rec) in enumerate(bad):
        g = good[k % len(good)] if k < 2 * len(good) else ("base again", clone(), 0, ())
        recs.append((g[0], g[1], False, g[2], g[3]))
        recs.append((name, rec, True, None, ()))
    recs.append(("base at the end", clone(), False, 0, ()))
    rows = [dict(name=name, bad=is_bad, twin=twin, skip=skip) for name, _, is_bad, twin, skip in recs]
    pr, faces = corridor.concat([rec for _, rec, _, _, _ in recs])
    i = [r["name"] for r in rows].index("face_begin = -1")
    pr["face_begin"][i] = -1  # (concat rebased it into the array)
    return pr, faces, rows


def window_boundary_problems():
    """Two records whose every trial is refuted at the root (initial speed 7 m/s along x against v_max = 5: record 1 of
    tests/test_gpu_parity.py::test_edge_cases): a window of exactly FH_MAX_TRIALS steps — 4097 trials, FH_ST_INFEASIBLE — and the same
    with f_final one ulp further: FH_ST_BAD_INPUT."""
    pr, faces, _ = corridor.whole_batch(2, seed=21)
    pr = pr.copy()
    pr[1] = pr[0]
    pr["x0"][:, 3] = 7.0
    pr["f_init"], pr["f_inc"] = 1.0, 1.0
    pr["f_final"][0] = 4097.0
    pr["f_final"][1] = np.nextafter(4097.0, np.inf)
    assert (pr["f_final"][0] - pr["f_init"][0]) / pr["f_inc"][0] == 4096.0
    return pr, faces


# ---- batches at the borders of the kernel builds -------------------------------------------------------------------------------------
BORDER_N = (1, 2, 3, 5, 6, 7, 9, 10, 11, 14, 15, 16)
BORDER_SIZE = 32


def border_cannot_be_half_solved(n_seg, force, n_poly):
    """Groups in which the oracle cannot solve half; they are run all the same, for their statuses.  A whole problem (force_final_pos
    = 1) fixes position, velocity and acceleration at the end: 9 equations on 3 n_seg jerks.  n_seg <= 2 has no trajectory at all unless
    x0 happens to allow one (a safe problem fixes final velocity and acceleration only: 6 equations, too many for n_seg = 1, solvable
    from n_seg = 2 on).  n_seg = 3 has exactly ONE trajectory per factor: it stays inside a corridor of up to three polytopes in more
    than half of the generator's problems (0.56 over 41 seeds), of four in a sixth (best of 41 seeds: 0.28), of five or more in none."""
    return n_seg == 1 or (force == 1 and n_seg == 2) or (force == 1 and n_seg == 3 and n_poly >= 4)


# (n_seg, force_final_pos, n_poly) -> seed where the default seed gives a group of which less than half is solvable although other
# seeds do: whole problems of 5 segments in 8 polytopes are solved for 0.41 of the seeds' median batch (0.38 with the default seed)
BORDER_SEEDS = {(5, 1, 8): 9036}


def border_group(n_seg, force, n_poly):
    """One group: BORDER_SIZE problems of n_seg segments and n_poly polytopes (n_poly = 0: a corridor of one polytope, its rows unused)"""
    seed = BORDER_SEEDS.get((n_seg, force, n_poly), 7000 + 100 * n_seg + 10 * force + n_poly)
    pr, faces, _ = corridor.make_batch(BORDER_SIZE, n_seg, (max(n_poly, 1),), bool(force), seed)
    pr = pr.copy()
    if n_poly == 0:
        pr["n_poly"] = 0
    return pr, faces


def border_batches():
    """[(n_seg, force_final_pos, n_poly, problems, faces)] for every n_seg of BORDER_N (the builds hold 6, 10, 15 and 16 segments: each
    border, one below, one above, and small problems in a large build), both kinds of problem and n_poly = 0 .. FH_MAX_POLY — every
    corridor the generator makes, the groups of border_cannot_be_half_solved included."""
    return [(n, force, P) + border_group(n, force, P) for n in BORDER_N for force in (0, 1) for P in range(abi.FH_MAX_POLY + 1)]


def build_of(n_seg):
    """segments of the kernel build that max_seg = n_seg selects (fh_solve_batch_device)"""
    return 6 if n_seg <= 6 else (10 if n_seg <= 10 else (15 if n_seg <= 15 else 16))


# ---- batches with an exact number of rows ------------------------------------------------------------------------------------------------
FACE_ROWS = (8, 9, 15, 16, 17, 63, 64, 65, 255, 256)
FACE_SIZE = 32


def face_cap_group(rows, n_seg):
    """(padded problems, padded rows, unpadded problems, unpadded rows): FACE_SIZE whole problems of n_seg segments with exactly `rows`
    rows each.  The generator gives a polytope 9-15 rows: up to 17 rows are ONE polytope cut to its first rows - 2 rows (its box and some
    of its planes: another corridor — the unpadded twin is cut the same way) and padded by two or more, 63-65 rows two to four
    polytopes, 255 / 256 four to eight."""
    seed = 8000 + 16 * rows + n_seg
    rng = np.random.default_rng(seed)
    p_choices = (1,) if rows <= 17 else ((2, 3, 4) if rows <= 65 else tuple(p for p in (4, 5, 6, 7, 8) if p <= max(n_seg - 2, 4)))
    pr, faces, _ = corridor.whole_batch(4 * FACE_SIZE, seed=seed, n_seg=n_seg, p_choices=p_choices)
    padded, plain = [], []
    for i in range(len(pr)):
        p = pr[i]
        polys = polys_of(p, faces)
        if rows <= 17:  # at least two rows of padding
            polys = [(A[:rows - 2], b[:rows - 2]) for A, b in polys]
        q0 = with_polys(p, polys)
        q1 = padded_to(q0[0][0], q0[1], rows, rng)
        if q1 is None:
            continue
        padded.append(q1)
        plain.append(q0)
        if len(padded) == FACE_SIZE:
            break
    assert len(padded) == FACE_SIZE, (rows, n_seg, len(padded))
    return corridor.concat(padded) + corridor.concat(plain)


def rows_of(pr):
    return pr["face_off"][np.arange(len(pr)), np.clip(pr["n_poly"], 0, abi.FH_MAX_POLY)] * (pr["n_poly"] > 0)
