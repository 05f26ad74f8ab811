"""The row scan of solve_kernel sliced over the lanes of unassigned segments (N = 6 and N = 10 buckets), restated in
numpy from that description and held against the serial sweep of one lane per (segment, control point), bit for bit on the (id, v)
the scan returns.  No GPU: the model is the lane map of bind_assignment, the sweep of a slice, the arg-max that joins the slices of a
group, the gather to the home lane and the unchanged tail (box before corridor within a lane, lowest lane across lanes, lowest row
within a (segment, control point)).  The max-join of analyze()'s row slices is modelled at the end.

Cases: nb = 0, 1, 4, 5, 8, 9, 10 assigned segments at N = 10 and 0, 4, 5, 6 at N = 6 (every slice count and both of its edges);
maxF in {1, 4, 5, 13, 16, 17}; polytopes of 1, 5, 13 and 17 rows in one problem (rows per slice no multiple of 4, slices wholly past a
short polytope).  Planted ties: a row duplicated at both ends of a polytope (the same value in the first and the last slice),
adjacent segments in one polytope (control point 3 of t is control point 0 of t + 1 with the same weight: two home lanes score the
same), a box row and a corridor row with the same scaled violation in one lane and in two lanes."""
import itertools

import numpy as np
import pytest

K_JBOX, K_POLY = 1, 4


def mk_id(kind, t, k, f):
    return (kind << 24) | (t << 16) | (k << 8) | f


def row_value(face, cp):
    # the device evaluates fma(a0, c0, fma(a1, c1, fma(a2, c2, b))); the data below is dyadic with few bits, so every rounding is exact
    # and the plain expression has the same bits
    return face[0] * cp[0] + (face[1] * cp[1] + (face[2] * cp[2] + face[3]))


class Problem:
    """faces[f] = (a0, a1, a2, b); face_off[p]; assign[t] (-1: free); cp[t][k]; wcp[4 t + k]; tolf[f]; box candidate (bs, bv, bid) per lane"""

    def __init__(self, N, counts, assign, rng, maxF=None, duplicate_ends=False, shared_cp=True):
        self.N = N
        self.face_off = np.concatenate([[0], np.cumsum(counts)]).astype(int)
        self.maxF = int(max(counts)) if maxF is None else maxF
        assert self.maxF >= max(counts)
        nf = int(self.face_off[-1])
        self.faces = np.concatenate([rng.integers(-4, 5, size=(nf, 3)) / 4.0, rng.integers(-24, 9, size=(nf, 1)) / 8.0], axis=1)
        if duplicate_ends:
            for p, c in enumerate(counts):
                if c > 1:
                    self.faces[self.face_off[p] + c - 1] = self.faces[self.face_off[p]]
        self.tolf = rng.integers(1, 9, size=nf) / 2.0 ** 32
        self.assign = np.asarray(assign, dtype=int)
        cp = rng.integers(-8, 9, size=(N, 4, 3)) / 4.0
        if shared_cp:
            for t in range(N - 1):
                cp[t + 1, 0] = cp[t, 3]  # the end of segment t is the start of segment t + 1
        self.cp = cp
        # weights: control point 3 of t and control point 0 of t + 1 have the same row norm (both are the position at knot t + 1);
        # segment 0: control points 0..2 do not depend on the unknowns (weight 0)
        knot = rng.integers(1, 5, size=N + 1) / 2.0
        inner = rng.integers(1, 5, size=(N, 4)) / 2.0
        self.wcp = np.zeros(64)
        for t in range(N):
            for k in range(4):
                self.wcp[4 * t + k] = knot[t] if k == 0 else (knot[t + 1] if k == 3 else inner[t, k])
        self.wcp[0:3] = 0.0
        self.bs = np.zeros(64)
        self.bv = np.zeros(64)
        self.bid = np.full(64, -1, dtype=int)

    def box(self, lane, bs, bv=None):
        self.bs[lane] = bs
        self.bv[lane] = bs if bv is None else bv
        self.bid[lane] = mk_id(K_JBOX, lane // 3, lane % 3, 0)


def tail(pr, bvt, bf):
    """From `if (bf >= 0)` on: the scan's text of before the slices.  bvt, bf per home lane 4 t + k."""
    bs, bv, bid = pr.bs.copy(), pr.bv.copy(), pr.bid.copy()
    bad = False
    for lane in range(4 * pr.N):
        if bf[lane] < 0:
            continue
        t, k = lane >> 2, lane & 3
        if pr.wcp[lane] == 0.0:
            bad = True
            continue
        sc = bvt[lane] * pr.wcp[lane]
        if sc > bs[lane]:
            bs[lane], bv[lane], bid[lane] = sc, bvt[lane] + pr.tolf[pr.face_off[pr.assign[t]] + bf[lane]], mk_id(K_POLY, t, k, bf[lane])
    mx = max(0.0, bs.max())
    if not mx > 0:
        return -1, 0.0, bad
    first = int(np.flatnonzero(bs == mx)[0])
    return int(bid[first]), float(bv[first]), bad


def serial_sweep(pr):
    """One lane per (segment, control point): all maxF rows in trips of four, the index clamped to the polytope's last row, strict `>`."""
    bvt, bf = np.zeros(64), np.full(64, -1, dtype=int)
    for lane in range(4 * pr.N):
        t, k = lane >> 2, lane & 3
        p = pr.assign[t]
        if p < 0:
            continue
        f0, F = pr.face_off[p], pr.face_off[p + 1] - pr.face_off[p]
        if F == 0:
            continue
        best = 0.0
        for f in range(4 * ((pr.maxF + 3) // 4)):
            vt = row_value(pr.faces[f0 + min(f, F - 1)], pr.cp[t, k])
            if vt > best:
                best, bf[lane] = vt, f
        bvt[lane] = best
    return bvt, bf


def lane_map(pr):
    """bind_assignment: sh, L and per lane (t, k, first row r0 of the slice, rows left F, first face f0, source lane, home flag)."""
    N = pr.N
    assigned = [t for t in range(N) if pr.assign[t] >= 0]
    nb = len(assigned)
    sh = 2 if nb <= 4 else (1 if nb <= 8 else 0)
    S = 1 << sh
    L = (pr.maxF + S - 1) >> sh
    lanes = []
    for lane in range(64):
        g, r = lane >> sh, lane & (S - 1)
        j, k = g >> 2, g & 3
        on = (j < nb) if sh else (lane < 4 * N)
        t = (assigned[j] if sh else j) if on else 0
        p = pr.assign[t]
        f0t = pr.face_off[p] if p >= 0 else 0
        Ft = pr.face_off[p + 1] - f0t if p >= 0 else 0
        r0 = r * L
        live = on and r0 < Ft
        th = lane >> 2
        mine = lane < 4 * N and pr.assign[th] >= 0
        src = ((4 * assigned.index(th) + (lane & 3)) << sh) if (mine and sh) else lane
        assert 0 <= src < 64
        lanes.append(dict(t=t, k=k, r0=r0, f0=f0t + r0 if live else 0, F=Ft - r0 if live else 0, src=src, mine=mine))
    return sh, L, lanes


def sliced_sweep(pr):
    sh, L, lanes = lane_map(pr)
    v, pk = np.zeros(64), np.full(64, -1, dtype=np.int64)
    for lane, m in enumerate(lanes):
        if m["F"] == 0:
            continue  # (a dead lane starts at +inf and never takes)
        best, bf = 0.0, -1
        for f in range(4 * ((L + 3) // 4)):  # a trip past the block of L rows reads rows of the next slice
            vt = row_value(pr.faces[m["f0"] + min(f, m["F"] - 1)], pr.cp[m["t"], m["k"]])
            if vt > best:
                best, bf = vt, f
        if bf >= 0:
            v[lane], pk[lane] = best, bf * 257 + ((m["f0"] << 8) + m["r0"])  # row within the polytope | index in faces[] << 8
    assert (pk < 2 ** 31).all()
    for step in range(sh):  # quad_perm [1,0,3,2], then [2,3,0,1]
        ov, opk = v[np.arange(64) ^ (1 << step)], pk[np.arange(64) ^ (1 << step)]
        take = (ov > v) | ((ov == v) & ((opk & 0xFFFFFFFF) < (pk & 0xFFFFFFFF)))
        v, pk = np.where(take, ov, v), np.where(take, opk, pk)
    if sh:
        src = np.array([m["src"] for m in lanes])
        v, pk = v[src], pk[src]
    pk = np.where([m["mine"] for m in lanes], pk, -1)
    bf = np.where(pk >= 0, pk & 255, -1)
    f0_home = (pk >> 8) - bf
    for lane in np.flatnonzero(bf >= 0):
        assert f0_home[lane] == pr.face_off[pr.assign[lane >> 2]]  # the tail reads tolf[f0 + bf] of the home lane's polytope
    return v, bf


def check(pr):
    sv, sf = serial_sweep(pr)
    lv, lf = sliced_sweep(pr)
    taken = sf >= 0
    assert np.array_equal(sf, lf)
    assert np.array_equal(sv[taken].view(np.uint64), lv[taken].view(np.uint64))
    a, b = tail(pr, sv, sf), tail(pr, lv, lf)
    assert a[0] == b[0] and np.float64(a[1]).view(np.uint64) == np.float64(b[1]).view(np.uint64) and a[2] == b[2]
    return a


def assignment(N, nb, P, rng, spread):
    a = np.full(N, -1, dtype=int)
    which = rng.choice(N, size=nb, replace=False) if spread else np.arange(nb)
    a[which] = rng.integers(0, P, size=nb)
    return a


@pytest.mark.parametrize("N,nb", [(10, 0), (10, 1), (10, 4), (10, 5), (10, 8), (10, 9), (10, 10), (6, 0), (6, 4), (6, 5), (6, 6)])
def test_every_slice_count_and_its_edges(N, nb):
    rng = np.random.default_rng(1000 * N + nb)
    taken = 0
    for trial, dup, spread in itertools.product(range(6), (False, True), (False, True)):
        counts = list(rng.permutation([1, 5, 13, 17]))
        pr = Problem(N, counts, assignment(N, nb, 4, rng, spread), rng, duplicate_ends=dup)
        rid, _, _ = check(pr)
        taken += rid >= 0
        pr.wcp[0:3] = 1.0  # (no jerk-independent row: the corridor candidates of segment 0 compete too)
        check(pr)
    assert taken > 0 or nb == 0


@pytest.mark.parametrize("maxF", [1, 4, 5, 13, 16, 17])
@pytest.mark.parametrize("N,nb", [(10, 3), (10, 7), (10, 10), (6, 2), (6, 5)])
def test_rows_per_slice(maxF, N, nb):
    rng = np.random.default_rng(77 * maxF + N + nb)
    for trial in range(8):
        counts = [maxF] + [int(c) for c in rng.integers(1, maxF + 1, size=3)]
        pr = Problem(N, counts, assignment(N, nb, 4, rng, True), rng, duplicate_ends=bool(trial & 1))
        check(pr)
        pr = Problem(N, [max(1, maxF // 2)], assignment(N, nb, 1, rng, True), rng, maxF=maxF)  # every polytope shorter than maxF
        check(pr)


def test_duplicated_end_row_resolves_to_the_lower_row():
    rng = np.random.default_rng(5)
    hits = 0
    for N, nb, c in itertools.product((10, 6), (1, 4, 5), (5, 13, 17)):
        for trial in range(12):
            pr = Problem(N, [c], assignment(N, nb, 1, rng, True), rng, duplicate_ends=True)
            pr.wcp[:] = np.where(pr.wcp > 0, 1.0, 0.0)
            pr.wcp[0:3] = 1.0
            sv, sf = serial_sweep(pr)
            lv, lf = sliced_sweep(pr)
            assert np.array_equal(sf, lf)
            hits += int(((sf == 0) & (sv > 0)).sum())  # the duplicated row is the maximum: row 0, never row c - 1
            assert not (sf == c - 1).any() or c == 1
            check(pr)
    assert hits > 10


def test_adjacent_segments_in_one_polytope_tie_across_home_lanes():
    rng = np.random.default_rng(6)
    ties = 0
    for N, nb in ((10, 2), (10, 4), (10, 6), (10, 10), (6, 3), (6, 6)):
        for trial in range(20):
            pr = Problem(N, [13, 5], np.where(np.arange(N) < nb, 0, -1), rng)
            pr.wcp[0:3] = 1.0
            rid, _, _ = check(pr)
            sv, sf = serial_sweep(pr)
            sc = sv * pr.wcp
            for t in range(nb - 1):
                if sf[4 * t + 3] >= 0 and sc[4 * t + 3] == sc.max():
                    assert sc[4 * t + 3] == sc[4 * t + 4] and sf[4 * t + 3] == sf[4 * t + 4]
                    assert rid == mk_id(K_POLY, t, 3, sf[4 * t + 3]) or sc[:4 * t + 3].max() == sc.max()  # the lower home lane
                    ties += 1
    assert ties > 5


@pytest.mark.parametrize("where", ["same lane", "lower lane", "higher lane"])
def test_box_row_and_corridor_row_with_the_same_scaled_violation(where):
    rng = np.random.default_rng(7)
    seen = 0
    for N, nb in ((10, 1), (10, 4), (10, 5), (10, 9), (6, 2), (6, 6)):
        for trial in range(10):
            pr = Problem(N, [5, 17, 13], assignment(N, nb, 3, rng, True), rng)
            pr.wcp[0:3] = 1.0
            sv, sf = serial_sweep(pr)
            sc = np.where(sf >= 0, sv * pr.wcp, 0.0)
            if not sc.max() > 0:
                continue
            lane = int(np.flatnonzero(sc == sc.max())[0])
            box = {"same lane": lane, "lower lane": lane - 1, "higher lane": lane + 1}[where]
            if not 0 <= box < 3 * N:
                continue
            pr.box(box, sc.max(), bv=123.0)
            rid, v, _ = check(pr)
            if where == "higher lane":
                assert rid >> 24 == K_POLY
            else:
                assert rid >> 24 == K_JBOX and v == 123.0  # box before corridor within a lane, the lower lane across lanes
            seen += 1
    assert seen > 5


# ---- analyze(): the worst row of (segment, polytope) over row slices, joined by a plain maximum ----
def analyze_serial(N, P, free, need, face_off, faces, cps, maxF):
    """viol[t][p] of the sweep over all N P pairs, one lane each: -inf for an assigned segment, +inf for a polytope that is excluded."""
    out = np.full((N, P), -np.inf)
    for t, p in itertools.product(range(N), range(P)):
        if free[t] and need[t, p]:
            f0, F = face_off[p], face_off[p + 1] - face_off[p]
            out[t, p] = max(row_value(faces[f0 + min(f, max(F - 1, 0))], cps[t, k]) for f in range(4 * ((maxF + 3) // 4)) for k in range(4))
        elif free[t]:
            out[t, p] = np.inf
    return out


def analyze_sliced(N, P, free, need, face_off, faces, cps, maxF):
    """All N P pairs, S lanes per pair by their number; a pair of an assigned segment needs nothing."""
    out = np.full((N, P), np.nan)
    need = need & free[:, None]
    segs = list(range(N))
    NP = N * P
    sh = 2 if NP <= 16 else (1 if NP <= 32 else 0)
    S = 1 << sh
    L = (maxF + S - 1) >> sh
    for pair0 in range(0, NP, 64 >> sh):
        worst = np.full(64, -np.inf)
        for lane in range(64):
            pair, r0 = pair0 + (lane >> sh), (lane & (S - 1)) * L
            if pair >= NP:
                continue
            t, p = segs[pair // P], pair % P
            Fp = face_off[p + 1] - face_off[p] if need[t, p] else 0
            mine = r0 == 0 or r0 < Fp
            if not need[t, p] or not mine:
                continue
            f0, F = face_off[p] + r0, Fp - r0
            worst[lane] = max(row_value(faces[f0 + min(f, max(F - 1, 0))], cps[t, k]) for f in range(4 * ((L + 3) // 4)) for k in range(4))
        for step in range(sh):
            worst = np.maximum(worst, worst[np.arange(64) ^ (1 << step)])
        for lane in range(0, 64, S):
            pair = pair0 + (lane >> sh)
            if pair < NP:
                t, p = segs[pair // P], pair % P
                out[t, p] = np.inf if (free[t] and not need[t, p]) else worst[lane]
    assert not np.isnan(out).any()  # every (t, p < P) is written
    return out


@pytest.mark.parametrize("N,P", [(10, 1), (10, 2), (10, 3), (10, 4), (10, 6), (10, 8), (6, 1), (6, 2), (6, 3), (6, 5), (6, 6), (6, 8)])
def test_analyze_row_slices_have_the_maximum_of_the_whole_sweep(N, P):
    rng = np.random.default_rng(100 * N + P)
    for nfree in sorted({0, 1, 2, 16 // P, 16 // P + 1, 32 // P, 32 // P + 1, N - 1, N} & set(range(N + 1))):
        for trial in range(3):
            counts = [int(c) for c in rng.permutation([1, 5, 13, 17, 4, 16, 9, 2])[:P]]
            maxF = max(counts) if trial % 2 else 17
            pr = Problem(N, counts, np.full(N, -1), rng, maxF=maxF)
            free = np.zeros(N, dtype=bool)
            free[rng.choice(N, size=nfree, replace=False)] = True
            need = rng.random((N, P)) < 0.7
            a = analyze_serial(N, P, free, need, pr.face_off, pr.faces, pr.cp, maxF)
            b = analyze_sliced(N, P, free, need, pr.face_off, pr.faces, pr.cp, maxF)
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
