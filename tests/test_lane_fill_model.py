"""The cross-lane trees of the half-wave reductions and of the sliced child-bound sweep (faster_amd/csrc/fh_wave.hip.hpp,
Solver::search in fh_solve.hip.hpp), restated in numpy from their description in DESIGN.md 4g: no device needed.

A wave64 reduction on the DPP network runs row_shr 1 / 2 / 4 / 8 inside each row of 16 lanes, then row_bcast:15 (lane 15 of a row
into every lane of the next row) and row_bcast:31 (lane 31 into rows 2 and 3), and reads lane 63.  In the N = 6 and N = 10 buckets
every reduced value lives in lanes < 32 and is the identity above them, and three shorter trees replace it:

  * `half_*`: the same stages without row_bcast:31, read from lane 31;
  * `half_sum2`: the first stage on a and b, then lanes 0..31 of b moved to lanes 32..63, the remaining stages once, read from
    lanes 31 and 63;
  * the child bounds: every (polytope, control point) sweeps its rows in S contiguous slices, and a maximum over each aligned group
    of 4 S lanes joins slices and control points.

Pinned here: each of them returns the BITS of what it replaces.  Additions are IEEE double additions in the order of the tree (numpy
adds element by element with one rounding each); the sign of a zero counts."""
import numpy as np
import pytest

LANES = 64


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def row_shr(v, n, fill):
    out = np.full_like(v, fill)
    lane = np.arange(LANES)
    ok = (lane % 16) >= n
    out[..., ok] = v[..., lane[ok] - n]
    return out


def row_bcast(v, src_lane_in_pair, rows, fill):
    """row_bcast:15 (src_lane_in_pair = 15: lane 15 of row r - 1 into the rows r in `rows`) and row_bcast:31 (lane 31 into `rows`)."""
    out = np.full_like(v, fill)
    for r in rows:
        src = 16 * (r - 1) + 15 if src_lane_in_pair == 15 else 31
        out[..., 16 * r:16 * r + 16] = v[..., src:src + 1]
    return out


OPS = {"sum": (np.add, 0.0), "max": (np.maximum, 0.0), "min": (np.minimum, np.inf)}


def in_rows(v, op, fill, shifts=(1, 2, 4, 8)):
    for n in shifts:
        v = op(v, row_shr(v, n, fill))
    return v


def six_stage(v, kind):
    op, fill = OPS[kind]
    v = in_rows(v, op, fill)
    v = op(v, row_bcast(v, 15, (1, 3) if kind == "min" else (1, 2, 3), fill))  # (the min keeps rows 0 and 2: row mask 0xa)
    v = op(v, row_bcast(v, 31, (2, 3), fill))
    return v[..., 63]


def five_stage(v, kind):
    op, fill = OPS[kind]
    v = in_rows(v, op, fill)
    v = op(v, row_bcast(v, 15, (1, 3) if kind == "min" else (1, 2, 3), fill))
    return v[..., 31]


def paired_sum(a, b):
    op, fill = OPS["sum"]
    a = op(a, row_shr(a, 1, fill))
    b = op(b, row_shr(b, 1, fill))
    v = np.concatenate([a[..., :32], b[..., :32]], axis=-1)  # the half exchange: lanes 32..63 take lanes 0..31 of b
    v = in_rows(v, op, fill, shifts=(2, 4, 8))
    v = op(v, row_bcast(v, 15, (1, 2, 3), fill))
    return v[..., 31], v[..., 63]


def half_vectors(kind, seed, live):
    """[B, 64] values of the kind a call site reduces, the identity in lanes >= live (live <= 32)."""
    rng = np.random.default_rng(seed)
    B = 4000
    if kind == "sum":      # squares and absolute values: non-negative, some exact zeros, wide range of magnitudes
        v = rng.uniform(-50.0, 50.0, size=(B, LANES)) * 10.0 ** rng.integers(-8, 3, size=(B, LANES))
        v = v * v if seed % 2 else np.abs(v)
        v[rng.random((B, LANES)) < 0.1] = 0.0
    elif kind == "max":    # scaled violations: non-negative
        v = np.abs(rng.normal(size=(B, LANES)))
        v[rng.random((B, LANES)) < 0.5] = 0.0
    else:                  # step ratios: positive, INFINITY where a row does not block
        v = np.abs(rng.normal(size=(B, LANES))) + 1e-300
        v[rng.random((B, LANES)) < 0.6] = np.inf
    v[:, live:] = OPS[kind][1]
    return v


@pytest.mark.parametrize("kind", ["sum", "max", "min"])
@pytest.mark.parametrize("live", [1, 15, 16, 17, 24, 30, 32])
def test_five_stages_give_the_bits_of_six(kind, live):
    for seed in (1, 2):
        v = half_vectors(kind, seed, live)
        assert np.array_equal(bits(five_stage(v, kind)), bits(six_stage(v, kind)))
    if kind == "sum":  # the trees ARE sums of all live lanes (not vacuous), and a different order than numpy's pairwise sum
        v = half_vectors(kind, 3, live)
        assert np.allclose(five_stage(v, kind), v.sum(axis=1), rtol=1e-13, atol=0)


@pytest.mark.parametrize("live_a,live_b", [(24, 30), (30, 24), (1, 32), (32, 32), (16, 17)])
def test_paired_sum_gives_the_bits_of_two_six_stage_sums(live_a, live_b):
    a = half_vectors("sum", 11, live_a)
    b = half_vectors("sum", 12, live_b)
    sa, sb = paired_sum(a, b)
    assert np.array_equal(bits(sa), bits(six_stage(a, "sum")))
    assert np.array_equal(bits(sb), bits(six_stage(b, "sum")))
    assert not np.array_equal(bits(sa), bits(sb))


def test_what_lanes_32_to_63_hold_is_not_read():
    """The half-wave forms reduce lanes 0..31 whatever lies above: a call site only owes the identity there to the six-stage form."""
    a = half_vectors("sum", 21, 30)
    b = half_vectors("sum", 22, 24)
    dirty_a, dirty_b = a.copy(), b.copy()
    dirty_a[:, 32:] = 7.0
    dirty_b[:, 32:] = -3.0
    assert np.array_equal(bits(five_stage(dirty_a, "sum")), bits(six_stage(a, "sum")))
    for x, y in zip(paired_sum(dirty_a, dirty_b), paired_sum(a, b)):
        assert np.array_equal(bits(x), bits(y))


def test_a_negative_zero_is_where_the_precondition_matters():
    """(0 + 0) + (r1 + r0) is r1 + r0 unless r1 + r0 is -0: the call sites sum squares and absolute values, never a -0."""
    v = np.zeros((1, LANES))
    v[0, :32] = -0.0
    assert np.signbit(five_stage(v, "sum"))[0] and not np.signbit(six_stage(v, "sum"))[0]


# ---- the child-bound sweep in slices ----

def bound_sequential(vt, F, w):
    """Today's sweep: m = max(0, vt of the rows f < F) per (polytope, control point), bnd = (m w)^2, the maximum over the four
    control points of each polytope.  vt [P, 4, maxF], F [P], w [4]."""
    P, _, maxF = vt.shape
    m = np.zeros((P, 4))
    for f in range(maxF):
        take = (f < F)[:, None] & (vt[:, :, f] > m)
        m = np.where(take, vt[:, :, f], m)
    bnd = m * w[None, :]
    bnd = bnd * bnd
    out = np.zeros(P)
    for k in range(4):
        out = np.fmax(out, bnd[:, k])
    return out


def group_max(v, group):
    """The maximum over each aligned group of 8 or 16 lanes in every lane of the group: quad_perm [1,0,3,2], [2,3,0,1],
    row_half_mirror, row_mirror."""
    lane = np.arange(LANES)
    v = np.maximum(v, v[lane ^ 1])
    v = np.maximum(v, v[lane ^ 2])
    v = np.maximum(v, v[(lane & ~7) | (7 - (lane & 7))])
    if group == 16:
        v = np.maximum(v, v[(lane & ~15) | (15 - (lane & 15))])
    return v


def bound_sliced(vt, F, w):
    P, _, maxF = vt.shape
    sh = 2 if 4 * P <= 16 else 1
    S = 1 << sh
    L = (maxF + S - 1) >> sh
    bnd = np.zeros(LANES)
    for lane in range(LANES):
        pk, r = lane >> sh, lane & (S - 1)
        p, k = pk >> 2, pk & 3
        if p >= P:
            continue
        m = 0.0
        for fb in range(0, L, 4):            # trips of four rows; a trip may run past the block into the next slice's rows
            for j in range(4):
                f = r * L + fb + j
                fl = min(f, max(F[p] - 1, 0))  # the clamp to the last row of the polytope
                if f < F[p] and vt[p, k, fl] > m:
                    m = vt[p, k, fl]
        bnd[lane] = (m * w[k]) * (m * w[k])
    g = group_max(bnd, 4 * S)
    return np.array([g[p << (sh + 2)] for p in range(P)])


@pytest.mark.parametrize("P", [1, 2, 4, 5, 8])
@pytest.mark.parametrize("faces", [(1,), (5, 13), (17, 1, 5), (4, 4, 4, 4), (16, 3)])
def test_sliced_child_bound_gives_the_bits_of_the_sequential_sweep(P, faces):
    rng = np.random.default_rng(100 * P + len(faces))
    for rep in range(40):
        F = np.array([faces[(p + rep) % len(faces)] for p in range(P)])
        maxF = int(F.max())
        vt = rng.normal(size=(P, 4, maxF)) * 10.0 ** rng.integers(-3, 2)
        if rep % 4 == 1:   # the largest row twice, in different slices
            vt[:, :, 0] = vt[:, :, maxF - 1] = np.abs(vt).max(axis=2) + 0.5
        if rep % 4 == 2:   # no violated row at all: the bound is +0
            vt = -np.abs(vt)
        if rep % 4 == 3:   # maxima one ulp apart in neighbouring slices
            top = np.abs(vt).max() + 1.0
            vt[:, :, 0] = top
            vt[:, :, maxF - 1] = np.nextafter(top, np.inf)
        w = np.abs(rng.normal(size=4))
        w[rep % 4] = 0.0 if rep % 5 == 0 else w[rep % 4]  # a control point that does not depend on y
        assert np.array_equal(bits(bound_sliced(vt, F, w)), bits(bound_sequential(vt, F, w))), (P, F, rep)
