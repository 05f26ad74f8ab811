"""The sliced child-bound sweep and the half-wave reductions of solve_kernel (N = 6 and N = 10 buckets, fh_solve.hip.hpp)
against the oracle, where the lane maps have their edges: P = 1, 4, 5, 8 polytopes (the sweep runs four row slices while 4 P <= 16 and
two above), polytopes of 1, 5, 13 and 17 faces in one corridor (max faces no multiple of the slices, one polytope far longer than the
others), a face row duplicated at both ends of a polytope's list, 0 .. 10 pinned segments, fused pairs with lazy and complete pair
outputs, work sharing on and off, the two-wavefront build, and one N = 15 case (the untouched path).

Bars as everywhere (tests/test_gpu_parity.py): solved, trials, factor, dt, status exact; cost 1e-7 relative; coefficients 1e-6."""
import numpy as np
import pytest
import torch  # noqa: F401  (before libfasterhip.so is loaded: one HIP runtime per process)

from faster_amd import abi, capi, corridor
from test_gpu_pair_interrupts import _bytes, launch_pairs
from test_gpu_parity import compare

pytestmark = pytest.mark.gpu

COUNTS = (1, 5, 13, 17)
FIELDS = ("solved", "trials", "status", "factor", "dt", "cost", "assign")


def reshape_corridors(pr, faces, counts=COUNTS, duplicate_ends=False, seed=0):
    """Every polytope p of problem i gets counts[(p + i) % len(counts)] rows: the first rows of its own list (fewer rows: a larger
    polytope), then rows that cut nothing off (a random normal, 50 m beyond the polytope's own rows).  duplicate_ends: the first row of
    each polytope once more as its last row."""
    rng = np.random.default_rng(seed)
    out_pr, rows = pr.copy(), []
    for i in range(len(pr)):
        fb, off, P = int(pr["face_begin"][i]), pr["face_off"][i], int(pr["n_poly"][i])
        new_off = [0]
        out_pr["face_begin"][i] = len(rows)
        for p in range(P):
            own = faces[fb + off[p]:fb + off[p + 1]]
            want = counts[(p + i) % len(counts)]
            keep = [(f["a"].copy(), float(f["b"])) for f in own[:min(want, len(own))]]
            while len(keep) < want - (1 if duplicate_ends and want > 1 else 0):
                nrm = rng.normal(size=3)
                nrm /= np.linalg.norm(nrm)
                keep.append((nrm, float(np.abs(own["b"]).max() + 50.0 + 20.0 * np.abs(nrm).sum())))
            if duplicate_ends and want > 1:
                keep.append((keep[0][0].copy(), keep[0][1]))
            rows += keep
            new_off.append(new_off[-1] + len(keep))
        out_pr["face_off"][i, :P + 1] = new_off
        out_pr["face_off"][i, P + 1:] = new_off[-1]
    out = np.zeros(len(rows), dtype=abi.face_dtype)
    out["a"] = np.array([r[0] for r in rows])
    out["b"] = np.array([r[1] for r in rows])
    return out_pr, out


def pair_run(whole, faces, tmpl, n_seg, pair_outputs, wpc=0, share=1):
    c = capi.Context(0, pair_outputs=pair_outputs, compact_results=False)
    try:
        c.set_pair_margin(0.05)
        if wpc:
            c.set_sched(workgroups_per_cu=wpc)
        if not share:
            par = abi.default_params()
            par["share"] = 0
            c.set_params(par)
        out = launch_pairs(c, whole, faces, tmpl, n_seg, fill=0xAB)
        return out, c.last_launch()[1]
    finally:
        c.close()


def same_bits(a, b, n_seg):
    for f in FIELDS:
        assert np.array_equal(_bytes(a[f]), _bytes(b[f])), f
    assert np.array_equal(_bytes(a["coeff"][:, :n_seg]), _bytes(b["coeff"][:, :n_seg])), "coeff"


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("n_seg,P", [(10, 1), (10, 4), (10, 5), (10, 8), (6, 1), (6, 4), (6, 5), (6, 8)])
def test_fused_pairs_with_uneven_polytopes_against_oracle(oracle, n_seg, P):
    """128 fused pairs whose polytopes have 1, 5, 13 and 17 rows: whole results, hand-off and safe results against the oracle (complete
    pair outputs); lazy pair outputs, work sharing off and the two-wavefront build give the same bits."""
    from oracle import pair_glue

    base, bf, _ = corridor.whole_batch(128, seed=200 + 10 * n_seg + P, n_seg=n_seg, p_choices=(P,))
    whole, faces = reshape_corridors(base, bf, seed=P)
    mf = int(np.diff(whole["face_off"][:, :P + 1], axis=1).max())
    assert mf == 17 and int(np.diff(whole["face_off"][:, :P + 1], axis=1).min()) == 1
    tmpl = corridor.safe_templates(whole)
    (wres, sres, safe, sfaces), name = pair_run(whole, faces, tmpl, n_seg, True)
    assert name.startswith("fh::solve_kernel<%d, true," % n_seg)
    wref = oracle.solve_batch(whole, faces)
    okw = compare(wres, wref)
    safe_ref, _ = pair_glue.glue(whole, wref, faces, tmpl, 0.5, 0.2, 3, r_margin=0.05)
    assert np.array_equal(safe["n_seg"], safe_ref["n_seg"]) and np.array_equal(safe["n_poly"], safe_ref["n_poly"])
    live = np.flatnonzero(safe_ref["n_seg"] > 0)
    oks = compare(sres[live], oracle.solve_batch(safe[live], sfaces))
    assert okw.sum() > 16 and len(live) > 16
    print("N = %d, P = %d: %d whole solved of 128, %d safe solved of %d" % (n_seg, P, okw.sum(), oks.sum(), len(live)))
    for kw in ({"pair_outputs": False}, {"pair_outputs": True, "share": 0}, {"pair_outputs": False, "wpc": 8}):
        (w2, s2, _, _), name2 = pair_run(whole, faces, tmpl, n_seg, **kw)
        if kw.get("wpc"):
            assert name2 == "fh::solve_kernel<%d, true, 2, false>" % n_seg
        same_bits(wres, w2, n_seg)
        same_bits(sres, s2, n_seg)


@pytest.mark.parametrize("n_seg", [10, 6])
def test_a_row_duplicated_at_both_ends_of_a_polytope(ctx, oracle, n_seg):
    """The first row of every polytope once more as its last: both copies have the same violation in different row slices, and the
    bounds, the row the scan selects (the lower one) and the results are those of the oracle."""
    base, bf, _ = corridor.whole_batch(128, seed=300 + n_seg, n_seg=n_seg, p_choices=(3, 4, 5))
    whole, faces = reshape_corridors(base, bf, counts=(9, 13, 6, 17), duplicate_ends=True, seed=5)
    got = ctx.solve_batch(whole, faces)
    assert ctx.last_launch()[1].startswith("fh::solve_kernel<%d, false," % n_seg)
    ok = compare(got, oracle.solve_batch(whole, faces))
    assert ok.sum() > 32


@pytest.fixture(scope="module")
def free_n10(ctx):
    pr, faces, _ = corridor.whole_batch(48, seed=77, n_seg=10, p_choices=(2, 3, 4, 5, 6))
    return pr, faces, ctx.solve_batch(pr, faces)


@pytest.mark.parametrize("pinned", [0, 4, 5, 8, 9, 10])
def test_pinned_segments(ctx, oracle, free_n10, pinned):
    """Exactly `pinned` segments (the first ones) bound to the polytope of the free optimum: that many segments have corridor rows to
    scan at the root.  The optimum of the free search stays the optimum."""
    pr, faces, free = free_n10
    keep = np.flatnonzero(free["solved"] == 1)
    assert len(keep) >= 24
    pin = pr[keep].copy()
    for j, i in enumerate(keep):
        abi.set_pins(pin[j], [int(free["assign"][i][t]) if t < pinned else -1 for t in range(10)])
    got = ctx.solve_batch(pin, faces)
    ok = compare(got, oracle.solve_batch(pin, faces))
    assert ok.all()
    assert np.array_equal(got["assign"][:, :10], free["assign"][keep][:, :10])
    np.testing.assert_allclose(got["cost"], free["cost"][keep], rtol=1e-7, atol=1e-9)


def test_n15_bucket_is_untouched(ctx, oracle):
    pr, bf, _ = corridor.whole_batch(96, seed=15, n_seg=15, p_choices=(4, 5, 8))
    whole, faces = reshape_corridors(pr, bf, seed=15)
    got = ctx.solve_batch(whole, faces)
    assert ctx.last_launch()[1].startswith("fh::solve_kernel<15, false,")
    ok = compare(got, oracle.solve_batch(whole, faces))
    assert ok.sum() > 16
