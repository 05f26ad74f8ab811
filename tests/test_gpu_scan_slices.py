"""The row scan sliced over the lanes of unassigned segments, and analyze() on row slices (N = 6 and N = 10 buckets, fh_solve.hip.hpp,
DESIGN.md 4h), against the oracle where the lane maps have their edges: fused pairs with P = 1, 3, 4, 6, 8 polytopes of 1, 5, 13 and
17 rows (rows per slice no multiple of four, slices wholly past a short polytope; N P crosses 16 and 32), with and without a row
duplicated at both ends of every polytope; 0, 1, 4, 5, 8, 9 and all segments pinned, so that the scan runs four, two and one slice from
the first node on; lazy and complete pair outputs, work sharing off and the two-wavefront build give the same bits; one N = 15 case,
the untouched path.

Bars as everywhere (tests/test_gpu_parity.py): solved, trials, factor, dt, status exact; cost 1e-7 relative; coefficients 1e-6."""
import numpy as np
import pytest
import torch  # noqa: F401  (before libfasterhip.so is loaded: one HIP runtime per process)

from faster_amd import abi, capi, corridor
from test_gpu_lane_fill import pair_run, reshape_corridors, same_bits
from test_gpu_parity import compare

pytestmark = pytest.mark.gpu

VARIANTS = ({"pair_outputs": False}, {"pair_outputs": True, "share": 0}, {"pair_outputs": False, "wpc": 8})


def pairs_against_oracle(oracle, whole, faces, n_seg, min_solved):
    """One fused launch with complete pair outputs against the oracle (whole problems, hand-off, safe problems), then the variants."""
    from oracle import pair_glue

    tmpl = corridor.safe_templates(whole)
    (wres, sres, safe, sfaces), name = pair_run(whole, faces, tmpl, n_seg, True)
    assert name.startswith("fh::solve_kernel<%d, true," % n_seg)
    wref = oracle.solve_batch(whole, faces)
    okw = compare(wres, wref)
    safe_ref, _ = pair_glue.glue(whole, wref, faces, tmpl, 0.5, 0.2, 3, r_margin=0.05)
    assert np.array_equal(safe["n_seg"], safe_ref["n_seg"]) and np.array_equal(safe["n_poly"], safe_ref["n_poly"])
    live = np.flatnonzero(safe_ref["n_seg"] > 0)
    oks = compare(sres[live], oracle.solve_batch(safe[live], sfaces))
    print("N = %d: %d whole solved of %d, %d safe solved of %d" % (n_seg, okw.sum(), len(whole), oks.sum(), len(live)))
    assert okw.sum() >= min_solved and len(live) >= min_solved
    for kw in VARIANTS:
        (w2, s2, _, _), name2 = pair_run(whole, faces, tmpl, n_seg, **kw)
        if kw.get("wpc"):
            assert name2 == "fh::solve_kernel<%d, true, 2, false>" % n_seg
        same_bits(wres, w2, n_seg)
        same_bits(sres, s2, n_seg)
    return wres


@pytest.mark.parametrize("duplicate_ends", [False, True], ids=["plain", "dup"])
@pytest.mark.parametrize("n_seg,P", [(n, p) for n in (10, 6) for p in (1, 3, 4, 6, 8)])
def test_fused_pairs_over_the_slice_counts(oracle, n_seg, P, duplicate_ends):
    base, bf, _ = corridor.whole_batch(128, seed=400 + 10 * n_seg + P, n_seg=n_seg, p_choices=(P,))
    whole, faces = reshape_corridors(base, bf, duplicate_ends=duplicate_ends, seed=P + 1)
    rows = np.diff(whole["face_off"][:, :P + 1], axis=1)
    assert int(rows.max()) == 17 and int(rows.min()) == 1
    pairs_against_oracle(oracle, whole, faces, n_seg, 16)


@pytest.fixture(scope="module")
def free_runs(oracle):
    """Per n_seg: 128 corridors with uneven polytopes and their free optimum (the pins below fix segments to it)."""
    out = {}
    for n_seg in (10, 6):
        base, bf, _ = corridor.whole_batch(128, seed=500 + n_seg, n_seg=n_seg, p_choices=(3, 4, 5, 6))
        whole, faces = reshape_corridors(base, bf, seed=n_seg)
        c = capi.Context(0)
        try:
            out[n_seg] = (whole, faces, c.solve_batch(whole, faces))
        finally:
            c.close()
    return out


@pytest.mark.parametrize("n_seg,pinned", [(10, k) for k in (0, 1, 4, 5, 8, 9, 10)] + [(6, k) for k in (0, 1, 4, 5, 6)])
def test_fused_pairs_with_pinned_segments(oracle, free_runs, n_seg, pinned):
    """The first `pinned` segments bound to the polytope of the free optimum: that many segments have corridor rows at the root, and
    the optimum of the free search stays the optimum."""
    whole, faces, free = free_runs[n_seg]
    pin = whole.copy()
    for i in np.flatnonzero(free["solved"] == 1):
        abi.set_pins(pin[i], [int(free["assign"][i][t]) if t < pinned else -1 for t in range(n_seg)])
    wres = pairs_against_oracle(oracle, pin, faces, n_seg, 24)
    ok = free["solved"] == 1
    assert np.array_equal(wres["solved"], free["solved"])
    assert np.array_equal(wres["assign"][ok][:, :n_seg], free["assign"][ok][:, :n_seg])
    np.testing.assert_allclose(wres["cost"][ok], free["cost"][ok], rtol=1e-7, atol=1e-9)


def test_n15_bucket_is_untouched(oracle):
    pr, bf, _ = corridor.whole_batch(64, seed=16, n_seg=15, p_choices=(3, 6, 8))
    whole, faces = reshape_corridors(pr, bf, duplicate_ends=True, seed=16)
    c = capi.Context(0)
    try:
        got = c.solve_batch(whole, faces)
        assert c.last_launch()[1].startswith("fh::solve_kernel<15, false,")
    finally:
        c.close()
    assert compare(got, oracle.solve_batch(whole, faces)).sum() > 16
