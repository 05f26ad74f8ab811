"""The half-wave split of compute_states (jerks) and moments() (states) in the N = 6 and N = 10 buckets of solve_kernel (3 NSEG <= 32:
lanes l and l + 32 share the sum of row l, fh_solve.hip.hpp), against the oracle where the split has its edges: K = 7 (whole) and
K = 8 (safe) reduced unknowns per axis at N = 10 — an odd and an even tail of the even / odd split of the jerks —, K = 0 .. 4 in the
N = 6 bucket (a half without terms; at N = 3 whole nothing to split at all) with n_seg below the bucket's NSEG (the upper half of
moments() sums segments that do not exist), the two-wavefront build of the same source bit for bit, the N = 15 bucket that keeps the
unsplit code, and problems with every segment pinned, whose corridor rows reach from the first state (tt = 1) to the last (tt = N):
the first and the last row of the new lane map of the states.

Bars as everywhere (tests/test_gpu_parity.py): solved, trials, factor, dt, status exact; cost 1e-7 relative; coefficients 1e-6."""
import numpy as np
import pytest
import torch  # noqa: F401  (before libfasterhip.so is loaded: one HIP runtime per process)

from faster_amd import abi, capi, corridor
from test_gpu_pair_interrupts import _bytes, launch_pairs
from test_gpu_parity import compare
from test_gpu_round3 import fused_pairs

pytestmark = pytest.mark.gpu

N10_PAIRS = 512
DUMP_FIELDS = ("solved", "trials", "status", "factor", "dt", "cost")   # what bench.py --dump-outputs compares (its DUMP_FIELDS)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def n10_batch():
    whole, faces, _ = corridor.whole_batch(N10_PAIRS, seed=11, n_seg=10, p_choices=(2, 3, 4, 5, 6))
    return whole, faces, corridor.safe_templates(whole)


def test_n10_fused_pairs_whole_and_safe_against_oracle(ctx, oracle, n10_batch):
    """512 fused pairs at N = 10: the whole problems (K = 7), the hand-off and the safe problems (K = 8) against the oracle."""
    from oracle import pair_glue

    whole, faces, tmpl = n10_batch
    wres, sres, safe, sfaces = fused_pairs(ctx, whole, faces, tmpl, 10, 0.05)
    assert ctx.last_launch()[1].startswith("fh::solve_kernel<10, true,")
    wref = oracle.solve_batch(whole, faces)
    okw = compare(wres, wref)
    safe_ref, _ = pair_glue.glue(whole, wref, faces, tmpl, 0.5, 0.2, 3, r_margin=0.05)
    assert np.array_equal(safe["n_seg"], safe_ref["n_seg"]) and np.array_equal(safe["n_poly"], safe_ref["n_poly"])
    np.testing.assert_allclose(safe["x0"], safe_ref["x0"], rtol=0, atol=1e-9)
    live = np.flatnonzero(safe_ref["n_seg"] > 0)
    oks = compare(sres[live], oracle.solve_batch(safe[live], sfaces))
    # both tails of the split: whole problems (final position fixed: K = N - 3 = 7) and safe ones (K = N - 2 = 8), solved ones of each
    assert (whole["n_seg"] == 10).all() and (whole["force_final_pos"] == 1).all() and okw.sum() > N10_PAIRS // 2
    assert (safe["n_seg"][live] == 10).all() and (safe["force_final_pos"][live] == 0).all() and oks.sum() > N10_PAIRS // 8
    print("N = 10: %d whole solved of %d, %d safe solved of %d" % (okw.sum(), N10_PAIRS, oks.sum(), len(live)))


@pytest.mark.parametrize("n_seg", [3, 4, 5, 6])
def test_n6_bucket_against_oracle(ctx, oracle, n_seg):
    """solve_kernel<6, false, ..>, plain launch: K = n_seg - 3 = 0 .. 3 (final position fixed, as in a whole problem) and
    K = n_seg - 2 = 1 .. 4 (final position free, as in a safe one)."""
    whole, faces, _ = corridor.whole_batch(256, seed=40 + n_seg, n_seg=n_seg, p_choices=(1, 2, 3))
    pr = whole.copy()
    pr["force_final_pos"][1::2] = 0   # every other problem with the final position free: the other K of this n_seg
    got = ctx.solve_batch(pr, faces)
    assert ctx.last_launch()[1].startswith("fh::solve_kernel<6, false,")
    ok = compare(got, oracle.solve_batch(pr, faces))
    assert ok[0::2].sum() > 0 and ok[1::2].sum() > 0
    print("N = %d: %d of 256 solved (%d with the final position free)" % (n_seg, ok.sum(), ok[1::2].sum()))


def test_n10_two_wavefront_build_gives_the_same_bits(n10_batch):
    """fh_sched.workgroups_per_cu = 8 selects solve_kernel<10, true, 2, false>, the same source compiled for two wavefronts per SIMD:
    every dumped field, the coefficients and the assignment of every pair equal those of the default build, bit for bit."""
    whole, faces, tmpl = n10_batch
    out, names = {}, {}
    for wpc in (0, 8, 12):
        c = capi.Context(0, pair_outputs=True, compact_results=False)
        try:
            c.set_pair_margin(0.05)
            if wpc:
                c.set_sched(workgroups_per_cu=wpc)
            out[wpc] = launch_pairs(c, whole, faces, tmpl, 10, fill=0xAB)
            names[wpc] = c.last_launch()[1]
        finally:
            c.close()
    assert names[8] == "fh::solve_kernel<10, true, 2, false>" and names[12] == "fh::solve_kernel<10, true, 3, false>"
    assert names[0] in (names[8], names[12])
    assert out[0][0]["solved"].mean() > 0.5 and out[0][1]["solved"].sum() > 0
    for wpc in (8, 12):
        for k, what in ((0, "whole"), (1, "safe")):
            a, b = out[0][k], out[wpc][k]
            for f in DUMP_FIELDS + ("assign",):
                assert np.array_equal(_bytes(a[f]), _bytes(b[f])), (wpc, what, f)
            assert np.array_equal(_bytes(a["coeff"][:, :10]), _bytes(b["coeff"][:, :10])), (wpc, what, "coeff")


def test_n15_bucket_keeps_working(ctx, oracle):
    """3 NSEG > 32: the N = 15 bucket runs the unsplit code."""
    pr, faces, _ = corridor.whole_batch(128, seed=15, n_seg=15, p_choices=(4, 5, 6, 7, 8))
    got = ctx.solve_batch(pr, faces)
    assert ctx.last_launch()[1].startswith("fh::solve_kernel<15, false,")
    ok = compare(got, oracle.solve_batch(pr, faces))
    assert ok.mean() > 0.5


def test_n10_every_segment_pinned(ctx, oracle):
    """32 problems at N = 10 with every segment pinned (fh_problem.pin) to the polytope the free search assigned it — and 8 of them
    to a shifted assignment, which the factor window cannot always meet: pure QPs whose corridor rows are active for every segment,
    the first (control point 3 of segment 0: the state at tt = 1, one segment before it) and the last (tt = N, all ten) included."""
    pr, faces, _ = corridor.whole_batch(32, seed=77, n_seg=10, p_choices=(2, 3, 4, 5, 6))
    free = ctx.solve_batch(pr, faces)
    assert free["solved"].sum() >= 24
    pinned = pr.copy()
    for i in range(len(pr)):
        P = int(pr["n_poly"][i])
        if free["solved"][i] and i % 4:
            a = [int(q) for q in free["assign"][i][:10]]
        else:
            a = [min(P - 1, (t * P) // 10 + (1 if t == 5 else 0)) for t in range(10)]
        assert all(0 <= q < P for q in a)
        abi.set_pins(pinned[i], a)
    got = ctx.solve_batch(pinned, faces)
    ok = compare(got, oracle.solve_batch(pinned, faces))
    keep = np.flatnonzero((free["solved"] == 1) & (np.arange(len(pr)) % 4 != 0))
    assert ok[keep].all()                                            # the assignment of the free optimum stays feasible when pinned
    assert np.array_equal(got["assign"][keep][:, :10], free["assign"][keep][:, :10])
    np.testing.assert_allclose(got["cost"][keep], free["cost"][keep], rtol=1e-7, atol=1e-9)
    assert np.array_equal(got["factor"][keep], free["factor"][keep])
