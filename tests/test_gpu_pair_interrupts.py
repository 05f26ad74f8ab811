"""Fused pairs (fh_solve_pairs_device) that do not run to the end: a stop request raised before the launch, and the work cap.

A pair whose whole problem ends FH_ST_INTERRUPTED has no whole trajectory and hence no safe problem; its safe result must say
FH_ST_INTERRUPTED as well (fasterhip.h: problems not finished report FH_ST_INTERRUPTED), never FH_ST_BAD_INPUT — a caller that
retries on INTERRUPTED and treats BAD_INPUT as its own error would otherwise misread the safe half of every interrupted pair.  A
whole problem that ends at a limit (or is bad input, or infeasible) leaves a safe result FH_ST_BAD_INPUT, as the three-launch
pipeline does.

Nothing here depends on how long anything takes: with the stop word raised before the launch, workgroup 0 polls the host word on
its first draw (every workgroup whose index is a multiple of 32 does, on its first chunk of tickets), so at least one pair is
interrupted before its whole problem is staged; the others are interrupted or finish, depending on when their workgroup sees the
word — each of them is checked against the un-stopped run."""
import numpy as np
import pytest
import torch  # noqa: F401  (before libfasterhip.so is loaded: one HIP runtime per process)

from faster_amd import abi, capi, corridor

pytestmark = pytest.mark.gpu

RS = abi.result_dtype.itemsize
WORK = ("nodes", "qp_iters", "kflops")          # work counters: they depend on which wavefronts shared a tree
HEAD = [f for f in abi.result_dtype.names if f not in WORK + ("coeff",)]
TEMPLATE = ("n_seg", "force_final_pos", "dc", "v_max", "a_max", "j_max", "f_init", "f_final", "f_inc", "xf", "pin")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


def _bytes(a):
    """Per-record bytes of a field (bit-for-bit comparisons; NaN compares equal to itself)."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(len(a), -1)


def same_records(a, b, rows):
    """Per-record mask: every field of the two fh_result arrays equal bit for bit, except the work counters; coefficient rows < rows."""
    eq = np.ones(len(a), dtype=bool)
    for f in HEAD:
        eq &= (_bytes(a[f]) == _bytes(b[f])).all(axis=1)
    eq &= (_bytes(a["coeff"][:, :rows]) == _bytes(b["coeff"][:, :rows])).all(axis=1)
    return eq


def interrupted_at_draw(r, rows):
    """Per-record mask: the record a problem gets when it is interrupted before it is staged (run_problem's bad path)."""
    return ((r["solved"] == 0) & (r["trials"] == 0) & (r["status"] == abi.FH_ST_INTERRUPTED) & (r["factor"] == 0.0) & (r["dt"] == 0.0)
            & (r["cost"] == 0.0) & ~r["coeff"][:, :rows].reshape(len(r), -1).any(axis=1) & (r["assign"] == -1).all(axis=1))


def launch_pairs(c, whole, faces, tmpl, max_seg, fill=0):
    """One fused launch on context c; the result buffers start as `fill` bytes.  Returns host copies of what the device left."""
    B = len(whole)
    mf = int(whole["face_off"][np.arange(B), np.clip(whole["n_poly"], 0, abi.FH_MAX_POLY)].max())
    d_whole, d_faces, d_safe = _dev(whole), _dev(faces), _dev(tmpl)
    d_sf = torch.full_like(d_faces, fill)
    d_wr = torch.full((B * RS,), fill, dtype=torch.uint8, device="cuda:0")
    d_sr = torch.full((B * RS,), fill, dtype=torch.uint8, device="cuda:0")
    c.solve_pairs_device(d_whole.data_ptr(), d_faces.data_ptr(), B, max_seg, mf, 0.5, 0.2, 3, d_wr.data_ptr(), d_safe.data_ptr(), d_sf.data_ptr(),
                         d_sr.data_ptr())
    c.sync()
    return (d_wr.cpu().numpy().view(abi.result_dtype).copy(), d_sr.cpu().numpy().view(abi.result_dtype).copy(),
            d_safe.cpu().numpy().view(abi.problem_dtype).copy(), d_sf.cpu().numpy().view(abi.face_dtype).copy())


def c4_like_batch(B=4096, seed=3):
    """C4's generator (N = 10, 2-6 polytopes) with pairs whose whole problem has no solution (f_final = 1) or is bad input."""
    whole, faces, _ = corridor.whole_batch(B, seed=seed, n_seg=10, p_choices=(2, 3, 4, 5, 6))
    whole = whole.copy()
    whole["f_final"][5::64] = 1.0              # mostly without a solution: no safe problem
    whole["n_seg"][7::128] = 0                 # bad input
    whole["x0"][9::128, 4] = np.nan            # bad input (found where x0 is staged)
    return whole, faces, corridor.safe_templates(whole)


@pytest.mark.parametrize("pair_outputs", [False, True], ids=["lazy", "complete"])
@pytest.mark.parametrize("wpc,waves", [(12, 3), (8, 2)], ids=["3waves", "2waves"])
def test_stop_raised_before_a_pair_launch(pair_outputs, wpc, waves):
    """fh_request_stop() before fh_solve_pairs_device: every pair either gives what the un-stopped launch gives (bit for bit, all fields
    but the work counters) or is unsolved with FH_ST_INTERRUPTED; a pair whose whole problem was interrupted has an interrupted safe
    result, equal field for field to that of a problem interrupted before it was staged (no trials, no factor, zero rows, no
    assignment) — not FH_ST_BAD_INPUT; with complete pair outputs its safe record is marked n_seg = 0.  After fh_clear_stop() the next
    launch equals the un-stopped one.  Both kernel builds (three and two wavefronts per SIMD), lazy and complete pair outputs."""
    N = 10
    whole, faces, tmpl = c4_like_batch()
    c = capi.Context(0, pair_outputs=pair_outputs, compact_results=not pair_outputs)
    try:
        c.set_pair_margin(0.05)
        c.set_sched(workgroups_per_cu=wpc)
        wref, sref, safe_ref, _ = launch_pairs(c, whole, faces, tmpl, N, fill=0xAB)
        info, name = c.last_launch()
        assert name == "fh::solve_kernel<10, true, %d, false>" % waves and info["workgroups_per_cu"] <= wpc
        assert (wref["status"][7::128] == abi.FH_ST_BAD_INPUT).all() and (wref["status"][9::128] == abi.FH_ST_BAD_INPUT).all()
        assert wref["solved"].mean() > 0.9 and 0.5 < sref["solved"].mean() < 1.0
        assert not (wref["status"] == abi.FH_ST_INTERRUPTED).any() and not (sref["status"] == abi.FH_ST_INTERRUPTED).any()
        c.request_stop()
        try:
            w, s, safe, _ = launch_pairs(c, whole, faces, tmpl, N, fill=0xCD)
            stats = c.share_stats()
        finally:
            c.clear_stop()
        w_int, s_int = w["status"] == abi.FH_ST_INTERRUPTED, s["status"] == abi.FH_ST_INTERRUPTED
        print("%s, pair_outputs %d: %d whole and %d safe results of %d interrupted (%d whole ones before they were staged)"
              % (name, pair_outputs, w_int.sum(), s_int.sum(), len(w), interrupted_at_draw(w, N).sum()))
        assert stats["interrupted"] != 0 and stats["error"] == 0
        # workgroup 0 polls the host's word on its first draw: its first pair is interrupted before its whole problem is staged
        assert interrupted_at_draw(w, N).any()
        # an interrupted whole problem: its safe result is interrupted too — the record of a problem interrupted before it was staged
        bad = np.flatnonzero(w_int & ~s_int)
        assert len(bad) == 0, ("safe status of interrupted pairs", np.unique(s["status"][bad], return_counts=True), bad[:8])
        assert interrupted_at_draw(s[w_int], N).all()
        # every result: as without the stop, or interrupted and unsolved
        for got, ref, hit, what in ((w, wref, w_int, "whole"), (s, sref, s_int, "safe")):
            eq = same_records(got, ref, N)
            assert np.all(eq | hit), (what, np.flatnonzero(~(eq | hit))[:8])
            assert not got["solved"][hit].any(), what
        fin = ~w_int
        if pair_outputs:
            assert (safe["n_seg"][w_int] == 0).all()
            for f in abi.problem_dtype.names:     # the hand-off of a pair that finished its whole problem: the same record
                assert (_bytes(safe[f][fin]) == _bytes(safe_ref[f][fin])).all(), f
        else:
            for f in TEMPLATE:                    # lazy outputs: the template fields are never written
                assert (_bytes(safe[f]) == _bytes(tmpl[f])).all(), f
        # the request is cleared: the next launch solves as before
        w2, s2, _, _ = launch_pairs(c, whole, faces, tmpl, N, fill=0xEF)
        assert same_records(w2, wref, N).all() and same_records(s2, sref, N).all()
    finally:
        c.clear_stop()
        c.close()


def test_work_cap_on_pairs_equals_three_launches(oracle):
    """fh_params.max_work on fused pairs: some whole problems end FH_ST_ITER_LIMIT (unsolved, so their pairs have no safe problem), and
    the fused kernel gives what the three launches (whole solve, fh_pair_glue_device, safe solve) give — whole results, safe problems,
    safe faces, safe results — field for field; the safe result of a capped pair says FH_ST_BAD_INPUT in both.  The whole problems below
    the cap are the oracle's."""
    B, N = 2048, 10
    whole, faces, _ = corridor.whole_batch(B, seed=41, n_seg=N, p_choices=(2, 3, 4, 5, 6))
    whole = whole.copy()
    whole["f_final"][:16] = 1.0
    tmpl = corridor.safe_templates(whole)
    mf = int(whole["face_off"][np.arange(B), whole["n_poly"]].max())
    par = abi.default_params()
    par["max_work"] = 60
    c = capi.Context(0)
    try:
        c.set_params(par)
        c.set_pair_margin(0.05)
        outs = []
        for fused in (False, True):
            d_whole, d_faces, d_safe = _dev(whole), _dev(faces), _dev(tmpl)
            d_sf = torch.zeros_like(d_faces)
            d_wr = torch.full((B * RS,), 0xAB, dtype=torch.uint8, device="cuda:0")
            d_sr = torch.full((B * RS,), 0xAB, dtype=torch.uint8, device="cuda:0")
            if fused:
                c.solve_pairs_device(d_whole.data_ptr(), d_faces.data_ptr(), B, N, mf, 0.5, 0.2, 3, d_wr.data_ptr(), d_safe.data_ptr(), d_sf.data_ptr(),
                                     d_sr.data_ptr())
            else:
                c.solve_batch_device(d_whole.data_ptr(), d_faces.data_ptr(), B, N, mf, d_wr.data_ptr())
                c.pair_glue_device(d_whole.data_ptr(), d_wr.data_ptr(), d_faces.data_ptr(), B, 0.5, 0.2, 3, d_safe.data_ptr(), d_sf.data_ptr())
                c.solve_batch_device(d_safe.data_ptr(), d_sf.data_ptr(), B, N, mf, d_sr.data_ptr())
            c.sync()
            outs.append((d_wr.cpu().numpy().view(abi.result_dtype).copy(), d_sr.cpu().numpy().view(abi.result_dtype).copy(),
                         d_safe.cpu().numpy().copy(), d_sf.cpu().numpy().copy()))
    finally:
        c.close()
    (w3, s3, safe3, sf3), (wf, sf, safef, sff) = outs
    for a, b, what in ((w3, wf, "whole"), (s3, sf, "safe")):
        for f in abi.result_dtype.names:
            if f not in WORK:
                assert (_bytes(a[f]) == _bytes(b[f])).all(), (what, f)
    assert np.array_equal(safe3, safef) and np.array_equal(sf3, sff)
    capped = wf["status"] == abi.FH_ST_ITER_LIMIT
    print("work cap 60: %d of %d whole problems capped, %d safe problems capped" % (capped.sum(), B, (sf["status"] == abi.FH_ST_ITER_LIMIT).sum()))
    assert 0 < capped.sum() < B // 2
    assert not wf["solved"][capped].any() and (sf["status"][capped] == abi.FH_ST_BAD_INPUT).all()
    assert (safef.view(abi.problem_dtype)["n_seg"][capped] == 0).all()
    # below the cap the whole problems are the oracle's (a subsample)
    idx = np.flatnonzero(~capped)[::8]
    ref = oracle.solve_batch(whole[idx], faces)
    got = wf[idx]
    for f in ("solved", "trials", "status", "factor", "dt"):
        assert np.array_equal(got[f], ref[f]), f
    ok = ref["solved"] == 1
    np.testing.assert_allclose(got["cost"][ok], ref["cost"][ok], rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(got["coeff"][ok], ref["coeff"][ok], rtol=0, atol=1e-6)
