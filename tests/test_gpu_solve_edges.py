"""A solve launch where it changes behaviour: batch sizes around every switch of launch_solve (two-wavefront build, dealing, order
windows, ticket chunks), the borders of the 6 / 10 / 15 / 16 kernel builds, the face caps and the LDS carve they size, and every clause
that makes a record unusable — through the device, host, speculative, pool and fused-pair entry points.

Every device result buffer is one record longer than the batch and starts as the byte 0xA5: the guard record must still be 0xA5 after
the launch, and no record of the batch may (a zeroed buffer would hide a record that was never written: zeros are a plausible "unsolved").
The inputs are proved on the CPU oracle in tests/test_solve_edges_oracle.py (tests/solve_edge_cases.py builds them)."""
import numpy as np
import pytest
import torch  # noqa: F401  (before libfasterhip.so is loaded: one HIP runtime per process)

import solve_edge_cases as sec
from faster_amd import abi, capi, corridor
from test_gpu_parity import _dev, check_assignment_valid, compare

pytestmark = pytest.mark.gpu

RS = abi.result_dtype.itemsize
POISON = 0xA5
# FH_TICKET_CHUNK (fh_solve.hip.hpp) and FH_ORDER_WINDOW (fh_capi.hip): the launch order interleaves ranks inside windows of
# FH_TICKET_CHUNK * FH_ORDER_WINDOW * grid tickets
TICKET_CHUNK, ORDER_WINDOW = 4, 2
RESULT_FIELDS = ("solved", "trials", "status", "factor", "dt", "cost", "coeff", "assign")  # everything but nodes, qp_iters, kflops
_O = {k: abi.result_dtype.fields[k][1] for k in abi.result_dtype.names}
_COLS = torch.tensor([b for b in range(RS) if not _O["nodes"] <= b < _O["factor"]])  # the bytes of RESULT_FIELDS
_COLS_COMPACT = {n: torch.tensor([b for b in range(RS) if not _O["nodes"] <= b < _O["factor"] and not _O["coeff"] + 96 * n <= b < _O["assign"]])
                 for n in (6, 10, 15, 16)}


def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def poisoned(n):
    """n result records and the guard record, every byte 0xA5"""
    return torch.full(((n + 1) * RS,), POISON, dtype=torch.uint8, device="cuda:0")


def check_guard_and_written(d_res, n, what, compact_build=0):
    r = d_res.view(n + 1, RS)
    assert bool((r[n] == POISON).all()), ("the guard record was written", what)
    if compact_build:  # rows [NSEG, 16) of every record are the caller's bytes
        dead = r[:n, _O["coeff"] + 96 * compact_build: _O["assign"]]
        assert bool((dead == POISON).all()), ("rows beyond the build were written", what)
        r = r[:, _COLS_COMPACT[compact_build].to(r.device)]
    assert not bool((r[:n] == POISON).all(dim=1).any()), ("a record was never written", what)


def records(d_res, n):
    return d_res.cpu().numpy()[: n * RS].view(abi.result_dtype).copy()


def same_on_device(d_res, d_ref, n, what, compact_build=0):
    """record i of d_res == record i of d_ref in every byte of RESULT_FIELDS (compact: of the rows the build writes)"""
    cols = (_COLS_COMPACT[compact_build] if compact_build else _COLS).to(d_res.device)
    a, b = d_res.view(-1, RS)[:n][:, cols], d_ref.view(-1, RS)[:n][:, cols]
    if not bool((a == b).all()):
        bad = torch.nonzero((a != b).any(dim=1)).flatten().cpu().numpy()
        raise AssertionError("%s: %d records differ from the reference, first %s" % (what, len(bad), bad[:8]))


def assert_fields_equal(a, b, what, fields=RESULT_FIELDS):
    for f in fields:
        assert np.ascontiguousarray(a[f]).tobytes() == np.ascontiguousarray(b[f]).tobytes(), (what, f)


def context(share=1, **sched):
    c = capi.Context(0, pair_outputs=bool(sched.pop("pair_outputs", 1)), compact_results=bool(sched.pop("compact_results", 0)))
    par = abi.default_params()
    par["share"] = share
    c.set_params(par)
    if sched:
        c.set_sched(**sched)
    return c


def solve_device(c, pr, faces, max_seg, max_faces, what):
    """fh_solve_batch_device into a poisoned, guarded buffer; returns the records"""
    n = len(pr)
    d_pr, d_f, d_res = _dev(pr), _dev(faces), poisoned(n)
    c.solve_batch_device(d_pr.data_ptr(), d_f.data_ptr(), n, max_seg, max_faces, d_res.data_ptr())
    c.sync()
    assert c.share_stats()["error"] == 0, what
    check_guard_and_written(d_res, n, what)
    return records(d_res, n)


def blank_bad_record():
    r = np.zeros(1, dtype=abi.result_dtype)
    r["status"], r["assign"] = abi.FH_ST_BAD_INPUT, -1
    return r


# ---- a. results do not depend on the batch size -------------------------------------------------------------------------------------------
def batch_sizes(cu, grid):
    W = TICKET_CHUNK * ORDER_WINDOW * grid
    sizes = [1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, cu - 1, cu, cu + 1, 8 * cu - 1, 8 * cu, 8 * cu + 1, grid - 1, grid, grid + 1]
    sizes += [4 * grid + r for r in range(4)] + [2047, 2048, 2049, 2050, 2051, W - 1, W, W + 1, W + 5, 2 * W + 3]
    return sorted(set(sizes)), W


def test_results_do_not_depend_on_the_batch_size(oracle):
    """One pool of 70 000 cheap problems (C2 safe problems, N = 6, and C4 whole problems, N = 10 with 2-6 polytopes, shuffled: short units and
    tree searches side by side), solved once at full size, then every prefix [0, n) for n at each switch of launch_solve, one below and
    one above: record i of every run is record i of the full run.  Mutations this catches: the `& ~(FH_TICKET_CHUNK - 1)` of
    order_scatter_kernel dropped (a remainder of 1-3 ranks is lost: a record stays poison), `n < 8 * n_cu` for `<=`, `done` reported in
    fours for a batch that is not a multiple of four (the launch never ends, or ends early), a claim dealt beyond n (the guard)."""
    parts = [corridor.safe_batch(35000, seed=1)[:2], corridor.whole_batch(35000, seed=3, n_seg=10, p_choices=(2, 3, 4, 5, 6))[:2]]
    pr, faces = corridor.concat(parts)
    pr = pr[np.random.default_rng(17).permutation(len(pr))]
    N, n_all = 10, len(pr)
    mf = int(sec.rows_of(pr).max())
    d_pr, d_f = _dev(pr), _dev(faces)
    cu = n_cu()

    c = context(launch_order=0)
    d_ref = poisoned(n_all)
    c.solve_batch_device(d_pr.data_ptr(), d_f.data_ptr(), n_all, N, mf, d_ref.data_ptr())
    c.sync()
    assert c.share_stats()["error"] == 0
    check_guard_and_written(d_ref, n_all, "reference")
    grid = c.last_launch()[0]["grid"]
    c.close()
    ref = records(d_ref, 512)
    compare(ref, oracle.solve_batch(pr[:512], faces))
    check_assignment_valid(pr[:512], faces, ref)
    assert 0.5 < ref["solved"].mean() and len(set(pr["n_seg"][:512])) == 2

    sizes, W = batch_sizes(cu, grid)
    assert 2 * W + 3 <= n_all, (grid, n_all)
    for order in (0, 2):
        for share in (0, 1):
            c = context(share=share, launch_order=order)
            for n in sizes:
                what = "n = %d, launch_order %d, share %d" % (n, order, share)
                d_res = poisoned(n)
                c.solve_batch_device(d_pr.data_ptr(), d_f.data_ptr(), n, N, mf, d_res.data_ptr())
                c.sync()
                assert c.share_stats()["error"] == 0, what
                check_guard_and_written(d_res, n, what)
                same_on_device(d_res, d_ref, n, what)
                info = c.last_launch()[0]
                # the rule of launch_solve: up to 8 problems per CU no more than 8 solves are resident per CU anyway — the two-wavefront build
                if n == 8 * cu:
                    assert info["waves_per_simd"] == 2, info
                if n == 8 * cu + 1:
                    assert info["waves_per_simd"] == 3, info
            c.close()
    # compact results: the rows beyond the build stay the caller's
    c = context(launch_order=2, compact_results=1)
    for n in [s for s in sizes if s >= 2047]:
        what = "n = %d, compact" % n
        d_res = poisoned(n)
        c.solve_batch_device(d_pr.data_ptr(), d_f.data_ptr(), n, N, mf, d_res.data_ptr())
        c.sync()
        assert c.share_stats()["error"] == 0, what
        check_guard_and_written(d_res, n, what, compact_build=N)
        same_on_device(d_res, d_ref, n, what, compact_build=N)
    c.close()


# ---- b. the same for the fused pair kernel ----------------------------------------------------------------------------------------------------
SAFE_OUTPUTS = ("n_seg", "x0", "n_poly", "face_off", "face_begin")


def poisoned_templates(tmpl):
    """the safe templates with the fields a pair launch OUTPUTS poisoned (n_seg is a template field and stays), and a guard record"""
    t = np.concatenate([tmpl, tmpl[:1]])
    b = t.view(np.uint8).reshape(len(t), -1)
    for f in ("x0", "n_poly", "face_off", "face_begin"):
        dt, off = abi.problem_dtype.fields[f][:2]
        b[:, off: off + dt.itemsize] = POISON
    b[-1] = POISON
    return t


@pytest.mark.parametrize("pair_outputs", [0, 1], ids=["lazy", "complete"])
def test_fused_pairs_do_not_depend_on_the_batch_size(pair_outputs):
    """fh_solve_pairs_device on prefixes of a C4 pool of 25 000 pairs against ONE three-launch run of the whole pool (solve -> hand-off ->
    solve, as test_fused_pair_kernel_equals_three_launches): both result arrays poisoned and guarded; with complete outputs the safe
    records too."""
    B, N = 25000, 10
    whole, faces, _ = corridor.whole_batch(B, seed=3, n_seg=N, p_choices=(2, 3, 4, 5, 6))
    tmpl = corridor.safe_templates(whole)
    mf = int(sec.rows_of(whole).max())
    d_whole, d_faces = _dev(whole), _dev(faces)
    c = context(pair_outputs=pair_outputs)
    d_safe_ref, d_sf_ref = _dev(poisoned_templates(tmpl) if pair_outputs else tmpl), torch.zeros_like(d_faces)
    d_wref, d_sref = poisoned(B), poisoned(B)
    c.solve_batch_device(d_whole.data_ptr(), d_faces.data_ptr(), B, N, mf, d_wref.data_ptr())
    c.pair_glue_device(d_whole.data_ptr(), d_wref.data_ptr(), d_faces.data_ptr(), B, 0.5, 0.2, 3, d_safe_ref.data_ptr(), d_sf_ref.data_ptr())
    c.solve_batch_device(d_safe_ref.data_ptr(), d_sf_ref.data_ptr(), B, N, mf, d_sref.data_ptr())
    c.sync()
    check_guard_and_written(d_wref, B, "staged whole")
    check_guard_and_written(d_sref, B, "staged safe")
    safe_ref = d_safe_ref.cpu().numpy().view(abi.problem_dtype)  # (what the hand-off leaves unwritten is poison on both sides)
    assert records(d_sref, B)["solved"].mean() > 0.5

    def fused(n):
        what = "%d pairs, pair_outputs %d" % (n, pair_outputs)
        d_safe, d_sf = _dev(poisoned_templates(tmpl[:n]) if pair_outputs else tmpl[:n]), torch.zeros_like(d_faces)
        d_wr, d_sr = poisoned(n), poisoned(n)
        c.solve_pairs_device(d_whole.data_ptr(), d_faces.data_ptr(), n, N, mf, 0.5, 0.2, 3, d_wr.data_ptr(), d_safe.data_ptr(), d_sf.data_ptr(),
                             d_sr.data_ptr())
        c.sync()
        assert c.share_stats()["error"] == 0, what
        for d_res, d_ref, name in ((d_wr, d_wref, "whole"), (d_sr, d_sref, "safe")):
            check_guard_and_written(d_res, n, (what, name))
            same_on_device(d_res, d_ref, n, (what, name))
        if pair_outputs:
            safe = d_safe.cpu().numpy().view(abi.problem_dtype)
            assert (safe[n: n + 1].view(np.uint8) == POISON).all(), ("the guard template was written", what)
            for f in SAFE_OUTPUTS:
                assert np.array_equal(safe[f][:n], safe_ref[f][:n]), (what, f)
        return c.last_launch()[0]["grid"]

    grid = fused(B)
    W = TICKET_CHUNK * ORDER_WINDOW * grid
    cu = n_cu()
    assert W + 1 <= B
    for n in (1, 3, 5, 65, 8 * cu - 1, 8 * cu + 1, 2047, 2049, 2051, W + 1):
        fused(n)
    c.close()


# ---- c. the borders of the kernel builds ---------------------------------------------------------------------------------------------------
def border_batch(n_seg, force):
    groups = [(pr, faces) for n, f, _, pr, faces in sec.border_batches() if (n, f) == (n_seg, force)]
    return corridor.concat(groups)


@pytest.mark.parametrize("n_seg", sec.BORDER_N)
def test_borders_of_the_kernel_builds(oracle, n_seg):
    """Problems of n_seg segments at, below and above the 6 / 10 / 15 / 16 builds: in the build max_seg = n_seg selects, in the 16 build
    (max_seg = 0) and through the host entry, each in both register builds — against the oracle; bit for bit between the register builds and between host and device.
    A record with one segment more than the selected build holds is FH_ST_BAD_INPUT, whatever max_seg the caller gave (fasterhip.h:
    the BUILD is the bound), and costs its neighbours nothing."""
    build = sec.build_of(n_seg)
    for force in (0, 1):
        pr, faces = border_batch(n_seg, force)
        ref = oracle.solve_batch(pr, faces)
        runs = {}
        for wpc in (8, 12):
            c = context(workgroups_per_cu=wpc)
            runs[("build %d" % build, wpc)] = solve_device(c, pr, faces, n_seg, 0, (n_seg, force, wpc, "own build"))
            info = c.last_launch()[0]
            assert info["n_seg"] == build and info["waves_per_simd"] == (2 if wpc == 8 else 3), info
            runs[("build 16", wpc)] = solve_device(c, pr, faces, 0, 0, (n_seg, force, wpc, "16 build"))
            assert c.last_launch()[0]["n_seg"] == 16
            runs[("host", wpc)] = c.solve_batch(pr, faces)
            assert c.last_launch()[0]["n_seg"] == build
            if n_seg == build and n_seg < 16:  # one segment more than the build holds
                planted = pr.copy()
                where = np.array([0, len(pr) // 2, len(pr) - 1])
                planted["n_seg"][where] = n_seg + 1
                assert not any(sec.header_says_bad(p) for p in planted[where])  # (a good record for a larger build)
                got = solve_device(c, planted, faces, n_seg, 0, (n_seg, force, wpc, "planted"))
                assert c.last_launch()[0]["n_seg"] == build
                for i in where:
                    assert got[i: i + 1].tobytes() == blank_bad_record().tobytes(), (n_seg, force, wpc, i)
                keep = np.setdiff1d(np.arange(len(pr)), where)
                assert_fields_equal(got[keep], runs[("build %d" % build, wpc)][keep], (n_seg, force, wpc, "neighbours of planted records"))
            c.close()
        first, worst = None, (0.0, None)
        for key, got in runs.items():
            ok = compare(got, ref)
            check_assignment_valid(pr, faces, got)
            if first is None:
                first = got
            else:
                d = float(np.abs(got["coeff"] - first["coeff"]).max())
                worst = max(worst, (d, key), key=lambda w: w[0])
        # Two against three wavefronts per SIMD and host against device are the same arithmetic in the same order: bit for bit.  The builds
        # for different segment counts are NOT: the 6 and 10 builds against the 16 build differ in the last bits of cost and coefficients of
        # some problems of 5-10 segments (largest coefficient difference seen: 4.3e-14, a whole problem of 6 segments; 9e-16 among safe
        # problems; n_seg <= 3 and 15 against 16: none).  Between them flag, trials, factor and dt are asserted equal, cost and coefficients
        # only within the oracle's bars above, and the largest difference is printed.
        print("n_seg %d force %d: largest coefficient difference between builds %.3e %s" % (n_seg, force, worst[0], worst[1]))
        for wpc in (8, 12):
            assert_fields_equal(runs[("host", wpc)], runs[("build %d" % build, wpc)], (n_seg, force, wpc, "host against device"))
        for kind in ("build %d" % build, "build 16"):
            assert_fields_equal(runs[(kind, 8)], runs[(kind, 12)], (n_seg, force, kind, "two against three wavefronts"))
        for f in ("solved", "trials", "status", "factor", "dt"):
            for got in runs.values():
                assert np.array_equal(got[f], first[f]), (n_seg, force, f)


# ---- d. face caps --------------------------------------------------------------------------------------------------------------------------
def one_more_row_than(cap, n_seg):
    """a good record of n_seg segments with cap + 1 rows (None beyond FH_MAX_FACES)"""
    rows = cap + 1
    if rows > abi.FH_MAX_FACES:
        return None
    pr, faces, _ = corridor.whole_batch(1, seed=8800 + cap, n_seg=n_seg, p_choices=(-(-rows // 64),))
    polys = sec.polys_of(pr[0], faces)
    if rows <= 17:
        polys = [(A[:rows - 2], b[:rows - 2]) for A, b in polys]
    q = sec.with_polys(pr[0], polys)
    q = sec.padded_to(q[0][0], q[1], rows, np.random.default_rng(cap))
    assert q is not None and not sec.header_says_bad(q[0][0]) and sec.rows_of(q[0])[0] == rows
    return q


@pytest.mark.parametrize("n_seg", [6, 10, 15, 16])
def test_face_caps(oracle, n_seg):
    """Batches with exactly m rows per problem, max_faces given exactly and as 0: the LDS carve is sized by max_faces rounded up to 8, and
    that — not the caller's number — is the bound (fasterhip.h): a record with rows up to the rounded cap is solved, one row more is
    FH_ST_BAD_INPUT and its neighbours are untouched.  256 rows at N = 16 is the largest carve the library asks for."""
    c = context()
    groups = {m: sec.face_cap_group(m, n_seg)[:2] for m in sec.FACE_ROWS}
    refs = {m: oracle.solve_batch(*groups[m]) for m in sec.FACE_ROWS}
    for m in sec.FACE_ROWS:
        cap = (m + 7) & ~7
        parts, ref = [groups[m]], [refs[m]]
        if cap != m and cap in groups:  # rows beyond the caller's max_faces, within the carve: good
            parts.append(groups[cap]); ref.append(refs[cap])
        pr, faces = corridor.concat(parts)
        ref = np.concatenate(ref)
        got = solve_device(c, pr, faces, n_seg, m, (n_seg, m))
        info = c.last_launch()[0]
        assert info["n_seg"] == sec.build_of(n_seg) and info["lds_bytes"] <= 160 * 1024, info
        ok = compare(got, ref)
        assert ok.mean() >= 0.5
        check_assignment_valid(pr, faces, got)
        extra = one_more_row_than(cap, n_seg)
        if extra is not None:
            k = len(pr) // 2
            pr2, faces2 = corridor.concat([(pr[:k], faces), extra, (pr[k:], np.zeros(0, dtype=abi.face_dtype))])
            pr2["face_begin"][k + 1:] = pr["face_begin"][k:]  # (their rows are in the first part)
            got2 = solve_device(c, pr2, faces2, n_seg, m, (n_seg, m, "one row more"))
            assert got2[k: k + 1].tobytes() == blank_bad_record().tobytes(), (n_seg, m)
            assert_fields_equal(np.delete(got2, k), got, (n_seg, m, "neighbours"))
            assert oracle.solve_batch(pr2[k: k + 1], faces2)["status"][0] != abi.FH_ST_BAD_INPUT  # (a good record for a larger carve)
    # max_faces = 0: the library's maximum, every group in one launch
    pr, faces = corridor.concat([groups[m] for m in sec.FACE_ROWS])
    got = solve_device(c, pr, faces, n_seg, 0, (n_seg, "max_faces 0"))
    compare(got, np.concatenate([refs[m] for m in sec.FACE_ROWS]))
    info = c.last_launch()[0]
    assert info["lds_bytes"] <= 160 * 1024, info
    c.close()


def test_257_rows_and_a_polytope_of_65_through_every_entry_point(oracle):
    pr, faces, rows = sec.bad_record_table()
    names = [r["name"] for r in rows]
    pick = [0, names.index("257 rows"), 2, names.index("polytope 0 with 65 rows"), 4]
    sub = pr[pick]
    ref = oracle.solve_batch(sub, faces)
    c = context()
    pool = capi.Pool([0, 0, 0])
    for name, got in (("device", solve_device(c, sub, faces, 0, 0, "257 / 65")), ("host", c.solve_batch(sub, faces)),
                      ("speculative", c.solve_batch_speculative(sub, faces, 4)), ("pool", pool.solve_batch(sub, faces))):
        assert list(got["status"]) == [0, abi.FH_ST_BAD_INPUT, 0, abi.FH_ST_BAD_INPUT, 0], name
        compare(got, ref)
    pool.close()
    c.close()


# ---- e. the table of unusable records ---------------------------------------------------------------------------------------------------------
def check_table(got, ref, rows, what, pr, faces):
    assert np.array_equal(got["status"], ref["status"]), what
    compare(got, ref)
    check_assignment_valid(pr, faces, got)
    worst = (0.0, None)
    for i, r in enumerate(rows):
        if r["bad"]:  # the oracle's record byte for byte: zeros, FH_ST_BAD_INPUT, no assignment
            assert got[i: i + 1].tobytes() == ref[i: i + 1].tobytes(), (what, r["name"])
        elif r["twin"] is not None:  # a good clone: its base's result bit for bit (solve_edge_cases.bad_record_table: why, and what `skip` is)
            d = float(np.abs(got["coeff"][i] - got["coeff"][r["twin"]]).max())
            worst = max(worst, (d, r["name"]), key=lambda w: w[0])
    print("%s: largest coefficient difference between a good clone and its base %.3e %s" % (what, worst[0], worst[1]))
    for i, r in enumerate(rows):
        if not r["bad"] and r["twin"] is not None:
            assert_fields_equal(got[i: i + 1], got[r["twin"]: r["twin"] + 1], (what, r["name"]), [f for f in RESULT_FIELDS if f not in r["skip"]])


def test_table_of_unusable_records_through_every_entry_point(oracle):
    """Each clause of bad_scalars / bad_corridor violated in one record, between good neighbours; records that must stay good (garbage in
    fields a solve must not read, +inf as a bound, an empty polytope, 64 rows, 256 rows, a window of exactly FH_MAX_TRIALS steps).
    Mutations this catches: `>` for `>=` (or `>=` for `>`) in any clause — the 64 / 65-row and 256 / 257-row and 4096-step pairs sit on
    both sides of each —, a clause dropped, face_off garbage copied into a loop bound, a bad record that leaves LDS state to its neighbour."""
    pr, faces, rows = sec.bad_record_table()
    ref = oracle.solve_batch(pr, faces)
    c = context()
    check_table(solve_device(c, pr, faces, 0, 0, "table"), ref, rows, "device", pr, faces)
    check_table(c.solve_batch(pr, faces), ref, rows, "host", pr, faces)
    check_table(c.solve_batch_speculative(pr, faces, 4), ref, rows, "speculative", pr, faces)
    pool = capi.Pool([0, 0, 0])
    check_table(pool.solve_batch(pr, faces), ref, rows, "pool", pr, faces)
    pool.close()

    # the table as the whole problems of fused pairs: a bad whole record gives a safe result FH_ST_BAD_INPUT, as the three launches do
    n = len(pr)
    tmpl = np.repeat(corridor.safe_templates(pr[:1]), n)
    d_whole, d_faces = _dev(pr), _dev(faces)

    def three_launches(whole_d, tm, n, max_seg):
        d_safe, d_sf = _dev(tm), torch.zeros_like(d_faces)
        d_wr, d_sr = poisoned(n), poisoned(n)
        c.solve_batch_device(whole_d.data_ptr(), d_faces.data_ptr(), n, max_seg, 0, d_wr.data_ptr())
        c.pair_glue_device(whole_d.data_ptr(), d_wr.data_ptr(), d_faces.data_ptr(), n, 0.5, 0.2, 3, d_safe.data_ptr(), d_sf.data_ptr())
        c.solve_batch_device(d_safe.data_ptr(), d_sf.data_ptr(), n, max_seg, 0, d_sr.data_ptr())
        c.sync()
        return d_wr, d_sr

    def fused(whole_d, tm, n, max_seg, what):
        d_safe, d_sf = _dev(tm), torch.zeros_like(d_faces)
        d_wr, d_sr = poisoned(n), poisoned(n)
        c.solve_pairs_device(whole_d.data_ptr(), d_faces.data_ptr(), n, max_seg, 0, 0.5, 0.2, 3, d_wr.data_ptr(), d_safe.data_ptr(), d_sf.data_ptr(),
                             d_sr.data_ptr())
        c.sync()
        assert c.share_stats()["error"] == 0, what
        check_guard_and_written(d_wr, n, (what, "whole"))
        check_guard_and_written(d_sr, n, (what, "safe"))
        return d_wr, d_sr

    w3, s3 = three_launches(d_whole, tmpl, n, 0)
    wf, sf = fused(d_whole, tmpl, n, 0, "table as whole problems")
    same_on_device(wf, w3, n, "pairs: whole")
    same_on_device(sf, s3, n, "pairs: safe")
    check_table(records(wf, n), ref, rows, "pairs: whole", pr, faces)
    safe = records(sf, n)
    for i, r in enumerate(rows):
        if r["bad"]:
            assert safe[i: i + 1].tobytes() == blank_bad_record().tobytes(), r["name"]

    # the bad scalars in the safe TEMPLATE (checked with the safe problem's own polytope count): good whole problems throughout
    N = 10
    cases = [("n_seg", 0), ("n_seg", N + 1), ("f_inc", 0.0), ("dc", np.nan), ("pin", None)]
    m = 2 * len(cases) + 1
    whole = np.repeat(pr[:1], m)
    tm = corridor.safe_templates(whole)
    for k, (field, v) in enumerate(cases):
        if field == "pin":
            abi.set_pins(tm[2 * k + 1], [abi.FH_MAX_POLY])  # polytope 8 of a safe corridor of at most 3
        else:
            tm[field][2 * k + 1] = v
    d_w = _dev(whole)
    w3, s3 = three_launches(d_w, tm, m, N)
    wf, sf = fused(d_w, tm, m, N, "bad safe templates")
    same_on_device(wf, w3, m, "bad templates: whole")
    same_on_device(sf, s3, m, "bad templates: safe")
    safe = records(sf, m)
    assert (safe["status"][1::2] == abi.FH_ST_BAD_INPUT).all() and (safe["solved"][0::2] == 1).all(), safe["status"]
    for i in range(1, m, 2):
        assert safe[i: i + 1].tobytes() == blank_bad_record().tobytes(), cases[i // 2]
    assert_fields_equal(safe[2::2], safe[:-2:2], "good neighbours of bad templates")
    c.close()


def test_window_of_4097_trials(oracle):
    pr, faces = sec.window_boundary_problems()
    ref = oracle.solve_batch(pr, faces)
    c = context()
    plain = c.solve_batch(pr, faces)
    spec = c.solve_batch_speculative(pr, faces, 64)
    c.close()
    for got in (plain, spec):
        assert got["trials"][0] == 4097 and got["status"][0] == abi.FH_ST_INFEASIBLE and got["solved"][0] == 0
        assert got[1: 2].tobytes() == blank_bad_record().tobytes()
        compare(got, ref)
    assert_fields_equal(plain, spec, "plain against speculative", ("trials", "status", "dt"))


def test_host_entries_refuse_rows_outside_the_face_array():
    """A record with a valid layout that points beyond n_faces: FH_ERR_ARG from the host entry points (the kernel cannot see n_faces; such
    a record is never handed to a device-pointer entry), the message names the faces, and the next call on the same context works.
    Anything else — face_begin < 0 included, which the kernel refuses before it reads a row — is the kernel's to report."""
    pr, faces, _ = corridor.whole_batch(8, seed=2)
    good = None
    c = context()
    pool = capi.Pool([0, 0, 0])
    for solve in (c.solve_batch, pool.solve_batch):
        bad = pr.copy()
        bad["face_begin"][5] = len(faces) - int(sec.rows_of(pr)[5]) + 1
        with pytest.raises(capi.FasterHipError, match=r"rc=-1 .*faces") as e:
            solve(bad, faces)
        assert "n_faces" in str(e.value)
        got = solve(pr, faces)
        good = got if good is None else good
        assert_fields_equal(got, good, "after a refused call")
        neg = pr.copy()
        neg["face_begin"][5] = -1
        got = solve(neg, faces)
        assert got["status"][5] == abi.FH_ST_BAD_INPUT
        assert_fields_equal(np.delete(got, 5), np.delete(good, 5), "neighbours of face_begin = -1")
    assert good["solved"].sum() >= 4
    pool.close()
    c.close()
