"""GPU tests of the certificate kernel (include/fasterhip_certify.h, faster_amd/csrc/fh_certify.hip.hpp): every field of every certificate
equals the numpy restatement of the header's model (tests/certify_model.py) BIT FOR BIT — on synthetic records that no solver has seen,
on ties, NaNs and infinities, on every structural flag, on the solver's own output, through the host form, next to a running solve launch
and through Fleet.certify()."""
import numpy as np
import pytest

from faster_amd import abi, capi, corridor

import certify_model as cm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FEAS = abi.certify_tol(1e-9)   # fh_params.feas_tol: the project's own number for "violated"


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch  # noqa: F401  (torch before the HIP library: one HIP runtime in the process)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def to_dev(a, pad_before=0, pad_after=0):
    """The bytes of a numpy array on the device, with slack in front and behind (filled with 0xff: NaNs, for a read that strays)."""
    import torch

    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    host = np.concatenate([np.full(pad_before, 0xff, np.uint8), raw, np.full(pad_after, 0xff, np.uint8)])
    return torch.from_numpy(host).to(DEV)


def dev_certify(c, pr, faces, res, tol=None, slack=16, before=None):
    """fh_certify_batch_device on copies of the three arrays; the face rows lie inside a larger allocation (slack rows on either side).
    before: called when the copies are on the device, just before the launch."""
    import torch

    FB = abi.face_dtype.itemsize
    d_p, d_r = to_dev(pr), to_dev(res, 0, abi.result_dtype.itemsize)
    d_f = to_dev(faces, slack * FB, slack * FB)
    d_o = torch.zeros(len(pr) * abi.certificate_dtype.itemsize, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    if before is not None:
        before()
    c.certify_batch_device(d_p.data_ptr(), d_f.data_ptr() + slack * FB, len(faces), d_r.data_ptr(), len(pr), d_o.data_ptr(), tol)
    c.sync()
    return d_o.cpu().numpy().view(abi.certificate_dtype).copy()


def assert_same(got, want, what):
    bad = cm.same_bits(got, want)
    if bad:
        k = bad[0]
        i = int(np.nonzero(np.ascontiguousarray(got[k]).view(np.uint64 if got[k].dtype == np.float64 else np.int32)
                           != np.ascontiguousarray(want[k]).view(np.uint64 if want[k].dtype == np.float64 else np.int32))[0][0])
        raise AssertionError("%s: fields %s differ; first: %s of record %d, device %r, model %r" % (what, bad, k, i, got[k][i], want[k][i]))
    assert not got["reserved_i"].any() and not got["reserved_d"].any(), what


SEG, POLY, FACES = (1, 2, 6, 10, 15, 16), (0, 1, 3, abi.FH_MAX_POLY), (0, 1, 4, 63, 64, 65, abi.FH_MAX_FACES_POLY)


def synthetic(n, seed):
    """Records no solver has seen: random finite coefficients, random rows, every n_seg x n_poly x force_final_pos of the lists above and
    every face count per polytope (an empty polytope among full ones included)."""
    rng = np.random.default_rng(seed)
    pr, res = abi.make_problems(n), np.zeros(n, dtype=abi.result_dtype)
    rows = []
    for i in range(n):
        N, Q = SEG[i % 6], POLY[(i // 6) % 4]
        counts = [FACES[(i + 3 * q) % 7] for q in range(Q)]
        pr["n_seg"][i], pr["n_poly"][i], pr["force_final_pos"][i] = N, Q, (i // 24) % 2
        pr["face_begin"][i] = sum(len(r) for r in rows)
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32) if Q else np.zeros(1, np.int32)
        pr["face_off"][i][:len(off)] = off
        pr["face_off"][i][len(off):] = off[-1]
        f = np.zeros(int(off[-1]), dtype=abi.face_dtype)
        f["a"], f["b"] = rng.normal(size=(len(f), 3)), rng.normal(scale=3.0, size=len(f))
        rows.append(f)
        pr["v_max"][i], pr["a_max"][i], pr["j_max"][i] = rng.uniform(0.5, 3.0, 3)
        pr["x0"][i], pr["xf"][i] = rng.normal(size=9), rng.normal(size=9)
        res["solved"][i], res["dt"][i], res["cost"][i] = 1, rng.uniform(0.1, 2.0), rng.uniform(0.0, 2000.0)
        res["coeff"][i][:N] = rng.normal(size=(N, 12))
        res["assign"][i] = -1
        if Q:
            res["assign"][i][:N] = rng.integers(0, Q, N)
    return pr, np.concatenate(rows), res


def test_synthetic_records_equal_the_model_bit_for_bit(ctx):
    """257 records of random coefficients (nowhere near feasible: every maximum is decided by competition) in batches of 1, 3, 4, 5 and
    257 (grid of 65 workgroups, the last with one wavefront), under tolerances that split the batch on every flag."""
    pr, faces, res = synthetic(257, 1)
    plain = cm.certify(pr, faces, res)
    tol = abi.certify_tol(float(np.median(plain["corridor_best"][np.isfinite(plain["corridor_best"])])),
                          float(np.median(np.concatenate([plain["x0_defect"], plain["xf_defect"], plain["continuity_defect"]]))),
                          float(np.median(np.maximum(np.maximum(plain["v_excess"], plain["a_excess"]), plain["j_excess"]))),
                          float(np.median(plain["cost_defect"] / np.maximum(1.0, np.abs(res["cost"])))))
    want = cm.certify(pr, faces, res, tol)
    for bit in (abi.FH_CERT_CORRIDOR, abi.FH_CERT_ASSIGNMENT, abi.FH_CERT_X0, abi.FH_CERT_XF, abi.FH_CERT_CONTINUITY, abi.FH_CERT_BOX, abi.FH_CERT_COST):
        share = float(((want["flags"] & bit) != 0).mean())
        assert 0.01 < share < 0.99, (bit, share)   # (one tol.state serves x0, xf and continuity, whose sizes differ: 5 records is the least)
    assert np.isneginf(want["corridor_best"]).any() and (want["worst_seg"] == -1).any() and (want["worst_seg"] > 0).any()
    assert_same(dev_certify(ctx, pr, faces, res), plain, "no tolerances")
    for n in (1, 3, 4, 5, 257):
        assert_same(dev_certify(ctx, pr[:n], faces, res[:n], tol), want[:n], "batch of %d" % n)


def one_record(coeff, polys, assign, dt=1.0, ffp=1):
    """One problem with the given [N][12] coefficients and polytopes [(A, b)]."""
    N = len(coeff)
    pr, res = abi.make_problems(1), np.zeros(1, dtype=abi.result_dtype)
    faces, off = abi.pack_faces(polys)
    pr["n_seg"], pr["n_poly"], pr["force_final_pos"] = N, len(polys), ffp
    pr["face_off"][0][:len(off)] = off
    pr["face_off"][0][len(off):] = off[-1]
    pr["v_max"], pr["a_max"], pr["j_max"] = 5.0, 5.0, 8.0
    res["solved"], res["dt"] = 1, dt
    res["coeff"][0][:N] = coeff
    res["assign"][0] = -1
    res["assign"][0][:N] = assign
    return pr, faces, res


def box(lo, hi):
    A = np.concatenate([np.eye(3), -np.eye(3)])
    return A, np.concatenate([np.full(3, float(hi)), -np.full(3, float(lo))])


def test_ties_nan_rows_and_infinite_offsets(ctx):
    """Segments 1 and 2 are the same polynomial and segment 0 lies deeper inside: worst_seg is 1, the smaller of the two that attain
    corridor_best.  Polytopes 0 and 1 are the same box: the same e, so the assignment to 1 costs nothing.  A NaN row is ignored.  A row
    with b = +inf has the value -inf: a polytope made of it alone contains everything, and the first segment attains -inf."""
    rng = np.random.default_rng(2)
    seg = rng.uniform(-1.0, 1.0, 12)
    coeff = np.stack([0.25 * seg, seg, seg])
    A, b = box(-0.5, 0.5)
    nan_row = (np.concatenate([A, [[np.nan, 1.0, 0.0]]]), np.concatenate([b, [0.0]]))
    pr, faces, res = one_record(coeff, [(A, b), nan_row], [1, 1, 0])
    want = cm.certify(pr, faces, res)
    assert want["worst_seg"][0] == 1 and want["corridor_best"][0] > 0 and want["corridor_best"][0] == want["corridor_assigned"][0]
    assert_same(dev_certify(ctx, pr, faces, res), want, "two segments and two polytopes tie")
    free = (np.array([[1.0, 0.0, 0.0]]), np.array([np.inf]))
    pr, faces, res = one_record(coeff, [(A, b), free], [0, 0, 0])
    want = cm.certify(pr, faces, res)
    assert np.isneginf(want["corridor_best"][0]) and want["worst_seg"][0] == 0 and want["corridor_assigned"][0] > 0
    assert_same(dev_certify(ctx, pr, faces, res), want, "a row with b = +inf")


def test_structural_flags_and_the_neighbours_of_a_bad_record(ctx):
    """One good record, copied; every second copy is spoilt in one way.  The spoilt ones get their flag and zeros, the good ones between
    them the certificate of the record alone.  The face rows lie inside a larger allocation and the results are followed by slack, so a
    read that strays would show as a wrong number."""
    pr0, faces, res0 = synthetic(48, 3)
    k = next(i for i in range(48) if pr0["n_seg"][i] == 10 and pr0["n_poly"][i] == 3 and pr0["face_off"][i][3] > 60)
    pr0, res0 = pr0[k:k + 1], res0[k:k + 1]
    nf, top = len(faces), int(pr0["face_off"][0][3])

    def f(name, index=None):
        def setter(p, r, v):
            rec = p if name in p.dtype.names else r
            if index is None:
                rec[name] = v
            else:
                rec[name][0][index] = v
        return setter

    U, B, NF = abi.FH_CERT_UNSOLVED, abi.FH_CERT_BAD_INPUT, abi.FH_CERT_NOT_FINITE
    cases = [("unsolved", f("solved"), 0, U), ("n_seg 0", f("n_seg"), 0, B), ("n_seg 17", f("n_seg"), 17, B), ("n_poly -1", f("n_poly"), -1, B),
             ("n_poly 9", f("n_poly"), 9, B), ("face_off[0] 1", f("face_off", 0), 1, B), ("face_off falls", f("face_off", 1), top + 1, B),
             ("face_begin -1", f("face_begin"), -1, B), ("rows past the end", f("face_begin"), nf - top + 1, B),
             ("assign n_poly", f("assign", 9), 3, B), ("assign -1", f("assign", 0), -1, B),
             ("NaN in row n_seg - 1", f("coeff", (9, 11)), np.nan, NF), ("inf in row 0", f("coeff", (0, 0)), np.inf, NF),
             ("dt 0", f("dt"), 0.0, NF), ("dt -1", f("dt"), -1.0, NF), ("dt inf", f("dt"), np.inf, NF), ("dt NaN", f("dt"), np.nan, NF),
             ("NaN in row n_seg, a dead row", f("coeff", (10, 0)), np.nan, 0), ("rows end at the end", f("face_begin"), nf - top, None)]
    n = 2 * len(cases) + 1
    pr, res = np.repeat(pr0, n), np.repeat(res0, n)
    for j, (_, setter, v, _) in enumerate(cases):
        setter(pr[2 * j + 1:2 * j + 2], res[2 * j + 1:2 * j + 2], v)
    alone = dev_certify(ctx, pr0, faces, res0, FEAS)
    assert_same(alone, cm.certify(pr0, faces, res0, FEAS), "the good record alone")
    assert alone["flags"][0] & abi.FH_CERT_STRUCTURAL == 0
    got, want = dev_certify(ctx, pr, faces, res, FEAS), cm.certify(pr, faces, res, FEAS)
    assert_same(got, want, "every second record spoilt")
    zero = np.zeros((), dtype=abi.certificate_dtype)
    for j, (name, _, _, flag) in enumerate(cases):
        assert got[2 * j].tobytes() == alone[0].tobytes() and got[2 * j + 2].tobytes() == alone[0].tobytes(), name
        g = got[2 * j + 1]
        if flag is None:
            assert g["flags"] & abi.FH_CERT_STRUCTURAL == 0, name
        elif flag == 0:
            assert g.tobytes() == alone[0].tobytes(), name
        else:
            zero["flags"] = flag
            assert g.tobytes() == zero.tobytes(), (name, g)
    assert_same(dev_certify(ctx, pr, faces, res), cm.certify(pr, faces, res), "the same without tolerances: only the structural bits")


def report(name, cert, solved):
    ok = solved & ((cert["flags"] & abi.FH_CERT_STRUCTURAL) == 0)
    worst = {k: float(cert[k][ok].max()) for k in cm.NUMBERS if k not in ("cost", "v_peak", "a_peak")} if ok.any() else {}
    print("%s: %d of %d solved; worst %s; v_peak %.3f a_peak %.3f" % (name, int(ok.sum()), len(cert), {k: "%.2e" % v for k, v in worst.items()},
                                                                      cert["v_peak"][ok].max() if ok.any() else 0, cert["a_peak"][ok].max() if ok.any() else 0))


def check_solver_output(c, name, pr, faces, res):
    got = dev_certify(c, pr, faces, res, FEAS)
    solved = res["solved"] == 1
    report(name, got, solved)
    assert_same(got, cm.certify(pr, faces, res, FEAS), name)
    assert np.array_equal(got["flags"][~solved], np.full(int((~solved).sum()), abi.FH_CERT_UNSOLVED)), name
    flagged = np.nonzero(solved & (got["flags"] != 0))[0]
    assert len(flagged) == 0, "%s: results %s exceed feas_tol = 1e-9: flags %s, %s" % (
        name, flagged[:8], got["flags"][flagged[:8]], [{k: got[k][i] for k in cm.NUMBERS} for i in flagged[:2]])
    return int(solved.sum())


def test_what_the_solver_returns_is_certified_at_feas_tol(ctx):
    """The fused pairs of whole_batch(256, 7) (whole and safe, N = 10, the safe problems and rows as the launch wrote them) and 64
    problems at N = 15 with up to 8 polytopes: the device certificate of the device's results equals the model's bit for bit, and no
    solved result has a flag under tol = feas_tol = 1e-9 in every member."""
    import torch

    B, N = 256, 10
    whole, faces, _ = corridor.whole_batch(B, 7)
    tmpl = corridor.safe_templates(whole)
    mf = int(whole["face_off"][np.arange(B), whole["n_poly"]].max())
    d_w, d_f, d_s = to_dev(whole), to_dev(faces), to_dev(tmpl)
    d_sf = torch.zeros_like(d_f)
    d_wr = torch.zeros(B * abi.result_dtype.itemsize, dtype=torch.uint8, device=DEV)
    d_sr = torch.zeros_like(d_wr)
    ctx.set_pair_margin(0.05)
    try:
        ctx.solve_pairs_device(d_w.data_ptr(), d_f.data_ptr(), B, N, mf, 0.5, 0.2, 3, d_wr.data_ptr(), d_s.data_ptr(), d_sf.data_ptr(), d_sr.data_ptr())
        ctx.sync()
    finally:
        ctx.set_pair_margin(-1.0)
    wres, sres = d_wr.cpu().numpy().view(abi.result_dtype), d_sr.cpu().numpy().view(abi.result_dtype)
    safe, sfaces = d_s.cpu().numpy().view(abi.problem_dtype), d_sf.cpu().numpy().view(abi.face_dtype)
    assert check_solver_output(ctx, "whole, N = 10", whole, faces, wres) > B // 2
    assert check_solver_output(ctx, "safe, N = 10", safe, sfaces, sres) > B // 4
    pr, fc, _ = corridor.whole_batch(64, 9, n_seg=15, p_choices=(4, 6, 8))
    assert check_solver_output(ctx, "whole, N = 15", pr, fc, ctx.solve_batch(pr, fc)) > 32


def test_host_form_and_a_solve_launch_on_another_context(ctx):
    """fh_certify_batch gives the bits of the device form; so does certifying on this context while another context runs a solve launch
    (the kernel uses no working buffer of any context)."""
    import torch

    pr, faces, res = synthetic(96, 4)
    tol = abi.certify_tol(0.5, 1.0, 1.0, 0.1)
    want = dev_certify(ctx, pr, faces, res, tol)
    assert_same(want, cm.certify(pr, faces, res, tol), "device form")
    assert_same(ctx.certify_batch(pr, faces, res, tol), want, "host form")
    assert_same(ctx.certify_batch(pr, faces, res), dev_certify(ctx, pr, faces, res), "host form, no tolerances")
    assert len(ctx.certify_batch(pr[:0], faces, res[:0])) == 0
    B = 4096
    whole, wf, _ = corridor.whole_batch(B, 11)
    mf = int(whole["face_off"][np.arange(B), whole["n_poly"]].max())
    other = capi.Context(0)
    try:
        d_w, d_f = to_dev(whole), to_dev(wf)
        d_wr = torch.zeros(B * abi.result_dtype.itemsize, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        during = dev_certify(ctx, pr, faces, res, tol,
                             before=lambda: other.solve_batch_device(d_w.data_ptr(), d_f.data_ptr(), B, 10, mf, d_wr.data_ptr()))
        other.sync()
        solved = d_wr.cpu().numpy().view(abi.result_dtype)["solved"]
    finally:
        other.close()
    assert_same(during, want, "next to a solve launch")
    assert solved.mean() > 0.5


def test_fleet_certify_equals_the_model_and_changes_nothing():
    """Four vehicles of the forest scene of tests/test_gpu_fleet.py, one cycle; vehicle 3 starts at its goal.  Fleet.certify() equals the
    model on the problems, rows and results fetched from the fleet; the vehicle that has arrived is UNSOLVED in both; and vehicles, plans
    and results are those of a fleet that was never asked."""
    import test_gpu_fleet as tf

    B = 4
    sc = tf.scenario(B, 1, 31)
    sc["goals"][:, 2] = np.minimum(sc["goals"][:, 2], 2.0)   # (the scene sends three vehicles above the map: bring them back)
    sc["goals"][3] = sc["states"]["pos"][3]
    seen = []
    for ask in (True, False):
        fl = tf.make_fleet(sc, B)
        try:
            fl.set_unknown(sc["flags"][0], sc["origin"], tf.P["res"], sc["dims"])
            fl.replan()
            if ask:
                plain, cert = fl.certify(), fl.certify(FEAS)
                rows = fl.faces()
            seen.append((fl.vehicles(), fl.plans(), fl.results()))
        finally:
            fl.close()
    (v, plans, r), (v2, plans2, r2) = seen
    assert v.tobytes() == v2.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(plans, plans2))
    assert all(np.asarray(r[k]).tobytes() == np.asarray(r2[k]).tobytes() for k in r)
    for kind, pk, rk in (("whole", "whole", "wres"), ("safe", "safe", "sres")):
        assert_same(cert[kind], cm.certify(r[pk], rows[kind], r[rk], FEAS), "fleet, " + kind)
        assert_same(plain[kind], cm.certify(r[pk], rows[kind], r[rk]), "fleet, %s, no tolerances" % kind)
        report("fleet " + kind, cert[kind], r[rk]["solved"] == 1)
        assert np.array_equal(cert[kind]["flags"] == abi.FH_CERT_UNSOLVED, r[rk]["solved"] == 0)
    assert v["status"][3] == abi.FH_VEHICLE_GOAL_REACHED
    assert cert["whole"]["flags"][3] == abi.FH_CERT_UNSOLVED and cert["safe"]["flags"][3] == abi.FH_CERT_UNSOLVED
    assert (cert["whole"]["flags"] == 0).any(), cert["whole"]["flags"]
