"""Every launch argument the solve kernel reads, on a path where a wrong value shows.

The kernel takes its arguments as single scalar values (Solver / SolveArgs / ShareArgs fields split at kernel entry).  What
can go wrong there is one field read as another, or read stale, on a path the bench batch seldom takes: so each field gets a case in
which another value changes something a caller can observe.  Expected values are the CPU oracle's (tests/test_gpu_parity.py's bars:
feasibility flag, trials, factor, dt and status exact, cost 1e-7 relative, coefficients 1e-6 absolute), for statuses the contract of
include/fasterhip.h; where two settings must not change a result, the runs are also compared with each other bit for bit.

Shapes: 256 problems (whole_batch, fixed seeds) at N = 6, 10 and 15 and 16 problems at N = 16 (the fourth kernel bucket), as plain
launches and as fused pairs with lazy and complete pair outputs.  A batch of 256 is no larger than the grid: workgroups that are done
wait for frames, so that min_nodes = 1, look_every = 2 make trees change hands at this size (asserted from share_stats()).
"""
import numpy as np
import pytest
import torch  # noqa: F401  (before libfasterhip.so is loaded: one HIP runtime per process)

from faster_amd import abi, capi, corridor

pytestmark = pytest.mark.gpu

RS = abi.result_dtype.itemsize
WORK = ("nodes", "qp_iters", "kflops")  # work counters: they depend on which wavefronts shared a tree
FIELDS = [f for f in abi.result_dtype.names if f not in WORK]
BATCHES = {6: dict(n=256, seed=5, p_choices=(2, 3, 4)), 10: dict(n=256, seed=3, p_choices=(4, 5, 6)),
           15: dict(n=256, seed=7, p_choices=(6, 7, 8)), 16: dict(n=16, seed=41, p_choices=(abi.FH_MAX_POLY,))}
PAIR = dict(r_frac=0.5, shrink=0.2, max_safe_poly=3, r_margin=0.05)
FORCE = dict(min_nodes=1, look_every=2, backlog=32)  # sharing at this size: one node is enough to give; look_every = 2 is the shortest
# period fh_set_sched accepts (a power of two >= 2): a tree looks at every second node, a shared one (look_mask >> 1) at every node


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


def _bytes(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(len(a), -1)


def same_bits(a, b, rows=None, fields=FIELDS):
    """Per-record mask: the fields equal bit for bit (coefficient rows < rows)."""
    eq = np.ones(len(a), dtype=bool)
    for f in fields:
        x, y = (a[f], b[f]) if f != "coeff" or rows is None else (a[f][:, :rows], b[f][:, :rows])
        eq &= (_bytes(x) == _bytes(y)).all(axis=1)
    return eq


def compare(got, ref, cost_rtol=1e-7, coeff_atol=1e-6):
    """The bars of tests/test_gpu_parity.py."""
    for f in ("solved", "trials", "factor", "dt", "status"):
        assert np.array_equal(got[f], ref[f]), (f, np.flatnonzero(got[f] != ref[f])[:8])
    ok = ref["solved"] == 1
    np.testing.assert_allclose(got["cost"][ok], ref["cost"][ok], rtol=cost_rtol, atol=1e-9)
    np.testing.assert_allclose(got["coeff"][ok], ref["coeff"][ok], rtol=0, atol=coeff_atol)
    return ok


@pytest.fixture(scope="module")
def cases(oracle):
    """The batches and the oracle's answers to their whole problems, computed once and left unchanged."""
    out = {}
    for N, b in BATCHES.items():
        whole, faces, _ = corridor.whole_batch(b["n"], seed=b["seed"], n_seg=N, p_choices=b["p_choices"])
        ref = oracle.solve_batch(whole, faces)
        ref.setflags(write=False)
        out[N] = (whole, faces, corridor.safe_templates(whole), ref)
    # trees large enough to change hands (the forced-sharing cases rest on this, not on what the device did)
    for N in (10, 15):
        assert (out[N][3]["nodes"] >= 8).sum() >= 8
    return out


def make_ctx(params=None, pair=PAIR, **sched):
    c = capi.Context(0, pair_outputs=bool(sched.pop("pair_outputs", 1)), compact_results=bool(sched.pop("compact_results", 0)))
    if params:
        par = abi.default_params()
        for k, v in params.items():
            par[k] = v
        c.set_params(par)
    c.set_pair_margin(pair["r_margin"])
    if sched:
        c.set_sched(**sched)
    return c


def max_faces(pr):
    return int(pr["face_off"][np.arange(len(pr)), np.clip(pr["n_poly"], 0, abi.FH_MAX_POLY)].max())


def launch_plain(c, pr, faces, N, fill=0xAB):
    n = len(pr)
    d_pr, d_faces = _dev(pr), _dev(faces)
    d_res = torch.full((n * RS,), fill, dtype=torch.uint8, device="cuda:0")
    c.solve_batch_device(d_pr.data_ptr(), d_faces.data_ptr(), n, N, max_faces(pr), d_res.data_ptr())
    c.sync()
    return d_res.cpu().numpy().view(abi.result_dtype).copy()


def launch_pairs(c, whole, faces, tmpl, N, pair=PAIR, fused=True, fill=0xAB):
    """One fused launch (or the three launches it stands for); host copies of (whole results, safe results, safe problems, safe rows)."""
    B, mf = len(whole), max_faces(whole)
    d_whole, d_faces, d_safe = _dev(whole), _dev(faces), _dev(tmpl)
    d_sf = torch.zeros_like(d_faces)
    d_wr = torch.full((B * RS,), fill, dtype=torch.uint8, device="cuda:0")
    d_sr = torch.full((B * RS,), fill, dtype=torch.uint8, device="cuda:0")
    a = (pair["r_frac"], pair["shrink"], pair["max_safe_poly"])
    if fused:
        c.solve_pairs_device(d_whole.data_ptr(), d_faces.data_ptr(), B, N, mf, *a, d_wr.data_ptr(), d_safe.data_ptr(), d_sf.data_ptr(), d_sr.data_ptr())
    else:
        c.solve_batch_device(d_whole.data_ptr(), d_faces.data_ptr(), B, N, mf, d_wr.data_ptr())
        c.pair_glue_device(d_whole.data_ptr(), d_wr.data_ptr(), d_faces.data_ptr(), B, *a, d_safe.data_ptr(), d_sf.data_ptr())
        c.solve_batch_device(d_safe.data_ptr(), d_sf.data_ptr(), B, N, mf, d_sr.data_ptr())
    c.sync()
    return (d_wr.cpu().numpy().view(abi.result_dtype).copy(), d_sr.cpu().numpy().view(abi.result_dtype).copy(),
            d_safe.cpu().numpy().view(abi.problem_dtype).copy(), d_sf.cpu().numpy().view(abi.face_dtype).copy())


def safe_reference(oracle, whole, wres, faces, tmpl, pair=PAIR):
    """The oracle's answers to the safe problems of the host restatement of the hand-off (oracle/pair_glue.py), fed with the whole results
    at hand — already held against the oracle — so that rounding cannot fork the hand-off."""
    from oracle import pair_glue

    safe, sfaces = pair_glue.glue(whole, wres, faces, tmpl, pair["r_frac"], pair["shrink"], pair["max_safe_poly"], pair["r_margin"])
    return safe, sfaces, oracle.solve_batch(safe, sfaces)


def check_pairs(oracle, case, out, pair=PAIR, pair_outputs=True):
    whole, faces, tmpl, wref = case
    wres, sres, safe, _ = out
    compare(wres, wref)
    safe_ref, _, sref = safe_reference(oracle, whole, wres, faces, tmpl, pair)
    compare(sres, sref)
    if pair_outputs:
        for f in ("n_seg", "n_poly", "face_off"):
            assert np.array_equal(safe[f], safe_ref[f]), f
        np.testing.assert_allclose(safe["x0"], safe_ref["x0"], rtol=0, atol=1e-11)
    return sref


# ---- plain launches and fused pairs, every kernel bucket ----

@pytest.mark.parametrize("N", [6, 10, 15, 16])
def test_plain_launch(oracle, cases, N):
    """n, max_faces, the tolerances, workspace, basis, the result pointer: the oracle's answers in all four buckets."""
    whole, faces, _, ref = cases[N]
    c = make_ctx()
    try:
        got = launch_plain(c, whole, faces, N)
        assert c.last_launch()[0]["n_seg"] == N and c.last_launch()[0]["pairs"] == 0
    finally:
        c.close()
    compare(got, ref)


@pytest.mark.parametrize("pair_outputs", [0, 1], ids=["lazy", "complete"])
@pytest.mark.parametrize("N", [6, 10, 15, 16])
def test_fused_pairs(oracle, cases, N, pair_outputs):
    """safe, sfaces, sres and the pair parameters: whole and safe results are the oracle's, with lazy and with complete pair outputs; with
    lazy outputs the template fields of the safe records are never written."""
    whole, faces, tmpl, _ = cases[N]
    c = make_ctx(pair_outputs=pair_outputs)
    try:
        out = launch_pairs(c, whole, faces, tmpl, N)
        assert c.last_launch()[0]["n_seg"] == N and c.last_launch()[0]["pairs"] == 1
    finally:
        c.close()
    sref = check_pairs(oracle, cases[N], out, pair_outputs=bool(pair_outputs))
    assert sref["solved"].sum() >= len(whole) // 4
    if not pair_outputs:
        for f in ("n_seg", "force_final_pos", "dc", "v_max", "a_max", "j_max", "f_init", "f_final", "f_inc", "xf", "pin"):
            assert (_bytes(out[2][f]) == _bytes(tmpl[f])).all(), f


# ---- sharing forced at this size ----

@pytest.mark.parametrize("waiting", [0, 1], ids=["default-waiters", "one-waiter"])
@pytest.mark.parametrize("N", [10, 15])
def test_plain_launch_shared(oracle, cases, N, waiting):
    """ctl, seqs, slots, slot_stride, recs, enabled, total_units, max_hungry, min_nodes, backlog, look_mask, giant_factor: frames change
    hands (share_stats), and the results are the bits of share = 0 and the oracle's."""
    whole, faces, _, ref = cases[N]
    c = make_ctx(params=dict(share=0))
    try:
        alone = launch_plain(c, whole, faces, N)
    finally:
        c.close()
    compare(alone, ref)
    sched = dict(FORCE, waiting_workgroups=waiting) if waiting else dict(FORCE)
    c = make_ctx(**sched)
    try:
        got = launch_plain(c, whole, faces, N)
        stats = c.share_stats()
    finally:
        c.close()
    print("N = %d, waiting_workgroups %d: %s" % (N, waiting, stats))
    assert stats["error"] == 0 and stats["donated"] > 0 and stats["stolen"] > 0 and stats["records_used"] > 0
    assert same_bits(got, alone).all(), np.flatnonzero(~same_bits(got, alone))[:8]
    compare(got, ref)


@pytest.mark.parametrize("waiting", [0, 1], ids=["default-waiters", "one-waiter"])
@pytest.mark.parametrize("pair_outputs", [0, 1], ids=["lazy", "complete"])
def test_fused_pairs_shared(oracle, cases, pair_outputs, waiting):
    """The same for pairs; with lazy outputs a safe problem that is shared is written to memory when its first frame is given
    (whole, wfaces, safe, sfaces, shrink, r_margin of ShareArgs)."""
    N = 10
    whole, faces, tmpl, _ = cases[N]
    c = make_ctx(params=dict(share=0), pair_outputs=pair_outputs)
    try:
        alone = launch_pairs(c, whole, faces, tmpl, N)
    finally:
        c.close()
    check_pairs(oracle, cases[N], alone, pair_outputs=bool(pair_outputs))
    sched = dict(FORCE, waiting_workgroups=waiting) if waiting else dict(FORCE)
    c = make_ctx(pair_outputs=pair_outputs, **sched)
    try:
        got = launch_pairs(c, whole, faces, tmpl, N)
        stats = c.share_stats()
    finally:
        c.close()
    print("pairs, pair_outputs %d, waiting_workgroups %d: %s" % (pair_outputs, waiting, stats))
    assert stats["error"] == 0 and stats["donated"] > 0 and stats["stolen"] > 0 and stats["records_used"] > 0
    for a, b, what in ((got[0], alone[0], "whole"), (got[1], alone[1], "safe")):
        assert same_bits(a, b).all(), (what, np.flatnonzero(~same_bits(a, b))[:8])
    if pair_outputs:
        assert np.array_equal(got[2], alone[2]) and np.array_equal(got[3], alone[3])
    check_pairs(oracle, cases[N], got, pair_outputs=bool(pair_outputs))


# ---- limits (fh_params) ----

@pytest.mark.parametrize("N", [6, 10, 15])
def test_node_cap(oracle, cases, N):
    """max_nodes = 1, one wavefront per problem: only the root of a trial is opened, and that root is the oracle's — so every record is
    the oracle's under the same cap: FH_ST_NODE_LIMIT with solved = 0 where the cap bit in the last trial, the sequential rule's
    answer elsewhere."""
    whole, faces, _, _ = cases[N]
    par = abi.default_params()
    par["max_nodes"] = 1
    capped = oracle.solve_batch(whole, faces, params=par)
    assert (capped["status"] == abi.FH_ST_NODE_LIMIT).sum() >= 8 and (capped["solved"] == 1).sum() >= 8
    c = make_ctx(params=dict(max_nodes=1, share=0))
    try:
        got = launch_plain(c, whole, faces, N)
    finally:
        c.close()
    compare(got, capped)
    assert not got["solved"][got["status"] == abi.FH_ST_NODE_LIMIT].any()


@pytest.mark.parametrize("N", [6, 10, 15])
def test_iteration_cap(oracle, cases, N):
    """max_iters = 1, one wavefront per problem.  The kernel and the oracle do not count the iterations of a QP alike (the kernel
    answers some roots without one), so the oracle under the same cap is no reference here; the contract is.  A trial in which a QP
    runs into the cap ends FH_ST_ITER_LIMIT whatever it had found, and the next factor is tried: so the cap can only lose trials —
    the factor that works is the uncapped one or a later one — and a record that says solved comes from a trial that ran to its end
    within the cap: it is the oracle's answer for that factor alone.  A problem whose last trial ran into the cap says
    FH_ST_ITER_LIMIT, unsolved."""
    whole, faces, _, ref = cases[N]
    c = make_ctx(params=dict(max_iters=1, share=0))
    try:
        got = launch_plain(c, whole, faces, N)
    finally:
        c.close()
    lim = got["status"] == abi.FH_ST_ITER_LIMIT
    ok = got["solved"] == 1
    print("N = %d, max_iters 1: %d solved, %d at the limit, %d at a later factor" % (N, ok.sum(), lim.sum(), (got["factor"][ok] > ref["factor"][ok]).sum()))
    assert lim.any() and not got["solved"][lim].any()
    assert set(np.unique(got["status"])) <= {abi.FH_ST_OPTIMAL, abi.FH_ST_INFEASIBLE, abi.FH_ST_ITER_LIMIT}
    assert np.array_equal(ok, got["status"] == abi.FH_ST_OPTIMAL)
    assert np.all(ref["solved"][ok] == 1) and np.all(got["factor"][ok] >= ref["factor"][ok]) and np.all(got["trials"][ok] >= ref["trials"][ok])
    one = whole[ok].copy()  # the factor each of them reports, alone
    one["f_init"] = got["factor"][ok]
    one["f_final"] = got["factor"][ok]
    at = oracle.solve_batch(one, faces)
    assert np.all(at["solved"] == 1)
    for f in ("factor", "dt"):
        assert np.array_equal(got[f][ok], at[f]), f
    np.testing.assert_allclose(got["cost"][ok], at["cost"], rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(got["coeff"][ok], at["coeff"], rtol=0, atol=1e-6)


@pytest.mark.parametrize("N", [10, 15])
def test_work_cap(oracle, cases, N):
    """max_work = 40: a problem over the cap ends FH_ST_ITER_LIMIT, unsolved; the cap is tested between nodes; the others are the oracle's."""
    whole, faces, _, ref = cases[N]
    c = make_ctx(params=dict(max_work=40))
    try:
        got = launch_plain(c, whole, faces, N)
        assert c.share_stats()["donated"] == 0  # (a work cap couples the nodes of a problem: no sharing)
    finally:
        c.close()
    over = got["status"] == abi.FH_ST_ITER_LIMIT
    assert over.sum() >= 8 and (~over).sum() >= 8
    assert not got["solved"][over].any()
    assert np.all(got["qp_iters"] <= 40 + abi.default_params()["max_iters"])
    assert np.all(got["qp_iters"][over] >= 40)
    compare(got[~over], ref[~over])


@pytest.mark.parametrize("N", [10, 15])
def test_mip_gap(oracle, cases, N):
    """mip_gap = 0.05 (sharing off): a gap prunes only against an incumbent, so feasibility, trials, factor and dt are the exact
    ones, and the cost lies between the optimum and optimum / (1 - gap)."""
    whole, faces, _, ref = cases[N]
    gap = 0.05
    c = make_ctx(params=dict(mip_gap=gap), **FORCE)
    try:
        got = launch_plain(c, whole, faces, N)
        stats = c.share_stats()
    finally:
        c.close()
    assert stats["donated"] == 0 and stats["stolen"] == 0
    for f in ("solved", "trials", "factor", "dt", "status"):
        assert np.array_equal(got[f], ref[f]), f
    ok = ref["solved"] == 1
    assert np.all(got["cost"][ok] >= ref["cost"][ok] * (1 - 1e-7))
    assert np.all(got["cost"][ok] * (1 - gap) <= ref["cost"][ok] * (1 + 1e-7))


# ---- scheduling fields that must not change a result ----

@pytest.mark.parametrize("N", [10, 15])
def test_child_bound_on_and_off(oracle, cases, N):
    whole, faces, _, ref = cases[N]
    outs = []
    for on in (1, 0):
        c = make_ctx(params=dict(share=0), child_bound=on)
        try:
            outs.append(launch_plain(c, whole, faces, N))
        finally:
            c.close()
        compare(outs[-1], ref)
    assert same_bits(outs[0], outs[1]).all()
    assert np.all(outs[0]["nodes"] <= outs[1]["nodes"]) and outs[0]["nodes"].sum() < outs[1]["nodes"].sum()  # the bound did skip children


@pytest.mark.parametrize("N", [6, 10])
def test_compact_results_on_and_off(oracle, cases, N):
    """compact_results = 1 writes the rows the kernel is built for; 0 writes all FH_MAX_SEG rows, zeros beyond the problem's."""
    whole, faces, _, ref = cases[N]
    outs = []
    for compact in (0, 1):
        c = make_ctx(compact_results=compact)
        try:
            outs.append(launch_plain(c, whole, faces, N, fill=0xAB))
        finally:
            c.close()
    full, comp = outs
    compare(full, ref)
    assert same_bits(full, comp, rows=N).all()
    assert not full["coeff"][:, N:].any()


def test_launch_order(oracle):
    """launch_order 0 / 1 / 2 on a batch large enough to be sorted (>= 2048 units): the order table is read, the results are the same."""
    N, B = 10, 2048
    whole, faces, _ = corridor.whole_batch(B, seed=2, n_seg=N, p_choices=(2, 3, 4, 5, 6))
    ref = oracle.solve_batch(whole, faces)
    outs = []
    for order in (0, 1, 2):
        c = make_ctx(launch_order=order)
        try:
            outs.append(launch_plain(c, whole, faces, N))
        finally:
            c.close()
        compare(outs[-1], ref)
    assert same_bits(outs[0], outs[1]).all() and same_bits(outs[0], outs[2]).all()


# ---- pair fields ----

PAIR_VARIANTS = [("base", {}), ("r_frac", dict(r_frac=0.3)), ("shrink", dict(shrink=0.05)), ("r_margin", dict(r_margin=0.2)),
                 ("max_safe_poly", dict(max_safe_poly=1))]


def test_pair_fields(oracle, cases):
    """r_frac, shrink, r_margin, max_safe_poly at two values each: the fused kernel gives what fh_pair_glue_device followed by
    fh_solve_batch_device gives (whole results, safe problems, safe rows, safe results), the safe results are the oracle's, and the
    second value of every field changes the safe problems."""
    N = 10
    whole, faces, tmpl, _ = cases[N]
    base = None
    for name, delta in PAIR_VARIANTS:
        pair = dict(PAIR, **delta)
        outs = []
        for fused in (False, True):
            c = make_ctx(pair=pair)
            try:
                outs.append(launch_pairs(c, whole, faces, tmpl, N, pair=pair, fused=fused))
            finally:
                c.close()
        three, one = outs
        assert same_bits(three[0], one[0]).all() and same_bits(three[1], one[1]).all(), name
        assert np.array_equal(three[2], one[2]) and np.array_equal(three[3], one[3]), name
        check_pairs(oracle, cases[N], one, pair=pair)
        if base is None:
            base = one
        else:
            assert not (np.array_equal(one[2], base[2]) and np.array_equal(one[3], base[3])), name


# ---- stop word and deadline ----

def _interrupted_or_reference(got, ref, rows):
    hit = got["status"] == abi.FH_ST_INTERRUPTED
    eq = same_bits(got, ref, rows=rows)
    assert np.all(eq | hit), np.flatnonzero(~(eq | hit))[:8]
    assert not got["solved"][hit].any()
    return hit


@pytest.mark.parametrize("how", ["stop", "deadline"])
@pytest.mark.parametrize("pair_outputs", [0, 1], ids=["lazy", "complete"])
def test_pairs_stopped_before_the_launch(oracle, cases, pair_outputs, how):
    """host_abort (a stop word raised before the launch) and deadline_ticks (a deadline of 100 ns: expired when the first ticket is
    drawn): every result is the un-stopped launch's (held against the oracle) or FH_ST_INTERRUPTED and unsolved, a pair whose whole
    problem was interrupted has an interrupted safe result, and the launch says it was interrupted."""
    N = 10
    whole, faces, tmpl, _ = cases[N]
    c = make_ctx(pair_outputs=pair_outputs)
    try:
        ref = launch_pairs(c, whole, faces, tmpl, N)
    finally:
        c.close()
    check_pairs(oracle, cases[N], ref, pair_outputs=bool(pair_outputs))
    c = make_ctx(params=dict(deadline_ms=1e-4) if how == "deadline" else None, pair_outputs=pair_outputs)
    try:
        if how == "stop":
            c.request_stop()
        try:
            got = launch_pairs(c, whole, faces, tmpl, N)
            stats = c.share_stats()
        finally:
            c.clear_stop()
    finally:
        c.close()
    assert stats["interrupted"] != 0 and stats["error"] == 0
    w_int = _interrupted_or_reference(got[0], ref[0], N)
    s_int = _interrupted_or_reference(got[1], ref[1], N)
    print("%s, pair_outputs %d: %d whole and %d safe results of %d interrupted" % (how, pair_outputs, w_int.sum(), s_int.sum(), len(whole)))
    assert w_int.any() and not (w_int & ~s_int).any()
