"""The return code of every fh_* entry point that takes a context, a map or a pool, for one well-formed call and one call per argument
clause it checks: a negative count, a null pointer, an out-of-range cap, a bad grid, a bad rule.  No GPU is needed: the context is one
without a device (fh_create with a device index no machine has keeps the handle and returns FH_ERR_DEVICE), the pool one without devices
(fh_pool_create with such an index), and no map exists without a device, so the map entry points are called without one.  The order of
an entry point's checks is part of its behaviour — arguments that are checked before the device give FH_ERR_ARG (-1), everything after it
FH_ERR_DEVICE (-2) — and the host layer may be rearranged without changing it.

THE EXPECTED CODES ARE LITERALS TAKEN FROM THE PARENT COMMIT of the change that introduced this file (the host-layer refactor: named
buffers, fh_host.hpp): the table below was run against a build of that commit before any of its code was touched, and passes unchanged
since.  A code that changes here is a change of the ABI's behaviour, not of a tolerance."""
import ctypes

import numpy as np
import pytest

from safe_corridor_edge_cases import SAFE_PATH_CAP
from faster_amd import abi

OK, ARG, DEV = 0, -1, -2
NO_SUCH_DEVICE = 1 << 20
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def L():
    from faster_amd import build as fb
    from faster_amd import capi

    fb.build_all()
    return capi.lib()


def grid(res=0.2, dims=(8, 8, 4)):
    g = np.zeros(1, dtype=abi.voxel_grid_dtype)
    g["origin"], g["res"], g["dims"] = (0, 0, 0), res, dims
    return g


def record(base, **fields):
    r = np.array(base).reshape(1).copy()
    for k, v in fields.items():
        if k.startswith("rule_"):
            r["rule"][k[5:]] = v
        else:
            r[k] = v
    return r


def context_table():
    """(entry point, arguments after the context, expected code).  `d` is a valid host address that no call of this table dereferences."""
    buf = np.zeros(4096, dtype=np.uint8)
    d, p = abi.ptr(buf), abi.ptr
    keep = [buf]

    def k(a):   # numpy records must outlive the table
        keep.append(a)
        return p(a)

    g, bbox = k(grid()), k(np.array([2.0, 2.0, 1.0]))
    g_res, g_dims, g_huge = k(grid(res=0.0)), k(grid(dims=(8, 0, 4))), k(grid(dims=(2048, 2048, 512)))
    sched, par = abi.default_sched(), abi.default_params()
    rule = np.zeros((), dtype=abi.pair_rule_dtype)
    rule["delta_h"], rule["delta_a"] = 1.0, 0.5
    fp, yp = abi.default_fleet_params(), abi.default_yaw_params()
    fpp, ypp = k(record(fp)), k(record(yp))
    fake_map = ctypes.c_void_p(1)   # (never read: a context without a device returns before it asks the map)
    t = [
        # ---- settings: stored without a device
        ("fh_set_sched", (k(record(sched)),), OK),
        ("fh_set_sched", (None,), ARG),
        ("fh_set_sched", (k(record(sched, struct_size=8)),), ARG),
        ("fh_set_sched", (k(record(sched, struct_size=0)),), OK),
        ("fh_set_sched", (k(record(sched, publish_factor=-1)),), ARG),
        ("fh_set_sched", (k(record(sched, backlog=513)),), ARG),
        ("fh_set_sched", (k(record(sched, backlog=512)),), OK),
        ("fh_set_sched", (k(record(sched, workgroups_per_cu=-1)),), ARG),
        ("fh_set_sched", (k(record(sched, launch_order=3)),), ARG),
        ("fh_set_sched", (k(record(sched, look_every=3)),), ARG),
        ("fh_set_sched", (k(record(sched, look_every=2048)),), ARG),
        ("fh_set_sched", (k(record(sched, look_every=16)),), OK),
        ("fh_set_params", (k(record(par)),), OK),
        ("fh_set_params", (None,), ARG),
        ("fh_set_params", (k(record(par, feas_tol=0.0)),), ARG),
        ("fh_set_params", (k(record(par, dep_tol=NAN)),), ARG),
        ("fh_set_params", (k(record(par, max_nodes=0)),), ARG),
        ("fh_set_params", (k(record(par, max_iters=0)),), ARG),
        ("fh_set_params", (k(record(par, max_work=-1)),), ARG),
        ("fh_set_params", (k(record(par, mip_gap=1.0)),), ARG),
        ("fh_set_params", (k(record(par, deadline_ms=INF)),), ARG),
        ("fh_set_stream", (None,), OK),
        ("fh_set_pair_margin", (0.1,), OK),
        ("fh_set_pair_margin", (-3.0,), OK),
        ("fh_set_pair_margin", (NAN,), ARG),
        ("fh_set_pair_rule", (k(record(rule)),), OK),
        ("fh_set_pair_rule", (None,), ARG),
        ("fh_set_pair_rule", (k(record(rule, mode=3)),), ARG),
        ("fh_set_pair_rule", (k(record(rule, mode=1, r_known=0.0)),), ARG),
        ("fh_set_pair_rule", (k(record(rule, mode=1, r_known=4.0)),), OK),
        ("fh_set_pair_rule", (k(record(rule, mode=2, drone_radius=0.0)),), ARG),
        ("fh_set_pair_rule", (k(record(rule, mode=2, drone_radius=0.4, delta_a=0.0)),), ARG),
        ("fh_set_pair_rule", (k(record(rule, mode=2, drone_radius=0.4)),), OK),     # (mode 2 stays set for the calls below: no grid yet)
        ("fh_pair_glue_device", (d, d, d, 4, 0.5, 0.2, 3, d, d), DEV),
        ("fh_set_unknown_grid_device", (g, d), OK),
        ("fh_set_unknown_grid_device", (None, None), OK),
        ("fh_set_unknown_grid_device", (None, d), ARG),
        ("fh_set_unknown_grid_device", (g_res, d), ARG),
        ("fh_set_unknown_grid_device", (g_dims, d), ARG),
        ("fh_set_unknown_grid_device", (g_huge, d), ARG),
        ("fh_set_unknown_views_device", (g, d, 256, None, 4), OK),
        ("fh_set_unknown_views_device", (None, None, 0, None, 0), OK),
        ("fh_set_unknown_views_device", (g, d, 256, None, 0), ARG),
        ("fh_set_unknown_views_device", (None, d, 256, None, 4), ARG),
        ("fh_set_unknown_views_device", (g_dims, d, 256, None, 4), ARG),
        ("fh_set_unknown_views_device", (g, d, 255, None, 4), ARG),
        ("fh_set_unknown_views_device", (g_res, d, 256, None, 4), ARG),
        ("fh_set_unknown_views_device", (g_huge, d, 1 << 31, None, 4), ARG),
        ("fh_set_pair_rule", (k(record(rule)),), OK),
        ("fh_set_sense_staging", (0,), OK),
        ("fh_set_sense_staging", (1,), OK),
        ("fh_set_sense_staging", (2,), ARG),
        ("fh_fleet_set_headings_device", (d, 4), OK),
        ("fh_fleet_set_headings_device", (d, 0), ARG),
        ("fh_fleet_set_headings_device", (None, 0), OK),
        ("fh_timing_reset", (), OK),
        ("fh_last_launch", (d,), ARG),        # (no launch yet)
        ("fh_last_launch", (None,), ARG),
        # ---- everything else needs the device, after its own argument checks
        ("fh_request_stop", (), DEV),
        ("fh_clear_stop", (), DEV),
        ("fh_sync", (), DEV),
        ("fh_share_stats_read", (d,), DEV),
        ("fh_share_stats_read", (None,), ARG),
        ("fh_share_profile_read", (d,), DEV),
        ("fh_share_profile_read", (None,), ARG),
        ("fh_fp64_peak", (d,), DEV),
        ("fh_fp64_peak", (None,), ARG),
        ("fh_timing_read", (d, 8), DEV),
        ("fh_timing_read", (None, 0), DEV),
        ("fh_timing_read", (d, -1), ARG),
        ("fh_timing_read", (None, 8), ARG),
        ("fh_pack_results_device", (d, 4, 6, d), DEV),
        ("fh_pack_results_device", (d, -1, 6, d), ARG),
        ("fh_pack_results_device", (d, 4, 0, d), ARG),
        ("fh_pack_results_device", (d, 4, 17, d), ARG),
        ("fh_pack_results_device", (None, 4, 6, d), DEV),    # (pointers are looked at after the device)
        ("fh_solve_batch_device", (d, d, 4, 10, 64, d), DEV),
        ("fh_solve_batch_device", (d, d, -1, 10, 64, d), ARG),
        ("fh_solve_batch_device", (d, d, 4, 99, 9999, d), DEV),   # (caps out of range mean the largest)
        ("fh_solve_batch_device", (None, d, 4, 10, 64, d), DEV),
        ("fh_solve_batch", (d, d, 8, 4, d), DEV),
        ("fh_solve_batch", (d, d, 8, -1, d), ARG),
        ("fh_solve_batch", (d, d, -1, 4, d), ARG),
        ("fh_solve_batch", (None, d, 8, 4, d), DEV),
        ("fh_solve_batch_speculative", (d, d, 8, 4, 4, d), DEV),
        ("fh_solve_batch_speculative", (d, d, 8, 4, 1, d), DEV),
        ("fh_solve_batch_speculative", (d, d, 8, -1, 4, d), ARG),
        ("fh_solve_batch_speculative", (d, d, -1, 4, 4, d), ARG),
        ("fh_sample_batch_device", (d, d, 4, 8, d, d), DEV),
        ("fh_sample_batch_device", (d, d, -1, 8, d, d), ARG),
        ("fh_sample_batch_device", (d, d, 4, -1, d, d), ARG),
        ("fh_sample_batch", (d, d, 4, 8, d, d), DEV),
        ("fh_sample_batch", (d, d, -1, 8, d, d), ARG),
        ("fh_sample_batch", (d, d, 4, -1, d, d), ARG),
        ("fh_sample_batch", (None, d, 4, 8, d, d), DEV),
        ("fh_dt_initial_batch_device", (d, 4, d), DEV),
        ("fh_dt_initial_batch_device", (d, -1, d), ARG),
        ("fh_dt_initial_batch", (d, 4, d), DEV),
        ("fh_dt_initial_batch", (d, -1, d), ARG),
        ("fh_pair_glue_device", (d, d, d, 4, 0.5, 0.2, 3, d, d), DEV),
        ("fh_pair_glue_device", (d, d, d, -1, 0.5, 0.2, 3, d, d), ARG),
        ("fh_pair_glue_device", (d, d, d, 4, 2.0, 0.2, 9, d, d), DEV),     # (r_frac and the polytope cap: after the device)
        ("fh_append_plans_device", (d, d, d, d, 4, 0.5, 8, d, d, None), DEV),
        ("fh_append_plans_device", (d, d, d, d, -1, 0.5, 8, d, d, None), ARG),
        ("fh_append_plans_device", (d, d, d, d, 4, 0.5, -1, d, d, None), ARG),
        ("fh_append_plans_device", (d, d, d, d, 4, 2.0, 8, d, d, None), ARG),
        ("fh_append_plans_device", (d, d, d, d, 4, NAN, 8, d, d, None), ARG),
        ("fh_next_goals_device", (d, d, d, 4, 8, 1, d, None), DEV),
        ("fh_next_goals_device", (d, d, d, -1, 8, 1, d, None), ARG),
        ("fh_next_goals_device", (d, d, d, 4, 0, 1, d, None), ARG),
        ("fh_next_goals_device", (d, d, d, 4, 8, 0, d, None), ARG),
        ("fh_solve_pairs_device", (d, d, 4, 10, 64, 0.5, 0.2, 3, d, d, d, d), DEV),
        ("fh_solve_pairs_device", (d, d, -1, 10, 64, 0.5, 0.2, 3, d, d, d, d), ARG),
        ("fh_solve_pairs_device", (d, d, 4, 10, 64, 2.0, 0.2, 9, d, d, d, d), DEV),
        ("fh_decompose_batch_device", (d, 16, d, 4, bbox, 0.05, 0.0, 64, d, d), DEV),
        ("fh_decompose_batch_device", (d, -1, d, 4, bbox, 0.05, 0.0, 64, d, d), ARG),
        ("fh_decompose_batch_device", (d, 16, d, -1, bbox, 0.05, 0.0, 64, d, d), ARG),
        ("fh_decompose_batch_device", (d, 16, d, 4, bbox, 0.05, 0.0, 7, d, d), ARG),
        ("fh_decompose_batch_device", (d, 16, d, 4, None, 0.05, 0.0, 64, d, d), ARG),
        ("fh_decompose_batch", (d, 16, d, 4, bbox, 0.05, 0.0, 64, d, d), DEV),
        ("fh_decompose_batch", (d, -1, d, 4, bbox, 0.05, 0.0, 64, d, d), ARG),
        ("fh_decompose_batch", (d, 16, d, -1, bbox, 0.05, 0.0, 64, d, d), ARG),
        ("fh_decompose_batch", (d, 16, d, 4, bbox, 0.05, 0.0, 7, d, d), ARG),
        ("fh_decompose_batch", (d, 16, d, 4, None, 0.05, 0.0, 64, d, d), DEV),
        ("fh_corridor_batch_device", (d, 16, d, d, 4, 8, 4, bbox, 0.05, 0.0, 96, d, d, d, None), DEV),
        ("fh_corridor_batch_device", (d, 16, d, d, -1, 8, 4, bbox, 0.05, 0.0, 96, d, d, d, None), ARG),
        ("fh_corridor_batch_device", (d, -1, d, d, 4, 8, 4, bbox, 0.05, 0.0, 96, d, d, d, None), ARG),
        ("fh_corridor_batch_device", (d, 16, d, d, 4, 1, 4, bbox, 0.05, 0.0, 96, d, d, d, None), ARG),
        ("fh_corridor_batch_device", (d, 16, d, d, 4, 8, 0, bbox, 0.05, 0.0, 96, d, d, d, None), ARG),
        ("fh_corridor_batch_device", (d, 16, d, d, 4, 8, 9, bbox, 0.05, 0.0, 96, d, d, d, None), ARG),
        ("fh_corridor_batch_device", (d, 16, d, d, 4, 8, 4, bbox, 0.05, 0.0, 7, d, d, d, None), ARG),
        ("fh_corridor_batch_device", (d, 16, d, d, 4, 8, 4, None, 0.05, 0.0, 96, d, d, d, None), ARG),
        ("fh_corridor_problems_device", (d, d, d, d, d, d, 4, 96, 6, d), DEV),
        ("fh_corridor_problems_device", (d, d, d, d, d, d, -1, 96, 6, d), ARG),
        ("fh_corridor_problems_device", (d, d, d, d, d, d, 4, 7, 6, d), ARG),
        ("fh_corridor_problems_device", (d, d, d, d, d, d, 4, 96, 0, d), ARG),
        ("fh_corridor_problems_device", (d, d, d, d, d, d, 4, 96, 17, d), ARG),
    ]
    safe = lambda **kw: tuple({**dict(w=d, wr=d, paths=d, npts=d, max_points=4, goals=d, cloud=d, n_cloud=4, grid=g, n=4, r_frac=0.5, max_poly=3,  # noqa: E731
                                      bbox=bbox, radius=0.05, zg=0.0, fpp=96, n_seg=6, safe=d, sfaces=d, spaths=None, snp=None), **kw}.values())
    t += [("fh_safe_corridor_batch_device", safe(), DEV)]
    t += [("fh_safe_corridor_batch_device", safe(**kw), ARG) for kw in (
        dict(n=-1), dict(n_cloud=-1), dict(max_points=1), dict(max_points=100), dict(max_points=SAFE_PATH_CAP + 1), dict(max_poly=0), dict(max_poly=9),
        dict(fpp=7), dict(bbox=None),
        dict(grid=None), dict(grid=g_res), dict(grid=g_dims), dict(n_seg=0), dict(n_seg=17), dict(r_frac=2.0), dict(r_frac=NAN))]
    t += [("fh_safe_corridor_batch_device", safe(w=None), DEV), ("fh_safe_corridor_batch_device", safe(max_points=SAFE_PATH_CAP), DEV)]
    bad_fleet = [None, k(record(fp, delta_t=0)), k(record(fp, goal_radius=-1.0)), k(record(fp, wdy=0.0)), k(record(fp, ra=0.0)), k(record(fp, rule_mode=0))]
    for name, args in (("fh_fleet_init_device", lambda q, n, ms: (q, d, d, n, ms, d, d)),
                       ("fh_fleet_begin_device", lambda q, n, ms: (q, d, d, n, ms, d, d, d, d, d, d)),
                       ("fh_fleet_commit_device", lambda q, n, ms: (q, d, d, n, ms, d, d, d, d, d))):
        t += [(name, args(fpp, 4, 8), DEV), (name, args(fpp, -1, 8), ARG), (name, args(fpp, 4, 0), ARG)]
        t += [(name, args(q, 4, 8), ARG) for q in bad_fleet]
    t += [
        ("fh_fleet_next_goals_device", (d, d, 4, 8, 1, 1, d), DEV),
        ("fh_fleet_next_goals_device", (d, d, -1, 8, 1, 1, d), ARG),
        ("fh_fleet_next_goals_device", (d, d, 4, 0, 1, 1, d), ARG),
        ("fh_fleet_next_goals_device", (d, d, 4, 8, 0, 1, d), ARG),
        ("fh_fleet_heading_init_device", (None, 4, d), DEV),
        ("fh_fleet_heading_init_device", (None, -1, d), ARG),
        ("fh_fleet_set_goals_device", (fpp, d, d, None, 4), DEV),
        ("fh_fleet_set_goals_device", (fpp, d, d, None, -1), ARG),
        ("fh_fleet_set_goals_device", (None, d, d, None, 4), ARG),
        ("fh_fleet_set_goals_device", (bad_fleet[5], d, d, None, 4), ARG),
        ("fh_fleet_next_goals_yaw_device", (ypp, d, d, d, 4, 8, 1, 1, d, d), DEV),
        ("fh_fleet_next_goals_yaw_device", (ypp, d, d, d, 4, 8, 65536, 1, d, d), DEV),
        ("fh_fleet_next_goals_yaw_device", (ypp, d, d, d, -1, 8, 1, 1, d, d), ARG),
        ("fh_fleet_next_goals_yaw_device", (ypp, d, d, d, 4, 0, 1, 1, d, d), ARG),
        ("fh_fleet_next_goals_yaw_device", (ypp, d, d, d, 4, 8, 0, 1, d, d), ARG),
        ("fh_fleet_next_goals_yaw_device", (ypp, d, d, d, 4, 8, 65537, 1, d, d), ARG),
        ("fh_fleet_next_goals_yaw_device", (None, d, d, d, 4, 8, 1, 1, d, d), ARG),
        ("fh_fleet_next_goals_yaw_device", (k(record(yp, w_max=-1.0)), d, d, d, 4, 8, 1, 1, d, d), ARG),
        ("fh_fleet_next_goals_yaw_device", (k(record(yp, alpha_filter_dyaw=2.0)), d, d, d, 4, 8, 1, 1, d, d), ARG),
        ("fh_fleet_next_goals_yaw_device", (k(record(yp, dc=0.0)), d, d, d, 4, 8, 1, 1, d, d), ARG),
    ]
    sense = lambda **kw: tuple({**dict(map=fake_map, r=3.0, grid=g, flags=d, stride=256, view_of=None, n_views=4, veh=d, n=4), **kw}.values())  # noqa: E731
    bad_sense = (dict(map=None), dict(n=-1), dict(n_views=0), dict(grid=None), dict(r=0.0), dict(r=INF), dict(grid=g_res), dict(grid=g_dims),
                 dict(stride=255), dict(grid=g_huge, stride=1 << 31))
    t += [("fh_fleet_sense_device", sense(), DEV)] + [("fh_fleet_sense_device", sense(**kw), ARG) for kw in bad_sense]
    t += [("fh_fleet_sense_fov_device", sense() + (d, 1.0, 0.5), DEV), ("fh_fleet_sense_fov_device", sense() + (None, 1.0, 0.5), ARG)]
    t += [("fh_fleet_sense_fov_device", sense(**kw) + (d, 1.0, 0.5), ARG) for kw in bad_sense]
    t += [("fh_fleet_sense_fov_device", sense() + (d, th, tv), ARG) for th, tv in ((0.0, 0.5), (1.0, 0.0), (NAN, 0.5), (1.0, INF))]
    return t, keep


def test_context_entry_points(L):
    h = ctypes.c_void_p()
    assert L.fh_create(ctypes.byref(h), NO_SUCH_DEVICE) == DEV and h.value
    assert L.fh_create(None, 0) == ARG
    table, keep = context_table()
    assert {name for name, _, _ in table} == {s for s in __import__("faster_amd.capi", fromlist=["SYMBOLS"]).SYMBOLS if s not in NOT_IN_THE_CONTEXT_TABLE}
    wrong = []
    try:
        for row, (name, args, want) in enumerate(table):
            got = getattr(L, name)(h, *args)
            if got != want:
                wrong.append((row, name, got, want))
        assert L.fh_last_kernel_ms(h) == -1.0 and L.fh_last_kernel_ms(None) == -1.0
        assert L.fh_last_error(None) == b"null context"
    finally:
        L.fh_destroy(h)
    assert not wrong, wrong
    # a null context is an argument error everywhere, whatever else is passed
    seen = set()
    for name, args, _ in table:
        if name not in seen:
            seen.add(name)
            assert getattr(L, name)(None, *args) == ARG, name


# entry points that take no context (maps, pools, host-side helpers, create / destroy, texts and sizes): the tests below, or none to return
NOT_IN_THE_CONTEXT_TABLE = {
    "fh_create", "fh_destroy", "fh_last_error", "fh_last_kernel_ms", "fh_default_params", "fh_default_sched", "fh_version", "fh_abi_version",
    "fh_packed_result_size", "fh_pack_results", "fh_unpack_results", "fh_control_points",
    "fh_pool_create", "fh_pool_destroy", "fh_pool_size", "fh_pool_last_error", "fh_pool_set_params", "fh_pool_set_pair_margin",
    "fh_pool_set_pair_rule", "fh_pool_set_unknown_grid", "fh_pool_solve_batch", "fh_pool_solve_pairs",
    "fh_map_create", "fh_map_destroy", "fh_map_last_error", "fh_map_set_stream", "fh_map_set_sched", "fh_map_set_search", "fh_map_set_records",
    "fh_map_workspace_bytes", "fh_map_set_sphere", "fh_map_sync", "fh_map_read", "fh_map_read_device", "fh_map_dims", "fh_map_occupancy",
    "fh_map_plan_batch", "fh_map_plan_batch_device", "fh_map_plan_batch_radius_device", "fh_map_occupancy_bits_device"}


def test_map_entry_points_without_a_map(L):
    """fh_map_create makes no map without its device, so all that can be asked of the others here is what they say to no map."""
    buf = np.zeros(4096, dtype=np.uint8)
    d = abi.ptr(buf)
    cells, center = np.array([8, 8, 4], dtype=np.int32), np.zeros(3)
    m = ctypes.c_void_p()
    assert L.fh_map_create(ctypes.byref(m), NO_SUCH_DEVICE) == DEV and not m.value
    assert L.fh_map_create(ctypes.byref(m), -1) == DEV and not m.value
    assert L.fh_map_create(None, 0) == ARG
    for name, args in (("fh_map_set_stream", (None,)), ("fh_map_set_sched", (0, 1)), ("fh_map_set_search", (0,)), ("fh_map_set_records", (-1,)),
                       ("fh_map_set_sphere", (0.0,)), ("fh_map_sync", ()), ("fh_map_read", (d, 4, abi.ptr(cells), 0.2, abi.ptr(center), 0.0, 3.0, 0.3)),
                       ("fh_map_read_device", (d, 4, abi.ptr(cells), 0.2, abi.ptr(center), 0.0, 3.0, 0.3)), ("fh_map_dims", (d, d)),
                       ("fh_map_occupancy_bits_device", (d, d)), ("fh_map_occupancy", (d,)), ("fh_map_plan_batch", (d, d, 4, 16, 0.0, 0, d, d, d)),
                       ("fh_map_plan_batch_device", (d, d, 4, 16, 0.0, 0, d, d, d)),
                       ("fh_map_plan_batch_radius_device", (d, d, d, None, 4, 16, 0.0, 0, d, d, d))):
        assert getattr(L, name)(None, *args) == ARG, name
    assert L.fh_map_workspace_bytes(None) == -1
    assert L.fh_map_last_error(None) == b"null map"
    L.fh_map_destroy(None)


def test_pool_entry_points_without_devices(L):
    """A pool that could not be given its device keeps its handle and has no devices: settings have nothing to reach (FH_OK), a solve
    checks its arguments and then reports the missing devices."""
    buf = np.zeros(4096, dtype=np.uint8)
    d = abi.ptr(buf)
    dev = np.array([NO_SUCH_DEVICE], dtype=np.int32)
    pool = ctypes.c_void_p()
    # (a machine without any device says FH_ERR_DEVICE, one with devices that the index is out of range)
    assert L.fh_pool_create(ctypes.byref(pool), abi.ptr(dev), 1) in (ARG, DEV) and pool.value
    assert L.fh_pool_create(None, None, 0) == ARG
    par, rule, g, g_dims = abi.default_params().reshape(1), np.zeros(1, dtype=abi.pair_rule_dtype), grid(), grid(dims=(0, 8, 4))
    bad_par = record(abi.default_params(), max_nodes=0)
    batch = lambda **kw: tuple({**dict(pr=d, faces=d, n_faces=8, n=4, res=d, root=0, d_root=None), **kw}.values())  # noqa: E731
    pairs = lambda **kw: tuple({**dict(pr=d, faces=d, n_faces=8, n=4, safe=d, r_frac=0.5, shrink=0.2, max_poly=3, wres=d, sres=d, root=0, d_wroot=None,  # noqa: E731
                                       d_sroot=None), **kw}.values())
    table = [
        ("fh_pool_size", (), 0),
        ("fh_pool_set_params", (abi.ptr(par),), OK),
        ("fh_pool_set_params", (abi.ptr(bad_par),), OK),      # (no device to refuse it)
        ("fh_pool_set_params", (None,), ARG),
        ("fh_pool_set_pair_margin", (0.1,), OK),
        ("fh_pool_set_pair_rule", (abi.ptr(rule),), OK),
        ("fh_pool_set_pair_rule", (None,), ARG),
        ("fh_pool_set_unknown_grid", (None, None), OK),
        ("fh_pool_set_unknown_grid", (abi.ptr(g), d), OK),
        ("fh_pool_set_unknown_grid", (None, d), ARG),
        ("fh_pool_set_unknown_grid", (abi.ptr(g_dims), d), ARG),
        ("fh_pool_solve_batch", batch(), DEV),
        ("fh_pool_solve_batch", batch(n=-1), ARG),
        ("fh_pool_solve_batch", batch(n_faces=-1), ARG),
        ("fh_pool_solve_batch", batch(n=0), DEV),
        ("fh_pool_solve_batch", batch(pr=None), DEV),
        ("fh_pool_solve_pairs", pairs(), DEV),
        ("fh_pool_solve_pairs", pairs(n=-1), ARG),
        ("fh_pool_solve_pairs", pairs(n_faces=-1), ARG),
        ("fh_pool_solve_pairs", pairs(safe=None), DEV),
    ]
    wrong = []
    try:
        for row, (name, args, want) in enumerate(table):
            got = getattr(L, name)(pool, *args)
            if got != want:
                wrong.append((row, name, got, want))
    finally:
        L.fh_pool_destroy(pool)
    assert not wrong, wrong
    for name, args, _ in table:
        assert getattr(L, name)(None, *args) == (0 if name == "fh_pool_size" else ARG), name
    assert L.fh_pool_last_error(None) == b"null pool"
