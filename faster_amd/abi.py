"""numpy / ctypes mirror of the C ABI structs declared in include/fasterhip.h.

The layouts are checked against `sizeof` exported by the shared libraries in tests/test_abi.py.
Field meaning: see include/fasterhip.h (each field cites the SolverGurobi member it replaces).
"""
import ctypes

import numpy as np

FH_MAX_SEG = 16
FH_MAX_POLY = 8
FH_MAX_FACES = 256
FH_MAX_FACES_POLY = 64

FH_ST_OPTIMAL, FH_ST_INFEASIBLE, FH_ST_NODE_LIMIT, FH_ST_ITER_LIMIT, FH_ST_BAD_INPUT, FH_ST_INTERRUPTED = range(6)

problem_dtype = np.dtype(
    [
        ("n_seg", "<i4"),
        ("n_poly", "<i4"),
        ("force_final_pos", "<i4"),
        ("face_begin", "<i4"),
        ("face_off", "<i4", (FH_MAX_POLY + 1,)),
        ("pin", "<u4", (2,)),
        ("reserved", "<i4"),
        ("dc", "<f8"),
        ("v_max", "<f8"),
        ("a_max", "<f8"),
        ("j_max", "<f8"),
        ("f_init", "<f8"),
        ("f_final", "<f8"),
        ("f_inc", "<f8"),
        ("x0", "<f8", (9,)),
        ("xf", "<f8", (9,)),
    ],
    align=True,
)

face_dtype = np.dtype([("a", "<f8", (3,)), ("b", "<f8")], align=True)

result_dtype = np.dtype(
    [
        ("solved", "<i4"),
        ("trials", "<i4"),
        ("status", "<i4"),
        ("nodes", "<i4"),
        ("qp_iters", "<i4"),
        ("kflops", "<i4"),
        ("factor", "<f8"),
        ("dt", "<f8"),
        ("cost", "<f8"),
        ("coeff", "<f8", (FH_MAX_SEG, 12)),
        ("assign", "i1", (FH_MAX_SEG,)),
    ],
    align=True,
)

state_dtype = np.dtype([("pos", "<f8", (3,)), ("vel", "<f8", (3,)), ("accel", "<f8", (3,)), ("jerk", "<f8", (3,))], align=True)

params_dtype = np.dtype([("feas_tol", "<f8"), ("dep_tol", "<f8"), ("max_nodes", "<i4"), ("max_iters", "<i4"), ("max_work", "<i4"),
                         ("share", "<i4"), ("mip_gap", "<f8"), ("deadline_ms", "<f8")], align=True)
share_stats_dtype = np.dtype([(k, "<u4") for k in ("donated", "stolen", "queue_full", "records_full", "records_used", "error",
                                                   "interrupted", "workgroups")], align=True)

assert problem_dtype.itemsize == 264, problem_dtype.itemsize
assert face_dtype.itemsize == 32
assert result_dtype.itemsize == 1600, result_dtype.itemsize
assert state_dtype.itemsize == 96
assert params_dtype.itemsize == 48


sched_dtype = np.dtype([("launch_order", "<i4"), ("publish_factor", "<i4"), ("backlog", "<i4"), ("waiting_workgroups", "<i4"),
                        ("min_nodes", "<i4"), ("cloud_blocks", "<i4"), ("workgroups_per_cu", "<i4"), ("no_child_bound", "<i4"), ("compact_results", "<i4"), ("pair_outputs", "<i4"),
                        ("look_every", "<i4"), ("struct_size", "<i4")])
assert sched_dtype.itemsize == 48
FH_ABI_VERSION = 9   # include/fasterhip.h: the layout generation of its structs (checked against fh_abi_version() when the library is loaded)

launch_info_dtype = np.dtype([("n_seg", "<i4"), ("pairs", "<i4"), ("waves_per_simd", "<i4"), ("grid", "<i4"), ("workgroups_per_cu", "<i4"),
                              ("lds_bytes", "<i4"), ("unknown_space", "<i4"), ("look_every", "<i4")])


def point_mask_words(n_cloud):
    """Words of one row of the point masks (fh_set_point_views_device): one bit per cloud point, 32 to a uint32."""
    return (int(n_cloud) + 31) // 32


voxel_grid_dtype = np.dtype([("origin", "<f8", (3,)), ("res", "<f8"), ("dims", "<i4", (3,)), ("reserved", "<i4")])
assert voxel_grid_dtype.itemsize == 48


pair_rule_dtype = np.dtype([("mode", "<i4"), ("reserved", "<i4"), ("r_known", "<f8"), ("drone_radius", "<f8"), ("delta_h", "<f8"),
                            ("delta_a", "<f8")])
assert pair_rule_dtype.itemsize == 40

# fh_vehicle / fh_fleet_params: steady-state replanning of a fleet (fh_fleet_*)
FH_VEHICLE_TRAVELING, FH_VEHICLE_GOAL_SEEN, FH_VEHICLE_GOAL_REACHED = 0, 1, 2
FH_VEHICLE_YAWING = 3
FH_FLEET_STAGE_NONE, FH_FLEET_STAGE_NO_PATH, FH_FLEET_STAGE_NO_WHOLE, FH_FLEET_STAGE_NO_SAFE = 0, 1, 2, 3
FH_FLEET_STAGE_COMMITTED, FH_FLEET_STAGE_OVERFLOW = 5, 6
vehicle_dtype = np.dtype([("g_term", "<f8", (3,)), ("state", state_dtype), ("status", "<i4"), ("plan_head", "<i4"), ("plan_size", "<i4"),
                          ("active", "<i4"), ("whole_init", "<f8"), ("whole_final", "<f8"), ("whole_inc", "<f8"), ("safe_init", "<f8"),
                          ("safe_final", "<f8"), ("safe_inc", "<f8"), ("safe_factor_worked", "<f8"), ("goal", "<f8", (3,)), ("ra", "<f8"),
                          ("dist_to_goal", "<f8"), ("stage", "<i4"), ("needed_safe", "<i4"), ("k_end_whole", "<i4"), ("k_safe", "<i4"),
                          ("index_h", "<i4"), ("n_whole", "<i4"), ("n_safe", "<i4"), ("reserved", "<i4"), ("whole_factor", "<f8"),
                          ("safe_factor", "<f8")], align=True)
assert vehicle_dtype.itemsize == 280, vehicle_dtype.itemsize
fleet_params_dtype = np.dtype([("delta_t", "<i4"), ("reserved", "<i4"), ("goal_radius", "<f8"), ("wdx", "<f8"), ("wdy", "<f8"), ("wdz", "<f8"),
                               ("ra", "<f8"), ("gamma_whole", "<f8"), ("gammap_whole", "<f8"), ("increment_whole", "<f8"), ("gamma_safe", "<f8"),
                               ("gammap_safe", "<f8"), ("increment_safe", "<f8"), ("rule", pair_rule_dtype)], align=True)
assert fleet_params_dtype.itemsize == 136, fleet_params_dtype.itemsize
# fh_heading / fh_yaw_params: yaw, the YAWING status and the forward sensor (fh_fleet_*_yaw_*, fh_fleet_sense_fov_device)
heading_dtype = np.dtype([("yaw", "<f8"), ("previous_yaw", "<f8"), ("dyaw_filtered", "<f8"), ("goal_yaw", "<f8"), ("goal_dyaw", "<f8"),
                          ("look_at", "<f8", (3,)), ("dir", "<f8", (2,)), ("reserved", "<f8", (2,))], align=True)
assert heading_dtype.itemsize == 96, heading_dtype.itemsize
yaw_params_dtype = np.dtype([("w_max", "<f8"), ("alpha_filter_dyaw", "<f8"), ("dc", "<f8")], align=True)
assert yaw_params_dtype.itemsize == 24, yaw_params_dtype.itemsize

# fh_certificate / fh_certify_tol: certificates of solved trajectories (include/fasterhip_certify.h)
FH_CERT_UNSOLVED, FH_CERT_BAD_INPUT, FH_CERT_NOT_FINITE, FH_CERT_CORRIDOR, FH_CERT_ASSIGNMENT = 1, 2, 4, 8, 16
FH_CERT_X0, FH_CERT_XF, FH_CERT_CONTINUITY, FH_CERT_BOX, FH_CERT_COST = 32, 64, 128, 256, 512
FH_CERT_STRUCTURAL = FH_CERT_UNSOLVED | FH_CERT_BAD_INPUT | FH_CERT_NOT_FINITE
CERT_NUMBERS = ("corridor_assigned", "corridor_best", "x0_defect", "xf_defect", "continuity_defect", "v_excess", "a_excess", "j_excess", "v_peak",
                "a_peak", "cost", "cost_defect")
certificate_dtype = np.dtype([("flags", "<i4"), ("worst_seg", "<i4"), ("reserved_i", "<i4", (2,))] + [(k, "<f8") for k in CERT_NUMBERS]
                             + [("reserved_d", "<f8", (2,))], align=True)
assert certificate_dtype.itemsize == 128, certificate_dtype.itemsize
certify_tol_dtype = np.dtype([("corridor", "<f8"), ("state", "<f8"), ("box", "<f8"), ("cost_rel", "<f8")], align=True)
assert certify_tol_dtype.itemsize == 32


# fh_audit_params / fh_plan_audit: the audit of committed plans (include/fasterhip_audit.h)
FH_AUDIT_BAD_PLAN, FH_AUDIT_NO_VIEW, FH_AUDIT_NOT_FINITE, FH_AUDIT_UNKNOWN, FH_AUDIT_OCCUPIED = 1, 2, 4, 8, 16
FH_AUDIT_LIST_POINTS, FH_AUDIT_SLAB_CELLS = 256, 65536   # the kernel's LDS point list and the cells of one LDS slab
audit_params_dtype = np.dtype([("r_unknown", "<f8"), ("r_occupied", "<f8"), ("cap", "<f8"), ("stride", "<i4"), ("count", "<i4")], align=True)
assert audit_params_dtype.itemsize == 32
plan_audit_dtype = np.dtype([("flags", "<i4"), ("n_tested", "<i4"), ("first_unknown", "<i4"), ("worst_unknown", "<i4"), ("first_occupied", "<i4"),
                             ("worst_occupied", "<i4"), ("view", "<i4"), ("reserved", "<i4"), ("min_unknown_d2", "<f8"), ("min_occupied_d2", "<f8"),
                             ("reserved_d", "<f8", (2,))], align=True)
assert plan_audit_dtype.itemsize == 64, plan_audit_dtype.itemsize


def default_audit_params(drone_radius):
    """fh_audit_params: near is closer than drone_radius on both sides, nothing beyond two radii is looked at, every state is tested."""
    p = np.zeros((), dtype=audit_params_dtype)
    p["r_unknown"] = p["r_occupied"] = drone_radius
    p["cap"], p["stride"], p["count"] = 2.0 * drone_radius, 1, 0
    return p


def audit_distances(audit):
    """(unknown, occupied): the distances of [n] plan_audit_dtype records, the square roots of the squared distances the device reports
    (inf: nothing within cap)."""
    return np.sqrt(audit["min_unknown_d2"]), np.sqrt(audit["min_occupied_d2"])


# fh_separation_params / fh_plan_separation: the committed plans against each other (include/fasterhip_separation.h)
FH_SEP_BAD_PLAN, FH_SEP_NOT_FINITE, FH_SEP_NEAR = 1, 4, 8
FH_SEP_LIST_VEHICLES, FH_SEP_MAX_CELLS = 256, 1 << 20   # the narrow phase's LDS list of vehicles; the most cells of the broad phase's grid
separation_params_dtype = np.dtype([("r", "<f8"), ("cap", "<f8"), ("stride", "<i4"), ("count", "<i4"), ("reserved", "<i4", (2,))], align=True)
assert separation_params_dtype.itemsize == 32
plan_separation_dtype = np.dtype([("flags", "<i4"), ("n_tested", "<i4"), ("first", "<i4"), ("first_other", "<i4"), ("worst", "<i4"),
                                  ("worst_other", "<i4"), ("n_near", "<i4"), ("reserved", "<i4"), ("min_d2", "<f8"), ("reserved_d", "<f8", (3,))],
                                 align=True)
assert plan_separation_dtype.itemsize == 64, plan_separation_dtype.itemsize


def default_separation_params(radius):
    """fh_separation_params: two vehicles are near when their centres are closer than `radius` (two hulls of drone_radius touch at twice
    that), nothing beyond two radii is looked at, every state is tested."""
    p = np.zeros((), dtype=separation_params_dtype)
    p["r"], p["cap"], p["stride"], p["count"] = radius, 2.0 * radius, 1, 0
    return p


def separation_distances(separation):
    """The distances of [n] plan_separation_dtype records: the square roots of the squared distances the device reports (inf: no other
    vehicle within cap)."""
    return np.sqrt(separation["min_d2"])


# fh_check_params / fh_plan_check: every commit against the other plans, the conflicts withheld (include/fasterhip_check.h)
FH_FLEET_STAGE_CONFLICT = 7   # fh_vehicle.stage of a commit that fh_fleet_revert_device took back
FH_CHECK_BAD_PLAN, FH_CHECK_NOT_FINITE, FH_CHECK_CANDIDATE, FH_CHECK_CONFLICT = 1, 4, 16, 32
FH_CHECK_LIST_OTHERS, FH_CHECK_MAX_CELLS = 256, 1 << 20   # the narrow phase's LDS list of others; the most cells of the broad phase's grid
check_params_dtype = np.dtype([("r", "<f8"), ("stride", "<i4"), ("count", "<i4"), ("reserved", "<i4", (4,))], align=True)
assert check_params_dtype.itemsize == 32
plan_check_dtype = np.dtype([("flags", "<i4"), ("n_tested", "<i4"), ("first", "<i4"), ("first_other", "<i4"), ("first_kind", "<i4"),
                             ("reserved", "<i4"), ("d2", "<f8")], align=True)
assert plan_check_dtype.itemsize == 32, plan_check_dtype.itemsize


def default_check_params(radius):
    """fh_check_params: a commit conflicts when its centre comes closer than `radius` to another vehicle's at a tested instant (two hulls
    of drone_radius touch at twice that); every instant from the first new state on is tested, which is the check the header's promise
    holds for."""
    p = np.zeros((), dtype=check_params_dtype)
    p["r"], p["stride"], p["count"] = radius, 1, 0
    return p


# fh_round_params / fh_plan_round: the priority rounds of a cycle, a class per vehicle (include/fasterhip_rounds.h)
FH_ROUNDS_MAX, FH_ROUNDS_LIST, FH_ROUNDS_MAX_PASSES, FH_ROUNDS_MAX_CELLS = 64, 64, 1024, 1 << 20
FH_ROUND_RESTORE, FH_ROUND_RETRY = -1, -2   # the `round` of fh_fleet_round_gate_device below zero
FH_ROUND_OVERFLOW, FH_ROUND_UNSETTLED, FH_ROUND_NOT_FINITE, FH_ROUND_BAD_PLAN = 1, 2, 4, 8
round_params_dtype = np.dtype([("reach", "<f8"), ("rounds", "<i4"), ("passes", "<i4"), ("stride", "<i4"), ("count", "<i4"),
                               ("reserved", "<i4", (2,))], align=True)
assert round_params_dtype.itemsize == 32
plan_round_dtype = np.dtype([("round_class", "<i4"), ("decided_pass", "<i4"), ("n_lower", "<i4"), ("flags", "<i4")], align=True)
assert plan_round_dtype.itemsize == 16


def default_round_params(reach, rounds):
    """fh_round_params: two vehicles whose plans come nearer than `reach` at one instant go into different ones of `rounds` rounds;
    every instant is tested, 32 passes settle every chain of up to 33 vehicles."""
    p = np.zeros((), dtype=round_params_dtype)
    p["reach"], p["rounds"], p["passes"], p["stride"], p["count"] = reach, rounds, 32, 1, 0
    return p


# fh_link_params: vehicles in radio range pool what their views know (include/fasterhip_link.h)
FH_LINK_MAX_PASSES, FH_LINK_MAX_CELLS = 1024, 1 << 20
FH_LINK_DEFAULT_PASSES = 32
link_params_dtype = np.dtype([("range", "<f8"), ("passes", "<i4"), ("reserved", "<i4", (5,))], align=True)
assert link_params_dtype.itemsize == 32


def default_link_params(range):  # noqa: A002  (the header's word)
    """fh_link_params: two speaking vehicles nearer than `range` are linked; FH_LINK_DEFAULT_PASSES passes of hook and jump (the header
    states what the worst arrangements of 64 and 1024 views needed)."""
    p = np.zeros((), dtype=link_params_dtype)
    p["range"], p["passes"] = range, FH_LINK_DEFAULT_PASSES
    return p


# fh_frontier_params, fh_frontier_record, fh_view_coverage: arrived vehicles take the nearest frontier voxel of their view as goal
# (include/fasterhip_frontier.h)
FH_FRONTIER_WANT_REACHED, FH_FRONTIER_WANT_NO_PATH, FH_FRONTIER_WANT_ALL = 1, 2, 4
FH_FRONTIER_WANTED, FH_FRONTIER_FOUND, FH_FRONTIER_NO_VIEW, FH_FRONTIER_BAD_POS = 1, 2, 4, 8
frontier_params_dtype = np.dtype([("r_max", "<f8"), ("r_avoid", "<f8"), ("z_lo", "<f8"), ("z_hi", "<f8"), ("want", "<i4"),
                                  ("reserved", "<i4", (7,))], align=True)
frontier_record_dtype = np.dtype([("flags", "<i4"), ("view", "<i4"), ("cell", "<i4"), ("candidates", "<i4"), ("d2", "<f8"),
                                  ("reserved", "<f8")], align=True)
view_coverage_dtype = np.dtype([("known", "<i8"), ("frontier", "<i8")], align=True)
assert (frontier_params_dtype.itemsize, frontier_record_dtype.itemsize, view_coverage_dtype.itemsize) == (64, 32, 16)


def default_frontier_params(r_max):
    """fh_frontier_params: the vehicles that have reached their goal look for the nearest frontier voxel nearer than r_max, at any
    height, with no region around the old goal excluded."""
    p = np.zeros((), dtype=frontier_params_dtype)
    p["r_max"], p["r_avoid"], p["z_lo"], p["z_hi"], p["want"] = r_max, 0.0, -np.inf, np.inf, FH_FRONTIER_WANT_REACHED
    return p


# fh_reach_params, fh_reach_record: the frontier voxel that a flood of known free space reaches in the fewest steps
# (include/fasterhip_reach.h); the record's flags are FH_FRONTIER_WANTED .. BAD_POS and these
FH_REACH_START_OUTSIDE, FH_REACH_BOX_TOO_LARGE, FH_REACH_CUT = 16, 32, 64
FH_REACH_MAX_WORDS = 1024
reach_params_dtype = np.dtype([("r_max", "<f8"), ("r_avoid", "<f8"), ("z_lo", "<f8"), ("z_hi", "<f8"), ("want", "<i4"), ("max_hops", "<i4"),
                               ("reserved", "<i4", (6,))], align=True)
reach_record_dtype = np.dtype([("flags", "<i4"), ("view", "<i4"), ("cell", "<i4"), ("hops", "<i4"), ("candidates", "<i4"),
                               ("reachable", "<i4"), ("reached", "<i4"), ("levels", "<i4"), ("d2", "<f8"), ("reserved", "<f8")], align=True)
assert (reach_params_dtype.itemsize, reach_record_dtype.itemsize) == (64, 48)


def default_reach_params(r_max):
    """fh_reach_params: default_frontier_params with no limit on the levels of the flood."""
    p = np.zeros((), dtype=reach_params_dtype)
    p["r_max"], p["r_avoid"], p["z_lo"], p["z_hi"], p["want"], p["max_hops"] = r_max, 0.0, -np.inf, np.inf, FH_FRONTIER_WANT_REACHED, 0
    return p


# fh_spread_params, fh_spread_record: the chooser of fasterhip_reach.h for a team, goals claimed by peers avoided
# (include/fasterhip_spread.h); the record's flags are those of fh_reach_record and these
FH_SPREAD_OVERFLOW, FH_SPREAD_UNSETTLED, FH_SPREAD_CLAIMED = 128, 256, 512
FH_SPREAD_LIST, FH_SPREAD_MAX_PASSES, FH_SPREAD_DEFAULT_PASSES = 32, 64, 8
spread_params_dtype = np.dtype([("r_max", "<f8"), ("r_avoid", "<f8"), ("z_lo", "<f8"), ("z_hi", "<f8"), ("want", "<i4"), ("max_hops", "<i4"),
                                ("r_spread", "<f8"), ("passes", "<i4"), ("reserved", "<i4", (7,))], align=True)
spread_record_dtype = np.dtype([("flags", "<i4"), ("view", "<i4"), ("cell", "<i4"), ("hops", "<i4"), ("candidates", "<i4"),
                                ("reachable", "<i4"), ("reached", "<i4"), ("levels", "<i4"), ("d2", "<f8"), ("group", "<i4"),
                                ("decided_pass", "<i4"), ("lower", "<i4"), ("claims", "<i4"), ("claimed", "<i4"), ("reserved", "<i4")], align=True)
assert (spread_params_dtype.itemsize, spread_record_dtype.itemsize) == (80, 64)


def default_spread_params(r_max, r_spread):
    """fh_spread_params: default_reach_params, no candidate nearer than r_spread to a peer's goal, FH_SPREAD_DEFAULT_PASSES passes."""
    p = np.zeros((), dtype=spread_params_dtype)
    p["r_max"], p["r_avoid"], p["z_lo"], p["z_hi"], p["want"], p["max_hops"] = r_max, 0.0, -np.inf, np.inf, FH_FRONTIER_WANT_REACHED, 0
    p["r_spread"], p["passes"] = r_spread, FH_SPREAD_DEFAULT_PASSES
    return p


# fh_gain_params, fh_gain_record: the reachable frontier voxel with the most unknown space around it for its steps
# (include/fasterhip_gain.h); the record's flags are those of fh_reach_record and FH_GAIN_ALL_POOR
FH_GAIN_MAX_RADIUS, FH_GAIN_MAX_HOP_COST, FH_GAIN_ALL_POOR = 31, 16384, 128
gain_params_dtype = np.dtype([("r_max", "<f8"), ("r_avoid", "<f8"), ("z_lo", "<f8"), ("z_hi", "<f8"), ("want", "<i4"), ("max_hops", "<i4"),
                              ("gain_radius", "<i4"), ("hop_cost", "<i4"), ("min_gain", "<i4"), ("reserved", "<i4", (3,))], align=True)
gain_record_dtype = np.dtype([("flags", "<i4"), ("view", "<i4"), ("cell", "<i4"), ("hops", "<i4"), ("candidates", "<i4"),
                              ("reachable", "<i4"), ("reached", "<i4"), ("levels", "<i4"), ("d2", "<f8"), ("gain", "<i4"), ("utility", "<i4"),
                              ("poor", "<i4"), ("best_gain", "<i4"), ("reserved", "<f8")], align=True)
assert (gain_params_dtype.itemsize, gain_record_dtype.itemsize) == (64, 64)


def default_gain_params(r_max, gain_radius):
    """fh_gain_params: default_reach_params, the unknown voxels within gain_radius voxels of a candidate weighed against its steps one
    for one (hop_cost 1), no candidate poor (min_gain 0)."""
    p = np.zeros((), dtype=gain_params_dtype)
    p["r_max"], p["r_avoid"], p["z_lo"], p["z_hi"], p["want"], p["max_hops"] = r_max, 0.0, -np.inf, np.inf, FH_FRONTIER_WANT_REACHED, 0
    p["gain_radius"], p["hop_cost"], p["min_gain"] = gain_radius, 1, 0
    return p


# fh_team_params, fh_team_record: the gain-aware chooser for a team, the space a peer's claim covers not counted twice
# (include/fasterhip_team.h); the first 64 bytes of the record are fh_spread_record's, its flags those of that record and
# FH_TEAM_ALL_POOR (FH_GAIN_ALL_POOR is FH_SPREAD_OVERFLOW's bit); the other constants are those two headers' under the header's names
FH_TEAM_OVERFLOW, FH_TEAM_UNSETTLED, FH_TEAM_CLAIMED, FH_TEAM_ALL_POOR = 128, 256, 512, 1024
FH_TEAM_LIST, FH_TEAM_MAX_PASSES, FH_TEAM_DEFAULT_PASSES, FH_TEAM_MAX_RADIUS, FH_TEAM_MAX_HOP_COST = 32, 64, 8, 31, 16384
team_params_dtype = np.dtype([("r_max", "<f8"), ("r_avoid", "<f8"), ("z_lo", "<f8"), ("z_hi", "<f8"), ("want", "<i4"), ("max_hops", "<i4"),
                              ("r_spread", "<f8"), ("passes", "<i4"), ("gain_radius", "<i4"), ("hop_cost", "<i4"), ("min_gain", "<i4"),
                              ("claim_radius", "<i4"), ("reserved", "<i4", (3,))], align=True)
team_record_dtype = np.dtype([("flags", "<i4"), ("view", "<i4"), ("cell", "<i4"), ("hops", "<i4"), ("candidates", "<i4"),
                              ("reachable", "<i4"), ("reached", "<i4"), ("levels", "<i4"), ("d2", "<f8"), ("group", "<i4"),
                              ("decided_pass", "<i4"), ("lower", "<i4"), ("claims", "<i4"), ("claimed", "<i4"), ("reserved0", "<i4"),
                              ("gain", "<i4"), ("utility", "<i4"), ("poor", "<i4"), ("best_gain", "<i4"), ("covered", "<i4"),
                              ("reserved", "<i4", (3,))], align=True)
assert (team_params_dtype.itemsize, team_record_dtype.itemsize) == (80, 96)


def default_team_params(r_max, r_spread, gain_radius, claim_radius=None):
    """fh_team_params: default_spread_params and default_gain_params together, and a claim that covers the ball of claim_radius voxels
    around it (None: gain_radius, what the peer's own gain counted; -1: claims cover nothing)."""
    p = np.zeros((), dtype=team_params_dtype)
    p["r_max"], p["r_avoid"], p["z_lo"], p["z_hi"], p["want"], p["max_hops"] = r_max, 0.0, -np.inf, np.inf, FH_FRONTIER_WANT_REACHED, 0
    p["r_spread"], p["passes"] = r_spread, FH_TEAM_DEFAULT_PASSES
    p["gain_radius"], p["hop_cost"], p["min_gain"] = gain_radius, 1, 0
    p["claim_radius"] = gain_radius if claim_radius is None else claim_radius
    return p


# fh_bid_params, fh_bid_record: team goals by bids, the best offer wins a contested frontier (include/fasterhip_bid.h); the params are
# fh_team_params field by field, the record is fh_team_record with `lower` read as `rivals` and `reserved0` as `searches`; the constants
# are that header's under this header's names, but for the list of 64
FH_BID_OVERFLOW, FH_BID_UNSETTLED, FH_BID_CLAIMED, FH_BID_ALL_POOR = 128, 256, 512, 1024
FH_BID_LIST, FH_BID_MAX_PASSES, FH_BID_DEFAULT_PASSES, FH_BID_MAX_RADIUS, FH_BID_MAX_HOP_COST = 64, 64, 8, 31, 16384
bid_params_dtype = np.dtype([("r_max", "<f8"), ("r_avoid", "<f8"), ("z_lo", "<f8"), ("z_hi", "<f8"), ("want", "<i4"), ("max_hops", "<i4"),
                             ("r_spread", "<f8"), ("passes", "<i4"), ("gain_radius", "<i4"), ("hop_cost", "<i4"), ("min_gain", "<i4"),
                             ("claim_radius", "<i4"), ("reserved", "<i4", (3,))], align=True)
bid_record_dtype = np.dtype([("flags", "<i4"), ("view", "<i4"), ("cell", "<i4"), ("hops", "<i4"), ("candidates", "<i4"),
                             ("reachable", "<i4"), ("reached", "<i4"), ("levels", "<i4"), ("d2", "<f8"), ("group", "<i4"),
                             ("decided_pass", "<i4"), ("rivals", "<i4"), ("claims", "<i4"), ("claimed", "<i4"), ("searches", "<i4"),
                             ("gain", "<i4"), ("utility", "<i4"), ("poor", "<i4"), ("best_gain", "<i4"), ("covered", "<i4"),
                             ("reserved", "<i4", (3,))], align=True)
assert (bid_params_dtype.itemsize, bid_record_dtype.itemsize) == (80, 96)


def default_bid_params(r_max, r_spread, gain_radius, claim_radius=None):
    """fh_bid_params: default_team_params under this header's name (claim_radius None: gain_radius; -1: claims cover nothing)."""
    p = np.zeros((), dtype=bid_params_dtype)
    p["r_max"], p["r_avoid"], p["z_lo"], p["z_hi"], p["want"], p["max_hops"] = r_max, 0.0, -np.inf, np.inf, FH_FRONTIER_WANT_REACHED, 0
    p["r_spread"], p["passes"] = r_spread, FH_BID_DEFAULT_PASSES
    p["gain_radius"], p["hop_cost"], p["min_gain"] = gain_radius, 1, 0
    p["claim_radius"] = gain_radius if claim_radius is None else claim_radius
    return p


# fh_sight_params, fh_sight_record: the gain chooser with a gain that counts only the unknown voxels a candidate has a line of sight to
# (include/fasterhip_sight.h); the params are fh_gain_params field by field, the record is fh_gain_record through best_gain, then
# ball_gain (the count without the test of sight) and walls; the constants are that header's under this header's names
FH_SIGHT_MAX_RADIUS, FH_SIGHT_MAX_HOP_COST, FH_SIGHT_ALL_POOR = 31, 16384, 128
sight_params_dtype = np.dtype([("r_max", "<f8"), ("r_avoid", "<f8"), ("z_lo", "<f8"), ("z_hi", "<f8"), ("want", "<i4"), ("max_hops", "<i4"),
                               ("gain_radius", "<i4"), ("hop_cost", "<i4"), ("min_gain", "<i4"), ("reserved", "<i4", (3,))], align=True)
sight_record_dtype = np.dtype([("flags", "<i4"), ("view", "<i4"), ("cell", "<i4"), ("hops", "<i4"), ("candidates", "<i4"),
                               ("reachable", "<i4"), ("reached", "<i4"), ("levels", "<i4"), ("d2", "<f8"), ("gain", "<i4"), ("utility", "<i4"),
                               ("poor", "<i4"), ("best_gain", "<i4"), ("ball_gain", "<i4"), ("walls", "<i4")], align=True)
assert (sight_params_dtype.itemsize, sight_record_dtype.itemsize) == (64, 64)


def default_sight_params(r_max, gain_radius):
    """fh_sight_params: default_gain_params under this header's name (hop_cost 1, min_gain 0)."""
    p = np.zeros((), dtype=sight_params_dtype)
    p["r_max"], p["r_avoid"], p["z_lo"], p["z_hi"], p["want"], p["max_hops"] = r_max, 0.0, -np.inf, np.inf, FH_FRONTIER_WANT_REACHED, 0
    p["gain_radius"], p["hop_cost"], p["min_gain"] = gain_radius, 1, 0
    return p


# fh_far_params, fh_far_record: the fallback for the vehicles another chooser left without a goal, a flood of the whole view over blocks
# of voxels (include/fasterhip_far.h); the record's flags are FH_FRONTIER_WANTED .. BAD_POS, FH_REACH_START_OUTSIDE, FH_REACH_CUT and this
FH_FAR_SKIPPED = 128
FH_FAR_MAX_WORDS = 512
far_params_dtype = np.dtype([("r_avoid", "<f8"), ("z_lo", "<f8"), ("z_hi", "<f8"), ("reserved_d", "<f8"), ("want", "<i4"), ("max_hops", "<i4"),
                             ("block", "<i4"), ("reserved", "<i4", (5,))], align=True)
far_record_dtype = np.dtype([("flags", "<i4"), ("view", "<i4"), ("cell", "<i4"), ("block_cell", "<i4"), ("hops", "<i4"), ("targets", "<i4"),
                             ("reachable", "<i4"), ("reached", "<i4"), ("levels", "<i4"), ("members", "<i4"), ("reserved", "<i4", (2,)),
                             ("d2", "<f8"), ("block_d2", "<f8")], align=True)
assert (far_params_dtype.itemsize, far_record_dtype.itemsize) == (64, 64)


def default_far_params(block):
    """fh_far_params: blocks of `block` voxels an edge, the vehicles that have reached their goal, at any height, no limit on the levels."""
    p = np.zeros((), dtype=far_params_dtype)
    p["r_avoid"], p["z_lo"], p["z_hi"], p["want"], p["max_hops"], p["block"] = 0.0, -np.inf, np.inf, FH_FRONTIER_WANT_REACHED, 0, block
    return p


# fh_apart_params, fh_apart_record: that fallback for a team, the target blocks a peer's claim covers are no targets
# (include/fasterhip_apart.h); the first 64 bytes of both are fh_far_params' and fh_far_record's, the record's flags that record's
# and these; the pass limits are those of fh_spread_params under the header's names
FH_APART_UNSETTLED, FH_APART_CLAIMED = 256, 512
FH_APART_MAX_PASSES, FH_APART_DEFAULT_PASSES = 64, 8
FH_APART_SKIPPED, FH_APART_MAX_WORDS = FH_FAR_SKIPPED, FH_FAR_MAX_WORDS   # (that header's own names for K21's two)
far_spread_params_dtype = np.dtype([("r_avoid", "<f8"), ("z_lo", "<f8"), ("z_hi", "<f8"), ("reserved_d", "<f8"), ("want", "<i4"), ("max_hops", "<i4"),
                                    ("block", "<i4"), ("reserved", "<i4", (5,)), ("r_spread", "<f8"), ("passes", "<i4"),
                                    ("reserved_tail", "<i4", (5,))], align=True)
far_spread_record_dtype = np.dtype([("flags", "<i4"), ("view", "<i4"), ("cell", "<i4"), ("block_cell", "<i4"), ("hops", "<i4"), ("targets", "<i4"),
                                    ("reachable", "<i4"), ("reached", "<i4"), ("levels", "<i4"), ("members", "<i4"), ("reserved", "<i4", (2,)),
                                    ("d2", "<f8"), ("block_d2", "<f8"), ("group", "<i4"), ("decided_pass", "<i4"), ("lower", "<i4"),
                                    ("standing", "<i4"), ("claims", "<i4"), ("claimed", "<i4"), ("reserved_tail", "<i4", (2,))], align=True)
assert (far_spread_params_dtype.itemsize, far_spread_record_dtype.itemsize) == (96, 96)


def default_far_spread_params(block, r_spread):
    """fh_apart_params: default_far_params, no target block nearer than r_spread to a peer's goal, FH_APART_DEFAULT_PASSES passes."""
    p = np.zeros((), dtype=far_spread_params_dtype)
    p["r_avoid"], p["z_lo"], p["z_hi"], p["want"], p["max_hops"], p["block"] = 0.0, -np.inf, np.inf, FH_FRONTIER_WANT_REACHED, 0, block
    p["r_spread"], p["passes"] = r_spread, FH_APART_DEFAULT_PASSES
    return p


# fh_prospect_params, fh_prospect_record: that fallback with a gain, the unknown voxels of a cube of blocks around a target block, chosen
# by utility = gain - hop_cost * hops over all levels (include/fasterhip_prospect.h); the params are fh_far_params with three of its
# reserved words in use, the first 64 bytes of the record are fh_far_record's
FH_PROSPECT_SKIPPED, FH_PROSPECT_MAX_WORDS = FH_FAR_SKIPPED, FH_FAR_MAX_WORDS   # (that header's own names for K21's two)
FH_PROSPECT_ALL_POOR = 1024
FH_PROSPECT_MAX_BLOCKS, FH_PROSPECT_MAX_HOP_COST = 5, 16384
far_gain_params_dtype = np.dtype([("r_avoid", "<f8"), ("z_lo", "<f8"), ("z_hi", "<f8"), ("reserved_d", "<f8"), ("want", "<i4"), ("max_hops", "<i4"),
                                  ("block", "<i4"), ("gain_blocks", "<i4"), ("hop_cost", "<i4"), ("min_gain", "<i4"), ("reserved", "<i4", (2,))],
                                 align=True)
far_gain_record_dtype = np.dtype([("flags", "<i4"), ("view", "<i4"), ("cell", "<i4"), ("block_cell", "<i4"), ("hops", "<i4"), ("targets", "<i4"),
                                  ("reachable", "<i4"), ("reached", "<i4"), ("levels", "<i4"), ("members", "<i4"), ("reserved", "<i4", (2,)),
                                  ("d2", "<f8"), ("block_d2", "<f8"), ("gain", "<i4"), ("utility", "<i4"), ("poor", "<i4"), ("best_gain", "<i4")],
                                 align=True)
assert (far_gain_params_dtype.itemsize, far_gain_record_dtype.itemsize) == (64, 80)


def default_far_gain_params(block, gain_blocks):
    """fh_prospect_params: default_far_params, the gain of a block over a cube of 2 gain_blocks - 1 blocks an edge, a block step worth
    the voxels of one face of a block (block * block; a judgement, not a measurement), no block is poor."""
    p = np.zeros((), dtype=far_gain_params_dtype)
    p["r_avoid"], p["z_lo"], p["z_hi"], p["want"], p["max_hops"], p["block"] = 0.0, -np.inf, np.inf, FH_FRONTIER_WANT_REACHED, 0, block
    p["gain_blocks"], p["hop_cost"], p["min_gain"] = gain_blocks, int(block) * int(block), 0
    return p


# fh_stake_params, fh_stake_record: the gain of fh_prospect_params inside the passes of fh_apart_params, a peer's claim covering a cube
# of blocks whose unknown voxels no gain of the vehicle counts (include/fasterhip_stake.h); the params are fh_apart_params with three
# reserved words of its first 64 bytes (fh_prospect_params' three) and the first of its tail in use, the first 96 bytes of the record
# are fh_apart_record's, then fh_prospect_record's four, then covered and removed
FH_STAKE_SKIPPED, FH_STAKE_MAX_WORDS = FH_FAR_SKIPPED, FH_FAR_MAX_WORDS   # (that header's own names for K21's two)
FH_STAKE_UNSETTLED, FH_STAKE_CLAIMED, FH_STAKE_ALL_POOR = FH_APART_UNSETTLED, FH_APART_CLAIMED, FH_PROSPECT_ALL_POOR
FH_STAKE_MAX_PASSES, FH_STAKE_DEFAULT_PASSES = FH_APART_MAX_PASSES, FH_APART_DEFAULT_PASSES
FH_STAKE_MAX_BLOCKS, FH_STAKE_MAX_HOP_COST = FH_PROSPECT_MAX_BLOCKS, FH_PROSPECT_MAX_HOP_COST
FH_STAKE_MAX_CLAIM_BLOCKS = 5
far_team_params_dtype = np.dtype([("r_avoid", "<f8"), ("z_lo", "<f8"), ("z_hi", "<f8"), ("reserved_d", "<f8"), ("want", "<i4"), ("max_hops", "<i4"),
                                  ("block", "<i4"), ("gain_blocks", "<i4"), ("hop_cost", "<i4"), ("min_gain", "<i4"), ("reserved", "<i4", (2,)),
                                  ("r_spread", "<f8"), ("passes", "<i4"), ("claim_blocks", "<i4"), ("reserved_tail", "<i4", (4,))], align=True)
far_team_record_dtype = np.dtype([("flags", "<i4"), ("view", "<i4"), ("cell", "<i4"), ("block_cell", "<i4"), ("hops", "<i4"), ("targets", "<i4"),
                                  ("reachable", "<i4"), ("reached", "<i4"), ("levels", "<i4"), ("members", "<i4"), ("reserved", "<i4", (2,)),
                                  ("d2", "<f8"), ("block_d2", "<f8"), ("group", "<i4"), ("decided_pass", "<i4"), ("lower", "<i4"),
                                  ("standing", "<i4"), ("claims", "<i4"), ("claimed", "<i4"), ("reserved_tail", "<i4", (2,)), ("gain", "<i4"),
                                  ("utility", "<i4"), ("poor", "<i4"), ("best_gain", "<i4"), ("covered", "<i4"), ("removed", "<i4"),
                                  ("reserved_end", "<i4", (2,))], align=True)
assert (far_team_params_dtype.itemsize, far_team_record_dtype.itemsize) == (96, 128)


def default_far_team_params(block, r_spread, gain_blocks):
    """fh_stake_params: default_far_spread_params and default_far_gain_params together; a claim covers the cube of a gain
    (claim_blocks = gain_blocks: what a peer's goal is weighed by is what it is taken to uncover)."""
    p = np.zeros((), dtype=far_team_params_dtype)
    p["r_avoid"], p["z_lo"], p["z_hi"], p["want"], p["max_hops"], p["block"] = 0.0, -np.inf, np.inf, FH_FRONTIER_WANT_REACHED, 0, block
    p["gain_blocks"], p["hop_cost"], p["min_gain"] = gain_blocks, int(block) * int(block), 0
    p["r_spread"], p["passes"], p["claim_blocks"] = r_spread, FH_STAKE_DEFAULT_PASSES, gain_blocks
    return p


# fh_traffic_params: the other vehicles' committed plans as occupied points of a vehicle's view (include/fasterhip_traffic.h)
FH_TRAFFIC_ALL, FH_TRAFFIC_YIELD_TO_LOWER = 0, 1
traffic_params_dtype = np.dtype([("range", "<f8"), ("hull", "<f8"), ("samples", "<i4"), ("stride", "<i4"), ("rule", "<i4"), ("first_point", "<i4"),
                                 ("reserved", "<i4", (4,))], align=True)
assert traffic_params_dtype.itemsize == 48


def _traffic_common(dtype, samples, stride, range, hull, rule, first_point):  # noqa: A002
    """A zeroed record of `dtype` with the six fields both traffic records begin with."""
    p = np.zeros((), dtype=dtype)
    p["range"], p["hull"], p["samples"], p["stride"], p["rule"], p["first_point"] = range, hull, samples, stride, rule, first_point
    return p


def default_traffic_params(samples, stride, range, hull=0.0, rule=FH_TRAFFIC_ALL, first_point=0):  # noqa: A002  (the header's word)
    """fh_traffic_params: `samples` instants of every plan, `stride` states apart, shown to the vehicles nearer than `range`; hull > 0
    inflates every sample to seven points.  first_point: the cloud index of the first traffic point, a multiple of 32."""
    return _traffic_common(traffic_params_dtype, samples, stride, range, hull, rule, first_point)


# fh_traffic_timed_params: the same points, the bits matched instant by instant (include/fasterhip_traffic_timed.h)
FH_TRAFFIC_TIMED_MAX_SAMPLES = 512
traffic_timed_params_dtype = np.dtype([("range", "<f8"), ("hull", "<f8"), ("samples", "<i4"), ("stride", "<i4"), ("rule", "<i4"), ("first_point", "<i4"),
                                       ("first_instant", "<i4"), ("window", "<i4"), ("reserved", "<i4", (2,))], align=True)
assert traffic_timed_params_dtype.itemsize == 48


def default_traffic_timed_params(samples, stride, range, hull=0.0, rule=FH_TRAFFIC_ALL, first_point=0, first_instant=0, window=0):  # noqa: A002
    """fh_traffic_timed_params: default_traffic_params' fields, and sample s is the instant first_instant + s stride; sample (k, s) is
    shown to vehicle i when a shown sample s' of i's own plan with |s - s'| <= window lies nearer than `range`."""
    p = _traffic_common(traffic_timed_params_dtype, samples, stride, range, hull, rule, first_point)
    p["first_instant"], p["window"] = first_instant, window
    return p


def traffic_points_per_sample(hull):
    """pps of include/fasterhip_traffic.h: seven points per sample with a hull, else one."""
    return 7 if float(hull) > 0 else 1


# fh_obstacle, fh_obstacle_params, fh_obstacle_audit_params, fh_plan_obstacle_audit: things that move and are no fleet member, as points
# and bits, and the audit against them (include/fasterhip_obstacles.h)
FH_OBSTACLE_ON = 1
FH_OBSTACLE_MAX_SAMPLES, FH_OBSTACLE_MAX_TICK, FH_OBSTACLE_AUDIT_CHUNK = 512, 1 << 62, 64
FH_OBSTACLE_BAD_PLAN, FH_OBSTACLE_NOT_FINITE, FH_OBSTACLE_HIT = 1, 4, 8
obstacle_dtype = np.dtype([("p0", "<f8", (3,)), ("v", "<f8", (3,)), ("radius", "<f8"), ("flags", "<i4"), ("reserved", "<i4")], align=True)
obstacle_params_dtype = np.dtype([("range", "<f8"), ("r_detect", "<f8"), ("dc", "<f8"), ("samples", "<i4"), ("stride", "<i4"), ("points", "<i4"),
                                  ("first_point", "<i4"), ("first_instant", "<i4"), ("window", "<i4"), ("reserved", "<i4", (4,))], align=True)
obstacle_audit_params_dtype = np.dtype([("r", "<f8"), ("dc", "<f8"), ("stride", "<i4"), ("count", "<i4"), ("reserved", "<i4", (2,))], align=True)
plan_obstacle_audit_dtype = np.dtype([("flags", "<i4"), ("n_tested", "<i4"), ("first", "<i4"), ("first_obstacle", "<i4"), ("worst", "<i4"),
                                      ("worst_obstacle", "<i4"), ("n_hit", "<i4"), ("reserved", "<i4"), ("min_d2", "<f8"),
                                      ("reserved_d", "<f8", (3,))], align=True)
assert (obstacle_dtype.itemsize, obstacle_params_dtype.itemsize, obstacle_audit_params_dtype.itemsize, plan_obstacle_audit_dtype.itemsize) == (64, 64, 32, 64)


def make_obstacles(p0, v=None, radius=0.0, on=True):
    """[m] fh_obstacle from [m][3] positions at clock 0, [m][3] velocities (None: at rest) and radii (a number or [m])."""
    p0 = np.asarray(p0, dtype=np.float64).reshape(-1, 3)
    o = np.zeros(len(p0), dtype=obstacle_dtype)
    o["p0"], o["radius"], o["flags"] = p0, radius, FH_OBSTACLE_ON if on else 0
    if v is not None:
        o["v"] = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    return o


def default_obstacle_params(samples, stride, range, dc, r_detect=0.0, points=7, first_point=0, first_instant=0, window=0):  # noqa: A002
    """fh_obstacle_params: `samples` instants of every obstacle's straight flight, `stride` states of `dc` apart from first_instant on,
    shown to vehicle i when a shown sample of i's own plan within `window` samples of the same instant lies nearer than range + the
    obstacle's radius, once i stands nearer than r_detect to where the obstacle is now (0: no detection, everything is known)."""
    p = np.zeros((), dtype=obstacle_params_dtype)
    p["range"], p["r_detect"], p["dc"], p["samples"], p["stride"], p["points"] = range, r_detect, dc, samples, stride, points
    p["first_point"], p["first_instant"], p["window"] = first_point, first_instant, window
    return p


def default_obstacle_audit_params(r, dc, stride=1, count=0):
    """fh_obstacle_audit_params: an obstacle hits a vehicle of radius r at a tested instant when their centres are nearer than
    r + the obstacle's radius; every state of the plan is tested (stride 1, count 0: all)."""
    p = np.zeros((), dtype=obstacle_audit_params_dtype)
    p["r"], p["dc"], p["stride"], p["count"] = r, dc, stride, count
    return p


# fh_track_params, fh_obstacle_track: the obstacles some vehicle sees, a ring of sightings each, a constant velocity fitted to it
# (include/fasterhip_track.h)
FH_TRACK_HISTORY = 8
FH_TRACK_SEEN, FH_TRACK_LOST, FH_TRACK_RESET, FH_TRACK_STALE, FH_TRACK_BAD_FIT = 1, 2, 4, 8, 16
track_params_dtype = np.dtype([("r_detect", "<f8"), ("dc", "<f8"), ("gate", "<f8"), ("grow", "<f8"), ("max_age", "<i8"), ("fit", "<i4"),
                               ("min_obs", "<i4"), ("reserved", "<i4", (4,))], align=True)
obstacle_track_dtype = np.dtype([("tick", "<i8", (FH_TRACK_HISTORY,)), ("pos", "<f8", (FH_TRACK_HISTORY, 3)), ("radius", "<f8"), ("count", "<i4"),
                                 ("head", "<i4"), ("flags", "<i4"), ("reserved", "<i4", (11,))], align=True)
assert (track_params_dtype.itemsize, obstacle_track_dtype.itemsize) == (64, 320)


def default_track_params(r_detect, dc, fit=4, min_obs=2, max_age=0, gate=0.0, grow=0.0):
    """fh_track_params: a vehicle sees an obstacle nearer than r_detect; the newest `fit` sightings are fitted, a record is on from
    min_obs sightings; a track not seen for more than max_age ticks of dc is forgotten (0: never), a sighting farther than `gate` from
    the prediction starts it anew (0: no gate), and the radius grows by `grow` per unit of time unseen."""
    p = np.zeros((), dtype=track_params_dtype)
    p["r_detect"], p["dc"], p["gate"], p["grow"], p["max_age"], p["fit"], p["min_obs"] = r_detect, dc, gate, grow, max_age, fit, min_obs
    return p


def certify_tol(corridor, state=None, box=None, cost_rel=None):
    """fh_certify_tol; one number stands for all four (the project's own number for "violated" is fh_params.feas_tol)."""
    t = np.zeros((), dtype=certify_tol_dtype)
    t["corridor"] = corridor
    t["state"], t["box"], t["cost_rel"] = (corridor if v is None else v for v in (state, box, cost_rel))
    return t


def default_yaw_params(dc=0.01):
    """fh_yaw_params with the values of faster/param/faster.yaml: w_max 4.0, alpha_filter_dyaw 0."""
    p = np.zeros((), dtype=yaw_params_dtype)
    p["w_max"], p["alpha_filter_dyaw"], p["dc"] = 4.0, 0.0, dc
    return p


def default_fleet_params():
    """fh_fleet_params with the values of faster/param/faster.yaml (deltaT of faster.hpp:131), unknown space as an input (rule mode 2)."""
    p = np.zeros((), dtype=fleet_params_dtype)
    p["delta_t"], p["goal_radius"], p["wdx"], p["wdy"], p["wdz"], p["ra"] = 10, 0.3, 20.0, 20.0, 4.0, 4.0
    for k in ("whole", "safe"):
        p["gamma_" + k], p["gammap_" + k], p["increment_" + k] = 20.0, 20.0, 1.0
    p["rule"]["mode"], p["rule"]["drone_radius"], p["rule"]["delta_h"], p["rule"]["delta_a"] = 2, 0.42, 1.0, 0.5
    return p


def default_sched():
    s = np.zeros((), dtype=sched_dtype)
    s["launch_order"], s["publish_factor"], s["backlog"], s["min_nodes"], s["cloud_blocks"], s["no_child_bound"] = 1, 4, 32, 2, 1, 0
    s["struct_size"] = sched_dtype.itemsize
    return s


def default_params():
    p = np.zeros((), dtype=params_dtype)
    p["feas_tol"] = 1e-9
    p["dep_tol"] = 1e-10
    p["max_nodes"] = 100000
    p["max_iters"] = 2000
    p["max_work"] = 0
    p["share"] = 1
    p["mip_gap"] = 0.0
    p["deadline_ms"] = 0.0
    return p


def ptr(a):
    """void* to the first byte of a C-contiguous numpy array."""
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(ctypes.c_void_p)


def make_problems(n):
    pr = np.zeros(n, dtype=problem_dtype)
    return pr


def pack_faces(polys):
    """polys: list of (A[F,3], b[F]) -> (faces array, face_off list)"""
    off = [0]
    rows = []
    for A, b in polys:
        A = np.asarray(A, dtype=np.float64).reshape(-1, 3)
        b = np.asarray(b, dtype=np.float64).reshape(-1)
        assert A.shape[0] == b.shape[0]
        for i in range(A.shape[0]):
            rows.append((A[i], b[i]))
        off.append(off[-1] + A.shape[0])
    faces = np.zeros(len(rows), dtype=face_dtype)
    for i, (a, bb) in enumerate(rows):
        faces[i]["a"] = a
        faces[i]["b"] = bb
    return faces, off


def set_pins(problem, assign):
    """Fix the binaries of one problem record: assign[t] = polytope index or -1 (free)."""
    w = 0
    for t, a in enumerate(assign):
        if a is not None and a >= 0:
            w |= (int(a) + 1) << (4 * t)
    problem["pin"][0] = w & 0xFFFFFFFF
    problem["pin"][1] = (w >> 32) & 0xFFFFFFFF
