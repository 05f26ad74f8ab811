"""One steady-state replan cycle of a fleet on the device (faster_amd/fleet.py), stage by stage: 65536 vehicles in the forest of
frontend.forest_queries, unknown space as an input (rule mode 2), the stages of bench.py's `replan_faithful` plus the three fleet kernels
(begin, commit, next goals).  Cycle 1 warms up; the vehicles then fly a few ticks, so that the timed cycles start from carried plans
(k_end_whole > 0).  Prints one JSON line: per-stage milliseconds (median of the timed cycles, each stage fenced by events on the fleet's
stream), the unfenced cycle time, the commit kernel's write rate and a device-to-device copy rate of the same device for scale.

--views adds, to the same JSON line, the cycle with one unknown-voxel view per vehicle (Fleet.set_unknown_views), twice:
  "views_same_flags": every view a copy of the shared grid and no sensing — the same work as the shared-grid cycle, so any difference is
      the price of the per-vehicle flags pointer;
  "views_sensing": every view starts all unknown, the vehicles sense (Fleet.sense, --r-sense metres, default 3) before every replan: the
      first sense, when every voxel in range still needs its ray ("sense_first_ms"), then the closed loop sense -> replan -> 5 ticks in
      steady state, sensing as a stage of its own.  --no-staging: sensing reads the occupancy in memory instead of staging it in LDS.
--fov TAN_H TAN_V (implies --views) adds "fov_sensing": the same closed loop with Fleet.enable_heading, the forward sensor
(Fleet.sense(r, fov=(TAN_H, TAN_V)): tangents of the half angles) in place of the omnidirectional one and the yaw variant of next goals;
its "sense_first_ms" and stage table stand beside the omnidirectional ones of the same run.
Memory of the views: vehicles x nx ny nz bytes (printed; 65536 vehicles in this forest: 12.6 GB).  A fleet that does not fit lets vehicles
share views (view_of).
--occupancy [TEAMS] adds "occupancy": occupied space per team (Fleet.set_point_views; TEAMS views, default 64, vehicle i in team i mod
TEAMS — the jump point search keeps 64 bytes per cell and view, so a view per vehicle is for small fleets), unknown views and point masks
all unknown at first, world inflation half a cell (with more than a cell the points inside a blob are never observed), the closed loop
sense -> observe -> replan -> 5 ticks with "observe" and "map_views" as stages of their own.
--audit adds "audit" beside every stage table: the plan audit (Fleet.audit_device: every committed state against the unknown space and the
points the fleet of that table has, radii = drone_radius, cap = twice that) after the last replan of that table, fenced by events like a
stage ("ms", the median of as many calls as there are timed cycles), with the states it tested and the vehicles it flags.
--separation adds "separation" beside the shared-grid stage table: the plans against each other (Fleet.separation_device: r = two
drone radii, cap = twice that, the default cell grid) after the last replan, fenced by events like a stage, twice: "head" with count =
delta_t, the states the next replan cannot change, and "all" with count = 0, every state; with the states tested, the vehicles flagged,
the largest half-extent H of a box and, from a sample of 1024 vehicles, how many candidates the narrow phase lists per vehicle.
--traffic [SAMPLES STRIDE RANGE] adds "traffic": a fleet with a view per vehicle that holds the shared unknown grid and knows every static
point (memory per view as for --occupancy, so a fleet of a few thousand at most), its stage table and --separation's report "before";
then Fleet.enable_traffic(SAMPLES, STRIDE, RANGE; default 8 samples 25 states apart, 6 m; hull = drone_radius, rule "all") and the loop
traffic -> replan -> 5 ticks with "traffic" as a stage of its own, and the same report "after".
--traffic-timed WINDOW adds "traffic_timed": the same scene and report with Fleet.enable_traffic(..., timed=True, window=WINDOW), the plans
matched instant by instant (SAMPLES, STRIDE and RANGE are --traffic's when that is given too, else its defaults), and the traffic bits
set per vehicle, which both reports carry.
--check adds "check" after the shared-grid stage table, on the same fleet: Fleet.enable_check (r = two drone radii, stride 1, count 0, the
default cell grid), one cycle to warm up, then the stage table again with "backup", "check" and "revert" as stages of their own; per
timed cycle how many vehicles were candidates and how many were withheld, and Fleet.separation_device with the same count, every state,
fenced like a stage on the plans as they stand at the end.
--rounds R [--round-reach M] [--retries T] adds "rounds": the fleet of --traffic-timed (or of --traffic, or without either the shared-grid
fleet), with Fleet.enable_check when --check is given (which --retries needs), timed first as it is ("without_rounds": traffic ->
replan -> 5 ticks) and then after Fleet.enable_rounds(R, reach = M, default Fleet's; retries = T): every stage of every round fenced
like the others ("stages_ms", names suffixed @r), the same summed over the rounds per stage ("by_stage_ms"), "round_classes" and the
mean of the gates on their own, and per timed cycle the vehicles per class, the flagged records and the commits withheld per round.
--listed-views (with --rounds, --traffic, --traffic-timed or --occupancy) calls Fleet.enable_listed_views on the fleets that have point
views: "view_list" becomes a stage of its own in front of every "map_views", which then rebuilds the listed views only; the rounds report
carries the views listed per round and timed cycle ("views_listed_per_round").
--link RANGE[,RANGE..] (with --views) adds "link": for every RANGE the closed loop of --views from views that are all unknown with
Fleet.link(RANGE) between sensing and the replan (sense -> link -> replan -> 5 ticks), "link_groups" and "link_merge" fenced as stages of
their own; the passes, the groups (roots), the linked pairs and whether the labels settled in the last timed cycle (--link-los: the link
stage of that loop is Fleet.link(RANGE, los=True), walls block a link, and "los" records side by side, on the fleet as the last timed cycle
left it, the groups stage of the plain link and of the link with a line of sight in ms with their spread, and the groups, linked pairs
and blocked pairs of both); and, fenced the same
way in the same run, a device-to-device copy of the views' bytes ("views_copy_ms": the yardstick of the merge) with the ratio of the two.
--explore R_MAX (with --views) adds "explore": the closed loop of --views from views that are all unknown, with headings, and
Fleet.explore(R_MAX) between sensing and the replan (sense -> explore -> replan -> 5 ticks): "frontier_goals" (want = reached: the steady
state, with the vehicles it wanted and found per timed cycle) and "set_goals" fenced as stages of their own; then, fenced the same way in
the same run and applied to nobody, frontier_goals with every vehicle wanted ("frontier_goals_all_ms", with the vehicles that found a
voxel and their candidates) and view_coverage ("view_coverage_ms"); and the known and the frontier voxels of the fleet after the first look
and at the end.
--reach (with --views --explore R_MAX) runs that loop with Fleet.explore_reachable in the place of Fleet.explore (include/fasterhip_reach.h):
the stage is reported under its name, "reach_goals", and with every vehicle wanted as "reach_goals_all_ms", beside frontier_goals with
every vehicle wanted in the same run; and, of that launch, the levels of the flood (mean, max), the voxels reached and the candidates
reachable per searched vehicle, and the vehicles whose box was too large.
--spread R_SPREAD (with --views --explore R_MAX --reach) runs that loop with Fleet.explore_spread in the place of Fleet.explore_reachable
(include/fasterhip_spread.h): the stage is reported as "spread_goals"; with every vehicle wanted as "spread_goals_all_ms", and with one and
two passes instead of the default eight (the difference is what the idle launches cost), beside reach_goals with every vehicle wanted
before and after it in the same run; the vehicles decided per pass, those left UNSETTLED or in OVERFLOW, and the longest list of lower
peers.  The peers are the vehicles of one view: with a view per vehicle nobody has one, unless --link RANGE is given too — then the
vehicles are linked once after the first look, with the first RANGE, and the groups of that link are the teams.
--gain G [--hop-cost K] [--min-gain M] (with --views --explore R_MAX --reach) runs that loop with Fleet.explore_gain in
the place of Fleet.explore_reachable (include/fasterhip_gain.h; G in voxels, K default 1, M default 0): the stage is reported as
"gain_goals"; with every vehicle wanted as "gain_goals_all_ms", beside reach_goals with every vehicle wanted before and after it in the same
run; and, of that launch, the candidates evaluated per searched vehicle (the reachable ones), the levels of the flood (every level with a
candidate costs a second barrier: at most min(levels + 1, reachable) of them), the gains, the poor candidates, and the vehicles whose
choice is not the one of reach_goals.
--spread R_SPREAD together with --gain G [--claim-radius R] runs that loop with Fleet.explore_team (include/fasterhip_team.h; R in voxels,
default G): the stage is reported as "team_goals"; with every vehicle wanted as "team_goals_all_ms", beside gain_goals and spread_goals
with every vehicle wanted in the same run, alternating; the vehicles decided per pass, those left UNSETTLED or in OVERFLOW, the mean of
`covered` over the searched vehicles, and the teammates that hold the same goal voxel.  --link RANGE makes the teams, as for --spread.
--bid beside --spread R_SPREAD --gain G runs that loop with Fleet.explore_bid (include/fasterhip_bid.h): the stage is reported as
"bid_goals"; with every vehicle wanted as "bid_goals_all_ms" beside "team_goals_all_ms" in the same run, alternating; the vehicles decided
per round, those left UNSETTLED or in OVERFLOW, the mean of `searches` over the searched vehicles, the sum of `hops` and the mean gain of the
goals given, each beside the figure of Fleet.explore_team on the same fleet.
--sight together with --gain G (and without --spread) runs that loop with Fleet.explore_sight (include/fasterhip_sight.h): the stage is
reported as "sight_goals"; with every vehicle wanted as "sight_goals_all_ms" beside "gain_goals_all_ms" in the same run, alternating;
and, of that launch, the vehicles with a wall in their box, the walls per box, the chosen voxels that see less than their ball holds,
and the vehicles whose choice is not the one of gain_goals.  --walls adds rooms to the world before anything reads it: planes of
points every 5 m in x and in y, floor to ceiling, with a door of 1.2 m in every stretch of 5 m.
--far BLOCK (with --views --explore R_MAX, beside any of the choosers above) runs Fleet.explore_far(BLOCK, after=<the chooser in use>)
after that chooser in every period (include/fasterhip_far.h): its stages are reported as "far_goals" and "far_set_goals"; under "far" the
launch with every vehicle wanted and nobody skipped as "far_goals_all_ms" beside "reach_goals_all_beside_ms" of the same call (medians of
five, fenced by events), and the levels, blocks reached, target blocks, hops and members of that launch.
--far BLOCK --far-spread R_SPREAD [--passes P] runs Fleet.explore_far_spread(BLOCK, R_SPREAD, passes=P, after=...) in its place
(include/fasterhip_apart.h; with --link the groups are those of one link() after the first look): the stages are
"far_spread_goals" and "far_spread_set_goals", and under "far_spread" the launch with every vehicle wanted and nobody skipped as
"far_spread_goals_all_ms" beside "far_goals_all_beside_ms" of the same call, the same launch with 1 and with 64 passes, the cost of a
pass from the two, the largest `lower`, and the vehicles left unsettled or with every target claimed.
--far BLOCK --far-gain G [--far-hop-cost H] [--far-min-gain M] runs Fleet.explore_far_gain(BLOCK, G, H, M, after=...) in place of
explore_far (include/fasterhip_prospect.h): its stages are reported as "far_gain_goals" and "far_gain_set_goals", and under "far_gain" the
launch with every vehicle wanted and nobody skipped as "far_gain_goals_all_ms" beside "far_goals_all_beside_ms" of the same call (medians
of five), and the same launch with gain_blocks 0, 1, 2 and 5.
--far BLOCK --far-spread R_SPREAD --far-gain G [--far-claim-blocks C] [--passes P] [--far-hop-cost H] [--far-min-gain M] runs
Fleet.explore_far_team(BLOCK, R_SPREAD, G, H, M, C, passes=P, after=...) in their place (include/fasterhip_stake.h): the stages are
"far_team_goals" and "far_team_set_goals", and under "far_team" the launch with every vehicle wanted and nobody skipped as
"far_team_goals_all_ms" beside "far_spread_goals_all_beside_ms" and "far_gain_goals_all_beside_ms" of the same call (medians of five), the
same launch with 1, 8 and 64 passes, the cost of an idle pass from the last two, and what the claims covered and removed.
--obstacles M [--obstacle-samples S] adds "obstacles" (include/fasterhip_obstacles.h): the fleet of --traffic-timed after two cycles
with time-aware traffic of S samples (default 64, stride 5, 6 m, window 2) and, behind it, Fleet.enable_obstacles with M obstacles
scattered over the map that fly up to 1 m/s; Fleet.traffic, Fleet.obstacles and Fleet.obstacle_audit_device fenced one by one in the same
run ("traffic_timed_ms", "obstacles_ms", "obstacle_audit_ms", medians with their spread), the bits set per vehicle and the vehicles hit.
--obstacles M --track R_DETECT [--track-los] adds Fleet.enable_tracking on those obstacles as the truth (include/fasterhip_track.h; fit 4,
min_obs 2; --track-los: the walls of the fleet's map hide an obstacle) and Fleet.track as "track_ms", fenced like the others between
traffic and obstacles, each timed call one tick later than the one before so that every sighting is appended and fitted; and what the last
call saw ("track_seen", "track_records_on").
    usage: python scripts/fleet_cycle.py [vehicles] [cycles] [--views [--link RANGE[,RANGE..] [--link-los]] [--explore R_MAX [--far BLOCK [--far-gain G [--far-hop-cost H] [--far-min-gain M]] [--far-spread R_SPREAD [--passes P]] [--far-claim-blocks C]] [--reach [--spread R_SPREAD] [--gain G [--hop-cost K] [--min-gain M] [--claim-radius R] [--bid] [--sight]]]]] [--walls] [--fov TAN_H TAN_V] [--occupancy [TEAMS]] [--r-sense R] [--no-staging]
                                         [--audit] [--separation] [--traffic [SAMPLES STRIDE RANGE]] [--traffic-timed WINDOW] [--check]
                                         [--rounds R [--round-reach M] [--retries T]] [--listed-views]
                                         [--obstacles M [--obstacle-samples S] [--track R_DETECT [--track-los]]]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from faster_amd import abi, capi, frontend  # noqa: E402
from faster_amd.fleet import Fleet  # noqa: E402


AUDIT = "--audit" in sys.argv
SEPARATION = "--separation" in sys.argv
LISTED_VIEWS = "--listed-views" in sys.argv
LINK = [float(r) for r in sys.argv[sys.argv.index("--link") + 1].split(",")] if "--link" in sys.argv else []
LINK_LOS = "--link-los" in sys.argv   # with --views --link: walls block a link (include/fasterhip_link_los.h)
EXPLORE = float(sys.argv[sys.argv.index("--explore") + 1]) if "--explore" in sys.argv else None
REACH = "--reach" in sys.argv
if REACH and not ("--views" in sys.argv and EXPLORE is not None):
    sys.exit("--reach needs --views --explore R_MAX")
SPREAD = float(sys.argv[sys.argv.index("--spread") + 1]) if "--spread" in sys.argv else None
if SPREAD is not None and not REACH:
    sys.exit("--spread needs --views --explore R_MAX --reach")
GAIN = int(sys.argv[sys.argv.index("--gain") + 1]) if "--gain" in sys.argv else None
HOP_COST = int(sys.argv[sys.argv.index("--hop-cost") + 1]) if "--hop-cost" in sys.argv else 1
MIN_GAIN = int(sys.argv[sys.argv.index("--min-gain") + 1]) if "--min-gain" in sys.argv else 0
if GAIN is not None and not REACH:
    sys.exit("--gain needs --views --explore R_MAX --reach")
TEAM = SPREAD is not None and GAIN is not None   # both: Fleet.explore_team
CLAIM_RADIUS = int(sys.argv[sys.argv.index("--claim-radius") + 1]) if "--claim-radius" in sys.argv else None
if CLAIM_RADIUS is not None and not TEAM:
    sys.exit("--claim-radius needs --spread R_SPREAD and --gain G")
BID = "--bid" in sys.argv
if BID and not TEAM:
    sys.exit("--bid needs --spread R_SPREAD and --gain G")
FAR = int(sys.argv[sys.argv.index("--far") + 1]) if "--far" in sys.argv else None
if FAR is not None and not ("--views" in sys.argv and EXPLORE is not None):
    sys.exit("--far needs --views --explore R_MAX")
FAR_SPREAD = float(sys.argv[sys.argv.index("--far-spread") + 1]) if "--far-spread" in sys.argv else None
if FAR_SPREAD is not None and FAR is None:
    sys.exit("--far-spread needs --far BLOCK")
PASSES = int(sys.argv[sys.argv.index("--passes") + 1]) if "--passes" in sys.argv else None
if PASSES is not None and FAR_SPREAD is None:
    sys.exit("--passes needs --far-spread R_SPREAD")
FAR_GAIN = int(sys.argv[sys.argv.index("--far-gain") + 1]) if "--far-gain" in sys.argv else None
if FAR_GAIN is not None and FAR is None:
    sys.exit("--far-gain needs --far BLOCK")
FAR_TEAM = FAR_SPREAD is not None and FAR_GAIN is not None   # both: Fleet.explore_far_team
FAR_CLAIM_BLOCKS = int(sys.argv[sys.argv.index("--far-claim-blocks") + 1]) if "--far-claim-blocks" in sys.argv else None
if FAR_CLAIM_BLOCKS is not None and not FAR_TEAM:
    sys.exit("--far-claim-blocks needs --far-spread R_SPREAD and --far-gain G")
FAR_HOP_COST = int(sys.argv[sys.argv.index("--far-hop-cost") + 1]) if "--far-hop-cost" in sys.argv else None
FAR_MIN_GAIN = int(sys.argv[sys.argv.index("--far-min-gain") + 1]) if "--far-min-gain" in sys.argv else 0
if ("--far-hop-cost" in sys.argv or "--far-min-gain" in sys.argv) and FAR_GAIN is None:
    sys.exit("--far-hop-cost and --far-min-gain need --far-gain G")
SIGHT = "--sight" in sys.argv
if SIGHT and (GAIN is None or SPREAD is not None):
    sys.exit("--sight needs --gain G and no --spread")
WALLS = "--walls" in sys.argv


def timed_audit(fl, cycles):
    """The audit of the plans as they stand, `cycles` times, fenced by events like a stage; the last records on the host for the counts."""
    ms = []
    fl.audit_device()   # (warm-up)
    for _ in range(max(cycles, 1)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(fl.stream)
        d_out = fl.audit_device()
        e1.record(fl.stream)
        fl.sync()
        ms.append(e0.elapsed_time(e1))
    rec = d_out.cpu().numpy().view(abi.plan_audit_dtype)
    return {"ms": float(np.median(ms)), "tested_states": int(rec["n_tested"].sum()),
            "near_unknown": int(((rec["flags"] & abi.FH_AUDIT_UNKNOWN) != 0).sum()),
            "near_occupied": int(((rec["flags"] & abi.FH_AUDIT_OCCUPIED) != 0).sum()),
            "not_finite": int(((rec["flags"] & abi.FH_AUDIT_NOT_FINITE) != 0).sum())}


def listed_candidates(fl, cap, count, sample=1024):
    """What the broad phase works with, restated with torch on the fleet's plans: the boxes of the positions a vehicle can show (its
    states below `count`, and its last state where it stands for the others), the largest half-extent per axis, and for a sample of
    vehicles how many other boxes meet theirs grown by cap: the candidates the narrow phase lists."""
    v = fl.vehicles()
    B, S = fl.n, fl.max_states
    head = torch.from_numpy(v["plan_head"].astype(np.int64)).to(fl.dev)[:, None]
    size = torch.from_numpy(v["plan_size"].astype(np.int64)).to(fl.dev)[:, None]
    m = torch.clamp(size, max=count) if count > 0 else size
    lo, hi = torch.empty((B, 3), dtype=torch.float64, device=fl.dev), torch.empty((B, 3), dtype=torch.float64, device=fl.dev)
    pos = fl.d_plans.view(torch.float64).view(B, S, 12)
    idx = torch.arange(S, device=fl.dev)[None, :]
    for a in range(0, B, 4096):   # (in pieces: the masked copies of the positions are temporaries)
        sl = slice(a, a + 4096)
        shown = (idx >= head[sl]) & (idx < head[sl] + m[sl])
        shown |= (idx == head[sl] + size[sl] - 1) & (size[sl] >= 1) & ((size[sl] < count) if count > 0 else True)
        p = pos[sl, :, :3]
        lo[sl] = torch.where(shown[..., None], p, torch.full_like(p, float("inf"))).amin(dim=1)
        hi[sl] = torch.where(shown[..., None], p, torch.full_like(p, -float("inf"))).amax(dim=1)
    boxed = (lo <= hi).all(dim=1)
    half = torch.where(boxed[:, None], 0.5 * (hi - lo), torch.zeros_like(lo))
    pick = torch.randperm(B, device=fl.dev)[:min(sample, B)]
    pick = pick[boxed[pick]]
    meet = ((hi[None, :, :] >= lo[pick][:, None, :] - cap) & (lo[None, :, :] <= hi[pick][:, None, :] + cap)).all(dim=2) & boxed[None, :]
    return {"half_extent_max": [float(x) for x in half.amax(dim=0)], "half_extent_mean": [float(x) for x in half.mean(dim=0)],
            "candidates_mean": float(meet.sum(dim=1).double().mean()) - 1.0, "candidates_max": int(meet.sum(dim=1).max()) - 1,
            "sample": int(pick.numel())}


def timed_separation(fl, cycles):
    """The separation of the plans as they stand, with count = delta_t and with every state, each `cycles` times and fenced by events
    like a stage; the last records on the host for the counts."""
    r = 2.0 * float(fl.params["rule"]["drone_radius"])
    out = {"r": r, "cap": 2.0 * r, "cells": list(fl.separation_cells(2.0 * r)[2]), "cell_res": fl.separation_cells(2.0 * r)[1]}
    for name, count in (("head", int(fl.params["delta_t"])), ("all", 0)):
        ms = []
        fl.separation_device(count=count)   # (warm-up)
        for _ in range(max(cycles, 1)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(fl.stream)
            d_out = fl.separation_device(count=count)
            e1.record(fl.stream)
            fl.sync()
            ms.append(e0.elapsed_time(e1))
        rec = d_out.cpu().numpy().view(abi.plan_separation_dtype)
        out[name] = dict(listed_candidates(fl, 2.0 * r, count), ms=float(np.median(ms)), count=count, tested_states=int(rec["n_tested"].sum()),
                         near=int(((rec["flags"] & abi.FH_SEP_NEAR) != 0).sum()), within_cap=int(np.isfinite(rec["min_d2"]).sum()),
                         near_others_mean=float(rec["n_near"].mean()), not_finite=int(((rec["flags"] & abi.FH_SEP_NOT_FINITE) != 0).sum()))
    return out


def check_cycles(fl, cycles):
    """The cycle after Fleet.enable_check: see the module docstring."""
    fl.enable_check()
    fl.replan()
    fl.next_goals(5)
    fl.sync()
    names = [n for n, _ in fl.stages()] + ["next_goals"]
    per = {n: [] for n in names}
    candidates, withheld, committed = [], [], []
    for _ in range(cycles):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)]
        ev[0].record(fl.stream)
        for j, (n, launch) in enumerate(fl.stages()):
            launch()
            ev[j + 1].record(fl.stream)
        fl.next_goals(5)
        ev[-1].record(fl.stream)
        fl.sync()
        for j, n in enumerate(names):
            per[n].append(ev[j].elapsed_time(ev[j + 1]))
        rec, v = fl.check_records(), fl.vehicles()
        candidates.append(int(((rec["flags"] & abi.FH_CHECK_CANDIDATE) != 0).sum()))
        withheld.append(int(((rec["flags"] & abi.FH_CHECK_CONFLICT) != 0).sum()))
        committed.append(int((v["stage"] == abi.FH_FLEET_STAGE_COMMITTED).sum()))
    med = {n: float(np.median(v)) for n, v in per.items()}
    ms = []
    fl.separation_device(count=0)   # (warm-up)
    for _ in range(max(cycles, 1)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(fl.stream)
        fl.separation_device(count=0)
        e1.record(fl.stream)
        fl.sync()
        ms.append(e0.elapsed_time(e1))
    return {"r": float(fl.check_par["r"]), "stride": 1, "count": 0, "cells": list(fl.check_cells[2]), "cell_res": fl.check_cells[1],
            "stages_ms": med, "cycle_fenced_ms": float(sum(med.values())), "check_stages_ms": med["backup"] + med["check"] + med["revert"],
            "candidates": candidates, "withheld": withheld, "committed_after_revert": committed,
            "first_kind_1_last": int((rec["first_kind"] == 1).sum()), "separation_count_0_ms": float(np.median(ms))}


def timed_cycles(fl, cycles, r_sense=None, fov=None, observe=False, traffic=False, link=None, los=False):
    """`cycles` cycles, every stage fenced by events: {stage: [ms]} (with r_sense: sensing first, as a stage of its own; fov: forward;
    observe: Fleet.observe after it, as another; traffic: Fleet.traffic after that; link: the two stages of Fleet.link(link) after those)."""
    linked = fl.link_stages(link, los=los) if link else []
    names = ((["sense"] if r_sense else []) + (["observe"] if observe else []) + (["traffic"] if traffic else []) + [n for n, _ in linked]
             + [n for n, _ in fl.stages()] + ["next_goals"])
    per = {n: [] for n in names}
    for _ in range(cycles):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)]
        ev[0].record(fl.stream)
        k = 0
        if r_sense:
            fl.sense(r_sense, fov=fov)
            k = 1
            ev[1].record(fl.stream)
        if observe:
            fl.observe()
            k += 1
            ev[k].record(fl.stream)
        if traffic:
            fl.traffic()
            k += 1
            ev[k].record(fl.stream)
        for _, launch in linked:
            launch()
            k += 1
            ev[k].record(fl.stream)
        for j, (n, launch) in enumerate(fl.stages()):
            launch()
            ev[k + j + 1].record(fl.stream)
        fl.next_goals(5)
        ev[-1].record(fl.stream)
        fl.sync()
        for j, n in enumerate(names):
            per[n].append(ev[j].elapsed_time(ev[j + 1]))
    return {n: float(np.median(v)) for n, v in per.items()}


def link_side_by_side(fl, r, cycles):
    """On the fleet as the last timed cycle left it: the groups stage of Fleet.link(r) and of Fleet.link(r, los=True), one after the other
    `cycles` times (at least 5), each fenced by events: the medians and the spread of both in ms, and what each found."""
    stages = [fl.link_stages(r)[0], fl.link_stages(r, los=True)[0]]
    ms, info = {n: [] for n, _ in stages}, {}
    for _ in range(max(cycles, 5)):
        for name, launch in stages:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(fl.stream)
            launch()
            e1.record(fl.stream)
            fl.sync()
            ms[name].append(e0.elapsed_time(e1))
            info[name] = fl.link_records()[1]
    plain, los = info["link_groups"], info["link_groups_los"]
    out = {"groups": int(plain[1]), "groups_los": int(los[1]), "linked_pairs": int(plain[2]), "linked_pairs_los": int(los[2]),
           "blocked_pairs": int(los[3]), "changed_last_pass_los": int(los[0])}
    for name, v in ms.items():
        out[name + "_ms"] = float(np.median(v))
        out[name + "_ms_min_max"] = [float(min(v)), float(max(v))]
    return out


def sensing_loop(fl, views, cycles, states, goals, r_sense, fov=None, link=None, los=False):
    """The closed loop from views that are all unknown: the first look, then sense -> [link ->] replan -> 5 ticks in steady state
    (los: walls block a link, Fleet.link(link, los=True))."""
    views.fill_(1)
    fl.init(states, goals)
    if fov is not None:
        u = goals - states["pos"]
        fl.enable_heading(yaw0=np.arctan2(u[:, 1], u[:, 0]))   # (looking towards the goal)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(fl.stream)
    fl.sense(r_sense, fov=fov)
    e1.record(fl.stream)
    fl.sync()
    first = e0.elapsed_time(e1)
    if link:
        fl.link(link, los=los)
    fl.replan()
    fl.next_goals(5)
    fl.sync()
    med = timed_cycles(fl, cycles, r_sense, fov, link=link, los=los)
    t = []
    for _ in range(cycles):
        fl.sync()
        t0 = time.perf_counter()
        fl.sense(r_sense, fov=fov)
        if link:
            fl.link(link, los=los)
        fl.replan()
        fl.next_goals(5)
        fl.sync()
        t.append(1e3 * (time.perf_counter() - t0))
    v = fl.vehicles()
    loop = {"stages_ms": med, "cycle_fenced_ms": float(sum(med.values())), "cycle_ms": float(np.median(t)),
            "committed_last": int((v["stage"] == abi.FH_FLEET_STAGE_COMMITTED).sum()),
            "unknown_fraction_end": float(views.float().mean().item())}
    if AUDIT:
        loop["audit"] = timed_audit(fl, cycles)
    return first, loop


def fenced_ms(fl, launch, reps):
    """`launch` `reps` times on the fleet's stream, each between two events: [ms]."""
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(fl.stream)
        launch()
        e1.record(fl.stream)
        fl.sync()
        ms.append(e0.elapsed_time(e1))
    return ms


def explore_loop(fl, views, cycles, states, goals, r_sense, r_max):
    """The closed loop with Fleet.explore from views that are all unknown: see the module docstring."""
    views.fill_(1)
    fl.init(states, goals)
    u = goals - states["pos"]
    fl.enable_heading(yaw0=np.arctan2(u[:, 1], u[:, 0]))
    fl.sense(r_sense)
    first = fl.coverage()
    # the chooser in use and the fallback behind it, as Fleet.CHOOSERS names them, with what the flags give their methods
    team_args = (SPREAD, GAIN, CLAIM_RADIUS, HOP_COST, MIN_GAIN)
    near, near_args = ("bid", team_args) if BID else ("team", team_args) if TEAM else ("spread", (SPREAD,)) if SPREAD is not None \
        else ("sight", (GAIN, HOP_COST, MIN_GAIN)) if SIGHT else ("gain", (GAIN, HOP_COST, MIN_GAIN)) if GAIN is not None \
        else ("reach", ()) if REACH else ("explore", ())
    far, far_args, far_kw = ("far_team", (FAR, FAR_SPREAD, FAR_GAIN, FAR_HOP_COST, FAR_MIN_GAIN, FAR_CLAIM_BLOCKS), {"passes": PASSES}) if FAR_TEAM \
        else ("far_spread", (FAR, FAR_SPREAD), {"passes": PASSES}) if FAR_SPREAD is not None \
        else ("far_gain", (FAR, FAR_GAIN, FAR_HOP_COST, FAR_MIN_GAIN), {}) if FAR_GAIN is not None else ("far", (FAR,), {}) if FAR is not None \
        else (None, (), {})
    ch = Fleet.CHOOSERS[near]
    goal_stage, explore_records = ch.stage, getattr(fl, near + "_records")
    explore_stages = lambda r, **kw: getattr(fl, ch.method + "_stages")(r, *near_args, **kw)   # noqa: E731
    far_after = "reachable" if near == "reach" else near
    far_kw["after"] = far_after
    # teams: the groups of one link() after the first look (without it every vehicle is a group of its own)
    if LINK and ch.labels:
        fl.link(LINK[0])
    getattr(fl, ch.method)(r_max, *near_args)
    if LINK and FAR_SPREAD is not None and SPREAD is None:   # (the choosers for a team above have linked)
        fl.link(LINK[0])
    if far:
        getattr(fl, Fleet.CHOOSERS[far].method)(*far_args, **far_kw)
    fl.replan()
    fl.next_goals(5)
    fl.sync()
    explore = explore_stages(r_max)
    if far:   # the fallback after the chooser in use, for the vehicles it left without a goal
        explore = explore + [(n if n == far + "_goals" else far + "_set_goals", f)
                             for n, f in getattr(fl, Fleet.CHOOSERS[far].method + "_stages")(*far_args, **far_kw)]
    names = ["sense"] + [n for n, _ in explore] + [n for n, _ in fl.stages()] + ["next_goals"]
    per, wanted, found = {n: [] for n in names}, [], []
    for _ in range(cycles):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)]
        ev[0].record(fl.stream)
        fl.sense(r_sense)
        ev[1].record(fl.stream)
        for j, (_, launch) in enumerate(explore + fl.stages()):
            launch()
            ev[j + 2].record(fl.stream)
        fl.next_goals(5)
        ev[-1].record(fl.stream)
        fl.sync()
        for j, n in enumerate(names):
            per[n].append(ev[j].elapsed_time(ev[j + 1]))
        rec = explore_records()[0]
        wanted.append(int((rec["flags"] & abi.FH_FRONTIER_WANTED != 0).sum()))
        found.append(int((rec["flags"] & abi.FH_FRONTIER_FOUND != 0).sum()))
    med = {n: float(np.median(v)) for n, v in per.items()}
    # every vehicle wanted, applied to nobody: the one launch of frontier_goals; and the coverage
    all_ms = fenced_ms(fl, fl.explore_stages(r_max, want="all")[0][1], max(cycles, 3))
    rec = fl.explore_records()[0]
    cov_ms = fenced_ms(fl, fl.coverage_stages()[0][1], max(cycles, 3))
    last = fl.coverage()
    reach = {}
    if REACH:   # every vehicle wanted, applied to nobody, as frontier_goals above
        reach_ms = fenced_ms(fl, fl.explore_reachable_stages(r_max, want="all")[0][1], max(cycles, 3))
        rr = fl.reach_records()[0]
        hit = (rr["flags"] & (abi.FH_REACH_START_OUTSIDE | abi.FH_REACH_BOX_TOO_LARGE | abi.FH_FRONTIER_NO_VIEW | abi.FH_FRONTIER_BAD_POS)) == 0
        reach = {"reach_goals_reached_ms": med.get("reach_goals"), "reach_goals_all_ms": float(np.median(reach_ms)),
                 "reach_goals_all_runs_ms": [float(x) for x in reach_ms], "reach_found_all": int((rr["flags"] & abi.FH_FRONTIER_FOUND != 0).sum()),
                 "reach_searched_all": int(hit.sum()), "reach_box_too_large": int((rr["flags"] & abi.FH_REACH_BOX_TOO_LARGE != 0).sum()),
                 "reach_start_outside": int((rr["flags"] & abi.FH_REACH_START_OUTSIDE != 0).sum()),
                 "levels_mean": float(rr["levels"][hit].mean()) if hit.any() else 0.0, "levels_max": int(rr["levels"].max()),
                 "reached_mean": float(rr["reached"][hit].mean()) if hit.any() else 0.0, "reached_max": int(rr["reached"].max()),
                 "hops_mean": float(rr["hops"][rr["hops"] >= 0].mean()) if (rr["hops"] >= 0).any() else -1.0,
                 "candidates_mean": float(rr["candidates"][hit].mean()) if hit.any() else 0.0,
                 "reachable_mean": float(rr["reachable"][hit].mean()) if hit.any() else 0.0,
                 "same_cell_as_frontier_goals": int((rr["cell"] == rec["cell"]).sum())}
    far = {}
    if FAR_TEAM:   # every vehicle wanted and nobody skipped, applied to nobody, beside far_spread_goals and far_gain_goals in the same call, medians of five
        tr = fl.far_team_records()[0]
        searched = lambda r: (r["flags"] & ~(abi.FH_FRONTIER_FOUND | abi.FH_REACH_CUT | abi.FH_STAKE_UNSETTLED | abi.FH_STAKE_CLAIMED |
                                             abi.FH_STAKE_ALL_POOR)) == abi.FH_FRONTIER_WANTED   # noqa: E731
        team_all = lambda passes: fl.explore_far_team_stages(FAR, FAR_SPREAD, FAR_GAIN, FAR_HOP_COST, FAR_MIN_GAIN, FAR_CLAIM_BLOCKS, want="all",
                                                             passes=passes)[0][1]   # noqa: E731
        runs = {}
        for label, passes in (("1", 1), ("8", 8), ("64", abi.FH_STAKE_MAX_PASSES), ("set", PASSES)):   # (the one asked for last: its records are read below)
            runs[label] = fenced_ms(fl, team_all(passes), 5)
        ta = fl.far_team_records()[0]
        spread_ms = fenced_ms(fl, fl.explore_far_spread_stages(FAR, FAR_SPREAD, want="all", passes=PASSES)[0][1], 5)
        sb = fl.far_spread_records()[0]
        gain_ms = fenced_ms(fl, fl.explore_far_gain_stages(FAR, FAR_GAIN, FAR_HOP_COST, FAR_MIN_GAIN, want="all")[0][1], 5)
        gb = fl.far_gain_records()[0]
        hit = searched(ta)
        chosen = ta["hops"] >= 0
        far = {"far_team": {"block": FAR, "r_spread": FAR_SPREAD, "gain_blocks": FAR_GAIN,
                            "hop_cost": int(FAR * FAR if FAR_HOP_COST is None else FAR_HOP_COST), "min_gain": FAR_MIN_GAIN,
                            "claim_blocks": int(FAR_GAIN if FAR_CLAIM_BLOCKS is None else FAR_CLAIM_BLOCKS),
                            "passes": int(PASSES or abi.FH_STAKE_DEFAULT_PASSES), "after": far_after, "linked": bool(LINK),
                            "work_bytes": int(fl.d_far_team_work.numel()),
                            "far_team_goals_loop_ms": med.get("far_team_goals"), "searchers_last_cycle": int(searched(tr).sum()),
                            "skipped_last_cycle": int((tr["flags"] & abi.FH_STAKE_SKIPPED != 0).sum()),
                            "far_team_goals_all_ms": float(np.median(runs["set"])), "far_team_goals_all_runs_ms": [float(x) for x in runs["set"]],
                            "far_team_goals_all_1_pass_ms": float(np.median(runs["1"])),
                            "far_team_goals_all_8_passes_ms": float(np.median(runs["8"])),
                            "far_team_goals_all_64_passes_ms": float(np.median(runs["64"])),
                            "idle_pass_ms": float((np.median(runs["64"]) - np.median(runs["8"])) / (abi.FH_STAKE_MAX_PASSES - 8)),
                            "far_spread_goals_all_beside_ms": float(np.median(spread_ms)),
                            "far_spread_goals_all_beside_runs_ms": [float(x) for x in spread_ms],
                            "far_gain_goals_all_beside_ms": float(np.median(gain_ms)), "far_gain_goals_all_beside_runs_ms": [float(x) for x in gain_ms],
                            "searchers_all": int(hit.sum()), "found_all": int((ta["flags"] & abi.FH_FRONTIER_FOUND != 0).sum()),
                            "far_spread_found_all_beside": int((sb["flags"] & abi.FH_FRONTIER_FOUND != 0).sum()),
                            "far_gain_found_all_beside": int((gb["flags"] & abi.FH_FRONTIER_FOUND != 0).sum()),
                            "lower_max": int(ta["lower"].max()), "standing_max": int(ta["standing"].max()), "claims_max": int(ta["claims"].max()),
                            "unsettled_all": int((ta["flags"] & abi.FH_STAKE_UNSETTLED != 0).sum()),
                            "all_claimed_all": int((ta["flags"] & abi.FH_STAKE_CLAIMED != 0).sum()),
                            "all_poor_all": int((ta["flags"] & abi.FH_STAKE_ALL_POOR != 0).sum()),
                            "claimed_mean": float(ta["claimed"][hit].mean()) if hit.any() else 0.0,
                            "covered_mean": float(ta["covered"][hit].mean()) if hit.any() else 0.0,
                            "removed_mean": float(ta["removed"][hit].mean()) if hit.any() else 0.0,
                            "gain_mean": float(ta["gain"][chosen].mean()) if chosen.any() else -1.0,
                            "far_gain_gain_mean_beside": float(gb["gain"][gb["hops"] >= 0].mean()) if (gb["hops"] >= 0).any() else -1.0,
                            "hops_mean": float(ta["hops"][chosen].mean()) if chosen.any() else -1.0,
                            "same_cell_as_far_spread_goals": int((ta["cell"] == sb["cell"]).sum()),
                            "same_cell_as_far_gain_goals": int((ta["cell"] == gb["cell"]).sum())}}
    elif FAR_SPREAD is not None:   # every vehicle wanted and nobody skipped, applied to nobody, beside far_goals in the same call, medians of five
        sr = fl.far_spread_records()[0]
        searched = lambda r: (r["flags"] & ~(abi.FH_FRONTIER_FOUND | abi.FH_REACH_CUT | abi.FH_APART_UNSETTLED | abi.FH_APART_CLAIMED)) \
            == abi.FH_FRONTIER_WANTED   # noqa: E731
        runs = {}
        for label, passes in (("set", PASSES), ("1", 1), ("64", abi.FH_APART_MAX_PASSES)):
            runs[label] = fenced_ms(fl, fl.explore_far_spread_stages(FAR, FAR_SPREAD, want="all", passes=passes)[0][1], 5)
            if label == "set":
                sa = fl.far_spread_records()[0]
        beside_ms = fenced_ms(fl, fl.explore_far_stages(FAR, want="all")[0][1], 5)
        fb = fl.far_records()[0]
        hit = searched(sa)
        far = {"far_spread": {"block": FAR, "r_spread": FAR_SPREAD, "passes": int(PASSES or abi.FH_APART_DEFAULT_PASSES), "after": far_after,
                              "linked": bool(LINK), "work_bytes": int(fl.d_far_spread_work.numel()),
                              "far_spread_goals_loop_ms": med.get("far_spread_goals"), "searchers_last_cycle": int(searched(sr).sum()),
                              "skipped_last_cycle": int((sr["flags"] & abi.FH_FAR_SKIPPED != 0).sum()),
                              "far_spread_goals_all_ms": float(np.median(runs["set"])), "far_spread_goals_all_runs_ms": [float(x) for x in runs["set"]],
                              "far_spread_goals_all_1_pass_ms": float(np.median(runs["1"])),
                              "far_spread_goals_all_64_passes_ms": float(np.median(runs["64"])),
                              "ms_per_pass": float((np.median(runs["64"]) - np.median(runs["1"])) / (abi.FH_APART_MAX_PASSES - 1)),
                              "far_goals_all_beside_ms": float(np.median(beside_ms)), "far_goals_all_beside_runs_ms": [float(x) for x in beside_ms],
                              "searchers_all": int(hit.sum()), "found_all": int((sa["flags"] & abi.FH_FRONTIER_FOUND != 0).sum()),
                              "far_found_all_beside": int((fb["flags"] & abi.FH_FRONTIER_FOUND != 0).sum()),
                              "lower_max": int(sa["lower"].max()), "standing_max": int(sa["standing"].max()), "claims_max": int(sa["claims"].max()),
                              "unsettled_all": int((sa["flags"] & abi.FH_APART_UNSETTLED != 0).sum()),
                              "all_claimed_all": int((sa["flags"] & abi.FH_APART_CLAIMED != 0).sum()),
                              "claimed_mean": float(sa["claimed"][hit].mean()) if hit.any() else 0.0,
                              "same_cell_as_far_goals": int((sa["cell"] == fb["cell"]).sum())}}
    elif FAR_GAIN is not None:   # every vehicle wanted and nobody skipped, applied to nobody, beside far_goals in the same call, medians of five
        gr = fl.far_gain_records()[0]
        searched = lambda r: (r["flags"] & ~(abi.FH_FRONTIER_FOUND | abi.FH_REACH_CUT | abi.FH_PROSPECT_ALL_POOR)) == abi.FH_FRONTIER_WANTED   # noqa: E731
        runs = {}
        for g in (0, 1, 2, 5, FAR_GAIN):   # (the one asked for last: its records are read below)
            runs[g] = fenced_ms(fl, fl.explore_far_gain_stages(FAR, g, FAR_HOP_COST, FAR_MIN_GAIN, want="all")[0][1], 5)
        ga = fl.far_gain_records()[0]
        beside_ms = fenced_ms(fl, fl.explore_far_stages(FAR, want="all")[0][1], 5)
        fb = fl.far_records()[0]
        hit = searched(ga)
        chosen = ga["hops"] >= 0
        _, _, dims_ = fl.grid
        view_bytes = int(dims_[0]) * int(dims_[1]) * int(dims_[2])
        far = {"far_gain": {"block": FAR, "gain_blocks": FAR_GAIN, "hop_cost": int(FAR * FAR if FAR_HOP_COST is None else FAR_HOP_COST),
                            "min_gain": FAR_MIN_GAIN, "after": far_after, "work_bytes": int(fl.d_far_gain_work.numel()),
                            "far_gain_goals_loop_ms": med.get("far_gain_goals"), "searched_last_cycle": int(searched(gr).sum()),
                            "skipped_last_cycle": int((gr["flags"] & abi.FH_PROSPECT_SKIPPED != 0).sum()),
                            "far_gain_goals_all_ms": float(np.median(runs[FAR_GAIN])), "far_gain_goals_all_runs_ms": [float(x) for x in runs[FAR_GAIN]],
                            "far_gain_goals_all_by_gain_blocks_ms": {str(g): float(np.median(runs[g])) for g in (0, 1, 2, 5)},
                            "far_goals_all_beside_ms": float(np.median(beside_ms)), "far_goals_all_beside_runs_ms": [float(x) for x in beside_ms],
                            "view_bytes": view_bytes, "summary_bytes_all": view_bytes * int(fl.n_views),
                            "searched_all": int(hit.sum()), "found_all": int((ga["flags"] & abi.FH_FRONTIER_FOUND != 0).sum()),
                            "all_poor_all": int((ga["flags"] & abi.FH_PROSPECT_ALL_POOR != 0).sum()),
                            "far_found_all_beside": int((fb["flags"] & abi.FH_FRONTIER_FOUND != 0).sum()),
                            "same_cell_as_far_goals": int((ga["cell"] == fb["cell"]).sum()),
                            "levels_mean": float(ga["levels"][hit].mean()) if hit.any() else 0.0,
                            "reachable_mean": float(ga["reachable"][hit].mean()) if hit.any() else 0.0,
                            "hops_mean": float(ga["hops"][chosen].mean()) if chosen.any() else -1.0,
                            "far_hops_mean_beside": float(fb["hops"][fb["hops"] >= 0].mean()) if (fb["hops"] >= 0).any() else -1.0,
                            "gain_mean": float(ga["gain"][chosen].mean()) if chosen.any() else -1.0,
                            "best_gain_max": int(ga["best_gain"].max())}}
    elif FAR is not None:   # every vehicle wanted and nobody skipped, applied to nobody, beside reach_goals in the same call, a median of five each
        fr = fl.far_records()[0]
        far_ms = fenced_ms(fl, fl.explore_far_stages(FAR, want="all")[0][1], 5)
        fa = fl.far_records()[0]
        beside_ms = fenced_ms(fl, fl.explore_reachable_stages(r_max, want="all")[0][1], 5)
        hit = (fa["flags"] & ~(abi.FH_FRONTIER_FOUND | abi.FH_REACH_CUT)) == abi.FH_FRONTIER_WANTED
        far = {"far": {"block": FAR, "after": far_after, "work_bytes": int(fl.d_far_work.numel()),
                       "far_goals_loop_ms": med.get("far_goals"), "far_searched_last_cycle": int(((fr["flags"] & ~(abi.FH_FRONTIER_FOUND | abi.FH_REACH_CUT))
                                                                                                    == abi.FH_FRONTIER_WANTED).sum()),
                       "far_skipped_last_cycle": int((fr["flags"] & abi.FH_FAR_SKIPPED != 0).sum()),
                       "far_goals_all_ms": float(np.median(far_ms)), "far_goals_all_runs_ms": [float(x) for x in far_ms],
                       "reach_goals_all_beside_ms": float(np.median(beside_ms)), "reach_goals_all_beside_runs_ms": [float(x) for x in beside_ms],
                       "far_searched_all": int(hit.sum()), "far_found_all": int((fa["flags"] & abi.FH_FRONTIER_FOUND != 0).sum()),
                       "levels_mean": float(fa["levels"][hit].mean()) if hit.any() else 0.0, "levels_max": int(fa["levels"].max()),
                       "reached_mean": float(fa["reached"][hit].mean()) if hit.any() else 0.0,
                       "targets_mean": float(fa["targets"][hit].mean()) if hit.any() else 0.0,
                       "hops_mean": float(fa["hops"][fa["hops"] >= 0].mean()) if (fa["hops"] >= 0).any() else -1.0,
                       "members_mean": float(fa["members"][fa["hops"] >= 0].mean()) if (fa["hops"] >= 0).any() else 0.0}}
    if BID:   # every vehicle wanted, applied to nobody: bid_goals and team_goals in turn, a median each
        reps = max(cycles, 5)
        runs = {"bid_goals": [], "team_goals": []}
        launches = {"bid_goals": explore_stages(r_max, want="all")[0][1],
                    "team_goals": fl.explore_team_stages(r_max, SPREAD, GAIN, CLAIM_RADIUS, HOP_COST, MIN_GAIN, want="all")[0][1]}
        for _ in range(reps):
            for name, launch in launches.items():
                runs[name] += fenced_ms(fl, launch, 1)
        one_ms = fenced_ms(fl, explore_stages(r_max, want="all", passes=1)[0][1], reps)
        launches["bid_goals"]()
        br, tr = fl.bid_records()[0], fl.team_records()[0]

        def figures(r, unsettled, overflow):
            searched = r["decided_pass"] > 0
            given = r["cell"] >= 0
            keys = np.stack([r["group"][given].astype(np.int64), r["cell"][given].astype(np.int64)], axis=1)
            _, counts = np.unique(keys, axis=0, return_counts=True) if len(keys) else (None, np.zeros(0, dtype=np.int64))
            return {"decided_per_pass": np.bincount(r["decided_pass"][searched], minlength=2)[1:].tolist(), "decided": int(searched.sum()),
                    "unsettled": int((r["flags"] & unsettled != 0).sum()), "overflow": int((r["flags"] & overflow != 0).sum()),
                    "goals_given": int(given.sum()), "hops_sum": int(r["hops"][given].sum()),
                    "gain_mean": float(r["gain"][given].mean()) if given.any() else -1.0,
                    "utility_sum": int(r["utility"][given].sum()), "same_goal_voxel": int((counts - 1).sum())}

        bid, team = figures(br, abi.FH_BID_UNSETTLED, abi.FH_BID_OVERFLOW), figures(tr, abi.FH_TEAM_UNSETTLED, abi.FH_TEAM_OVERFLOW)
        took = br["searches"] > 0
        bid.update({"searches_mean": float(br["searches"][took].mean()) if took.any() else 0.0, "searches_max": int(br["searches"].max()),
                    "searches_sum": int(br["searches"].sum()), "rivals_max": int(br["rivals"].max()), "claims_max": int(br["claims"].max())})
        team.update({"lower_max": int(tr["lower"].max()), "claims_max": int(tr["claims"].max())})
        reach.update({"r_spread": SPREAD, "gain_radius": GAIN, "claim_radius": GAIN if CLAIM_RADIUS is None else CLAIM_RADIUS, "hop_cost": HOP_COST,
                      "min_gain": MIN_GAIN, "passes": abi.FH_BID_DEFAULT_PASSES, "bid_goals_reached_ms": med["bid_goals"],
                      "bid_goals_all_ms": float(np.median(runs["bid_goals"])), "bid_goals_all_runs_ms": [float(x) for x in runs["bid_goals"]],
                      "bid_goals_all_one_pass_ms": float(np.median(one_ms)),
                      "team_goals_all_ms": float(np.median(runs["team_goals"])), "team_goals_all_runs_ms": [float(x) for x in runs["team_goals"]],
                      "groups": int(len(np.unique(br["group"]))), "bid": bid, "team": team})
    elif TEAM:   # every vehicle wanted, applied to nobody: team_goals, gain_goals and spread_goals in turn, a median each
        reps = max(cycles, 5)
        runs = {"team_goals": [], "gain_goals": [], "spread_goals": []}
        launches = {"team_goals": explore_stages(r_max, want="all")[0][1],
                    "gain_goals": fl.explore_gain_stages(r_max, GAIN, HOP_COST, MIN_GAIN, want="all")[0][1],
                    "spread_goals": fl.explore_spread_stages(r_max, SPREAD, want="all")[0][1]}
        for _ in range(reps):
            for name, launch in launches.items():
                runs[name] += fenced_ms(fl, launch, 1)
        tr, t_goals, _ = fl.team_records()
        gr, sr = fl.gain_records()[0], fl.spread_records()[0]
        searched = tr["decided_pass"] > 0
        passes = np.bincount(tr["decided_pass"][searched], minlength=2)

        def shared_goals(r):   # teammates (one group) that hold the same goal voxel
            held = r["cell"] >= 0
            keys = np.stack([tr["group"][held].astype(np.int64), r["cell"][held].astype(np.int64)], axis=1)
            _, counts = np.unique(keys, axis=0, return_counts=True) if len(keys) else (None, np.zeros(0, dtype=np.int64))
            return int((counts - 1).sum())

        reach.update({"r_spread": SPREAD, "gain_radius": GAIN, "claim_radius": GAIN if CLAIM_RADIUS is None else CLAIM_RADIUS, "hop_cost": HOP_COST,
                      "min_gain": MIN_GAIN, "passes": abi.FH_TEAM_DEFAULT_PASSES, "team_goals_reached_ms": med["team_goals"],
                      "team_goals_all_ms": float(np.median(runs["team_goals"])), "team_goals_all_runs_ms": [float(x) for x in runs["team_goals"]],
                      "gain_goals_all_ms": float(np.median(runs["gain_goals"])), "gain_goals_all_runs_ms": [float(x) for x in runs["gain_goals"]],
                      "spread_goals_all_ms": float(np.median(runs["spread_goals"])), "spread_goals_all_runs_ms": [float(x) for x in runs["spread_goals"]],
                      "decided_per_pass": passes[1:].tolist(), "unsettled": int((tr["flags"] & abi.FH_TEAM_UNSETTLED != 0).sum()),
                      "overflow": int((tr["flags"] & abi.FH_TEAM_OVERFLOW != 0).sum()), "spread_overflow": int((sr["flags"] & abi.FH_SPREAD_OVERFLOW != 0).sum()),
                      "lower_max": int(tr["lower"].max()), "claims_max": int(tr["claims"].max()), "groups": int(len(np.unique(tr["group"]))),
                      "covered_mean": float(tr["covered"][searched].mean()) if searched.any() else 0.0, "covered_max": int(tr["covered"].max()),
                      "team_found_all": int((tr["cell"] >= 0).sum()), "gain_found_all": int((gr["cell"] >= 0).sum()),
                      "team_gain_mean": float(tr["gain"][tr["cell"] >= 0].mean()) if (tr["cell"] >= 0).any() else -1.0,
                      "all_poor": int((tr["flags"] & abi.FH_TEAM_ALL_POOR != 0).sum()),
                      "same_goal_voxel_team": shared_goals(tr), "same_goal_voxel_gain": shared_goals(gr)})
    elif SPREAD is not None:   # every vehicle wanted, applied to nobody: all passes, and one pass (the difference: the idle launches)
        reps = max(cycles, 3)
        spread_ms = fenced_ms(fl, explore_stages(r_max, want="all")[0][1], reps)
        sr = fl.spread_records()[0]
        one_ms = fenced_ms(fl, explore_stages(r_max, want="all", passes=1)[0][1], reps)
        two_ms = fenced_ms(fl, explore_stages(r_max, want="all", passes=2)[0][1], reps)
        again_ms = fenced_ms(fl, fl.explore_reachable_stages(r_max, want="all")[0][1], reps)
        passes = np.bincount(sr["decided_pass"][sr["decided_pass"] > 0], minlength=2)
        reach.update({"r_spread": SPREAD, "passes": abi.FH_APART_DEFAULT_PASSES, "spread_goals_reached_ms": med["spread_goals"],
                      "spread_goals_all_ms": float(np.median(spread_ms)), "spread_goals_all_runs_ms": [float(x) for x in spread_ms],
                      "spread_goals_all_one_pass_ms": float(np.median(one_ms)), "spread_goals_all_two_passes_ms": float(np.median(two_ms)),
                      "reach_goals_all_after_ms": float(np.median(again_ms)), "reach_goals_all_after_runs_ms": [float(x) for x in again_ms],
                      "decided_per_pass": passes[1:].tolist(), "passes_that_decided": int((passes[1:] > 0).sum()),
                      "unsettled": int((sr["flags"] & abi.FH_SPREAD_UNSETTLED != 0).sum()),
                      "overflow": int((sr["flags"] & abi.FH_SPREAD_OVERFLOW != 0).sum()),
                      "claimed_vehicles": int((sr["claimed"] > 0).sum()), "lower_max": int(sr["lower"].max()), "claims_max": int(sr["claims"].max()),
                      "groups": int(len(np.unique(sr["group"]))), "spread_found_all": int((sr["flags"] & abi.FH_FRONTIER_FOUND != 0).sum()),
                      "same_cell_as_reach_goals": int((sr["cell"] == rr["cell"]).sum())})
    if SIGHT:   # every vehicle wanted, applied to nobody: sight_goals and gain_goals in turn, a median each
        reps = max(cycles, 5)
        runs = {"sight_goals": [], "gain_goals": []}
        launches = {"sight_goals": explore_stages(r_max, want="all")[0][1],
                    "gain_goals": fl.explore_gain_stages(r_max, GAIN, HOP_COST, MIN_GAIN, want="all")[0][1]}
        for _ in range(reps):
            for name, launch in launches.items():
                runs[name] += fenced_ms(fl, launch, 1)
        sr, gr = fl.sight_records()[0], fl.gain_records()[0]
        chosen, both = sr["cell"] >= 0, (sr["cell"] >= 0) & (gr["cell"] >= 0)
        reach.update({"gain_radius": GAIN, "hop_cost": HOP_COST, "min_gain": MIN_GAIN, "sight_goals_reached_ms": med["sight_goals"],
                      "sight_goals_all_ms": float(np.median(runs["sight_goals"])), "sight_goals_all_runs_ms": [float(x) for x in runs["sight_goals"]],
                      "gain_goals_all_ms": float(np.median(runs["gain_goals"])), "gain_goals_all_runs_ms": [float(x) for x in runs["gain_goals"]],
                      "sight_found_all": int(chosen.sum()), "gain_found_all": int((gr["cell"] >= 0).sum()),
                      "evaluated_total": int(sr["reachable"].sum()), "evaluated_mean": float(sr["reachable"][hit].mean()) if hit.any() else 0.0,
                      "vehicles_with_walls": int((sr["walls"] > 0).sum()), "walls_mean": float(sr["walls"][hit].mean()) if hit.any() else 0.0,
                      "walls_max": int(sr["walls"].max()), "chosen_seeing_less_than_ball": int((sr["gain"][chosen] < sr["ball_gain"][chosen]).sum()),
                      "sight_gain_mean": float(sr["gain"][chosen].mean()) if chosen.any() else -1.0,
                      "sight_ball_gain_mean": float(sr["ball_gain"][chosen].mean()) if chosen.any() else -1.0,
                      "gain_gain_mean": float(gr["gain"][gr["cell"] >= 0].mean()) if (gr["cell"] >= 0).any() else -1.0,
                      "poor_total": int(sr["poor"].sum()), "all_poor": int((sr["flags"] & abi.FH_SIGHT_ALL_POOR != 0).sum()),
                      "same_counts_as_gain_goals": bool(all(np.array_equal(sr[k], gr[k]) for k in ("candidates", "reachable", "reached", "levels"))),
                      "other_cell_than_gain_goals": int((sr["cell"][both] != gr["cell"][both]).sum()), "chosen_by_both": int(both.sum())})
    if GAIN is not None and not TEAM and not SIGHT:   # every vehicle wanted, applied to nobody, with reach_goals after it again
        reps = max(cycles, 3)
        gain_ms = fenced_ms(fl, explore_stages(r_max, want="all")[0][1], reps)
        gr = fl.gain_records()[0]
        again_ms = fenced_ms(fl, fl.explore_reachable_stages(r_max, want="all")[0][1], reps)
        both = (gr["cell"] >= 0) & (rr["cell"] >= 0)
        chosen = gr["cell"] >= 0
        reach.update({"gain_radius": GAIN, "hop_cost": HOP_COST, "min_gain": MIN_GAIN, "gain_goals_reached_ms": med["gain_goals"],
                      "gain_goals_all_ms": float(np.median(gain_ms)), "gain_goals_all_runs_ms": [float(x) for x in gain_ms],
                      "reach_goals_all_after_ms": float(np.median(again_ms)), "reach_goals_all_after_runs_ms": [float(x) for x in again_ms],
                      "gain_found_all": int(chosen.sum()), "evaluated_mean": float(gr["reachable"][hit].mean()) if hit.any() else 0.0,
                      "evaluated_max": int(gr["reachable"].max()), "evaluated_total": int(gr["reachable"].sum()),
                      "levels_with_candidates_bound_mean": float(np.minimum(gr["levels"] + 1, gr["reachable"])[hit].mean()) if hit.any() else 0.0,
                      "gain_mean": float(gr["gain"][chosen].mean()) if chosen.any() else -1.0, "gain_max": int(gr["best_gain"].max()),
                      "gain_hops_mean": float(gr["hops"][chosen].mean()) if chosen.any() else -1.0,
                      "poor_total": int(gr["poor"].sum()), "all_poor": int((gr["flags"] & abi.FH_GAIN_ALL_POOR != 0).sum()),
                      "same_first_40_bytes_counts": bool(all(np.array_equal(gr[k], rr[k]) for k in ("candidates", "reachable", "reached", "levels"))),
                      "other_cell_than_reach_goals": int((gr["cell"][both] != rr["cell"][both]).sum()), "chosen_by_both": int(both.sum())})
    return {"r_max": r_max, "goal_stage": goal_stage, **reach, **far, "stages_ms": med, "cycle_fenced_ms": float(sum(med.values())), "wanted_per_cycle": wanted, "found_per_cycle": found,
            "frontier_goals_reached_ms": med.get("frontier_goals"), "frontier_goals_all_ms": float(np.median(all_ms)),
            "frontier_goals_all_runs_ms": [float(x) for x in all_ms], "found_all": int((rec["flags"] & abi.FH_FRONTIER_FOUND != 0).sum()),
            "candidates_all_mean": float(rec["candidates"].mean()), "view_coverage_ms": float(np.median(cov_ms)),
            "view_coverage_runs_ms": [float(x) for x in cov_ms],
            "known_first": int(first["known"].sum()), "frontier_first": int(first["frontier"].sum()),
            "known_last": int(last["known"].sum()), "frontier_last": int(last["frontier"].sum())}


def views_cycles(B, cycles, p, world, r_sense, staging, fov=None):
    """The cycle with a view per vehicle: see the module docstring."""
    cloud, cells, res, center, zmax, infl, states, goals, flags, origin, dims = world
    n_cells = dims[0] * dims[1] * dims[2]
    out = {"views_bytes": B * n_cells, "r_sense": r_sense, "sense_staging": bool(staging)}
    print("views: %d x %d bytes = %.2f GB" % (B, n_cells, B * n_cells / 1e9), file=sys.stderr)
    fl = Fleet(B, p, max_states=1024)
    try:
        fl.ctx.set_sense_staging(staging)
        fl.set_map(cloud, cells, res, center, zmax, infl)
        views = torch.from_numpy(flags.reshape(1, -1)).to(fl.dev).repeat(B, 1)
        fl.set_unknown_views(views, origin=origin, res=res, dims=dims)
        fl.init(states, goals)
        fl.replan()
        fl.next_goals(5)
        fl.sync()
        med = timed_cycles(fl, cycles)
        out["views_same_flags"] = {"stages_ms": med, "cycle_fenced_ms": float(sum(med.values()))}
        if AUDIT:
            out["views_same_flags"]["audit"] = timed_audit(fl, cycles)
        # the closed loop: everything unknown at first, the vehicles back at their starts
        out["sense_first_ms"], out["views_sensing"] = sensing_loop(fl, views, cycles, states, goals, r_sense)
        if fov is not None:
            first, loop = sensing_loop(fl, views, cycles, states, goals, r_sense, fov)
            out["fov_sensing"] = dict(loop, sense_first_ms=first, tan_half_h=fov[0], tan_half_v=fov[1])
        if LINK:
            out["link"] = {"passes": abi.FH_LINK_DEFAULT_PASSES, "ranges": {}}
            for r in LINK:
                _, loop = sensing_loop(fl, views, cycles, states, goals, r_sense, link=r, los=LINK_LOS)
                labels, info = fl.link_records()
                groups_stage = "link_groups_los" if LINK_LOS else "link_groups"
                loop.update({"changed_last_pass": int(info[0]), "groups": int(info[1]), "linked_pairs": int(info[2]),
                             "largest_group": int(np.bincount(labels).max()), "link_ms": loop["stages_ms"][groups_stage] + loop["stages_ms"]["link_merge"]})
                if LINK_LOS:
                    loop["blocked_pairs"] = int(info[3])
                    loop["los"] = link_side_by_side(fl, r, cycles)
                out["link"]["ranges"]["%g" % r] = loop
            # the yardstick of the merge: the views' bytes copied device to device on the fleet's stream, fenced the same way
            other, ms = torch.empty_like(views), []
            with torch.cuda.stream(fl.stream):
                other.copy_(views)
                for _ in range(5):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(fl.stream)
                    other.copy_(views)
                    e1.record(fl.stream)
                    fl.sync()
                    ms.append(e0.elapsed_time(e1))
            out["link"]["views_copy_ms"] = float(np.median(ms))
            for loop in out["link"]["ranges"].values():
                loop["merge_over_copy"] = loop["stages_ms"]["link_merge"] / out["link"]["views_copy_ms"]
        if EXPLORE is not None:
            out["explore"] = explore_loop(fl, views, cycles, states, goals, r_sense, EXPLORE)
    finally:
        fl.close()
    return out


def occupancy_cycles(B, cycles, p, world, r_sense, teams):
    """The closed loop with occupied space per team: see the module docstring."""
    cloud, cells, res, center, zmax, _, states, goals, flags, _, _ = world
    infl = 0.5 * res   # (below one cell: a point marks its own cell only, so its voxel can be seen and the point observed)
    probe = capi.Map(0)
    probe.read(cloud, cells, res, center, 0.0, zmax, infl)
    dims, origin = probe.dims()
    probe.close()
    dims = [int(d) for d in dims]
    n_cells = dims[0] * dims[1] * dims[2]
    words = abi.point_mask_words(len(cloud))
    out = {"teams": teams, "world_inflation": infl, "bytes_per_view": {"unknown_flags": n_cells, "grid": 4 * ((n_cells + 31) // 32), "mask": 4 * words, "jump_tables": 64 * n_cells}}
    fl = Fleet(B, p, max_states=1024)
    try:
        fl.set_map(cloud, cells, res, center, zmax, infl)
        fl.set_unknown_views(view_of=np.arange(B, dtype=np.int32) % teams, n_views=teams, origin=origin, res=res, dims=dims)
        fl.set_point_views()
        if LISTED_VIEWS:
            fl.enable_listed_views()
            out["listed_views"] = True
        fl.init(states, goals)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record(fl.stream)
        fl.sense(r_sense)
        e[1].record(fl.stream)
        fl.observe()
        e[2].record(fl.stream)
        fl.replan()
        fl.next_goals(5)
        fl.sync()
        out["sense_first_ms"], out["observe_first_ms"] = e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])
        med = timed_cycles(fl, cycles, r_sense, observe=True)
        v = fl.vehicles()
        known = fl.point_masks()
        out.update({"stages_ms": med, "cycle_fenced_ms": float(sum(med.values())),
                    "committed_last": int((v["stage"] == abi.FH_FLEET_STAGE_COMMITTED).sum()),
                    "points_known_fraction_end": float(np.unpackbits(known.view(np.uint8)).sum() / (teams * len(cloud))),
                    "unknown_fraction_end": float(fl.view_flags.float().mean().item())})
        if AUDIT:
            out["audit"] = timed_audit(fl, cycles)
    finally:
        fl.close()
    return {"occupancy": out}


def traffic_cycles(B, cycles, p, world, samples, stride, reach, window=None):
    """The cycle before and after Fleet.enable_traffic (window: timed, with that window): see the module docstring."""
    cloud, cells, res, center, zmax, infl, states, goals, flags, origin, dims = world
    n_cells = dims[0] * dims[1] * dims[2]
    out = {"samples": samples, "stride": stride, "range": reach, "rule": "all", "hull": float(p["rule"]["drone_radius"]),
           "static_points": int(len(cloud))}
    fl = Fleet(B, p, max_states=1024)
    try:
        fl.set_map(cloud, cells, res, center, zmax, infl)
        fl.set_unknown_views(torch.from_numpy(flags.reshape(1, -1)).to(fl.dev).repeat(B, 1), origin=origin, res=res, dims=dims)
        fl.set_point_views(torch.full((B, abi.point_mask_words(len(cloud))), -1, dtype=torch.int32, device=fl.dev))
        fl.init(states, goals)
        fl.replan()
        fl.next_goals(5)
        fl.sync()
        med = timed_cycles(fl, cycles)
        out["before"] = {"stages_ms": med, "cycle_fenced_ms": float(sum(med.values())), "separation": timed_separation(fl, cycles)}
        fl.enable_traffic(samples, stride, reach, timed=window is not None, window=window or 0)
        if window is not None:
            out.update({"window": int(window), "first_instant": int(fl.traffic_par["first_instant"])})
        if LISTED_VIEWS:
            fl.enable_listed_views()
            out["listed_views"] = True
        out.update({"traffic_points": fl.n_cloud_all - int(fl.traffic_par["first_point"]), "cloud_points": fl.n_cloud_all,
                    "mask_bytes": int(fl.point_mask.numel()) * 4, "unknown_views_bytes": B * n_cells})
        fl.traffic()
        fl.replan()
        fl.next_goals(5)
        fl.sync()
        med = timed_cycles(fl, cycles, traffic=True)
        bits = fl.point_mask[:, int(fl.traffic_par["first_point"]) // 32:]
        shown = sum(int(((bits >> b) & 1).sum().item()) for b in range(32))
        v = fl.vehicles()
        out["after"] = {"stages_ms": med, "cycle_fenced_ms": float(sum(med.values())), "separation": timed_separation(fl, cycles),
                        "traffic_bits_set_per_vehicle": shown / B, "committed_last": int((v["stage"] == abi.FH_FLEET_STAGE_COMMITTED).sum())}
    finally:
        fl.close()
    return {"traffic" if window is None else "traffic_timed": out}


def obstacle_cycles(B, cycles, p, world, m, samples, rng, track=None, track_los=False):
    """--obstacles M: the fleet of --traffic-timed after two cycles, then time-aware traffic (samples, stride 5, 6 m, window 2) timed as a
    stage of its own, then Fleet.enable_obstacles with M obstacles scattered over the map that fly up to 1 m/s (the same samples,
    stride, range and window, seven points, no detection radius) and Fleet.obstacles and Fleet.obstacle_audit_device timed one by one,
    each fenced by events, max(cycles, 5) times: the medians and the spread in ms, and what each found."""
    cloud, cells, res, center, zmax, infl, states, goals, flags, origin, dims = world
    out = {"obstacles": m, "samples": samples, "stride": 5, "range": 6.0, "window": 2, "points": 7}
    fl = Fleet(B, p, max_states=1024)
    try:
        fl.set_map(cloud, cells, res, center, zmax, infl)
        fl.set_unknown_views(torch.from_numpy(flags.reshape(1, -1)).to(fl.dev).repeat(B, 1), origin=origin, res=res, dims=dims)
        fl.set_point_views(torch.full((B, abi.point_mask_words(len(cloud))), -1, dtype=torch.int32, device=fl.dev))
        fl.init(states, goals)
        for _ in range(2):
            fl.replan()
            fl.next_goals(5)
        fl.enable_traffic(samples, 5, 6.0, timed=True, window=2)
        lo, hi = cloud.min(axis=0), cloud.max(axis=0)
        obs = abi.make_obstacles(rng.uniform(lo, hi, size=(m, 3)), rng.uniform(-1.0, 1.0, size=(m, 3)) / np.sqrt(3.0), 0.3)
        fl.enable_obstacles(obs, samples, 5, 6.0, window=2)
        out.update({"cloud_points": fl.n_cloud_all, "mask_bytes": int(fl.point_mask.numel()) * 4})
        stages = [("traffic_timed", fl.traffic), ("obstacles", fl.obstacles), ("obstacle_audit", fl.obstacle_audit_device)]
        if track is not None:   # --track: the obstacles as the truth; the records obstacles() reads are the tracker's from here on
            fl.enable_tracking(obs, track, los=track_los)
            out.update({"track_r_detect": track, "track_los": track_los})

            def track_next():   # (one tick later each time: a sighting at the tick of the last one would be stale and not appended)
                fl.track_tick += 1
                fl.truth_tick += 1
                fl.track()
            stages.insert(1, ("track", track_next))
        ms = {n: [] for n, _ in stages}
        for name, launch in stages:
            launch()   # (warm-up: the working buffers of the context grow)
        fl.sync()
        for _ in range(max(cycles, 5)):
            for name, launch in stages:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(fl.stream)
                launch()
                e1.record(fl.stream)
                fl.sync()
                ms[name].append(e0.elapsed_time(e1))
        for name, v in ms.items():
            out[name + "_ms"] = float(np.median(v))
            out[name + "_ms_min_max"] = [float(min(v)), float(max(v))]
        bits = fl.point_mask[:, int(fl.obstacle_par["first_point"]) // 32:]
        rec = fl.obstacle_audit()
        if track is not None:
            info = fl.track_records()[3]
            out.update({"track_seen": int(info[0]), "track_records_on": int(info[1])})
        out.update({"obstacle_bits_set_per_vehicle": sum(int(((bits >> b) & 1).sum().item()) for b in range(32)) / B,
                    "audit_hit": int(((rec["flags"] & abi.FH_OBSTACLE_HIT) != 0).sum()), "audit_n_tested_mean": float(rec["n_tested"].mean())})
    finally:
        fl.close()
    return {"obstacles": out}


def rounds_cycles(B, cycles, p, world, rounds, reach, retries, traffic, window, check):
    """The cycle before and after Fleet.enable_rounds: see the module docstring."""
    cloud, cells, res, center, zmax, infl, states, goals, flags, origin, dims = world
    out = {"rounds": rounds, "retries": retries, "check": bool(check)}
    fl = Fleet(B, p, max_states=1024)
    try:
        fl.set_map(cloud, cells, res, center, zmax, infl)
        with_traffic = traffic is not None or window is not None
        if with_traffic:
            samples, stride, rng = traffic or (8, 25, 6.0)
            fl.set_unknown_views(torch.from_numpy(flags.reshape(1, -1)).to(fl.dev).repeat(B, 1), origin=origin, res=res, dims=dims)
            fl.set_point_views(torch.full((B, abi.point_mask_words(len(cloud))), -1, dtype=torch.int32, device=fl.dev))
            fl.init(states, goals)
            fl.enable_traffic(samples, stride, rng, timed=window is not None, window=window or 0)
            out["traffic"] = {"samples": samples, "stride": stride, "range": rng, "window": window}
        else:
            fl.set_unknown(flags, origin, res, dims)
            fl.init(states, goals)
        if check:
            fl.enable_check()
        listed = LISTED_VIEWS and fl.point_mask is not None
        if listed:
            fl.enable_listed_views()
        out["listed_views"] = bool(listed)
        for _ in range(2):
            if with_traffic:
                fl.traffic()
            fl.replan()
            fl.next_goals(5)
        fl.sync()
        med = timed_cycles(fl, cycles, traffic=with_traffic)
        out["without_rounds"] = {"stages_ms": med, "cycle_fenced_ms": float(sum(med.values()))}
        fl.enable_rounds(rounds, reach=reach, retries=retries)
        out["reach"], out["passes"] = float(fl.round_par["reach"]), int(fl.round_par["passes"])
        out["cells"], out["cell_res"] = list(fl.round_cells[2]), fl.round_cells[1]
        fl.replan()
        fl.next_goals(5)
        fl.sync()
        names = [n for n, _ in fl.stages()] + ["next_goals"]
        per = {n: [] for n in names}
        per_class, flagged, withheld, views_listed = [], [], [], []
        for _ in range(cycles):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)]
            ev[0].record(fl.stream)
            for j, (n, launch) in enumerate(fl.stages()):
                launch()
                ev[j + 1].record(fl.stream)
            fl.next_goals(5)
            ev[-1].record(fl.stream)
            fl.sync()
            for j, n in enumerate(names):
                per[n].append(ev[j].elapsed_time(ev[j + 1]))
            rec = fl.round_records()
            per_class.append(np.bincount(rec["round_class"], minlength=rounds).tolist())
            flagged.append({"overflow": int(((rec["flags"] & abi.FH_ROUND_OVERFLOW) != 0).sum()),
                            "unsettled": int(((rec["flags"] & abi.FH_ROUND_UNSETTLED) != 0).sum()), "n_lower_max": int(rec["n_lower"].max())})
            if check:
                withheld.append([int(((r["flags"] & abi.FH_CHECK_CONFLICT) != 0).sum()) for r in fl.check_records_by_round()])
            if listed:
                views_listed.append(fl.view_lists()[1].tolist())
        med = {n: float(np.median(v)) for n, v in per.items()}
        by_stage = {}
        for n, v in med.items():
            by_stage[n.split("@")[0]] = by_stage.get(n.split("@")[0], 0.0) + v
        gates = [v for n, v in med.items() if n.startswith("gate")]
        out["with_rounds"] = {"stages_ms": med, "by_stage_ms": by_stage, "cycle_fenced_ms": float(sum(med.values())),
                              "round_classes_ms": med.get("round_classes"), "gate_mean_ms": float(np.mean(gates)), "gates": len(gates),
                              "vehicles_per_class": per_class, "flagged": flagged, "withheld_per_round": withheld,
                              "views_listed_per_round": views_listed,
                              "committed_last": int((fl.vehicles()["stage"] == abi.FH_FLEET_STAGE_COMMITTED).sum())}
    finally:
        fl.close()
    return {"rounds": out}


def main():
    argv = sys.argv[1:]
    r_sense, fov, teams, traffic, window = 3.0, None, 0, None, None
    rounds, round_reach, retries = 0, None, 0
    for opt in ("--rounds", "--round-reach", "--retries"):
        if opt in argv:
            k = argv.index(opt)
            if opt == "--rounds":
                rounds = int(argv[k + 1])
            elif opt == "--retries":
                retries = int(argv[k + 1])
            else:
                round_reach = float(argv[k + 1])
            del argv[k:k + 2]
    if "--link" in argv:         # (read into LINK above)
        k = argv.index("--link")
        del argv[k:k + 2]
    if "--link-los" in argv:     # (read into LINK_LOS above)
        argv.remove("--link-los")
    if "--explore" in argv:      # (read into EXPLORE above)
        k = argv.index("--explore")
        del argv[k:k + 2]
    if "--far" in argv:          # (read into FAR above)
        k = argv.index("--far")
        del argv[k:k + 2]
    for opt in ("--far-spread", "--passes", "--far-gain", "--far-hop-cost", "--far-min-gain", "--far-claim-blocks"):   # (read into FAR_SPREAD .. FAR_MIN_GAIN above)
        if opt in argv:
            k = argv.index(opt)
            del argv[k:k + 2]
    if "--reach" in argv:        # (read into REACH above)
        argv.remove("--reach")
    if "--spread" in argv:       # (read into SPREAD above)
        k = argv.index("--spread")
        del argv[k:k + 2]
    for opt in ("--gain", "--hop-cost", "--min-gain", "--claim-radius"):   # (read into GAIN, HOP_COST, MIN_GAIN, CLAIM_RADIUS above)
        if opt in argv:
            k = argv.index(opt)
            del argv[k:k + 2]
    track, track_los = None, "--track-los" in argv
    if track_los:
        argv.remove("--track-los")
    if "--track" in argv:
        k = argv.index("--track")
        track = float(argv[k + 1])
        del argv[k:k + 2]
    n_obstacles, obstacle_samples = 0, 64
    for opt in ("--obstacles", "--obstacle-samples"):
        if opt in argv:
            k = argv.index(opt)
            if opt == "--obstacles":
                n_obstacles = int(argv[k + 1])
            else:
                obstacle_samples = int(argv[k + 1])
            del argv[k:k + 2]
    if "--traffic-timed" in argv:
        k = argv.index("--traffic-timed")
        window = int(argv[k + 1])
        del argv[k:k + 2]
    if "--traffic" in argv:
        k = argv.index("--traffic")
        has = k + 3 < len(argv) and argv[k + 1].isdigit() and argv[k + 2].isdigit()
        traffic = (int(argv[k + 1]), int(argv[k + 2]), float(argv[k + 3])) if has else (8, 25, 6.0)
        del argv[k:k + (4 if has else 1)]
    if "--occupancy" in argv:
        k = argv.index("--occupancy")
        has = k + 1 < len(argv) and argv[k + 1].isdigit()
        teams = int(argv[k + 1]) if has else 64
        del argv[k:k + (2 if has else 1)]
    if "--r-sense" in argv:      # (an option's values leave by position, not by text: `1 3 --fov 1 0.5` keeps its first two)
        k = argv.index("--r-sense")
        r_sense = float(argv[k + 1])
        del argv[k:k + 2]
    if "--fov" in argv:
        k = argv.index("--fov")
        fov = (float(argv[k + 1]), float(argv[k + 2]))
        del argv[k:k + 3]
    args = [a for a in argv if not a.startswith("--")]
    B = int(args[0]) if len(args) > 0 else 65536
    cycles = int(args[1]) if len(args) > 1 else 3
    res, infl, zmax = 0.2, 0.3, 3.0
    cloud, cells, center, starts, goals, rng = frontend.forest_queries(B, 7, return_rng=True)
    if WALLS:   # rooms: planes of points every 5 m in x and in y, floor to ceiling, a door of 1.2 m in every stretch of 5 m
        lo, hi = cloud[:, :2].min(axis=0), cloud[:, :2].max(axis=0)
        along = [np.arange(lo[k], hi[k], 0.1) for k in range(2)]
        walls = []
        for k in range(2):
            run = along[1 - k][np.mod(along[1 - k] - lo[1 - k], 5.0) >= 1.2]
            for at in np.arange(lo[k] + 5.0, hi[k] - 1.0, 5.0):
                a, z = np.meshgrid(run, np.arange(0.05, 3.0, 0.1), indexing="ij")
                pts = np.zeros((a.size, 3))
                pts[:, k], pts[:, 1 - k], pts[:, 2] = at, a.ravel(), z.ravel()
                walls.append(pts)
        cloud = np.concatenate([cloud] + walls).astype(cloud.dtype)
    u = goals - starts
    u /= np.maximum(np.linalg.norm(u, axis=1, keepdims=True), 1e-9)
    states = np.zeros(B, dtype=abi.state_dtype)
    states["pos"], states["vel"] = starts, u * rng.uniform(0, 1.5, size=(B, 1))
    probe = capi.Map(0)
    probe.read(cloud, cells, res, center, 0.0, zmax, infl)
    dims, origin = probe.dims()
    probe.close()
    dims = [int(d) for d in dims]
    iz, iy, ix = np.meshgrid(np.arange(dims[2]), np.arange(dims[1]), np.arange(dims[0]), indexing="ij")
    centres = np.stack([(ix + 0.5) * res + origin[0], (iy + 0.5) * res + origin[1], (iz + 0.5) * res + origin[2]], axis=-1)
    seen = np.zeros(iz.shape, dtype=bool)
    for c, r in zip(rng.uniform([1, 1, 1.5], [19, 19, 1.5], size=(24, 3)), rng.uniform(2.0, 3.5, 24)):
        seen |= np.linalg.norm(centres - c, axis=-1) < r
    flags = (~seen).astype(np.uint8)
    p = abi.default_fleet_params()
    p["wdx"], p["wdy"], p["wdz"] = 8.0, 8.0, 4.0
    p["rule"]["drone_radius"] = 0.3
    fl = Fleet(B, p, max_states=1024)
    out = {"vehicles": B, "unknown_fraction": float(flags.mean())}
    try:
        fl.set_map(cloud, cells, res, center, zmax, infl)
        fl.set_unknown(flags, origin, res, dims)
        fl.init(states, goals)
        fl.replan()
        fl.next_goals(5)
        fl.sync()
        names = [n for n, _ in fl.stages()] + ["next_goals"]
        per = {n: [] for n in names}
        commit_bytes, committed, kend = [], [], []
        for _ in range(cycles):
            before = fl.vehicles()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)]
            ev[0].record(fl.stream)
            for j, (n, launch) in enumerate(fl.stages()):
                launch()
                ev[j + 1].record(fl.stream)
            fl.next_goals(5)
            ev[-1].record(fl.stream)
            fl.sync()
            after = fl.vehicles()
            for j, n in enumerate(names):
                per[n].append(ev[j].elapsed_time(ev[j + 1]))
            ok = after["stage"] == abi.FH_FLEET_STAGE_COMMITTED
            committed.append(int(ok.sum()))
            kend.append(int((ok & (after["k_end_whole"] > 0)).sum()))
            # what the commit kernel writes: the committed states (the moved prefix and the new samples) and the vehicle records
            moved = np.where(before["plan_head"] != 0, before["plan_size"] - after["k_end_whole"] - 1, 0)
            new = after["k_safe"] + 1 + after["n_safe"]
            commit_bytes.append(int(abi.state_dtype.itemsize * (new[ok].sum() + moved[ok].sum()) + abi.vehicle_dtype.itemsize * B))
        # the whole cycle without fences between the stages
        t = []
        for _ in range(cycles):
            fl.sync()
            t0 = time.perf_counter()
            fl.replan()
            fl.next_goals(5)
            fl.sync()
            t.append(1e3 * (time.perf_counter() - t0))
        med = {n: float(np.median(v)) for n, v in per.items()}
        fleet_ms = med["begin"] + med["commit"] + med["next_goals"]
        # device-to-device copy of 2 GiB: read + write bytes per second
        a = torch.empty(2 << 30, dtype=torch.uint8, device="cuda:0")
        b = torch.empty_like(a)
        b.copy_(a)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        copy_gbs = 5 * 2 * a.numel() / (e0.elapsed_time(e1) * 1e-3) / 1e9
        cb = float(np.median(commit_bytes))
        out.update({"stages_ms": med, "cycle_fenced_ms": float(sum(med.values())), "cycle_ms": float(np.median(t)),
                    "fleet_kernels_ms": fleet_ms, "fleet_kernels_share": fleet_ms / float(sum(med.values())),
                    "committed": committed, "committed_with_k_end_whole": kend, "commit_bytes": cb,
                    "commit_write_gbs": cb / (med["commit"] * 1e-3) / 1e9, "hbm_copy_gbs": copy_gbs})
        if AUDIT:
            out["audit"] = timed_audit(fl, cycles)
        if SEPARATION:
            out["separation"] = timed_separation(fl, cycles)
        if "--check" in sys.argv:
            out["check"] = check_cycles(fl, cycles)
    finally:
        fl.close()
    if "--views" in sys.argv or fov is not None:
        world = (cloud, cells, res, center, zmax, infl, states, goals, flags, origin, dims)
        out.update(views_cycles(B, cycles, p, world, r_sense, "--no-staging" not in sys.argv, fov))
    if teams:
        world = (cloud, cells, res, center, zmax, infl, states, goals, flags, origin, dims)
        out.update(occupancy_cycles(B, cycles, p, world, r_sense, min(teams, B)))
    if traffic:
        world = (cloud, cells, res, center, zmax, infl, states, goals, flags, origin, dims)
        out.update(traffic_cycles(B, cycles, p, world, *traffic))
    if window is not None:
        world = (cloud, cells, res, center, zmax, infl, states, goals, flags, origin, dims)
        out.update(traffic_cycles(B, cycles, p, world, *(traffic or (8, 25, 6.0)), window=window))
    if n_obstacles:
        world = (cloud, cells, res, center, zmax, infl, states, goals, flags, origin, dims)
        out.update(obstacle_cycles(B, cycles, p, world, n_obstacles, obstacle_samples, rng, track, track_los))
    if rounds:
        world = (cloud, cells, res, center, zmax, infl, states, goals, flags, origin, dims)
        out.update(rounds_cycles(B, cycles, p, world, rounds, round_reach, retries, traffic, window, "--check" in sys.argv))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
