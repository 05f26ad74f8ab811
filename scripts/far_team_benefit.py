"""What the far choosers for a fleet buy ("What it buys"; the `what_it_buys` block of
profiles/far_team_fleet_cycle.json): the eight-vehicle open scene of tests/test_gpu_frontier.py, two teams of four that share a view each,
periods of sense -> observe -> explore_gain(3, 12) -> a far chooser with after="gain" -> replan -> next_goals(60 ticks).  One run each of
explore_far_spread(8, 2.0), explore_far_gain(8, 2) and explore_far_team(8, 2.0, 2) with claim_blocks 2 (the default), 1 and 3, all in
one process; per run the known voxels per team after 12, 24, 36 and 48 periods, the goals given by either chooser, the pairs of
teammates given one block in one period, and the sums of hops, gains, covered and removed.  Needs a GPU.
    usage: python scripts/far_team_benefit.py [OUT.json]"""
import json
import os
import sys

import numpy as np
import torch  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]   # (the scene and the fleet's parameters are the tests')
from faster_amd import abi  # noqa: E402
from faster_amd.fleet import Fleet  # noqa: E402
import test_gpu_frontier as tf  # noqa: E402
from test_gpu_fleet import P, fleet_params  # noqa: E402

PERIODS, MARKS = 48, (12, 24, 36, 48)
team = np.array([0, 0, 0, 0, 1, 1, 1, 1], dtype=np.int32)


def run(sc, views, chooser, **kw):
    X = Fleet(8, fleet_params(), n_seg=P["N"], max_poly=P["max_poly"], dc=P["dc"], v_max=P["v_max"], a_max=P["a_max"], j_max=P["j_max"],
              decomp_radius=P["decomp_radius"], dist_max_vertexes=P["dist_max_vertexes"])
    out = {"chooser": chooser, **{k: v for k, v in kw.items()}, "known": {}, "goals_gain": 0, "goals_far": 0, "no_path": 0, "same_block_pairs": 0,
           "unsettled": 0, "all_claimed": 0, "all_poor": 0, "covered_sum": 0, "removed_sum": 0, "far_gain_sum": 0, "far_hops_sum": 0}
    try:
        X.set_map(sc["cloud"], tf.SCENE_CELLS, P["res"], tf.SCENE_CENTER, P["z_max"], 0.1)
        X.init(sc["starts"], sc["goals"])
        X.set_unknown_views(views.copy(), view_of=team, n_views=2, origin=sc["origin"], res=P["res"], dims=sc["dims"])
        X.set_point_views()
        X.enable_heading()
        for c in range(PERIODS):
            X.sense(tf.R_SENSE)
            X.observe()
            X.explore_gain(3.0, 12, z=tf.Z_EXPLORE)
            out["goals_gain"] += int(X.gain_records()[2].sum())
            if chooser == "far_spread":
                X.explore_far_spread(8, 2.0, z=tf.Z_EXPLORE, after="gain")
                rec, _, mask = X.far_spread_records()
            elif chooser == "far_gain":
                X.explore_far_gain(8, 2, z=tf.Z_EXPLORE, after="gain")
                rec, _, mask = X.far_gain_records()
            else:
                X.explore_far_team(8, 2.0, 2, z=tf.Z_EXPLORE, after="gain", **kw)
                rec, _, mask = X.far_team_records()
            out["goals_far"] += int(mask.sum())
            given = np.nonzero(mask)[0]
            out["far_hops_sum"] += int(rec["hops"][given].sum())
            for a in given:
                for b in given:
                    if a < b and team[a] == team[b] and rec["block_cell"][a] == rec["block_cell"][b]:
                        out["same_block_pairs"] += 1
            if "gain" in rec.dtype.names:
                out["far_gain_sum"] += int(rec["gain"][given].sum())
                out["all_poor"] += int((rec["flags"] & abi.FH_PROSPECT_ALL_POOR != 0).sum())
            if "claimed" in rec.dtype.names:
                out["unsettled"] += int((rec["flags"] & abi.FH_APART_UNSETTLED != 0).sum())
                out["all_claimed"] += int((rec["flags"] & abi.FH_APART_CLAIMED != 0).sum())
            if "covered" in rec.dtype.names:
                out["covered_sum"] += int(rec["covered"].sum())
                out["removed_sum"] += int(rec["removed"].sum())
            X.replan()
            out["no_path"] += int((X.vehicles()["stage"] == abi.FH_FLEET_STAGE_NO_PATH).sum())
            X.next_goals(tf.LOOP_TICKS, follow=True)
            if c + 1 in MARKS:
                out["known"][str(c + 1)] = [int(k) for k in X.coverage()["known"]]
        print(json.dumps(out), flush=True)
    finally:
        X.close()
    return out


if __name__ == "__main__":
    scene = tf.open_scene()
    shared = np.stack([scene["views"][team == v].min(axis=0) for v in (0, 1)])   # a team knows what one of its four knows
    runs = [run(scene, shared, "far_spread"), run(scene, shared, "far_gain"), run(scene, shared, "far_team"),
            run(scene, shared, "far_team", claim_blocks=1), run(scene, shared, "far_team", claim_blocks=3)]
    result = {"scene": "eight vehicles, two teams of four that share a view each, 60 ticks a period, sensor 2.5 m, explore_gain(3, 12) then the "
                       "far chooser after it, block 8, r_spread 2.0, gain_blocks 2, 48 periods", "runs": runs}
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(result, f, indent=1)
