"""What a line of sight changes for the radio link ("What it changes"; the `what_it_changes` block of
profiles/link_los_fleet_cycle.json).  Two scenes, each once with Fleet.link(RANGE) and once with Fleet.link(RANGE, los=True), all in one
process.  Needs a GPU.
  open:  the eight-vehicle open scene of tests/test_gpu_frontier.py (K18's and K22's: four thin pillars, no wall), a view per vehicle, the
         teams made by link(6.0) every period instead of by a fixed view_of: periods of sense -> observe -> link -> explore_team(3, 2, 12)
         -> replan -> next_goals(60 ticks).  Per period the groups, the linked and the blocked pairs; after 24 periods the known voxels
         of every vehicle's view.
  rooms: the two rooms of tests/test_gpu_link_los.py (tests/link_los_cases.py: a wall across a map of 4 m x 4 m, a door one cell wide),
         eight vehicles that stand still, four a room, a view each that starts all unknown, link(8.0): one period of sense(1.0) -> link,
         with the wall plugged, with the door open, and with a ninth vehicle in the doorway.
    usage: python scripts/link_los_benefit.py [OUT.json]"""
import json
import os
import sys

import numpy as np
import torch  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]   # (the scenes and the fleet's parameters are the tests')
from faster_amd.fleet import Fleet  # noqa: E402
import link_los_cases as lc  # noqa: E402
import test_gpu_frontier as tf  # noqa: E402
from test_gpu_fleet import P, fleet_params  # noqa: E402
from test_gpu_link_los import DOORWAY, LEFT, RIGHT  # noqa: E402

PERIODS, RANGE_OPEN, RANGE_ROOMS = 24, 6.0, 8.0


def new_fleet(n):
    return Fleet(n, fleet_params(), n_seg=P["N"], max_poly=P["max_poly"], dc=P["dc"], v_max=P["v_max"], a_max=P["a_max"], j_max=P["j_max"],
                 decomp_radius=P["decomp_radius"], dist_max_vertexes=P["dist_max_vertexes"])


def open_run(sc, los):
    X = new_fleet(8)
    out = {"scene": "open", "los": los, "groups": [], "linked_pairs": [], "blocked_pairs": [], "unsettled_periods": 0}
    try:
        X.set_map(sc["cloud"], tf.SCENE_CELLS, P["res"], tf.SCENE_CENTER, P["z_max"], 0.1)
        X.init(sc["starts"], sc["goals"])
        X.set_unknown_views(sc["views"].copy(), origin=sc["origin"], res=P["res"], dims=sc["dims"])
        X.set_point_views()
        X.enable_heading()
        for c in range(PERIODS):
            X.sense(tf.R_SENSE)
            X.observe()
            X.link(RANGE_OPEN, los=los)
            _, info = X.link_records()
            out["groups"].append(int(info[1]))
            out["linked_pairs"].append(int(info[2]))
            out["blocked_pairs"].append(int(info[3]))
            out["unsettled_periods"] += int(info[0] != 0)
            X.explore_team(3.0, 2.0, 12, z=tf.Z_EXPLORE)
            X.replan()
            X.next_goals(tf.LOOP_TICKS, follow=True)
        out["known_per_vehicle"] = [int(k) for k in X.coverage()["known"]]
        print(json.dumps(out), flush=True)
    finally:
        X.close()
    return out


def rooms_run(name, cloud, positions, los):
    n = len(positions)
    X = new_fleet(n)
    try:
        X.set_map(cloud, lc.READ["cells"], lc.RES, lc.READ["center"], lc.READ["z_max"], lc.READ["inflation"])
        X.init(np.array(positions), np.array(positions))
        X.set_unknown_views(np.ones((n, int(np.prod(lc.DIMS))), dtype=np.uint8), origin=lc.ORIGIN, res=lc.RES, dims=list(lc.DIMS))
        X.sense(1.0)
        before = [int(k) for k in X.coverage()["known"]]
        X.link(RANGE_ROOMS, los=los)
        labels, info = X.link_records()
        out = {"scene": "rooms, " + name, "los": los, "groups": int(info[1]), "linked_pairs": int(info[2]), "blocked_pairs": int(info[3]),
               "labels": labels.tolist(), "known_per_vehicle_sensed": before, "known_per_vehicle": [int(k) for k in X.coverage()["known"]]}
        print(json.dumps(out), flush=True)
    finally:
        X.close()
    return out


if __name__ == "__main__":
    scene = tf.open_scene()
    runs = [open_run(scene, False), open_run(scene, True)]
    plugged = np.concatenate([lc.cloud(), np.array([lc.centre(10, iy, iz) for iy in (13, 14, 15) for iz in range(10)])])
    for name, cloud, positions in (("the wall plugged", plugged, LEFT + RIGHT), ("the door open", lc.cloud(), LEFT + RIGHT),
                                   ("the door open, a ninth vehicle in the doorway", lc.cloud(), LEFT + RIGHT + [DOORWAY])):
        runs += [rooms_run(name, cloud, positions, False), rooms_run(name, cloud, positions, True)]
    result = {"open": "eight vehicles, a view each, link(%g) every period, explore_team(3, 2, 12), 60 ticks a period, sensor 2.5 m, %d periods"
                      % (RANGE_OPEN, PERIODS),
              "rooms": "eight (nine) vehicles that stand still in two rooms of 2 m x 4 m, a view each, sense(1.0) then link(%g), one period" % RANGE_ROOMS,
              "runs": runs}
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(result, f, indent=1)
