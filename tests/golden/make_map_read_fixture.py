"""Records what the reference's compiled readMap (oracle/_ref/libref_frontend.so through oracle.ref_frontend.ref.Map) answers for the
cases of tests/map_read_edge_cases.py that lie inside its defined range, the clouds rounded to float32 as a pcl::PointXYZ holds them:
the flat ids of the occupied cells as runs [first id, count], each distinct answer once ("answers") and its number per case ("case"),
and the reference's own origin per lattice, into tests/golden/map_read_ref.json.  Outputs of the reference only; the model is not asked.  tests/test_map_read_edge_cases.py compares the model with this file where no compiled reference is present.

Run where the reference library is built:  python tests/golden/make_map_read_fixture.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]


def runs_of(ids):
    """sorted ids -> [[first, count], ...]"""
    out = []
    for i in ids:
        if out and out[-1][0] + out[-1][1] == i:
            out[-1][1] += 1
        else:
            out.append([i, 1])
    return out


def main():
    import map_read_edge_cases as mc
    from oracle.ref_frontend import ref

    if ref.build() is None:
        raise SystemExit("the reference library is not built")
    out = {"source": "MapUtil::readMap (jps3d, jps_collision/map_util.h:30-185), clouds as float32", "origin": {}, "answers": [], "case": {}}
    for c in mc.cases():
        if not mc.in_reference_range(c, c.cloud32):
            continue
        m = ref.Map(*c.args(c.cloud32))
        assert tuple(m.dims) == c.lat.dims, (c.name, m.dims)
        out["origin"][c.lat.name] = [float(o).hex() for o in m.origin]      # (the reference's own origin, bit for bit)
        runs = runs_of(np.flatnonzero(m.occupancy().reshape(-1)).tolist())
        if runs not in out["answers"]:
            out["answers"].append(runs)
        out["case"][c.name] = out["answers"].index(runs)
        m.close()
    with open(os.path.join(HERE, "map_read_ref.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print(len(out["case"]), "cases,", len(out["answers"]), "distinct answers,", sum(len(v) for v in out["answers"]), "runs")


if __name__ == "__main__":
    main()
