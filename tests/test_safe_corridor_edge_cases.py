"""The inputs of tests/test_gpu_safe_corridor_edges.py proved on the CPU with the restatements alone (oracle/pair_glue.safe_path with its trace,
the restated lattice_range and nearest_unknown of tests/safe_corridor_edge_cases.py, frontend.decompose): every case is the edge it claims
to be, and a kernel that is wrong in one of the ways below would change the expected output of a named case by more than the
comparison's tolerance."""
import numpy as np
import pytest

import safe_corridor_edge_cases as sce
from faster_amd import frontend
from oracle import pair_glue

ATOL = 1e-9   # the tolerance of the safe-path comparison on the device


@pytest.fixture(scope="module", autouse=True)
def built():
    from faster_amd import build as fb

    fb.build_frontend()


@pytest.fixture(scope="module")
def march():
    return sce.march_group(sce.MAX_POLY)


@pytest.fixture(scope="module")
def boundary():
    return sce.boundary_group()


def host_rows(g, p, path, cloud=None):
    cloud = sce.decomposition_cloud(g, p)[0] if cloud is None else cloud
    return [np.column_stack([A, b]) for A, b in frontend.decompose(path, cloud, drone_radius=g["decomp_radius"], z_ground=g["z_ground"], bbox=g["bbox"])[0]]


def test_constants_are_read_from_the_headers():
    assert sce.SAFE_PATH_CAP >= 8 and sce.MAX_POLY + 1 < sce.SAFE_PATH_CAP
    assert sce.CAP < sce.CAP_IDS < sce.CAP_GLOBAL and sce.MAX_FACES_POLY >= 16


# ---- the march ------------------------------------------------------------------------------------------------------------------------------
def test_vertex_counts(march):
    for n in (2, sce.SAFE_PATH_CAP - 1, sce.SAFE_PATH_CAP):
        p = sce.pair_named(march, "n_points=%d" % n)
        e = sce.expected(march, p)
        assert p["n_points"] == n == len(p["path"]) and e["live"] and 2 <= len(e["path"]) <= march["max_poly_safe"] + 1
    for n in (0, 1, -1, -2):
        assert not sce.expected(march, sce.pair_named(march, "n_points=%d" % n))["live"]
    assert march["max_points"] == sce.SAFE_PATH_CAP


def test_long_march(march):
    """at least five iterations, one of them erases two or more vertices, the cut lands beyond vertex 20; max_poly_safe 1, 3 and
    FH_MAX_POLY truncate it; with the near slab the cut path is shorter than FH_MAX_POLY + 1"""
    p = sce.pair_named(march, "n_points=%d" % sce.SAFE_PATH_CAP)
    full, tr = sce.full_march(march, p)
    erased = [last + 1 for _, last, _ in tr if last is not None]
    print("iterations %d, erased per iteration %s, %d vertices after the cut" % (len(tr), erased, len(full)))
    assert len(tr) >= 5 and max(erased) >= 2 and tr[-1][1] is None and tr[-1][0] < march["rule"]["drone_radius"]
    cut_after = sce.SAFE_PATH_CAP - tr[-1][2]   # vertices of JPS_in in front of the cut: eliminated - 1
    assert cut_after > 20 and len(full) > 21
    for mps in (1, 3, sce.MAX_POLY):
        g = sce.march_group(mps)
        e = sce.expected(g, sce.pair_named(g, p["name"]))
        assert len(e["path"]) == mps + 1 < len(full) and np.array_equal(e["path"][1:], full[1:mps + 1])
    near, _ = sce.full_march(march, sce.pair_named(march, "near slab"))
    assert 2 < len(near) < sce.MAX_POLY + 1


def test_back_off_walks_back_over_several_legs(march):
    p = sce.pair_named(march, "back-off")
    full, tr = sce.full_march(march, p)
    assert tr[-1][1] is None and len(tr) >= 2
    eliminated = len(p["path"]) - tr[-1][2] + 1        # the cut path before the back-off: eliminated vertices of JPS_in and the cut point
    legs_back = eliminated + 1 - len(full)
    print("back-off: %d vertices -> %d before the back-off -> %d, %d legs walked back" % (len(p["path"]), eliminated + 1, len(full), legs_back))
    assert legs_back >= 3 and len(full) <= sce.MAX_POLY + 1   # (the device's output holds the whole of it)
    # the new end lies on a leg of JPS_in, drone_radius (along the path) before the cut point
    assert np.array_equal(full[1:-1], p["path"][1:len(full) - 1]) and abs(full[-1][1]) < 1e-12 and full[-2][0] < full[-1][0] < full[-2][0] + 0.05


def test_boundary_of_the_cut(boundary):
    g, dr = boundary, boundary["rule"]["drone_radius"]
    e = sce.expected(g, sce.pair_named(g, "stub"))
    assert len(e["trace"]) == 1 and 0 < e["trace"][0][0] < dr and len(e["path"]) == 2
    p = sce.pair_named(g, "stub")
    assert np.array_equal(e["path"][1], p["path"][0] + [0.01, 0, 0])
    e = sce.expected(g, sce.pair_named(g, "exactly drone_radius"))
    assert e["trace"][0][0] == dr and e["trace"][0][1] is not None and len(e["trace"]) > 1 and len(e["path"]) > 2
    e = sce.expected(g, sce.pair_named(g, "on the first vertex"))
    assert e["trace"] == [(0.0, None, 4)] and len(e["path"]) == 2
    e = sce.expected(g, sce.pair_named(g, "on the second vertex"))
    assert e["trace"][0][:2] == (1.5, 1) and e["trace"][1][:2] == (0.0, None)


def test_nothing_to_hit(march):
    """A voxel beyond the farthest vertex: the search ends through the cap exit and the path comes out as it was.  All flags zero and a view
    number out of range: rule mode 2 then finds no sample near unknown space, so no safe problem is posed at all."""
    p = sce.pair_named(march, "far voxel")
    e = sce.expected(march, p)
    cap = max(march["rule"]["drone_radius"], np.linalg.norm(p["path"][1:] - p["path"][0], axis=1).max())
    widths = []
    d, how = sce.nearest_unknown(march, p["flags"], p["path"][0], cap, widths)
    assert how == "cap" and d > cap and len(widths) >= 3
    assert len(e["trace"]) == 1 and e["trace"][0][1] is None and e["trace"][0][0] > cap
    full, _ = sce.full_march(march, p)
    assert np.array_equal(full[1:], p["path"][1:])
    for name in ("no flags", "view out of range", "view negative"):
        assert not sce.expected(march, sce.pair_named(march, name))["live"]
    p = sce.pair_named(march, "no flags")
    assert not p["flags"].any()
    # ... and the march itself (it runs for such a pair when heading records are attached) leaves the path as it was: an empty lattice ends
    # the search through the cap exit with a value above every radius, a missing view with infinity
    cap = max(march["rule"]["drone_radius"], np.linalg.norm(p["path"][1:] - p["path"][0], axis=1).max())
    assert sce.nearest_unknown(march, p["flags"], p["path"][0], cap) == (1e300, "cap") and sce.nearest_unknown(march, None, p["path"][0], cap)[0] == np.inf


def test_nearest_voxel_outside_the_first_cube(boundary):
    g = boundary
    p = sce.pair_named(g, "second cube")
    v, res = p["path"][0], g["res"]
    cell = np.array(sce.cell_of(g, v))
    cells = np.argwhere(p["flags"] != 0)[:, ::-1] - cell
    assert sorted(map(tuple, cells)) == [(-1, -1, -1), (2, 0, 0)]
    pts = sce.flagged(g, p["flags"])
    d = np.linalg.norm(pts - v, axis=1) / res
    assert abs(d.min() - 1.51) < 1e-9 and abs(d.max() - np.sqrt(1.49 ** 2 + 2)) < 1e-9
    widths = []
    r, how = sce.nearest_unknown(g, p["flags"], v, np.inf, widths)
    assert widths[0] == 1 and len(widths) >= 2 and how == "found" and r == sce.nearest(pts, v) == sce.expected(g, p)["trace"][0][0]
    # two voxels at exactly the same distance
    p = sce.pair_named(g, "equal distance")
    d = np.sort(np.linalg.norm(sce.flagged(g, p["flags"]) - p["path"][0], axis=1))
    assert d[0] == d[1] == 1.0 < d[2]


def test_far_corner_takes_several_cubes():
    g = sce.far_corner_group()
    p = g["pairs"][0]
    widths = []
    cap = np.linalg.norm(p["path"][1:] - p["path"][0], axis=1).max()
    d, how = sce.nearest_unknown(g, p["flags"], p["path"][0], cap, widths)
    print("far corner: cube half-widths %s" % widths)
    assert len(widths) >= 4 and how == "covered" and d == sce.nearest(sce.flagged(g, p["flags"]), p["path"][0])
    assert np.array_equal(np.argwhere(p["flags"] != 0)[0], [15, 63, 63]) and sce.cell_of(g, p["path"][0]) == (2, 2, 2)
    assert len(sce.expected(g, p)["trace"]) == 2


@pytest.mark.parametrize("nz", [3, 1])
def test_vertices_outside_the_lattice(nz):
    g = sce.outside_group(nz)
    assert g["dims"] == (7, 5, nz) and np.all(np.abs(g["origin"] / g["res"] - np.round(g["origin"] / g["res"])) > 0.1)
    for p in g["pairs"][:6]:
        cell, (a, s) = sce.cell_of(g, p["path"][0]), ("xyz".index(p["name"][-1]), p["name"][-2])
        assert (cell[a] < 0) if s == "-" else (cell[a] >= g["dims"][a]), (p["name"], cell)
        e = sce.expected(g, p)
        assert e["live"] and e["trace"][-1][0] < g["rule"]["drone_radius"]
    assert sce.cell_of(g, g["pairs"][6]["path"][0])[0] > 200


def test_modelled_unknown_space():
    e = {r: sce.expected(g, g["pairs"][0]) for r in sce.MODELLED_R_KNOWN for g in [sce.modelled_group(r)]}
    assert e[2.5]["trace"][0][0] == 2.5 and e[2.5]["trace"][1][:2] == (0.0, None)   # the next centre lies on the sphere: clamped to 0
    assert e[0.0]["trace"] == [(0.0, None, 5)] and len(e[0.0]["path"]) == 2
    assert e[100.0]["trace"][0][1] is None and np.array_equal(e[100.0]["path"][1:], sce.modelled_group(100.0)["pairs"][0]["path"][1:4])


# ---- the lattice in the decomposition ---------------------------------------------------------------------------------------------------------
def test_list_lengths_with_lattice_ids():
    g = sce.homes_group()
    print("eligible cell centres: %d" % g["n_eligible"])
    assert g["n_eligible"] >= sce.CAP_GLOBAL + 1
    assert [int(p["name"][2:]) for p in g["pairs"]] == [sce.CAP - 1, sce.CAP, sce.CAP + 1, sce.CAP_IDS - 1, sce.CAP_IDS, sce.CAP_IDS + 1, sce.CAP_GLOBAL,
                                                         sce.CAP_GLOBAL + 1]
    for p in g["pairs"]:
        e = sce.expected(g, p)
        seg = np.concatenate([e["path"][0], e["path"][1]])
        assert np.array_equal(seg, g["segment"]) and len(e["path"]) == 2
        sce.assert_list_length(g, p, seg, int(p["name"][2:]))
        assert p["no_corridor"] == (int(p["name"][2:]) > sce.CAP_GLOBAL)


def test_split_lists_and_the_tie():
    g = sce.split_group()
    for p, k in zip(g["pairs"], (sce.CAP + 1, sce.CAP_IDS + 1)):
        e = sce.expected(g, p)
        seg = np.concatenate([e["path"][0], e["path"][1]])
        sce.assert_list_length(g, p, seg, k)
        cloud, n_unk = sce.decomposition_cloud(g, p)
        inside = sce.plane_depth(seg, cloud) >= sce.MARGIN_IN
        assert 0 < inside[:n_unk].sum() < k and inside[n_unk:].sum() == 100
    p = g["pairs"][0]
    e = sce.expected(g, p)
    cloud, n_unk = sce.decomposition_cloud(g, p)
    lst = cloud[sce.plane_depth(g["segment"], cloud) >= sce.MARGIN_IN]
    ia, ib = (int(np.nonzero(np.all(lst == q, axis=1))[0][0]) for q in (sce.TIE_VOXEL, sce.TIE_POINT))
    assert ia < ib and np.array_equal(sce.TIE_VOXEL * [1, -1, 1], sce.TIE_POINT) and e["R"][1] == 0.0 and e["R"][2] == 1.5
    first, swapped = host_rows(g, p, e["path"]), host_rows(g, p, e["path"], np.vstack([cloud[n_unk:], cloud[:n_unk]]))
    assert len(first[0]) == len(swapped[0]) and not np.array_equal(first[0], swapped[0])
    # the winner's plane is the first row: through the voxel (y > 0) when the voxels are listed first, its mirror image otherwise
    assert first[0][0, 1] > 0.9 and np.array_equal(first[0][0] * [1, -1, 1, 1], swapped[0][0])


def test_sub_block_sizes():
    totals = []
    for dims in sce.BLOCK_DIMS:
        g = sce.block_group(dims)
        cen = sce.centres(g["origin"], g["res"], dims).reshape(-1, 3)
        for p, nearest in zip(g["pairs"], (0, len(cen) - 1)):
            e = sce.expected(g, p)
            seg = np.concatenate([e["path"][0], e["path"][1]])
            lo, hi = sce.box_aabb(seg)
            r = sce.lattice_range(g["origin"], g["res"], dims, lo, hi)
            assert r[1::2][:3] == dims and r[6] == int(np.prod(dims)), (dims, r)
            assert sce.plane_depth(seg, cen).min() >= sce.MARGIN_IN
            mid = (seg[:3] + seg[3:]) / 2
            assert int(np.argmin(np.linalg.norm(cen - mid, axis=1))) == nearest   # the first / the last cell of the sweep is the nearest point
            if len(cen) > 1:                                                     # ... and decides the first plane: without it the rows differ
                cloud = np.delete(cen, nearest, axis=0)
                assert not np.array_equal(host_rows(g, p, e["path"])[0], host_rows(g, p, e["path"], cloud)[0])
        totals.append(r[6])
    assert totals == [1, 63, 64, 65, 255, 256, 257]


@pytest.mark.parametrize("nz", [sce.C_DIMS[2], 1])
def test_clipped_sub_blocks(nz):
    g = sce.clip_group(nz)
    for p in g["pairs"]:
        e = sce.expected(g, p)
        assert len(e["path"]) == 2, p["name"]
        seg = np.concatenate([e["path"][0], e["path"][1]])
        lo, hi = sce.box_aabb(seg)
        r = sce.lattice_range(g["origin"], g["res"], g["dims"], lo, hi)
        below = [np.floor((lo[a] - g["origin"][a]) / g["res"]) - 1 < 0 for a in range(3)]
        above = [np.floor((hi[a] - g["origin"][a]) / g["res"]) + 1 > g["dims"][a] - 1 for a in range(3)]
        if p["name"] == "outside":
            cloud, n_unk = sce.decomposition_cloud(g, p)
            assert r[6] == 0 and hi[0] < g["origin"][0] - 0.3
            assert sce.plane_depth(seg, cloud[:n_unk]).max() < -0.3 and (sce.plane_depth(seg, g["cloud"]) > sce.MARGIN_IN).sum() == 3
            assert np.array_equal(np.vstack(host_rows(g, p, e["path"])), np.vstack(host_rows(g, p, e["path"], g["cloud"])))
            continue
        a, side = "xyz".index(p["name"][1]), p["name"][0]
        assert (below if side == "-" else above)[a], (p["name"], lo, hi)
        assert r[6] > 0 and sce.range_margin(g["origin"], g["res"], lo, hi) > 1e-6
        cloud, n_unk = sce.decomposition_cloud(g, p)
        listed = sce.plane_depth(seg, cloud[:n_unk]) > 0
        assert listed.sum() >= 20 and np.abs(sce.plane_depth(seg, cloud[:n_unk])).min() > 1e-4
        if nz == 1:
            assert r[5] == 1 and below[2] and above[2]


def test_1024_cells_per_axis():
    g, g5 = sce.fine_group(1024), sce.fine_group(1025)
    assert g["range"][1] == 1024 and g["range"][6] == 1024 * g["range"][3] * g["range"][5] > 0
    assert g5["range"][1] == 1025 and g5["range"][6] == -1 and g5["res"] == g["res"] and g5["pairs"][0]["no_corridor"]
    p = g["pairs"][0]
    e = sce.expected(g, p)
    assert np.array_equal(np.concatenate([e["path"][0], e["path"][1]]), g["segment"])
    cols = np.argwhere(p["flags"] != 0)[:, 2] - g["range"][0]
    assert 1023 in cols and 0 in cols and 63 in cols and 64 in cols
    pts = sce.flagged(g, p["flags"])
    depth = sce.plane_depth(g["segment"], pts)
    assert np.abs(depth).min() > 1e-4 and depth[np.argmax(pts[:, 0])] > 1e-3   # column 1023 is in the local box: its packed id is listed
    assert len(host_rows(g, p, e["path"])[0]) > 7


def test_cell_centre_exactly_on_the_sphere():
    g, gb = sce.sphere_group(False), sce.sphere_group(True)
    p = g["pairs"][0]
    A, cell = p["problem"]["x0"][:3], g["cell"]
    d = cell - A
    assert d[0] * d[0] + d[1] * d[1] + d[2] * d[2] == 6.25 == g["rule"]["r_known"] ** 2 > gb["rule"]["r_known"] ** 2
    unk, unk_b = (pair_glue.unknown_voxels(x["origin"], x["res"], np.array(x["dims"]), A, x["rule"]["r_known"]) for x in (g, gb))
    assert not np.any(np.all(unk == cell, axis=1)) and np.any(np.all(unk_b == cell, axis=1)) and len(unk_b) > len(unk)
    e, eb = sce.expected(g, p), sce.expected(gb, gb["pairs"][0])
    assert np.array_equal(e["path"], eb["path"])
    seg = np.concatenate([e["path"][0], e["path"][1]])
    cen = sce.centres(g["origin"], g["res"], g["dims"]).reshape(-1, 3)
    assert np.abs(sce.plane_depth(seg, cen)).min() > 1e-4 and sce.plane_depth(seg, cell)[0] > sce.MARGIN_IN
    rows, rows_b = host_rows(g, p, e["path"])[0], host_rows(gb, gb["pairs"][0], e["path"])[0]
    assert rows.shape != rows_b.shape or np.abs(rows - rows_b).max() > 1e-6


# ---- finalize -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mps", [1, 3, sce.MAX_POLY])
def test_where_xf_lands(mps):
    g = sce.march_group(mps)
    for name, inside in (("G inside", True), ("G outside", False), ("G on the ground", True)):
        p = sce.pair_named(g, name)
        e = sce.expected(g, p)
        rows = host_rows(g, p, e["path"])[-1]
        v = rows[:, :3] @ p["goal"] - rows[:, 3]
        assert (not np.any(v > 0)) == inside, (name, v.max())
        if name == "G on the ground":
            ground = np.nonzero(np.all(rows == [0.0, 0.0, -1.0, -g["z_ground"]], axis=1))[0]
            assert len(ground) == 1 and v[ground[0]] == 0.0 and np.delete(v, ground[0]).max() < -0.05
        else:
            assert np.abs(v).min() > 0.05


def test_table_sizes(march):
    e = sce.expected(march, sce.pair_named(march, "n_points=%d" % sce.SAFE_PATH_CAP))
    assert len(e["path"]) == sce.MAX_POLY + 1                                   # eight legs: all nine face_off entries
    g = sce.shell_group()
    rows = host_rows(g, g["pairs"][0], sce.expected(g, g["pairs"][0])["path"])
    print("shell: %d rows on the host" % len(rows[0]))
    assert len(rows) == 1 and len(rows[0]) > sce.MAX_FACES_POLY
    g = sce.rows_group()
    totals = [sum(len(r) for r in host_rows(g, p, sce.expected(g, p)["path"])) for p in g["pairs"]]
    assert sorted(totals)[-1] > sorted(totals)[-2] and max(totals) <= g["fpp"]   # one pair alone has the largest total


# ---- wrong variants: each changes the expected output of a named case ------------------------------------------------------------------------------
def march_variant(g, p, first_cube=False, le=False, eliminated_off=0, last_leg_only=False):
    """pair_glue.safe_path restated with switches for the mistakes a kernel could make (all off: the restatement itself)"""
    e = sce.expected(g, p)
    rule, unk = g["rule"], e["unknown"]
    orig = [np.array(v) for v in p["path"][:p["n_points"]]]
    cur = [v.copy() for v in orig]
    A = p["problem"]["x0"][:3]
    it = 0
    while cur:
        if rule["mode"] == 2:
            if first_cube:   # the nearest voxel of the first cube that holds one
                cell = np.array(sce.cell_of(g, cur[0]))
                idx = np.argwhere(p["flags"] != 0)[:, ::-1]
                ring = np.abs(idx - cell).max(axis=1)
                r = sce.nearest(unk[ring == max(ring.min(), 1)] if ring.min() > 1 else unk[ring <= 1], cur[0])
            else:
                r = sce.nearest(unk, cur[0])
        else:
            r = max(rule["r_known"] - pair_glue._norm3(cur[0] - A), 0.0)
        if (r <= rule["drone_radius"]) if le else (r < rule["drone_radius"]):
            if it == 0:
                orig = [orig[0], orig[0] + np.array([0.01, 0.0, 0.0])]
            else:
                orig = orig[:len(orig) - len(cur) + 1 + eliminated_off] + [cur[0]]
                if last_leg_only:
                    v = orig[-1] - orig[-2]
                    ln = np.linalg.norm(v)
                    orig[-1] = orig[-2] + v / ln * max(ln - rule["drone_radius"], 0.0)
                else:
                    orig = pair_glue._shorten_by(orig, rule["drone_radius"])
            break
        inters, last_id, none_outside = pair_glue._sphere_exit(cur, r, cur[0])
        if none_outside:
            break
        cur = [inters] + cur[last_id + 1:]
        it += 1
    orig[0] = e["R"][:3]
    return np.array(orig[:g["max_poly_safe"] + 1])


def differs(a, b):
    return a.shape != b.shape or np.abs(a - b).max() > 1000 * ATOL


def test_the_variant_without_mistakes_is_the_restatement(march, boundary):
    for g in (march, boundary, sce.far_corner_group(), sce.outside_group(3), sce.modelled_group(2.5)):
        for p in g["pairs"]:
            e = sce.expected(g, p)
            if e["live"]:
                assert np.array_equal(march_variant(g, p), e["path"]), (g["name"], p["name"])


def test_wrong_variants_are_caught(march, boundary):
    want = lambda g, name: sce.expected(g, sce.pair_named(g, name))["path"]  # noqa: E731
    got = lambda g, name, **kw: march_variant(g, sce.pair_named(g, name), **kw)  # noqa: E731
    assert differs(got(boundary, "second cube", first_cube=True), want(boundary, "second cube"))
    assert differs(got(boundary, "exactly drone_radius", le=True), want(boundary, "exactly drone_radius"))
    for off in (-1, 1):   # (a case whose cut path fits max_poly_safe legs: the end of a longer one is not part of the output)
        assert differs(got(march, "near slab", eliminated_off=off), want(march, "near slab"))
        assert differs(got(boundary, "equal distance", eliminated_off=off), want(boundary, "equal distance"))
    assert differs(got(march, "back-off", last_leg_only=True), want(march, "back-off"))
    # `>=` for `>` at the sphere lists the cell on it: the rows of "sphere exact" become those of "sphere below" (they differ, above);
    # the lattice listed after the cloud: the occupied point wins the tie of "split k=CAP + 1" (test_split_lists_and_the_tie)
    g = sce.sphere_group(False)
    p = g["pairs"][0]
    A, r = p["problem"]["x0"][:3], g["rule"]["r_known"]
    cen = sce.centres(g["origin"], g["res"], g["dims"]).reshape(-1, 3)
    ge = cen[((cen - A) ** 2).sum(axis=1) >= r * r]
    e = sce.expected(g, p)
    a, b = host_rows(g, p, e["path"])[0], host_rows(g, p, e["path"], ge)[0]
    assert a.shape != b.shape or np.abs(a - b).max() > 1e-6
