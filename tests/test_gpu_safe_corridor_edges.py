"""fh_safe_corridor_batch_device at the edges of its three kernels: the march of safe_path_kernel (vertex counts up to SAFE_PATH_CAP, many
iterations, a back-off across legs, the strict `<` at drone_radius, nothing to hit), nearest_unknown (a nearest voxel outside the first
cube, the cap exit, vertices outside the lattice), decomp_kernel with an UnknownLattice (lattice ids in every list home, sub-blocks around
the trips of 64 and 256 cells, clipped and empty sub-blocks, 1024 cells per axis, the strict `>` of the sphere model) and
safe_finalize_kernel (where xf lands, the table sizes).

The inputs come from tests/safe_corridor_edge_cases.py and are proved on the CPU in tests/test_safe_corridor_edge_cases.py.  A group is
one launch; its pairs read views of their own.  x0 is compared with tests/sample_model.py within its bound, the safe path with
oracle/pair_glue.safe_path at 1e-9 (the crossing point is a restated single-precision result), the polytopes with the host decomposition of
the DEVICE's safe path against [unknown voxels, z-major | occupied points] by np.array_equal, xf by the G-inside rule on the host rows.
Every output buffer is one slot longer than the batch and starts as the byte 0xA5."""
import numpy as np
import pytest
import torch  # noqa: F401  (before libfasterhip.so is loaded: one HIP runtime per process)

import safe_corridor_edge_cases as sce
from faster_amd import abi, capi, frontend

pytestmark = pytest.mark.gpu

FS = abi.face_dtype.itemsize
PS = abi.problem_dtype.itemsize
HS = abi.heading_dtype.itemsize
POISON = 0xA5
DEV = "cuda:0"
OUTPUT_FIELDS = ("x0", "xf", "n_seg", "n_poly", "face_off", "face_begin")
BIT_EQUAL = [0, 0]   # vertices behind the first of all safe paths compared: bit-equal, all


@pytest.fixture(scope="module", autouse=True)
def built():
    from faster_amd import build as fb

    fb.build_frontend()


@pytest.fixture(scope="module")
def c():
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


def poisoned(nbytes):
    return torch.full((nbytes,), POISON, dtype=torch.uint8, device=DEV)


def to_dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8) if a.dtype.names else a).to(DEV)


def records(items, dtype):
    out = np.zeros(len(items), dtype=dtype)
    for i, r in enumerate(items):
        out[i] = r
    return out


def templates(g):
    """the safe problems as the caller prepares them: bounds, dc and factor window of the whole problem, and values in every field the
    launch may write that no launch would write"""
    n = len(g["pairs"])
    t = np.zeros(n, dtype=abi.problem_dtype)
    for i, p in enumerate(g["pairs"]):
        t[i] = p["problem"]
        t["x0"][i] = 70.0 + i + np.arange(9)
        t["xf"][i] = -70.0 - i - np.arange(9)
    t["n_seg"], t["n_poly"], t["face_off"], t["face_begin"], t["force_final_pos"] = 13, -5, -7, -9, 0
    return t


def launch(ctx, g, fpp=None, headings=False):
    """one fh_safe_corridor_batch_device over the pairs of g -> dict(safe, faces [n][fpp] rows, paths [n][mps + 1][3], raw path bytes, np).
    headings: heading records are attached (fh_fleet_set_headings_device), the march then also runs for a pair that needs no safe path"""
    n, mp, mps = len(g["pairs"]), g["max_points"], g["max_poly_safe"]
    fpp = g["fpp"] if fpp is None else fpp
    whole, wres = records([p["problem"] for p in g["pairs"]], abi.problem_dtype), records([p["result"] for p in g["pairs"]], abi.result_dtype)
    paths = np.full((n, mp, 3), np.nan)
    for i, p in enumerate(g["pairs"]):
        assert p["n_points"] <= mp and len(p["path"]) <= mp
        paths[i, :len(p["path"])] = p["path"]
    npts = np.array([p["n_points"] for p in g["pairs"]], dtype=np.int32)
    goals = np.array([p["goal"] for p in g["pairs"]])
    tmpl = templates(g)
    d_whole, d_wres, d_paths, d_np, d_goals = to_dev(whole), to_dev(wres), to_dev(paths), to_dev(npts), to_dev(goals)
    d_cloud = to_dev(g["cloud"]) if len(g["cloud"]) else None
    d_safe = poisoned((n + 1) * PS)
    d_safe[:n * PS] = to_dev(tmpl)
    d_sf, d_sp, d_snp = poisoned((n + 1) * fpp * FS), poisoned((n + 1) * (mps + 1) * 24), poisoned((n + 1) * 4)
    rule = g["rule"]
    keep = []
    if rule["mode"] == 2:
        views = [p["flags"] for p in g["pairs"] if p["flags"] is not None]
        cells = int(np.prod(g["dims"]))
        view_of, j = [], 0
        for p in g["pairs"]:
            if p["flags"] is not None:
                assert p["flags"].shape == g["dims"][::-1] and p["flags"].dtype == np.uint8
                view_of.append(j)
                j += 1
            else:
                assert not 0 <= p["view"] < len(views)
                view_of.append(p["view"])
        d_flags, d_view_of = to_dev(np.stack(views).reshape(len(views), cells)), to_dev(np.array(view_of, dtype=np.int32))
        keep = [d_flags, d_view_of]
        ctx.set_unknown_views_device(d_flags.data_ptr(), cells, d_view_of.data_ptr(), len(views), g["origin"], g["res"], g["dims"])
    ctx.set_pair_rule(**rule)
    d_head = poisoned((n + 1) * HS)
    if headings:
        ctx.fleet_set_headings_device(d_head.data_ptr(), n)
    try:
        ctx.safe_corridor_batch_device(d_whole.data_ptr(), d_wres.data_ptr(), d_paths.data_ptr(), d_np.data_ptr(), mp, d_goals.data_ptr(),
                                       d_cloud.data_ptr() if d_cloud is not None else None, len(g["cloud"]), g["origin"], g["res"], g["dims"], n,
                                       g["r_frac"], mps, g["bbox"], g["decomp_radius"], g["z_ground"], fpp, sce.N_SEG_SAFE, d_safe.data_ptr(),
                                       d_sf.data_ptr(), d_sp.data_ptr(), d_snp.data_ptr())
        ctx.sync()
    finally:
        ctx.set_pair_rule(mode=0)
        ctx.set_unknown_views_device(None)
        ctx.fleet_set_headings_device(None, 0)
    del keep
    for d, per in ((d_safe, PS), (d_sf, fpp * FS), (d_sp, (mps + 1) * 24), (d_snp, 4), (d_head, HS)):
        assert bool((d[n * per:] == POISON).all()), (g["name"], "the guard slot was written")
    return {"safe": d_safe[:n * PS].cpu().numpy().view(abi.problem_dtype), "tmpl": tmpl, "fpp": fpp, "head": d_head[:n * HS].cpu().numpy().reshape(n, HS),
            "faces": d_sf[:n * fpp * FS].cpu().numpy().view(abi.face_dtype).reshape(n, fpp),
            "face_bytes": d_sf[:n * fpp * FS].cpu().numpy().reshape(n, fpp, FS),
            "paths": d_sp[:n * (mps + 1) * 24].cpu().numpy().view(np.float64).reshape(n, mps + 1, 3),
            "path_bytes": d_sp[:n * (mps + 1) * 24].cpu().numpy().reshape(n, mps + 1, 24), "np": d_snp[:n * 4].cpu().numpy().view(np.int32)}


def host_polys(g, p, path):
    cloud, _ = sce.decomposition_cloud(g, p)
    return frontend.decompose(path, cloud, drone_radius=g["decomp_radius"], z_ground=g["z_ground"], bbox=g["bbox"])[0]


def check(g, out, failing=()):
    """every comparison of the module's docstring, pair by pair -> {pair name: row total of the host decomposition}"""
    safe, tmpl, fpp = out["safe"], out["tmpl"], out["fpp"]
    totals = {}
    for name in abi.problem_dtype.names:   # bounds, dc, factor window, force_final_pos, ...: as the caller set them
        if name not in OUTPUT_FIELDS:
            assert np.array_equal(safe[name], tmpl[name]), (g["name"], name)
    for i, p in enumerate(g["pairs"]):
        what = "%s / %s" % (g["name"], p["name"])
        e = sce.expected(g, p)
        snp = int(out["np"][i])
        assert np.all(out["path_bytes"][i, max(snp, 0):] == POISON), (what, "vertices behind n_points were written")
        if not e["live"]:
            print("%s: no safe problem, n_points %d n_seg %d" % (what, snp, safe["n_seg"][i]))
            assert snp == 0 and safe["n_seg"][i] == 0, (what, snp, safe["n_seg"][i])
            for name in ("x0", "xf", "n_poly", "face_off", "face_begin"):
                assert np.array_equal(safe[name][i], tmpl[name][i]), (what, name)
            assert np.all(out["face_bytes"][i] == POISON), what
            continue
        want, got = e["path"], out["paths"][i, :snp]
        err = np.abs(safe["x0"][i] - e["R"])
        print("%s: k %d, n_points %d (restatement %d), x0 error %.2e of %.2e" % (what, e["k"], snp, len(want), err.max(), e["R_bound"].max()))
        assert np.all(err <= e["R_bound"]), (what, err, e["R_bound"])
        assert snp == len(want), (what, snp, len(want))
        assert np.array_equal(got[0], safe["x0"][i, :3]), what
        same = int(np.all(got[1:] == want[1:], axis=1).sum())
        BIT_EQUAL[0] += same
        BIT_EQUAL[1] += snp - 1
        print("%s: %d of %d vertices behind R bit-equal, largest difference %.2e" % (what, same, snp - 1, np.abs(got[1:] - want[1:]).max()))
        np.testing.assert_allclose(got[1:], want[1:], rtol=0, atol=1e-9, err_msg=what)
        if p["untouched"]:
            assert np.array_equal(got[1:], p["path"][1:snp]), what
        if p["no_corridor"] or p["name"] in failing:
            print("%s: n_seg %d" % (what, safe["n_seg"][i]))
            assert safe["n_seg"][i] == 0, (what, safe["n_seg"][i])
            assert np.array_equal(safe["xf"][i], tmpl["xf"][i]), what
            if not p["no_corridor"]:
                totals[p["name"]] = sum(len(b) for _, b in host_polys(g, p, got))
            continue
        polys = host_polys(g, p, got)
        ends = np.cumsum([len(b) for _, b in polys])
        totals[p["name"]] = int(ends[-1])
        assert ends[-1] <= fpp, (what, ends, fpp)
        want_off = np.concatenate([[0], ends, np.full(8 - len(ends), ends[-1])]).astype(np.int32)
        assert safe["n_seg"][i] == sce.N_SEG_SAFE and safe["n_poly"][i] == len(polys) == snp - 1, (what, safe["n_seg"][i], safe["n_poly"][i], len(polys))
        assert np.array_equal(safe["face_off"][i], want_off), (what, safe["face_off"][i], want_off)
        assert safe["face_begin"][i] == i * fpp, what
        rows = out["faces"][i, :ends[-1]]
        assert np.array_equal(rows["a"], np.vstack([A for A, _ in polys])) and np.array_equal(rows["b"], np.concatenate([b for _, b in polys])), what
        assert np.all(out["face_bytes"][i, ends[-1]:] == POISON), (what, "rows behind the pair's total were written")
        Al, bl = polys[-1]
        inside = not np.any(Al @ p["goal"] - bl > 0)
        assert np.array_equal(safe["xf"][i, :3], p["goal"] if inside else got[-1]), (what, inside, safe["xf"][i, :3])
        assert np.array_equal(safe["xf"][i, 3:], tmpl["xf"][i, 3:]), what
    return totals


def run(ctx, g, **kw):
    return check(g, launch(ctx, g), **kw)


# ---- the march ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_poly_safe", [1, 3, sce.MAX_POLY])
def test_march_vertex_counts_long_march_back_off_and_nothing_to_hit(c, max_poly_safe):
    """One launch with max_points = SAFE_PATH_CAP: paths of 2, SAFE_PATH_CAP - 1 and SAFE_PATH_CAP vertices (seven iterations that erase five
    vertices each, cut beyond vertex 20, truncated to max_poly_safe legs), n_points 0, 1, -1, -2 (no safe problem), a slab so near that the cut
    path is shorter than max_poly_safe + 1, a back-off over several 5 cm legs, a voxel beyond the farthest vertex (the cap exit: the path as
    it was), pairs without unknown voxels (no flags, a view number out of range: no safe problem, nothing written), and G inside, outside and
    on the ground plane of the last polytope.  With FH_MAX_POLY legs all nine face_off entries differ."""
    g = sce.march_group(max_poly_safe)
    out = launch(c, g)
    check(g, out)
    if max_poly_safe == sce.MAX_POLY:
        i = [p["name"] for p in g["pairs"]].index("n_points=%d" % sce.SAFE_PATH_CAP)
        assert out["safe"]["n_poly"][i] == sce.MAX_POLY and np.all(np.diff(out["safe"]["face_off"][i]) > 0)
    for name, inside in (("G inside", True), ("G outside", False), ("G on the ground", True)):
        i = [p["name"] for p in g["pairs"]].index(name)
        assert np.array_equal(out["safe"]["xf"][i, :3], g["pairs"][i]["goal"]) == inside, name


def test_march_without_unknown_voxels_leaves_the_path_as_it_was(c):
    """In rule mode 2 a pair without unknown voxels needs no safe path, and the march only runs for it when heading records are attached:
    look_at is then the last vertex of the path as the march left it.  All flags zero (the search proves every voxel farther than the cap)
    and a view number out of range (no flags at all): the last vertex of JPS_in, bit for bit; nothing else of the record is written, and
    a pair without a usable path gets no look_at.  A pair with a safe problem looks at the end of its safe path, or at G when G is inside."""
    g = sce.march_group(3)
    out = launch(c, g, headings=True)
    check(g, out)
    off = abi.heading_dtype.fields["look_at"][1]
    for i, p in enumerate(g["pairs"]):
        rec = out["head"][i]
        assert np.all(rec[:off] == POISON) and np.all(rec[off + 24:] == POISON), p["name"]
        look = rec[off:off + 24].copy().view(np.float64)
        if not 2 <= p["n_points"] <= sce.SAFE_PATH_CAP:
            assert np.all(rec == POISON), p["name"]
        elif not sce.expected(g, p)["live"]:
            print("%s: look_at %s" % (p["name"], look))
            assert p["name"] in ("no flags", "view out of range", "view negative") and np.array_equal(look, p["path"][p["n_points"] - 1]), (p["name"], look)
        else:
            snp = int(out["np"][i])
            at_g = np.array_equal(out["safe"]["xf"][i, :3], p["goal"]) and out["safe"]["n_seg"][i] > 0
            assert np.array_equal(look, p["goal"] if at_g else out["paths"][i, snp - 1]), (p["name"], look)


def test_boundary_of_the_cut_and_nearest_voxel_outside_the_first_cube(c):
    """drone_radius 0.25 on cells of 0.5 m, every number exact: a first vertex 0.2 m from a voxel (the 1 cm stub), exactly 0.25 m (`<` is
    strict: the march goes on), on it, a voxel on the second vertex; the nearest voxel two cells away along x with a farther one in the
    first cube; two voxels at equal distance."""
    run(c, sce.boundary_group())


def test_lone_voxel_in_the_far_corner(c):
    """64 x 64 x 16 cells, the only unknown voxel in the corner opposite the path's start: the cube grows until it covers the lattice"""
    run(c, sce.far_corner_group())


@pytest.mark.parametrize("nz", [3, 1])
def test_vertices_outside_the_lattice(c, nz):
    """7 x 5 x nz cells whose origin is no multiple of the cell size; the first vertex 1 m outside the lattice on each of its six sides,
    and 100 m away"""
    run(c, sce.outside_group(nz))


@pytest.mark.parametrize("r_known", sce.MODELLED_R_KNOWN)
def test_modelled_unknown_space(c, r_known):
    """rule mode 0: the path crosses the sphere of r_known (the next centre lies on it: r clamped to 0), r_known = 0 (the stub), r_known
    large (the path as it was, no unknown voxel in the decomposition)"""
    run(c, sce.modelled_group(r_known))


# ---- the lattice in the decomposition ---------------------------------------------------------------------------------------------------------
def test_lattice_ids_in_every_list_home(c):
    """Exactly k flagged cells in the local box, k on either side of FH_DECOMP_CAP, FH_DECOMP_CAP_IDS and FH_DECOMP_CAP_GLOBAL; one more than
    the last gives no corridor"""
    run(c, sce.homes_group())


def test_list_split_between_voxels_and_occupied_points(c):
    """FH_DECOMP_CAP + 1 and FH_DECOMP_CAP_IDS + 1 entries, the voxels first; the nearest two are a voxel and an occupied point that mirror
    each other: the voxel wins the tie"""
    run(c, sce.split_group())


@pytest.mark.parametrize("dims", sce.BLOCK_DIMS, ids=lambda d: "%dx%dx%d" % d)
def test_sub_block_sizes_around_the_trips(c, dims):
    """1, 63, 64, 65, 255, 256 and 257 cells, all flagged: the first plane goes through the first cell of the sweep for one pair and
    through the last for the other"""
    run(c, sce.block_group(dims))


@pytest.mark.parametrize("nz", [sce.C_DIMS[2], 1])
def test_sub_block_clipped_by_the_lattice(c, nz):
    """the local box sticks out of the lattice on each side in turn, lies entirely outside it (rows of the occupied points alone), and a
    lattice one cell thick"""
    run(c, sce.clip_group(nz))


@pytest.mark.parametrize("cx", [1024, 1025])
def test_1024_cells_per_axis(c, cx):
    """a sub-block of 1024 cells along x whose last column is listed equals the host; 1025: the segment fails, n_seg = 0"""
    run(c, sce.fine_group(cx))


@pytest.mark.parametrize("below", [False, True])
def test_cell_centre_exactly_on_the_sphere(c, below):
    """rule mode 0, a cell centre exactly r_known = 2.5 from A is not unknown (`>` is strict); it is for the next double below 2.5"""
    run(c, sce.sphere_group(below))


# ---- the table -------------------------------------------------------------------------------------------------------------------------------
def test_faces_per_problem_at_the_rows_needed(c):
    """faces_per_problem = T, the largest row total: every pair is kept; T - 1: exactly the pairs with T rows get n_seg = 0 and the others
    keep their bytes"""
    g = sce.rows_group()
    full = launch(c, g)
    totals = check(g, full)
    T = max(totals.values())
    at_T = {k for k, t in totals.items() if t == T}
    assert 1 <= len(at_T) < len(totals), totals
    assert check(g, launch(c, g, fpp=T)) == totals
    less = launch(c, g, fpp=T - 1)
    assert check(g, less, failing=at_T) == totals
    for i, p in enumerate(g["pairs"]):
        if p["name"] not in at_T:
            t = totals[p["name"]]
            assert np.array_equal(less["face_bytes"][i, :t], full["face_bytes"][i, :t]) and np.array_equal(less["safe"]["face_off"][i], full["safe"]["face_off"][i])


def test_polytope_of_more_rows_than_fh_max_faces_poly(c):
    """a leg inside a dense shell of unknown voxels: hundreds of rows on the host, no corridor on the device"""
    g = sce.shell_group()
    run(c, g)
    e = sce.expected(g, g["pairs"][0])
    assert max(len(b) for _, b in host_polys(g, g["pairs"][0], e["path"])) > sce.MAX_FACES_POLY


def test_zz_bit_equal_vertices_are_reported():
    print("safe path vertices behind R, all cases of this module: %d of %d bit-equal to oracle/pair_glue.safe_path" % tuple(BIT_EQUAL))
