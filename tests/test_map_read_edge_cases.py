"""The cases of tests/map_read_edge_cases.py on the CPU: the model of the map read (tests/map_read_model.py) against the host restatement
(VoxelGrid::build through frontend.plan_batch), against what each case says in its own words, against the planted mutants of the model,
and against the reference's compiled readMap — live where oracle/_ref is built, and as recorded in tests/golden/map_read_ref.json
everywhere.  Every comparison is exact."""
import functools
import json
import os

import numpy as np
import pytest

import map_read_edge_cases as mc
import map_read_model as mm
import path_edge_cases as pe
from faster_amd import build as fb
from faster_amd import frontend

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = mc.cases()
NAMES = [c.name for c in CASES]
MASKS = mc.mask_cases()


@pytest.fixture(scope="module", autouse=True)
def built():
    fb.build_frontend()


def host_grid(lat, cloud):
    none = np.zeros((0, 3))
    return frontend.plan_batch(*lat.args(cloud), none, none, max_points=4, want_grid=True)[3:]


def ids_of(occ):
    return np.flatnonzero(occ.reshape(-1)).tolist()


# ---- the model against the host restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_model_equals_the_host_restatement(name):
    c = mc.case(name)
    occ, dims, origin = host_grid(c.lat, c.cloud)
    assert tuple(dims) == c.lat.dims and np.array_equal(origin, c.lat.origin)
    assert np.array_equal(occ, c.occ), (name, ids_of(occ)[:16], ids_of(c.occ)[:16])


@pytest.mark.parametrize("k", range(len(MASKS)), ids=[k.name for k in MASKS])
def test_model_equals_the_host_restatement_on_every_view_of_the_mask_cases(k):
    mk = MASKS[k]
    for v in range(mk.n_views):
        occ, dims, _ = host_grid(mk.lat, mk.cloud[mk.known(v)])
        assert tuple(dims) == mk.lat.dims and np.array_equal(occ, mk.occ(v)), (mk.name, v)


# ---- the cases do what they say -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_case_does_what_it_says(name):
    c = mc.case(name)
    if c.ids is not None:
        assert ids_of(c.occ) == c.ids, (name, c.says)
    kind = name.split("/")[0]
    if kind == "notfinite" or name == "far/wrap32":
        assert c.ids == [] and not c.occ.any(), name
    elif kind == "far":
        a = int(np.argmax(np.abs(c.cloud[0] - c.lat.centre(c.lat.mid))))      # the axis along which the point is far
        if c.cloud[0, a] > 0:
            assert c.ids == [] and not c.occ.any(), name
        else:                              # a finite point below the window: the cell of the low face (contract 3), nothing else
            want = list(c.lat.mid)
            want[a] = 0
            z, y, x = np.nonzero(c.occ)
            assert len(x) == 1 and [int(x[0]), int(y[0]), int(z[0])] == want, name


def test_lattices_are_what_the_cases_assume():
    assert [b.dims for b in mc.BIN] == [(8, 6, 4), (13, 11, 4), (18, 16, 4)] and mc.WRAP.dims == (8, 8, 4)
    assert np.array_equal(mc.BIN[0].origin, [-2.0, -1.5, 0.0]) and mc.DEC.m == 2
    nx, ny, nz = mc.DEC.dims
    assert (nx, ny) == (9 + 10, 7 + 10) and nz < 20            # widened by 5 * inflation / res, clipped by z_ground and z_max
    assert any(o / mc.DEC.res != round(o / mc.DEC.res) for o in mc.DEC.origin)


def test_faces_of_the_binary_lattices_are_exact_and_the_boundary_belongs_to_the_cell_above():
    for lat in mc.BIN:
        below = 0
        for a in range(3):
            for k in range(lat.dims[a] + 1):
                f = lat.face(a, k)
                got = []
                for x in (np.nextafter(f, -np.inf), f, np.nextafter(f, np.inf)):
                    p = lat.centre(lat.mid)
                    p[a] = float(x)
                    got.append(mc.exact_cell(p, lat.origin, lat.res)[a])
                    assert mm.cell_of(p, lat.origin, lat.res) == mc.exact_cell(p, lat.origin, lat.res)
                assert (f - float(lat.origin[a])) / lat.res == k and got[1:] == [k, k] and got[0] in (max(k - 1, 0), k), (lat.name, a, k, got)
                below += int(k > 0 and got[0] == k - 1)
        assert 0 < below < sum(lat.dims), (lat.name, below)      # (some neighbours below a boundary stay below it in the expression, some do not)


def test_faces_of_the_decimal_lattice_are_decided_by_rounding():
    """on the decimal lattice the boundary point lands in cell k for some k and in cell k - 1 for others"""
    lat = mc.DEC
    above = under = 0
    for a in range(3):
        for k in range(1, lat.dims[a] + 1):
            p = lat.centre(lat.mid)
            p[a] = lat.face(a, k)
            got = mc.exact_cell(p, lat.origin, lat.res)[a]
            assert got in (k - 1, k)
            above, under = above + int(got == k), under + int(got == k - 1)
    print("decimal lattice: %d boundary points in the cell above, %d in the cell below" % (above, under))
    assert above > 0 and under > 0


def test_near_outside_cases_wrap_as_the_contract_says():
    for lat in mc.BIN:
        nx, ny, nz = lat.dims
        mx, my, mz = lat.mid
        occ = mc.case("near/%s/x%+d" % (lat.name, nx)).occ                 # beyond the high x face: cell 0 of the next row
        assert occ[mz, my + 1, 0] and (lat.m > 0 or occ.sum() == 100)
        occ = mc.case("near/%s/y%+d" % (lat.name, ny)).occ                 # beyond the high y face: row 0 of the next layer
        assert occ[mz + 1, 0, mx] and (lat.m > 0 or occ.sum() == 100)
        assert not mc.case("near/%s/z%+d" % (lat.name, nz + lat.m + 1)).occ.any()
        for a in range(3):                                                 # below: exactly what a point in cell 0 marks
            low = list(lat.mid)
            low[a] = 0
            want = mm.occupancy(*lat.args([lat.centre(low)]))[0]
            for ca in (-1, -lat.m - 1):
                assert want.any() and np.array_equal(mc.case("near/%s/%s%+d" % (lat.name, "xyz"[a], ca)).occ, want)


def test_nowhere_cloud_marks_nothing_and_counts_are_counts():
    cloud = mc.nowhere_cloud()
    assert len(cloud) == 28 and not mm.occupancy(*mc.BIN[0].args(cloud))[0].any()
    assert [len(mc.case("counts/%d" % n).cloud) for n in (0, 1, 255, 256, 257)] == [0, 1, 255, 256, 257]
    assert len(mc.case("counts/300-copies").cloud) == 300
    for n in (255, 256, 257):      # (the clouds are not trivial: cells marked, cells free, points beyond a face)
        c = mc.case("counts/%d" % n)
        inside = ((c.cloud >= c.lat.origin) & (c.cloud < np.asarray(c.lat.origin) + c.lat.res * np.array(c.lat.dims))).all(axis=1)
        assert 0 < c.occ.sum() // 100 < c.lat.total and 0 < inside.sum() < n


def test_mask_cases_are_what_they_say():
    by = {k.name: k for k in MASKS}
    assert [len(by["masks/%d" % n].cloud) for n in (31, 32, 33, 64, 65)] == [31, 32, 33, 64, 65]
    assert by["masks/spare-words"].mask.shape[1] == 5 and len(by["masks/spare-words"].cloud) == 40
    b = by["masks/bits-beyond"]
    assert not np.array_equal(b.mask[0], b.mask[1]) and np.array_equal(b.known(0), b.known(1)) and np.array_equal(b.occ(0), b.occ(1)) and b.occ(0).any()
    s = by["masks/empty-and-shared"]
    assert not s.occ(1).any() and len(np.intersect1d(s.known(0), s.known(2))) == 8 and not np.array_equal(s.occ(0), s.occ(2))
    w = by["masks/nowhere-view"]
    assert len(w.known(1)) == 28 and not w.occ(1).any() and w.occ(0).any() and np.array_equal(w.occ(0), w.occ(2))
    for k in MASKS:                 # every random row sets bits beyond n_cloud in its last word, and no two views are equal
        if k.name.startswith("masks/") and k.name[6:].isdigit() and len(k.cloud) % 32:
            assert ((k.mask[:, len(k.cloud) // 32] >> np.uint32(len(k.cloud) % 32)) == (2 ** 32 - 1) >> (len(k.cloud) % 32)).all()
            assert len({k.occ(v).tobytes() for v in range(k.n_views)}) == k.n_views


# ---- the mutants ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", mm.MUTANTS)
def test_every_mutant_of_the_model_fails_a_case(mutant):
    failed = [c.name for c in CASES if not np.array_equal(mm.occupancy(*c.args(), mutant=mutant)[0], c.occ)]
    print("mutant %s fails %d of %d cases: %s" % (mutant, len(failed), len(CASES), ", ".join(failed[:6])))
    assert failed, mutant
    kinds = {n.split("/")[0] for n in failed}
    want = {"floor": "faces", "ties_even": "faces", "no_clamp": "near", "axis_clip": "corners", "wrap32": "far", "nan_cell0": "notfinite",
            "inf_saturates": "notfinite"}[mutant]
    assert want in kinds, (mutant, kinds)
    if mutant == "wrap32":      # the case that was made for it: a flat index of 2^32 + 26 comes back as cell (2, 3, 0)
        c = mc.case("far/wrap32")
        assert "far/wrap32" in failed and mm.occupancy(*c.args(), mutant=mutant)[0][0, 3, 2] == 100


# ---- the reference -------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture():
    """-> ({case: flat ids}, {lattice: origin}) as recorded (read once)"""
    with open(os.path.join(HERE, "golden", "map_read_ref.json")) as f:
        d = json.load(f)
    answers = [[i for first, count in runs for i in range(first, first + count)] for runs in d["answers"]]
    ids = {name: answers[k] for name, k in d["case"].items()}
    return ids, {name: [float.fromhex(h) for h in o] for name, o in d["origin"].items()}


REF_NAMES = [c.name for c in CASES if mc.in_reference_range(c, c.cloud32)]


def test_reference_range_holds_what_it_should():
    kinds = {n.split("/")[0] for n in REF_NAMES}
    assert {"faces", "corners", "near", "counts", "far"} <= kinds and "notfinite" not in kinds
    assert "far/wrap32" not in REF_NAMES and "far/cell/x+2147483647" not in REF_NAMES and "far/cell/z+1048576" in REF_NAMES
    assert sorted(fixture()[0]) == sorted(REF_NAMES)


@pytest.mark.parametrize("name", REF_NAMES)
def test_recorded_reference_equals_the_model(name):
    """readMap's own answer for the float32 cloud, as tests/golden/make_map_read_fixture.py recorded it: no reference needed"""
    c = mc.case(name)
    ids, origin = fixture()
    assert ids[name] == ids_of(mm.occupancy(*c.args(c.cloud32))[0]), name
    assert np.array_equal(origin[c.lat.name], c.lat.origin), (name, origin[c.lat.name], c.lat.origin)      # bit for bit


@pytest.fixture(scope="module")
def ref():
    from oracle.ref_frontend import ref as r

    if r.build() is None:
        pytest.skip("oracle/_ref/libref_frontend.so is not built and the reference's sources are not present")
    return r


@pytest.mark.parametrize("name", REF_NAMES)
def test_compiled_reference_equals_the_model_and_the_fixture(ref, name):
    c = mc.case(name)
    m = ref.Map(*c.args(c.cloud32))
    try:
        assert tuple(m.dims) == c.lat.dims
        assert np.array_equal(m.origin, c.lat.origin), (name, m.origin, c.lat.origin)      # bit for bit: the faces are decided there
        got = ids_of(m.occupancy())
    finally:
        m.close()
    assert got == ids_of(mm.occupancy(*c.args(c.cloud32))[0]) and got == fixture()[0][name], name


# ---- the long lattices of the jump-table saturation tests -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", mc.LONG)
@pytest.mark.parametrize("axis", range(3), ids=["x", "y", "z"])
def test_long_lattices_have_the_runs_they_claim_and_the_host_answers_them(axis, length):
    """The model's grid of every long scene: the row of the start is free from end to end (a straight run of `length` cells, length - 1
    steps to the face), the goal lies one row beside the far end (goal_on_ray does not answer), and in the `forced` scenes the one occupied
    cell lies beside the ray, outside the cubes freed around start and goal, length - 2 steps from the start.  The host's jump point search
    gives answers with the properties P1 - P4."""
    for end in mc.LONG_ENDS:
        for side in (0, 1):
            sc = mc.long_scene(axis, length, end, side)
            assert sc.dims == ((length, 3, 2), (3, length, 2), (3, 3, length))[axis] and len(sc.starts) == 1
            s, t = sc.cell(sc.starts[0]), sc.cell(sc.goals[0])
            line = [slice(None) if b == axis else s[b] for b in (2, 1, 0)]    # occ is [z][y][x]
            row = sc.occ[tuple(line)]
            assert row.shape == (length,) and not row.any() and s[axis] == (0, length - 1)[side]
            assert abs(t[axis] - s[axis]) == length - 1 and sorted(abs(t[b] - s[b]) for b in range(3) if b != axis) == [0, 1]
            z, y, x = np.nonzero(sc.occ)
            if end == "face":
                assert len(x) == 0
            else:
                o = (int(x[0]), int(y[0]), int(z[0]))
                assert len(x) == 1 and abs(o[axis] - s[axis]) == length - 2
                assert sorted(abs(o[b] - s[b]) for b in range(3) if b != axis) == [0, 1]                       # beside the ray
                assert max(abs(o[b] - t[b]) for b in range(3)) > sc.m_free and max(abs(o[b] - s[b]) for b in range(3)) > sc.m_free
            with frontend.host_settings("jps", 0.0):
                hp, hn, _ = frontend.plan_batch(*sc.map_args(), sc.starts, sc.goals, max_points=16)
            assert hn[0] >= 2
            pe.check_answer(sc, 0, hp[0], hn[0], "host jps")


def test_long_runs_lie_on_both_sides_of_the_saturation_threshold():
    """an entry becomes "not known" when the next one reaches +-32766: runs to the face of 32765 .. 32768 steps, to the forced cell of 32764 .. 32767"""
    assert mc.LONG == (32766, 32767, 32768, 32769)
    assert [n - 1 for n in mc.LONG] == [32765, 32766, 32767, 32768] and [n - 2 for n in mc.LONG] == [32764, 32765, 32766, 32767]
