"""The map read on the device (mark_kernel, mark_views_kernel, mark_views_listed_kernel and the jump tables built from their grids) at its
rounding, wrap, range, count and mask edges, at the launch split at 32768 views and at the saturation of the jump tables.

Every case of tests/map_read_edge_cases.py goes through every entry point (Map.read, read_device, read_views_device,
read_views_listed_device) and the grid that comes back equals the model of tests/map_read_model.py cell for cell; why each case means
something, and that the model is the contract, is asserted on the CPU in tests/test_map_read_edge_cases.py.  The searches are compared
with the host restatement bit for bit (assert_p5 of tests/test_gpu_path_edges.py).  No tolerance anywhere."""
import numpy as np
import pytest
import torch  # noqa: F401  (before libfasterhip.so is loaded: one HIP runtime per process)

import frontier_model as fm
import map_read_edge_cases as mc
import map_read_model as mm
import path_edge_cases as pe
import test_gpu_path_edges as tp
from faster_amd import abi, capi, frontend

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KINDS = ["faces", "corners", "near", "far", "notfinite", "counts"]
ENTRIES = ["read", "read_device", "read_views_device", "read_views_listed_device"]


@pytest.fixture(scope="module", autouse=True)
def built():
    from faster_amd import build as fb

    fb.build_frontend()


@pytest.fixture(scope="module")
def m():
    vmap = capi.Map(0)
    yield vmap
    vmap.close()


@pytest.fixture(scope="module")
def ms():
    """one wavefront per CU: per-cell records of the long lattices for every wavefront of the default would be gigabytes of memset per map"""
    vmap = capi.Map(0)
    vmap.set_sched(waves_per_cu=1)
    yield vmap
    vmap.close()


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def ids_of(occ):
    return np.flatnonzero(occ.reshape(-1)).tolist()


def same_grid(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), (what, ids_of(got)[:12], ids_of(want)[:12])


def mask_rows(n_cloud, rows, words=None):
    """[len(rows)][words] uint32 from lists of point indices; the bits of the last word beyond n_cloud are SET (they mean nothing)"""
    words = max((n_cloud + 31) // 32, 1) if words is None else words
    out = np.zeros((len(rows), words), dtype=np.uint32)
    for v, idx in enumerate(rows):
        for i in idx:
            out[v, i >> 5] |= np.uint32(1 << (i & 31))
    if n_cloud % 32:
        out[:, n_cloud // 32] |= np.uint32(((1 << 32) - 1) >> (n_cloud % 32) << (n_cloud % 32))
    return out


_SUB = {}


def model_of(c, idx, key):
    """the model's grid of a part of the cloud of a case (computed once)"""
    if (c.name, key) not in _SUB:
        _SUB[(c.name, key)] = mm.occupancy(*c.args(c.cloud[idx]))[0] if len(idx) else np.zeros_like(c.occ)
    return _SUB[(c.name, key)]


def lattice_is(vmap, lat):
    dims, origin = vmap.dims()
    assert tuple(int(d) for d in dims) == lat.dims and np.array_equal(origin, lat.origin)


def read_views(vmap, lat, d_cloud, n_cloud, mask, listed=None):
    d_mask = to_dev(mask.view(np.int32))
    args = (ptr(d_cloud), n_cloud, d_mask.data_ptr() if n_cloud else None, mask.shape[1], mask.shape[0], lat.cells, lat.res, lat.center, lat.z_ground,
            lat.z_max, lat.inflation)
    if listed is None:
        vmap.read_views_device(*args)
    else:
        d_list = to_dev(np.array(listed + [-1] * (mask.shape[0] - len(listed)), dtype=np.int32))
        d_count = to_dev(np.array([len(listed)], dtype=np.int32))
        vmap.read_views_listed_device(*args, d_list.data_ptr(), d_count.data_ptr())
    vmap.sync()


# ---- every case through every entry point --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("kind", KINDS)
def test_every_case_through_every_entry_point(m, kind, entry):
    """The grid of the map (Map.read, read_device) and of three views (read_views_device: every point, none, the points with odd numbers)
    equals the model of the same points.  read_views_listed_device after a full read in which every view knew every point, with other masks
    (0: none, 1: the odd points, 2: the even points) and the list [0, 2]: views 0 and 2 are the model of their new points, view 1 is byte for
    byte what it was."""
    cases = [c for c in mc.cases() if c.name.split("/")[0] == kind]
    assert cases
    for c in cases:
        n = len(c.cloud)
        every, odd, even = np.arange(n), np.arange(1, n, 2), np.arange(0, n, 2)
        d_cloud = to_dev(c.cloud) if n else None
        if entry == "read":
            m.read(*c.args())
            lattice_is(m, c.lat)
            same_grid(m.occupancy(), c.occ, (c.name, entry))
            continue
        m.read_device(ptr(d_cloud), n, c.lat.cells, c.lat.res, c.lat.center, c.lat.z_ground, c.lat.z_max, c.lat.inflation)
        m.sync()
        lattice_is(m, c.lat)
        if entry == "read_device":
            same_grid(m.occupancy(), c.occ, (c.name, entry))
        elif entry == "read_views_device":
            read_views(m, c.lat, d_cloud, n, mask_rows(n, [every, [], odd]))
            same_grid(m.view_occupancy(0), c.occ, (c.name, entry, "every point"))
            assert not m.view_occupancy(1).any(), (c.name, entry, "no point")
            same_grid(m.view_occupancy(2), model_of(c, odd, "odd"), (c.name, entry, "odd points"))
        else:
            read_views(m, c.lat, d_cloud, n, mask_rows(n, [every, every, every]))
            before = m.view_occupancy(1).tobytes()
            assert before == c.occ.tobytes()
            read_views(m, c.lat, d_cloud, n, mask_rows(n, [[], odd, even]), listed=[0, 2])
            assert not m.view_occupancy(0).any(), (c.name, entry, "no point")
            assert m.view_occupancy(1).tobytes() == before, (c.name, entry, "the view that is not listed")
            same_grid(m.view_occupancy(2), model_of(c, even, "even"), (c.name, entry, "even points"))


@pytest.mark.parametrize("k", range(len(mc.mask_cases())), ids=[k.name for k in mc.mask_cases()])
def test_mask_cases_through_both_view_entry_points(m, k):
    """Word boundaries of the mask, spare words, bits beyond n_cloud, an empty row, shared points, a view of far and non-finite points only:
    every view equals the model of the points it knows.  Then a full read under the complement of the mask and a listed read of the first
    and the last view under the mask itself: those two equal the model, the views between keep the complement's grid byte for byte."""
    mk = mc.mask_cases()[k]
    n = len(mk.cloud)
    d_cloud = to_dev(mk.cloud)
    m.read_device(ptr(d_cloud), n, mk.lat.cells, mk.lat.res, mk.lat.center, mk.lat.z_ground, mk.lat.z_max, mk.lat.inflation)
    lattice_is(m, mk.lat)
    read_views(m, mk.lat, d_cloud, n, mk.mask)
    for v in range(mk.n_views):
        same_grid(m.view_occupancy(v), mk.occ(v), (mk.name, v))
    read_views(m, mk.lat, d_cloud, n, ~mk.mask)
    before = [m.view_occupancy(v).tobytes() for v in range(mk.n_views)]
    last = mk.n_views - 1
    read_views(m, mk.lat, d_cloud, n, mk.mask, listed=[0, last])
    for v in range(mk.n_views):
        if v in (0, last):
            same_grid(m.view_occupancy(v), mk.occ(v), (mk.name, "listed", v))
        else:
            assert m.view_occupancy(v).tobytes() == before[v], (mk.name, "not listed", v)


# ---- the launch split at 32768 views ---------------------------------------------------------------------------------------------------------------------
N_VIEWS = 32769


class Split:
    """32769 views of a 6 x 4 x 2 lattice.  View 32768 (the first view of the second launch) knows a wall with a gap, view 32767 (the last
    of the first launch) three other points, every other view nothing."""

    def __init__(self):
        wall = np.zeros((2, 4, 6), dtype=bool)
        wall[:, :, 3] = True
        wall[1, 0, 3] = False                    # the gap
        other = np.zeros((2, 4, 6), dtype=bool)
        other[0, 1, 1] = other[1, 2, 4] = other[0, 3, 2] = True
        starts, goals = pe.centres([(0, 2, 0), (0, 0, 1)]), pe.centres([(5, 2, 0), (5, 3, 0)])
        self.wall, self.other = pe.Scene("split wall", wall, starts, goals), pe.Scene("split other", other, starts, goals)
        self.empty = pe.Scene("split empty", np.zeros((2, 4, 6), dtype=bool), starts, goals)
        assert self.wall.dims == (6, 4, 2) and self.other.dims == self.wall.dims and np.array_equal(self.other.origin, self.wall.origin)
        self.cloud = np.vstack([self.wall.cloud, self.other.cloud])
        nw, n = len(self.wall.cloud), len(self.cloud)
        assert (nw, n) == (7, 10)
        self.mask = np.zeros((N_VIEWS, 1), dtype=np.uint32)
        self.mask[32768, 0] = (1 << nw) - 1
        self.mask[32767, 0] = ((1 << n) - 1) ^ ((1 << nw) - 1)


@pytest.fixture(scope="module")
def split():
    return Split()


@pytest.fixture(scope="module")
def split_map(split):
    """a map with the 32769 grids read (once, shared and left unchanged by the tests that use it)"""
    vmap = capi.Map(0)
    vmap.set_sched(waves_per_cu=1)
    vmap.set_search("jps")
    vmap.set_records(0)
    sc = split.wall
    vmap.read(*sc.map_args())       # the map itself: the wall (the lattice of the views is the map's)
    read_views(vmap, mc.Lattice("split", sc.cells, pe.RES, sc.center, sc.z_ground, sc.z_max, sc.inflation), to_dev(split.cloud), len(split.cloud), split.mask)
    yield vmap
    vmap.close()


def test_split_views_on_either_side_of_the_launch_boundary_have_their_own_grid(split, split_map):
    for v, sc in ((0, split.empty), (1, split.empty), (32766, split.empty), (32767, split.other), (32768, split.wall)):
        same_grid(split_map.view_occupancy(v), sc.occ, ("view", v))
    assert split.wall.occ.any() and split.other.occ.any() and not np.array_equal(split.wall.occ, split.other.occ)


def test_split_searches_read_the_grid_and_the_jump_tables_of_their_view(split, split_map):
    """jump point searches in views 32768, 32767 and 0 (the view tables are built in launches of 32768 views too): what the host restatement
    gives on the cloud of that view, bit for bit; the wall makes the answers differ"""
    nq = len(split.wall.starts)
    answers = []
    for v, sc in ((32768, split.wall), (32767, split.other), (0, split.empty)):
        dev = tp.plan(split_map, sc.starts, sc.goals, entry="views", view_of=[v] * nq, n_views=N_VIEWS)
        hst = tp.host(sc, "jps", max_points=16)
        tp.assert_p5(dev, hst, ("view", v))
        for q in range(nq):
            pe.check_answer(sc, q, dev[0][q], dev[1][q], ("view", v))
        answers.append(hst[0][:, :4].tobytes() + hst[1].tobytes())
    assert answers[0] != answers[2]
    mixed = tp.plan(split_map, split.wall.starts, split.wall.goals, entry="views", view_of=[32768, 0], n_views=N_VIEWS)   # one launch, both sides
    for q, sc in enumerate((split.wall, split.empty)):
        hst = tp.host(sc, "jps", max_points=16)
        tp.assert_p5(tuple(a[q:q + 1] for a in mixed[:3]), tuple(a[q:q + 1] for a in hst[:3]), ("mixed", q))


def test_split_view_coverage_over_32769_flag_rows(split_map):
    """fh_map_view_coverage_device splits its launches at 32768 views as well: rows 32767 and 32768 differ from each other and from the rest"""
    dims, stride = (6, 4, 2), 48 + 3
    rng = np.random.default_rng(7)
    flags = np.ones((N_VIEWS, stride), dtype=np.uint8)          # unknown everywhere (and in the gap bytes)
    flags[::1000, :48] = 0                                      # some views know everything
    flags[32767, :48] = rng.integers(0, 2, 48)
    flags[32768, :48] = rng.integers(0, 2, 48)
    flags[32766, :20] = 0
    rows, inverse = np.unique(flags, axis=0, return_inverse=True)       # (the model once per distinct row)
    want = fm.view_coverage(rows.reshape(-1), len(rows), stride, dims)[inverse.reshape(-1)]
    assert want[32767] != want[32768] and want["frontier"][32768] > 0 and want["known"][32766] == 20 and want["known"][1] == 0
    d_f = to_dev(flags.reshape(-1))
    out = torch.full((16 * (N_VIEWS + 2),), 0xA5, dtype=torch.uint8, device=DEV)
    grid = (np.zeros(3), 0.25, dims)
    split_map.view_coverage_device(grid, d_f.data_ptr(), stride, N_VIEWS, out.data_ptr() + 16)
    split_map.sync()
    h = out.cpu().numpy()
    assert (h[:16] == 0xA5).all() and (h[-16:] == 0xA5).all()
    got = h[16:-16].view(abi.view_coverage_dtype)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (bad[:8], got[bad[:8]], want[bad[:8]])


# ---- the saturation of the jump tables -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", mc.LONG)
@pytest.mark.parametrize("axis", range(3), ids=["x", "y", "z"])
def test_jump_tables_saturate_where_a_free_run_is_longer_than_a_short_holds(ms, axis, length):
    """A free straight run of 32766 .. 32769 cells, ended by the lattice face (negative entries) or by a forced neighbour one cell before it
    (positive entries), searched from either end with per-cell and with hashed records: n_points, expansions and vertices equal the host
    restatement's bit for bit (the host walks every jump and has no tables)."""
    for end in mc.LONG_ENDS:
        for side in (0, 1):
            sc = mc.long_scene(axis, length, end, side)
            with frontend.host_settings("jps", 0.0):
                hst = frontend.plan_batch(*sc.map_args(), sc.starts, sc.goals, max_points=16)
            assert hst[1][0] >= 2
            for records in (0, 1024):
                tp.read(ms, sc, "jps", records)
                if records == 0:
                    same_grid(ms.occupancy(), sc.occ, sc.name)
                dev = tp.plan(ms, sc.starts, sc.goals)
                tp.assert_p5(dev, hst, (sc.name, records))
