"""Clouds for the map read at its rounding, wrap, range and count edges (tests/test_gpu_map_read_edges.py on the device,
tests/test_map_read_edge_cases.py on the CPU, where every case's reason to exist is asserted against tests/map_read_model.py and the
planted mutants of that model are shown to fail).

A case is one lattice and one cloud.  Where the contract (include/fasterhip.h at fh_map_read_device) can be said in other words than
the model's, the case carries what it expects: `ids`, the flat ids that must be marked, from `carried` (the cube of a cell by carrying
x into the rows and y into the layers, no flat index anywhere) or written out by hand.  The binary lattices have res 0.5 and origins
that are multiples of it: faces, centres and every neighbour of a face are exact doubles, a case means what it says.  On the decimal
lattice (res 0.15, a centre that is no multiple of it) the rounding of the double expression decides, and only the comparisons with the
host restatement and the compiled reference say what is right."""
import functools
import itertools
import math

import numpy as np

import map_read_model as mm

INT_MAX = 2 ** 31 - 1


class Lattice:
    def __init__(self, name, cells, res, center, z_ground, z_max, inflation):
        self.name, self.cells, self.res, self.center = name, tuple(cells), float(res), np.array(center, dtype=np.float64)
        self.z_ground, self.z_max, self.inflation = float(z_ground), float(z_max), float(inflation)
        self.dims, self.origin = mm.lattice(self.cells, self.res, self.center, self.z_ground, self.z_max, self.inflation)
        self.total = self.dims[0] * self.dims[1] * self.dims[2]
        self.m = int(math.floor(self.inflation / self.res))

    def args(self, cloud):
        return np.asarray(cloud, dtype=np.float64).reshape(-1, 3), self.cells, self.res, self.center, self.z_ground, self.z_max, self.inflation

    def face(self, axis, k):
        """the coordinate of cell boundary k of an axis, as the double expression gives it"""
        return float(self.origin[axis]) + k * self.res

    def centre(self, c):
        return [float(self.origin[a]) + (c[a] + 0.5) * self.res for a in range(3)]

    @property
    def mid(self):
        return tuple(d // 2 for d in self.dims)


def binary(inflation, cells=(8, 6, 4)):
    lat = Lattice("bin%dx%dx%d/m%d" % (cells + (int(inflation / 0.5),)), cells, 0.5, (0.0, 0.0, 1.0), 0.0, 50.0, inflation)
    k = int(5 * inflation / 0.5)
    assert lat.dims == (cells[0] + k, cells[1] + k, 4) and np.array_equal(lat.origin, [-(cells[0] + k) / 4.0, -(cells[1] + k) / 4.0, 0.0]), (lat.dims, lat.origin)
    return lat


BIN = [binary(0.0), binary(0.5), binary(1.0)]                     # m = 0, 1, 2; 8 x 6 x 4, 13 x 11 x 4, 18 x 16 x 4
assert BIN[0].dims == (8, 6, 4) and np.array_equal(BIN[0].origin, [-2.0, -1.5, 0.0]) and [b.m for b in BIN] == [0, 1, 2]
WRAP = binary(0.0, cells=(8, 8, 4))                               # nx ny = 64 = 2^6: cell z = 2^26 is flat index 2^32
DEC = Lattice("dec", (9, 7, 20), 0.15, (0.37, -1.21, 1.3), 0.4, 2.2, 0.3)


class Case:
    def __init__(self, name, lat, cloud, ids=None, says=""):
        self.name, self.lat, self.says = name, lat, says
        self.cloud = np.array(cloud, dtype=np.float64).reshape(-1, 3)
        self.ids = None if ids is None else sorted(ids)   # what the case expects, in words other than the model's (None: no such words)

    def args(self, cloud=None):
        return self.lat.args(self.cloud if cloud is None else cloud)

    @functools.cached_property
    def occ(self):
        """the model's grid (computed once and shared by every test that needs it)"""
        return mm.occupancy(*self.args())[0]

    @functools.cached_property
    def cloud32(self):
        """the cloud as a pcl::PointXYZ holds it"""
        with np.errstate(over="ignore"):   # (1e300 becomes inf: outside the reference's range)
            return self.cloud.astype(np.float32).astype(np.float64)


def carried(lat, c):
    """The cube of +-m cells around cell c as the contract's words give it, with no flat index: a cell beyond an x face comes back on the
    next (or the previous) row, a row beyond a y face on the next (previous) layer, a layer outside the lattice is nothing."""
    nx, ny, nz = lat.dims
    out = set()
    for i, j, k in itertools.product(range(-lat.m, lat.m + 1), repeat=3):
        x, y, z = c[0] + i, c[1] + j, c[2] + k
        y, x = y + x // nx, x % nx
        z, y = z + y // ny, y % ny
        if 0 <= z < nz:
            out.add(x + nx * (y + ny * z))
    return out


def exact_cell(p, origin, res):
    """The cell of a finite point from exact rationals: every operation of v = (p - origin) / res - 0.5 is carried out exactly and then
    rounded once to the nearest double (float(Fraction) rounds correctly, ties to even), which is what IEEE arithmetic without contraction
    means; the halves are told from the rest exactly.  Shares no floating-point operation with the model."""
    from fractions import Fraction as F

    c = []
    for a in range(3):
        d = float(F(float(p[a])) - F(float(origin[a])))
        q = float(F(d) / F(float(res)))
        v = F(float(F(q) - F(1, 2)))
        k = int(abs(v) + F(1, 2)) * (1 if v >= 0 else -1)     # halves away from zero
        c.append(max(k, 0))
    return tuple(c)


def in_reference_range(case, cloud):
    """The reference's readMap has defined behaviour for this cloud: every conversion to int and every int sum and product fits 32 bits."""
    nx, ny, nz = case.lat.dims
    m = case.lat.m
    for p in np.asarray(cloud).reshape(-1, 3).tolist():
        c = []
        for a in range(3):
            v = (p[a] - float(case.lat.origin[a])) / case.lat.res - 0.5
            if not math.isfinite(v) or not -2 ** 31 <= mm.round_half_away(v) <= INT_MAX:
                return False
            c.append(max(mm.round_half_away(v), 0))
        for s in (-m, m):
            t = (c[0] + s, nx * (c[1] + s), nx * ny * (c[2] + s))
            if any(abs(w) > INT_MAX for w in (c[0] + s, c[1] + s, c[2] + s, t[0], t[1], t[2], t[0] + t[1], t[0] + t[1] + t[2])):
                return False
    return True


# ---- faces -------------------------------------------------------------------------------------------------------------------------------------
def _faces():
    """For every axis and every cell boundary k = 0 .. n three clouds of one point each: the point on the boundary and its two neighbours
    in double (`below`, `on`, `above`); the other two coordinates are those of the centre of the middle cell.  One point per cloud, so that
    the cell of every one of them is pinned by itself.  Expected: the cube of the cell that exact_cell gives.  Binary lattices: the
    boundary itself belongs to the cell above it (v = k - 0.5 rounds away from zero; k = 0 gives -1, clamped); the neighbour below belongs
    to cell k - 1 unless p - origin already rounds it onto the boundary (where the origin is larger than the coordinate)."""
    out = []
    for lat in BIN + [DEC]:
        for a in range(3):
            for k in range(lat.dims[a] + 1):
                f = lat.face(a, k)
                for word, x in (("below", np.nextafter(f, -np.inf)), ("on", f), ("above", np.nextafter(f, np.inf))):
                    p = lat.centre(lat.mid)
                    p[a] = float(x)
                    out.append(Case("faces/%s/%s%d/%s" % (lat.name, "xyz"[a], k, word), lat, [p], carried(lat, exact_cell(p, lat.origin, lat.res)),
                                    "%s boundary %d of axis %d" % (word, k, a)))
    return out


# ---- corners -----------------------------------------------------------------------------------------------------------------------------------
# the cube of corner cell (0, 0, 0) and of corner cell (12, 10, 3) of the 13 x 11 x 4 lattice (m = 1), worked out by hand: (x, y, z) of every
# marked cell.  Of the 27 cube cells of (0, 0, 0) 8 are inside; 6 of the 9 with x = -1 come back as x = 12 of the row before (those of row
# y = -1, z = 0 lie before the map), and the 6 of row y = -1, z = 1 come back as row 10 of layer 0 (x = -1 of that row: x = 12 of row 9).
HAND = {
    ("bin8x6x4/m1", (0, 0, 0)): [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1), (1, 1, 1),
                                 (12, 0, 0), (12, 9, 0), (12, 10, 0), (12, 0, 1),
                                 (0, 10, 0), (1, 10, 0)],
    # (12, 10, 3): 8 inside; x = 13 comes back as x = 0 of the next row: rows 10, 11 -> (0, 10), and row 11 is row 0 of the next layer; layer
    # 4 is outside.  Rows y = 11 of layer 2: row 0 of layer 3.
    ("bin8x6x4/m1", (12, 10, 3)): [(11, 9, 2), (12, 9, 2), (11, 10, 2), (12, 10, 2), (11, 9, 3), (12, 9, 3), (11, 10, 3), (12, 10, 3),
                                   (0, 10, 2), (0, 10, 3), (0, 0, 3), (0, 1, 3),
                                   (11, 0, 3), (12, 0, 3)],
}


def border_cells(lat):
    """the 8 corner cells, one cell in the middle of each of the 12 edges and of the 6 faces"""
    out = []
    for pick in itertools.product((0, 1, 2), repeat=3):     # 0: low face, 1: the middle, 2: high face
        if pick == (1, 1, 1):
            continue
        out.append(tuple((0, lat.dims[a] // 2, lat.dims[a] - 1)[pick[a]] for a in range(3)))
    return out


def _corners():
    out = []
    for lat in BIN:
        for c in border_cells(lat):
            ids = carried(lat, c)
            if (lat.name, c) in HAND:
                nx, ny, _ = lat.dims
                hand = {x + nx * (y + ny * z) for x, y, z in HAND[(lat.name, c)]}
                assert hand == ids, (lat.name, c, sorted(hand ^ ids))
            out.append(Case("corners/%s/%d.%d.%d" % ((lat.name,) + c), lat, [lat.centre(c)], ids, "the cube of a border cell, clipped and wrapped"))
    return out


# ---- near outside -------------------------------------------------------------------------------------------------------------------------------
def _near():
    """Cells -1, -m - 1, n, n + m and n + m + 1 of every axis, the other two in the middle.  Below the lattice: clamped to the low face (the
    cube of cell 0).  Beyond the high x face: the next row; beyond the high y face: the next layer; beyond the high z face by more than m:
    nothing."""
    out = []
    for lat in BIN:
        for a in range(3):
            n = lat.dims[a]
            for ca in dict.fromkeys((-1, -lat.m - 1, n, n + lat.m, n + lat.m + 1)):   # (m = 0: three positions)
                c = list(lat.mid)
                c[a] = ca
                seen = list(c)
                seen[a] = max(ca, 0)
                out.append(Case("near/%s/%s%+d" % (lat.name, "xyz"[a], ca), lat, [lat.centre(c)], carried(lat, seen),
                                "low: the cube of cell 0" if ca < 0 else "high: wrapped, or nothing"))
    return out


# ---- far ------------------------------------------------------------------------------------------------------------------------------------------
def _far():
    """One point each.  A point far beyond a high face marks nothing; a finite point far below a low face is clamped like any other
    (contract 3) and marks the cell of the low face."""
    lat = BIN[0]
    out = []
    for a in range(3):
        for ca in (2 ** 20, 2 ** 31 - 1, 2 ** 31, 2 ** 40):
            for s in (1, -1):
                c = list(lat.mid)
                c[a] = s * ca
                p = lat.centre(c)
                assert (p[a] - float(lat.origin[a])) / lat.res - 0.5 == s * ca      # the cell coordinate is exact
                seen = list(lat.mid)
                seen[a] = 0
                out.append(Case("far/cell/%s%+d" % ("xyz"[a], s * ca), lat, [p], set() if s > 0 else carried(lat, seen), "far cell"))
        for x in (1e15, 1e300, -1e300):
            p = lat.centre(lat.mid)
            p[a] = x
            seen = list(lat.mid)
            seen[a] = 0
            out.append(Case("far/coord/%s%+.0e" % ("xyz"[a], x), lat, [p], set() if x > 0 else carried(lat, seen), "far coordinate"))
    # the z cell whose flat index is 2^32 + (2 + 8 * 3): a 32-bit index comes back as cell (2, 3, 0)
    nx, ny, _ = WRAP.dims
    assert nx * ny == 64
    out.append(Case("far/wrap32", WRAP, [WRAP.centre((2, 3, 2 ** 32 // (nx * ny)))], set(), "flat index 2^32 + 26"))
    return out


# ---- not finite -----------------------------------------------------------------------------------------------------------------------------------
def _not_finite():
    out = []
    for lat in (BIN[0], BIN[1]):
        for a in range(3):
            for x, word in ((np.nan, "nan"), (np.inf, "+inf"), (-np.inf, "-inf")):
                p = lat.centre(lat.mid)
                p[a] = x
                out.append(Case("notfinite/%s/%s%s" % (lat.name, "xyz"[a], word), lat, [p], set(), "marks nothing"))
    return out


# ---- counts -----------------------------------------------------------------------------------------------------------------------------------------
def scatter(lat, n, seed):
    """n points in and a little around the window (a tenth of them beyond a face)"""
    rng = np.random.default_rng(seed)
    lo = np.asarray(lat.origin) - 0.1 * lat.res * np.array(lat.dims)
    hi = np.asarray(lat.origin) + 1.1 * lat.res * np.array(lat.dims)
    return rng.uniform(lo, hi, (n, 3))


def _counts():
    lat = BIN[0]      # (m = 0: a few hundred points leave about half of the 384 cells free)
    out = [Case("counts/%d" % n, lat, scatter(lat, n, 100 + n), set() if n == 0 else None, "%d points" % n) for n in (0, 1, 255, 256, 257)]
    out.append(Case("counts/300-copies", lat, [lat.centre((3, 5, 1))] * 300, carried(lat, (3, 5, 1)), "300 copies of one point"))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = _faces() + _corners() + _near() + _far() + _not_finite() + _counts()
    assert len({c.name for c in out}) == len(out)
    return out


def case(name):
    return next(c for c in cases() if c.name == name)


def nowhere_cloud():
    """every far point beyond a high face and every point that is not finite, in one cloud: it marks nothing"""
    return np.vstack([c.cloud for c in cases() if (c.name.startswith("far/") or c.name.startswith("notfinite/bin8x6x4/m0")) and not c.ids])


# ---- masks (the view entry points) ------------------------------------------------------------------------------------------------------------------
class MaskCase:
    """A cloud and the rows of a point mask [n_views][words] uint32 (bit i & 31 of word i >> 5: view knows point i)."""

    def __init__(self, name, lat, cloud, mask, says=""):
        self.name, self.lat, self.says = name, lat, says
        self.cloud = np.array(cloud, dtype=np.float64).reshape(-1, 3)
        self.mask = np.ascontiguousarray(mask, dtype=np.uint32)
        assert self.mask.ndim == 2 and self.mask.shape[1] * 32 >= len(self.cloud)

    @property
    def n_views(self):
        return self.mask.shape[0]

    def known(self, v):
        """the indices of the points that view v knows: bits at and beyond n_cloud mean nothing"""
        i = np.arange(len(self.cloud))
        return i[((self.mask[v, i >> 5] >> (i & 31).astype(np.uint32)) & 1).astype(bool)] if len(i) else i

    @functools.lru_cache(maxsize=None)
    def occ(self, v):
        return mm.occupancy(*self.lat.args(self.cloud[self.known(v)]))[0]


def _rows(n_views, words, n_cloud, seed):
    rows = np.random.default_rng(seed).integers(0, 2 ** 32, (n_views, words), dtype=np.uint64)
    if n_cloud % 32:
        rows[:, n_cloud // 32] |= (2 ** 32 - 1) >> (n_cloud % 32) << (n_cloud % 32)     # every bit of that word beyond the cloud is set
    return rows.astype(np.uint32)


@functools.lru_cache(maxsize=None)
def mask_cases():
    lat = BIN[0]
    out = []
    for n in (31, 32, 33, 64, 65):   # random rows; the bits of the last word beyond n are set at random too
        out.append(MaskCase("masks/%d" % n, lat, scatter(lat, n, 200 + n), _rows(3, (n + 31) // 32, n, 300 + n), "%d points, the word boundary" % n))
    out.append(MaskCase("masks/spare-words", lat, scatter(lat, 40, 240), _rows(3, 5, 40, 340), "5 mask words for 40 points"))
    beyond = np.zeros((2, 2), dtype=np.uint32)
    beyond[0] = (0x00000005, 0)                 # view 0: points 0 and 2
    beyond[1] = (0xfffffc05, 0xffffffff)        # view 1: the same two, and every bit from 10 on (the cloud has 10 points)
    out.append(MaskCase("masks/bits-beyond", lat, scatter(lat, 10, 241), beyond, "bits beyond n_cloud are ignored: two equal views"))
    shared = np.zeros((3, 1), dtype=np.uint32)
    shared[0, 0], shared[2, 0] = 0x0000ffff, 0x00ffff00        # view 1 has an empty row; views 0 and 2 share points 8 .. 15
    out.append(MaskCase("masks/empty-and-shared", lat, scatter(lat, 24, 242), shared, "an empty row, two views that share points"))
    both = np.vstack([scatter(lat, 20, 243), nowhere_cloud()])            # view 0: the 20 points inside; view 1: only far and non-finite points; view 2: all
    rows = np.zeros((3, 2), dtype=np.uint32)
    for i in range(len(both)):
        for v in ((0, 2) if i < 20 else (1, 2)):
            rows[v, i >> 5] |= np.uint32(1 << (i & 31))
    out.append(MaskCase("masks/nowhere-view", lat, both, rows, "a view that holds only far and non-finite points is empty"))
    return out


# ---- long lattices: the saturation of the jump tables --------------------------------------------------------------------------------------------
# jps_table_lines stores a jump as a short and turns an entry into 0 ("not known") when the next one reaches +-32766: only a free straight
# run of that many cells gets there.  L x 3 x 2, 3 x L x 2 and 3 x 3 x L cells, the row (column) through the middle free from end to end.
LONG = (32766, 32767, 32768, 32769)
LONG_ENDS = ("face", "forced")


@functools.lru_cache(maxsize=4)
def long_scene(axis, length, end, side):
    """One query along the long axis, from its low end (side 0) or its high end (side 1), to the cell one row beside the far end.
    end = "face": nothing is occupied, the run ends at the lattice face (negative table entries); "forced": one occupied cell beside the ray,
    on the other side than the goal and one cell before the far end: a forced neighbour length - 2 steps from the start (positive entries)."""
    import path_edge_cases as pe

    dims = [3, 3, 2]
    dims[axis] = length
    nx, ny, nz = dims
    pattern = np.zeros((nz, ny, nx), dtype=bool)
    other = 0 if axis != 0 else 1                     # the axis along which goal and obstacle lie beside the ray
    s = [1, 1, 0]
    far = length - 1 if side == 0 else 0
    s[axis] = length - 1 - far
    t = list(s)
    t[axis], t[other] = far, s[other] + 1
    if end == "forced":
        o = list(s)
        o[axis], o[other] = (far - 1 if side == 0 else far + 1), s[other] - 1
        pattern[o[2], o[1], o[0]] = True
    return pe.Scene("long %s%d %s %d" % ("xyz"[axis], length, end, side), pattern, pe.centres([s]), pe.centres([t]))
