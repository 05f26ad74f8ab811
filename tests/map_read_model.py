"""The map read (MapUtil::readMap; fh_map_read_device, VoxelGrid::build) as its contract states it (include/fasterhip.h at
fh_map_read_device), one point at a time with Python floats (IEEE double, nothing contracted) and Python integers (exact, unbounded).
No numpy integer cast, no 32-bit or 64-bit index: what a conversion or an overflow could do to the device, the host restatement or the
reference cannot happen here.

For a point p:  v = round_half_away((p - origin) / res - 0.5) per axis; any v not finite: the point marks nothing; c = max(v, 0);
every offset (i, j, k) in [-m, m]^3, m = floor(inflation / res), gives id = (cx + i) + nx (cy + j) + nx ny (cz + k); the cell is marked
iff 0 <= id < nx ny nz.  No per-axis clipping.

The keyword `mutant` plants one wrong reading of that contract (MUTANTS); tests/test_map_read_edge_cases.py shows that the cases of
tests/map_read_edge_cases.py tell every one of them from the contract."""
import math

import numpy as np

import path_model   # (its own import of this module is inside path_model.occupancy)

MUTANTS = ("floor", "ties_even", "no_clamp", "axis_clip", "wrap32", "nan_cell0", "inf_saturates")
INT_MAX = 2 ** 31 - 1


def round_half_away(v):
    """C's round() of a finite double -> int.  math.trunc is exact and so is v - trunc(v)."""
    t = math.trunc(v)
    f = v - t
    return t + (1 if f >= 0.5 else (-1 if f <= -0.5 else 0))


def _round_even(v):
    t = math.floor(v)
    f = v - t
    return t + (1 if f > 0.5 or (f == 0.5 and t % 2 != 0) else 0)


def _wrap32(i):
    return (i + 2 ** 31) % 2 ** 32 - 2 ** 31


def lattice(cells, res, center, z_ground, z_max, inflation):
    """readMap's dimensions and origin (path_model.geometry: kept there, it is the lattice of every path test too)"""
    return path_model.geometry(cells, res, center, z_ground, z_max, inflation)


def cell_of(p, origin, res, mutant=None):
    """(cx, cy, cz) after the clamp, or None: the point marks nothing"""
    c = []
    for a in range(3):
        v = (float(p[a]) - float(origin[a])) / float(res) - 0.5
        if math.isnan(v):
            if mutant != "nan_cell0":
                return None
            c.append(0)
            continue
        if math.isinf(v):
            if mutant != "inf_saturates":
                return None
            c.append(INT_MAX if v > 0 else 0)   # a saturating conversion, then the clamp
            continue
        if mutant == "floor":
            k = math.floor(v)
        elif mutant == "ties_even":
            k = _round_even(v)
        else:
            k = round_half_away(v)
        c.append(k if mutant == "no_clamp" else max(k, 0))
    return tuple(c)


def marked_ids(cloud, dims, origin, res, inflation, mutant=None):
    """the flat ids that the cloud marks, as a sorted list of Python integers"""
    assert mutant is None or mutant in MUTANTS, mutant
    nx, ny, nz = (int(d) for d in dims)
    total = nx * ny * nz
    m = int(math.floor(inflation / res))
    cells = set()
    for p in np.asarray(cloud, dtype=np.float64).reshape(-1, 3).tolist():
        c = cell_of(p, origin, res, mutant)
        if c is not None:
            cells.add(c)
    ids = set()
    for cx, cy, cz in cells:
        for k in range(cz - m, cz + m + 1):
            for j in range(cy - m, cy + m + 1):
                if mutant == "axis_clip":
                    if 0 <= j < ny and 0 <= k < nz:
                        ids.update(i + nx * j + nx * ny * k for i in range(max(cx - m, 0), min(cx + m, nx - 1) + 1))
                    continue
                first = (cx - m) + nx * j + nx * ny * k   # the ids of one x run are consecutive
                if mutant == "wrap32":
                    ids.update(w for w in (_wrap32(first + i) for i in range(2 * m + 1)) if 0 <= w < total)
                else:
                    ids.update(range(max(first, 0), min(first + 2 * m + 1, total)))
    return sorted(ids)


def occupancy(cloud, cells, res, center, z_ground, z_max, inflation, mutant=None):
    """-> (occ [nz][ny][nx] int8 (0 free, 100 occupied), dims, origin)"""
    (nx, ny, nz), origin = lattice(cells, res, center, z_ground, z_max, inflation)
    occ = np.zeros(nx * ny * nz, dtype=np.int8)
    ids = marked_ids(cloud, (nx, ny, nz), origin, res, inflation, mutant)
    if ids:
        occ[np.array(ids, dtype=np.int64)] = 100
    return occ.reshape(nz, ny, nx), (nx, ny, nz), origin
