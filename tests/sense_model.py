"""The sensor model of fh_fleet_sense_device (include/fasterhip.h) restated in numpy, operation for operation, for the tests that compare
the device's flags byte for byte.  Not a test file.

A voxel of the lattice with centre q = ((i + 0.5) res + origin) is in range of a vehicle at p when sqrt(dx dx + dy dy + dz dz) < r_sense
(d = q - p), and visible when none of the points p + (q - p) (j / K), j = 1 .. K - 1, K = max(1, ceil(|q - p| / (0.5 res_map))), lies in an
occupied cell of the map (cell of a point: floor((x - origin_map) / res_map); outside the map: free) other than the map cell q itself
lies in: an occupied cell is seen, what is behind it is not.  In range and visible: flag = 0."""
import numpy as np


def sense_one(view, p, r_sense, origin, res, occ, m_origin, m_res):
    """One vehicle at p looks around; `view` ([nz][ny][nx] uint8) is updated in place.  occ: [mz][my][mx], non-zero = occupied.
    Returns the number of cells in range that were unknown and stay unknown because something hides them."""
    p = np.asarray(p, dtype=np.float64)
    if not np.all(np.isfinite(p)):
        return 0
    nz, ny, nx = view.shape
    # a generous box around the sphere (what decides is the distance test below), clipped to the lattice
    lo = np.floor((p - r_sense - origin) / res) - 2
    hi = np.floor((p + r_sense - origin) / res) + 2
    lo = np.clip(lo, 0, [nx, ny, nz]).astype(np.int64)
    hi = np.clip(hi, -1, [nx - 1, ny - 1, nz - 1]).astype(np.int64)
    if np.any(hi < lo):
        return 0
    iz, iy, ix = np.meshgrid(np.arange(lo[2], hi[2] + 1), np.arange(lo[1], hi[1] + 1), np.arange(lo[0], hi[0] + 1), indexing="ij")
    ix, iy, iz = ix.ravel(), iy.ravel(), iz.ravel()
    dx = (ix + 0.5) * res + origin[0] - p[0]
    dy = (iy + 0.5) * res + origin[1] - p[1]
    dz = (iz + 0.5) * res + origin[2] - p[2]
    d = np.sqrt(dx * dx + dy * dy + dz * dz)
    pick = (d < r_sense) & (view[iz, iy, ix] != 0)   # (a voxel that is known already stays known: no ray needed)
    ix, iy, iz, dx, dy, dz, d = ix[pick], iy[pick], iz[pick], dx[pick], dy[pick], dz[pick], d[pick]
    K = np.maximum(1.0, np.ceil(d / (0.5 * m_res)))
    blocked = np.zeros(len(d), dtype=bool)
    mz, my, mx = occ.shape
    qfx = np.floor(((ix + 0.5) * res + origin[0] - m_origin[0]) / m_res)   # the map cell of q itself: not tested
    qfy = np.floor(((iy + 0.5) * res + origin[1] - m_origin[1]) / m_res)
    qfz = np.floor(((iz + 0.5) * res + origin[2] - m_origin[2]) / m_res)
    for j in range(1, int(K.max()) if len(K) else 1):
        live = np.nonzero((j < K) & ~blocked)[0]
        if not len(live):
            continue
        t = j / K[live]
        fx = np.floor((p[0] + dx[live] * t - m_origin[0]) / m_res)
        fy = np.floor((p[1] + dy[live] * t - m_origin[1]) / m_res)
        fz = np.floor((p[2] + dz[live] * t - m_origin[2]) / m_res)
        inside = (fx >= 0) & (fx < mx) & (fy >= 0) & (fy < my) & (fz >= 0) & (fz < mz)
        inside &= ~((fx == qfx[live]) & (fy == qfy[live]) & (fz == qfz[live]))
        hit = np.zeros(len(live), dtype=bool)
        hit[inside] = occ[fz[inside].astype(np.int64), fy[inside].astype(np.int64), fx[inside].astype(np.int64)] != 0
        blocked[live[hit]] = True
    view[iz[~blocked], iy[~blocked], ix[~blocked]] = 0
    return int(blocked.sum())


def sense(views, view_of, positions, r_sense, origin, res, occ, m_origin, m_res):
    """Every vehicle senses into views[view_of[i]] (view_of None: view i); views: [n_views][nz][ny][nx] uint8, updated in place.  The order
    of the vehicles does not matter: flags only ever go to zero, and skipping a flag that is zero already skips a ray whose only effect
    would be to store that zero again.  Returns the number of (vehicle, cell) pairs in range that stay unknown because they are hidden."""
    origin, m_origin = np.asarray(origin, dtype=np.float64), np.asarray(m_origin, dtype=np.float64)
    hidden = 0
    for i, p in enumerate(positions):
        v = i if view_of is None else int(view_of[i])
        if 0 <= v < len(views):
            hidden += sense_one(views[v], p, float(r_sense), origin, float(res), occ, m_origin, float(m_res))
    return hidden
