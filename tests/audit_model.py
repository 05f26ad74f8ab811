"""The audit of committed plans (include/fasterhip_audit.h) restated in numpy: brute force over the candidates a generous prefilter
(cap + 2 res around the tested positions) leaves, then the exact test d2 < cap * cap.  Everything is IEEE double and numpy fuses no
multiply-add, so `audit()` is what the device must return bit for bit.  `variant` names one deliberate mistake (tests/test_audit_model.py
shows which hand case each one changes); None is the model."""
import numpy as np

from faster_amd import abi

VARIANTS = ("le", "corner", "last_on_ties", "floor_n_tested", "mask_word_64")
INF = float("inf")


def tested_indexes(plan_size, stride, count, variant=None):
    m = min(count, plan_size) if count > 0 else plan_size
    n = m // stride if variant == "floor_n_tested" else -(-m // stride)
    return np.arange(n, dtype=np.int64) * stride, n


def _d2(q, p):
    """[T, C] squared distances of points q [C, 3] from positions p [T, 3]: d = q - p, products summed x, y, z left to right."""
    d = q[None, :, :] - p[:, None, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _side(pos, js, candidates, r, cap, variant):
    """(min d2, worst j, first j) of tested positions pos [T, 3] (finite ones only, plan indexes js) against the points
    candidates(lo, hi) [C, 3]: every point that can lie within cap of the box [lo, hi], and any others."""
    best, worst, first = INF, -1, -1
    cap2, r2 = cap * cap, r * r
    for a in range(0, len(js), 64):
        p, j = pos[a:a + 64], js[a:a + 64]
        q = candidates(p.min(axis=0), p.max(axis=0))
        if len(q) == 0:
            continue
        with np.errstate(over="ignore", invalid="ignore"):
            d2 = _d2(q, p)
        seen = (d2 <= cap2) if variant == "le" else (d2 < cap2)
        d2 = np.where(seen, d2, INF)
        near = ((d2 <= r2) if variant == "le" else (d2 < r2)) & seen
        m = d2.min(axis=1)  # per tested state
        for k in range(len(j)):
            if m[k] < best or (variant == "last_on_ties" and m[k] == best and m[k] < INF):
                best, worst = float(m[k]), int(j[k])
            if first < 0 and near[k].any():
                first = int(j[k])
    return best, worst, first


def unknown_points(flags_view, origin, res, dims, lo, hi, reach, variant=None):
    """Centres of the non-zero voxels of one view ([nz][ny][nx] or flat) whose centre lies within `reach` of the box [lo, hi]."""
    nx, ny, nz = dims
    f = np.asarray(flags_view).reshape(nz, ny, nx)
    half = 0.0 if variant == "corner" else 0.5
    axes = []
    for a, n in enumerate((nx, ny, nz)):
        c = (np.arange(n, dtype=np.float64) + half) * res + origin[a]
        axes.append((np.nonzero((c >= lo[a] - reach) & (c <= hi[a] + reach))[0], c))
    (ix, cx), (iy, cy), (iz, cz) = axes
    if not (len(ix) and len(iy) and len(iz)):
        return np.zeros((0, 3))
    sub = f[np.ix_(iz, iy, ix)]
    kz, ky, kx = np.nonzero(sub)
    return np.stack([cx[ix[kx]], cy[iy[ky]], cz[iz[kz]]], axis=1)


def known_points(cloud, mask_row, variant=None):
    cloud = np.asarray(cloud, dtype=np.float64).reshape(-1, 3)
    keep = np.isfinite(cloud).all(axis=1)
    if mask_row is not None:
        k = np.arange(len(cloud))
        word = (k >> 6) if variant == "mask_word_64" else (k >> 5)
        keep &= ((np.asarray(mask_row, dtype=np.uint32)[word] >> (k & 31).astype(np.uint32)) & 1).astype(bool)
    return cloud[keep]


def audit(par, vehicles, plans, max_states, grid=None, flags=None, view_of=None, n_views=0, shared_grid=False, cloud=None, point_mask=None,
          variant=None):
    """[n] abi.plan_audit_dtype.  plans: [n][max_states] abi.state_dtype; flags: [n_views][cells] uint8 or None (no unknown side);
    shared_grid: view_stride == 0 with n_views == 1; cloud: [m][3] or None; point_mask: [n_views][words] uint32 or None."""
    n = len(vehicles)
    out = np.zeros(n, dtype=abi.plan_audit_dtype)
    out["first_unknown"] = out["worst_unknown"] = out["first_occupied"] = out["worst_occupied"] = out["view"] = -1
    out["min_unknown_d2"] = out["min_occupied_d2"] = INF
    ru, ro, cap, stride, count = float(par["r_unknown"]), float(par["r_occupied"]), float(par["cap"]), int(par["stride"]), int(par["count"])
    cloud = None if cloud is None or len(cloud) == 0 else np.asarray(cloud, dtype=np.float64).reshape(-1, 3)
    side_u, side_o = flags is not None, cloud is not None
    masked = side_o and point_mask is not None
    plans = np.asarray(plans).reshape(n, max_states)
    for i in range(n):
        o = out[i]
        head, size = int(vehicles["plan_head"][i]), int(vehicles["plan_size"][i])
        if head < 0 or size < 0 or head + size > max_states:
            o["flags"] = abi.FH_AUDIT_BAD_PLAN
            continue
        js, o["n_tested"] = tested_indexes(size, stride, count, variant)
        view, do_u, fl = -1, side_u, 0
        if side_u or masked:
            view = 0 if (side_u and shared_grid and n_views == 1) else (int(view_of[i]) if view_of is not None else i)
            o["view"] = view
            if view < 0 or view >= n_views:
                fl |= abi.FH_AUDIT_NO_VIEW
                do_u = False
        pos = plans[i, head + js]["pos"] if len(js) else np.zeros((0, 3))
        ok = np.isfinite(pos).all(axis=1)
        if not ok.all():
            fl |= abi.FH_AUDIT_NOT_FINITE
        pos, js = pos[ok], js[ok]
        if len(js):
            if do_u:
                origin, res, dims = grid
                cand = lambda lo, hi: unknown_points(flags[view], origin, res, dims, lo, hi, cap + 2 * res, variant)  # noqa: E731
                o["min_unknown_d2"], o["worst_unknown"], o["first_unknown"] = _side(pos, js, cand, ru, cap, variant)
            if side_o and not (masked and fl & abi.FH_AUDIT_NO_VIEW):
                known = known_points(cloud, point_mask[view] if masked else None, variant)
                reach = cap + 2 * (grid[1] if grid is not None else cap)
                cand = lambda lo, hi: known[((known >= lo - reach) & (known <= hi + reach)).all(axis=1)]  # noqa: E731
                o["min_occupied_d2"], o["worst_occupied"], o["first_occupied"] = _side(pos, js, cand, ro, cap, variant)
        if o["first_unknown"] >= 0:
            fl |= abi.FH_AUDIT_UNKNOWN
        if o["first_occupied"] >= 0:
            fl |= abi.FH_AUDIT_OCCUPIED
        o["flags"] = fl
    return out


def device_box(lo, hi, cap, grid):
    """The cells [a, b] per axis of the box the kernel stages for tested positions inside [lo, hi] (fh_audit.hip.hpp: audit_cells), or
    None; used to BUILD cases at the kernel's slab borders, never to decide an expected value."""
    origin, res, dims = grid
    box = []
    for k in range(3):
        grow = cap + (res + 1e-9 * (cap + abs(lo[k]) + abs(hi[k]) + abs(origin[k])))
        fa, fb = np.floor(((lo[k] - grow) - origin[k]) / res) - 1.0, np.floor(((hi[k] + grow) - origin[k]) / res) + 1.0
        if not fa <= dims[k] - 1 or not fb >= 0:
            return None
        box.append((int(max(fa, 0)), int(min(fb, dims[k] - 1))))
    return box


def one_plan(positions, max_states=None, head=0):
    """(vehicles [1], plans [1][max_states]) holding one plan with these positions."""
    positions = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    max_states = max_states or max(len(positions) + head, 1)
    v = np.zeros(1, dtype=abi.vehicle_dtype)
    v["plan_head"], v["plan_size"] = head, len(positions)
    pl = np.zeros((1, max_states), dtype=abi.state_dtype)
    pl["pos"][0, head:head + len(positions)] = positions
    return v, pl


def params(r_unknown, r_occupied, cap, stride=1, count=0):
    p = np.zeros((), dtype=abi.audit_params_dtype)
    p["r_unknown"], p["r_occupied"], p["cap"], p["stride"], p["count"] = r_unknown, r_occupied, cap, stride, count
    return p


def assert_equal_records(got, want, what=""):
    """Every field of every record, bit for bit (the doubles as their 64-bit patterns)."""
    assert got.dtype == want.dtype == abi.plan_audit_dtype and got.shape == want.shape
    for k in abi.plan_audit_dtype.names:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.dtype.kind == "f":
            a, b = a.view(np.uint64), b.view(np.uint64)
        bad = np.nonzero((a != b).reshape(len(got), -1).any(axis=1))[0]
        assert not len(bad), "%s field %s differs at records %s: device %s, model %s" % (what, k, bad[:8], got[k][bad[:8]], want[k][bad[:8]])
