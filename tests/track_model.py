"""The tracker of moving obstacles (include/fasterhip_track.h) restated in plain Python and numpy: brute force over all (obstacle,
vehicle) pairs and all samples of every ray, the header's model word for word.  Python floats and numpy float64 are IEEE doubles and
neither fuses a multiply-add, so `track()` is what fh_fleet_obstacle_track_device must write in every byte.  It shares nothing with the
kernel: no wavefront, no chunk, no ring in registers.  occ is the grid fh_map_occupancy returns ([mz][my][mx], non-zero = occupied), or
None for map = NULL; m_origin and m_res its lattice.  `variant` names one deliberate mistake (tests/test_track_model.py shows the case
each one changes); None is the model.  Not a test file."""
import math

import numpy as np

from faster_amd import abi

VARIANTS = ("le", "ray_from_obstacle", "end_cells_tested", "seer_largest", "newest_first", "no_gate", "age_inclusive", "stale_accepted")
H = abi.FH_TRACK_HISTORY
MAX_TICK = abi.FH_OBSTACLE_MAX_TICK


def finite(*xs):
    return all(math.isfinite(float(x)) for x in xs)


def d2(ax, ay, az, bx, by, bz):
    """d2(a - b): the three products summed from left to right."""
    dx, dy, dz = ax - bx, ay - by, az - bz
    return dx * dx + dy * dy + dz * dz


def measurement(rec, truth_tick0, dc):
    """Step 1: (visible, z, radius) of one abi.obstacle_dtype record."""
    p0, v, radius = [float(x) for x in rec["p0"]], [float(x) for x in rec["v"]], float(rec["radius"])
    tau = float(int(truth_tick0)) * float(dc)
    with np.errstate(all="ignore"):
        z = [float(np.float64(p0[a]) + np.float64(v[a]) * np.float64(tau)) for a in range(3)]
    valid = bool(int(rec["flags"]) & abi.FH_OBSTACLE_ON) and finite(*p0) and finite(*v) and finite(radius) and radius >= 0.0
    return valid and finite(*z), z, radius


def blocked(p, q, occ, m_origin, m_res, variant=None):
    """fasterhip_link_los.h's "Blocked" for the ray from p to q, sample by sample."""
    res = float(m_res)
    d = [q[a] - p[a] for a in range(3)]
    dist = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    K = max(1, int(math.ceil(dist / (0.5 * res))))
    mz, my, mx = occ.shape
    cell = lambda x: tuple(math.floor((x[a] - float(m_origin[a])) / res) for a in range(3))  # noqa: E731
    pc, qc = cell(p), cell(q)
    for j in range(1, K):
        t = float(j) / float(K)
        c = cell([p[a] + d[a] * t for a in range(3)])
        if variant != "end_cells_tested" and (c == pc or c == qc):
            continue
        if 0 <= c[0] < mx and 0 <= c[1] < my and 0 <= c[2] < mz and occ[c[2], c[1], c[0]] != 0:
            return True
    return False


def sees(par, z, pos, occ, m_origin, m_res, variant=None):
    """Step 3 for one visible obstacle at z: [n] bool, vehicle by vehicle."""
    r = float(par["r_detect"])
    r2 = r * r
    out = np.zeros(len(pos), dtype=bool)
    for i, p in enumerate(pos):
        p = [float(x) for x in p]
        if not finite(*p):
            continue
        dd = d2(z[0], z[1], z[2], p[0], p[1], p[2])
        if not (dd <= r2 if variant == "le" else dd < r2):
            continue
        if occ is None:
            out[i] = True
        elif variant == "ray_from_obstacle":
            out[i] = not blocked(z, p, occ, m_origin, m_res, variant)
        else:
            out[i] = not blocked(p, z, occ, m_origin, m_res, variant)
    return out


def read_track(rec):
    """Reading a track: the sightings [(tick, x, y, z)] from the oldest to the newest, head and radius; a bad record reads as empty."""
    count, head = int(rec["count"]), int(rec["head"])
    if not (0 <= count <= H and 0 <= head < H) or count == 0:
        return [], 0, 0.0
    s = [(int(rec["tick"][(head + q) % H]),) + tuple(float(x) for x in rec["pos"][(head + q) % H]) for q in range(count)]
    if any(not 0 <= e[0] <= MAX_TICK for e in s):
        return [], 0, 0.0
    return s, head, float(rec["radius"])


def estimate(s, radius, par, tick, variant=None):
    """Step 5 for the sightings s (not empty): (p0 [3], v [3], radius_est, usable)."""
    dc, k = float(par["dc"]), min(len(s), int(par["fit"]))
    newest = s[-1][0]
    used = s[len(s) - k:]
    if variant == "newest_first":
        used = used[::-1]
    su = suu = 0.0
    sp, sup = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
    for e in used:
        u = float(e[0] - newest) * dc
        su = su + u
        suu = suu + u * u
        for a in range(3):
            sp[a] = sp[a] + e[1 + a]
            sup[a] = sup[a] + u * e[1 + a]
    kk, D = float(k), 1.0
    with np.errstate(all="ignore"):
        if k == 1:
            v, a0 = [0.0, 0.0, 0.0], list(s[-1][1:])
        else:
            D = kk * suu - su * su
            v = [float((np.float64(kk) * sup[a] - np.float64(su) * sp[a]) / np.float64(D)) for a in range(3)]
            a0 = [float((np.float64(sp[a]) - np.float64(v[a]) * su) / kk) for a in range(3)]
        age = float(int(tick) - newest) * dc
        p0 = [float(np.float64(a0[a]) + np.float64(v[a]) * age) for a in range(3)]
        r_est = float(np.float64(radius) + np.float64(float(par["grow"])) * age)
    return p0, v, r_est, finite(*p0) and finite(*v) and finite(r_est) and D > 0.0


def track(par, truth, truth_tick0, tick, pos, tracks, occ=None, m_origin=None, m_res=None, variant=None):
    """One call: (tracks [m] abi.obstacle_track_dtype, est [m] abi.obstacle_dtype, seer [m] int32, info [4] int64).  pos: [n][3]."""
    m, tick = len(truth), int(tick)
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    out = np.zeros(m, dtype=abi.obstacle_track_dtype)
    est = np.zeros(m, dtype=abi.obstacle_dtype)
    seer = np.full(m, -1, dtype=np.int32)
    info = np.zeros(4, dtype=np.int64)
    gate, max_age = float(par["gate"]), int(par["max_age"])
    for o in range(m):
        visible, z, truth_radius = measurement(truth[o], truth_tick0, par["dc"])
        s, head, radius = read_track(tracks[o])
        flags = 0
        if s and max_age > 0 and (tick - s[-1][0] >= max_age if variant == "age_inclusive" else tick - s[-1][0] > max_age):
            s, head, radius = [], 0, 0.0
            flags |= abi.FH_TRACK_LOST
        if visible:
            who = np.flatnonzero(sees(par, z, pos, occ, m_origin, m_res, variant))
            if len(who):
                seer[o] = who[-1] if variant == "seer_largest" else who[0]
        if seer[o] >= 0:
            if s and tick <= s[-1][0] and variant != "stale_accepted":
                flags |= abi.FH_TRACK_STALE
            else:
                if gate > 0 and s and variant != "no_gate":
                    pred = estimate(s, radius, par, tick, variant)[0]
                    if not d2(z[0], z[1], z[2], pred[0], pred[1], pred[2]) < gate * gate:   # (a NaN does not hold)
                        s, head, radius = [], 0, 0.0
                        flags |= abi.FH_TRACK_RESET
                if len(s) == H:
                    s, head = s[1:], (head + 1) % H
                s = s + [(tick, z[0], z[1], z[2])]
                radius = truth_radius
                flags |= abi.FH_TRACK_SEEN
        if s:
            p0, v, r_est, usable = estimate(s, radius, par, tick, variant)
            if len(s) >= int(par["min_obs"]):
                if usable:
                    est[o]["p0"], est[o]["v"], est[o]["radius"], est[o]["flags"] = p0, v, r_est, abi.FH_OBSTACLE_ON
                else:
                    flags |= abi.FH_TRACK_BAD_FIT
        for q, e in enumerate(s):
            out[o]["tick"][(head + q) % H] = e[0]
            out[o]["pos"][(head + q) % H] = e[1:]
        out[o]["radius"], out[o]["count"], out[o]["head"], out[o]["flags"] = radius, len(s), head, flags
        info += [seer[o] >= 0, bool(est[o]["flags"]), bool(flags & abi.FH_TRACK_RESET), bool(flags & abi.FH_TRACK_LOST)]
    return out, est, seer, info
