"""The heading model of include/fasterhip.h (fh_heading: fh_fleet_next_goals_yaw_device, fh_fleet_set_goals_device,
fh_fleet_sense_fov_device) restated in Python, operation for operation, for the tests that compare the device exactly.  Not a test file.

Python floats are IEEE doubles and math.atan2 / math.fmod / math.copysign are the C library's, so yaw_ticks is what a g++ build of
fhreplan::Planner::getNextGoalYaw computes (tests/test_fleet_heading_abi.py checks that).  The device's atan2 may differ from the
host's in the last bit; that can change a result only on a tick whose wrapped diff is within a rounding error of 0 (the sign),
+-0.04 (YAWING ends) or +-pi (the wrap): near_ticks counts those, and the GPU tests' inputs are chosen so that there are none."""
import math

import numpy as np

import sense_model  # noqa: F401  (the omnidirectional model this one extends)

TRAVELING, GOAL_SEEN, GOAL_REACHED, YAWING = 0, 1, 2, 3
NEAR = 1e-9


def angle_wrap(diff):
    """utils.cpp:496-502"""
    diff = math.fmod(diff + math.pi, 2 * math.pi)
    if diff < 0:
        diff += 2 * math.pi
    diff -= math.pi
    return diff


def yaw_ticks(status, h, g_term, plan_xy, ticks, follow, w_max, alpha, dc):
    """getNextGoal with getDesiredYaw `ticks` times for one vehicle with a plan of len(plan_xy) >= 1 states.  h: dict with yaw,
    previous_yaw, dyaw_filtered, goal_yaw, goal_dyaw, look_at (updated in place).  Returns (status, log, near): log[t] = (yaw, dyaw,
    status after tick t), near = the ticks whose wrapped diff is within NEAR of 0, +-0.04 or +-pi."""
    size = len(plan_xy)
    log, near = [], 0
    for t in range(ticks):
        gx, gy = plan_xy[min(t, size - 1)]
        if status == GOAL_REACHED:
            dyaw = 0.0
            yaw = h["previous_yaw"]
        else:
            tx, ty = (g_term[0], g_term[1]) if status == YAWING else (h["look_at"][0], h["look_at"][1])
            desired = math.atan2(ty - gy, tx - gx)
            diff = angle_wrap(desired - h["yaw"])
            if min(abs(diff), abs(abs(diff) - 0.04), abs(abs(diff) - math.pi)) < NEAR:
                near += 1
            if abs(diff) < 0.04 and status == YAWING:
                status = TRAVELING
            not_filtered = math.copysign(1.0, diff) * w_max
            h["dyaw_filtered"] = (1 - alpha) * not_filtered + alpha * h["dyaw_filtered"]
            dyaw = h["dyaw_filtered"]
            yaw = h["previous_yaw"] + h["dyaw_filtered"] * dc
        h["previous_yaw"] = yaw
        h["goal_yaw"], h["goal_dyaw"] = yaw, dyaw
        if follow:
            h["yaw"] = yaw
        log.append((yaw, dyaw, status))
    return status, log, near


def project_to_box(c, p, w):
    """projectPointToBox as fleet_begin_kernel computes it (utils.cpp:1065-1115)."""
    c, p = [float(x) for x in c], [float(x) for x in p]
    lo = [c[a] - w[a] / 2 for a in range(3)]
    hi = [c[a] + w[a] / 2 for a in range(3)]
    if all(lo[a] < p[a] < hi[a] for a in range(3)):
        return p
    best, out = math.inf, list(p)
    for ax in range(3):
        for side in range(2):
            plane, den = (lo[ax] if side else hi[ax]), p[ax] - c[ax]
            if den == 0:
                continue
            t = (plane - c[ax]) / den
            if t < 0 or t > 1:
                continue
            x = [c[a] + (p[a] - c[a]) * t for a in range(3)]
            d = [x[a] - c[a] for a in range(3)]
            dist = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
            if dist < best:
                best, out = dist, x
    return out


def set_goals(vehicles, new_goals, mask, w):
    """fh_fleet_set_goals_device on a copy of `vehicles` (abi.vehicle_dtype): g_term, goal, GOAL_REACHED -> YAWING."""
    v = vehicles.copy()
    for i in range(len(v)):
        if mask is not None and not mask[i]:
            continue
        v["g_term"][i] = new_goals[i]
        v["goal"][i] = project_to_box(v["state"]["pos"][i], new_goals[i], w)
        if v["status"][i] == GOAL_REACHED:
            v["status"][i] = YAWING
    return v


def scan_box(p, dirv, th, tv, r):
    """What the forward sensor's box spans from p per axis ((lo, hi) x 3): the frustum cut at r inside the sphere's box.  The model does
    not need it (the predicate decides); it is here so that a test can tell which vehicles' boxes the lattice clips."""
    c, s = dirv
    n = math.hypot(c, s)
    c, s = c / n, s / n
    return ((max(-r, min(0.0, r * (c - abs(s) * th))), min(r, max(0.0, r * (c + abs(s) * th)))),
            (max(-r, min(0.0, r * (s - abs(c) * th))), min(r, max(0.0, r * (s + abs(c) * th)))),
            (max(-r, -r * tv), min(r, r * tv)))


def sense_one_fov(view, p, dirv, th, tv, r_sense, origin, res, occ, m_origin, m_res):
    """sense_model.sense_one through a field of view: with (c, s) = dirv and d = q - p, f = c dx + s dy, l = c dy - s dx; in view:
    f > 0, |l| <= f th, |dz| <= f tv.  dirv = None: omnidirectional (sense_model.sense_one).  `view` is updated in place.  Returns
    (hidden, out_of_view): unknown cells in range and in view that stay unknown because something hides them; unknown cells in range
    that are not in view."""
    p = np.asarray(p, dtype=np.float64)
    if not np.all(np.isfinite(p)):
        return 0, 0
    if dirv is not None and not np.all(np.isfinite(np.asarray(dirv, dtype=np.float64))):
        return 0, 0
    nz, ny, nx = view.shape
    lo = np.floor((p - r_sense - origin) / res) - 2
    hi = np.floor((p + r_sense - origin) / res) + 2
    lo = np.clip(lo, 0, [nx, ny, nz]).astype(np.int64)
    hi = np.clip(hi, -1, [nx - 1, ny - 1, nz - 1]).astype(np.int64)
    if np.any(hi < lo):
        return 0, 0
    iz, iy, ix = np.meshgrid(np.arange(lo[2], hi[2] + 1), np.arange(lo[1], hi[1] + 1), np.arange(lo[0], hi[0] + 1), indexing="ij")
    ix, iy, iz = ix.ravel(), iy.ravel(), iz.ravel()
    dx = (ix + 0.5) * res + origin[0] - p[0]
    dy = (iy + 0.5) * res + origin[1] - p[1]
    dz = (iz + 0.5) * res + origin[2] - p[2]
    d = np.sqrt(dx * dx + dy * dy + dz * dz)
    pick = (d < r_sense) & (view[iz, iy, ix] != 0)
    out_of_view = 0
    if dirv is not None:
        c, s = float(dirv[0]), float(dirv[1])
        f = c * dx + s * dy
        l = c * dy - s * dx
        in_view = (f > 0) & (np.abs(l) <= f * th) & (np.abs(dz) <= f * tv)
        out_of_view = int((pick & ~in_view).sum())
        pick &= in_view
    ix, iy, iz, dx, dy, dz, d = ix[pick], iy[pick], iz[pick], dx[pick], dy[pick], dz[pick], d[pick]
    K = np.maximum(1.0, np.ceil(d / (0.5 * m_res)))
    blocked = np.zeros(len(d), dtype=bool)
    mz, my, mx = occ.shape
    qfx = np.floor(((ix + 0.5) * res + origin[0] - m_origin[0]) / m_res)
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
    return int(blocked.sum()), out_of_view


def sense_fov(views, view_of, positions, dirs, th, tv, r_sense, origin, res, occ, m_origin, m_res):
    """Every vehicle senses into views[view_of[i]] (None: view i) through its field of view.  Returns the summed (hidden, out_of_view)."""
    origin, m_origin = np.asarray(origin, dtype=np.float64), np.asarray(m_origin, dtype=np.float64)
    hidden = out = 0
    for i, p in enumerate(positions):
        v = i if view_of is None else int(view_of[i])
        if 0 <= v < len(views):
            h, o = sense_one_fov(views[v], p, None if dirs is None else dirs[i], float(th), float(tv), float(r_sense), origin, float(res), occ,
                                 m_origin, float(m_res))
            hidden += h
            out += o
    return hidden, out


# ---- the inputs of the GPU yaw test (tests/test_gpu_fleet_heading.py), here so that the CPU test can assert the condition on them ----
YAW_SEED = 5
YAW_N = 257
YAW_TICKS = (1, 2, 7, 39, 40, 41, 200)


def yaw_case(seed=YAW_SEED, n=YAW_N):
    """n vehicles: status cycling through all four, plans of 1 .. 40 states (vehicle i: 1 + i % 40) along a random walk, a target
    (g_term and look_at) behind, ahead or across the +-pi cut of the initial yaw.  Returns a dict of arrays."""
    rng = np.random.default_rng(seed)
    status = (np.arange(n) % 4).astype(np.int32)
    size = 1 + (np.arange(n) % 40)
    size[-1] = 40
    start = rng.uniform(-5, 5, size=(n, 3))
    steps = rng.uniform(-0.03, 0.03, size=(n, 40, 3))
    plans = start[:, None, :] + np.cumsum(steps, axis=1)
    yaw0 = rng.uniform(-math.pi, math.pi, size=n)
    kind = (np.arange(n) // 4) % 3          # 0 ahead, 1 behind, 2 across the cut: yaw near +-pi, the target on the other side of it
    yaw0[kind == 2] = np.where(rng.random((kind == 2).sum()) < 0.5, 1, -1) * rng.uniform(2.9, 3.1, size=(kind == 2).sum())
    bearing = np.where(kind == 0, yaw0 + rng.uniform(-0.3, 0.3, size=n), np.where(kind == 1, yaw0 + math.pi + rng.uniform(-0.3, 0.3, size=n),
                                                                                   -yaw0 + rng.uniform(-0.1, 0.1, size=n)))
    dist = rng.uniform(2.0, 8.0, size=n)
    target = start + np.stack([dist * np.cos(bearing), dist * np.sin(bearing), np.zeros(n)], axis=1)
    other = start + rng.uniform(-6, 6, size=(n, 3))   # what the status at hand does NOT look at
    yawing = status == YAWING
    g_term = np.where(yawing[:, None], target, other)
    look_at = np.where(yawing[:, None], other, target)
    return {"status": status, "size": size, "plans": plans, "yaw0": yaw0, "prev0": yaw0 + rng.uniform(-0.05, 0.05, size=n),
            "dyaw0": rng.uniform(-4, 4, size=n), "g_term": g_term, "look_at": look_at}


def yaw_case_model(case, ticks, follow, alpha, w_max=4.0, dc=0.01):
    """The model on every vehicle of yaw_case: (status [n], headings as a list of dicts, near ticks in total)."""
    out_status, out_h, near = [], [], 0
    for i in range(len(case["status"])):
        h = {"yaw": float(case["yaw0"][i]), "previous_yaw": float(case["prev0"][i]), "dyaw_filtered": float(case["dyaw0"][i]), "goal_yaw": 0.0,
             "goal_dyaw": 0.0, "look_at": [float(x) for x in case["look_at"][i]]}
        plan_xy = [(float(p[0]), float(p[1])) for p in case["plans"][i, :case["size"][i]]]
        st, _, k = yaw_ticks(int(case["status"][i]), h, [float(x) for x in case["g_term"][i]], plan_xy, ticks, follow, w_max, alpha, dc)
        out_status.append(st)
        out_h.append(h)
        near += k
    return np.array(out_status, dtype=np.int32), out_h, near
