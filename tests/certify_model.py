"""numpy restatement of the certificate of include/fasterhip_certify.h, the header's model word for word: IEEE double, one rounding per
operation, the operation order written there.  Result by result; arrays are used only elementwise (the same scalar operation on every
element), never `@`, `dot` or `sum`, whose summation order is not stated.  The device kernel is compared with this bit for bit
(tests/test_gpu_certify.py); tests/test_certify_model.py shows on oracle results and on cases worked by hand that it is worth comparing with."""
import numpy as np

from faster_amd import abi

INF = float("inf")
NUMBERS = abi.CERT_NUMBERS


def vmax(m, x):
    """m = x > m ? x : m"""
    return x if x > m else m


def vmin(m, x):
    return x if x < m else m


def amax(values):
    """The header's max over an array: from -inf, a NaN never wins (the value does not depend on the order, up to the sign of a zero)."""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    v = v[v == v]
    return float(v.max()) if v.size else -INF


def pos(a, b, c, d, tau):
    return a * tau * tau * tau + b * tau * tau + c * tau + d


def vel(a, b, c, tau):
    return 3 * a * tau * tau + 2 * b * tau + c


def acc(a, b, tau):
    return 6 * a * tau + 2 * b


def control_points(co, dt):
    """co: [N][12] -> [N][4][3], the expressions of fh_control_points."""
    a, b, c, d = co[:, 0:3], co[:, 3:6], co[:, 6:9], co[:, 9:12]
    Bn, Cn = b * dt * dt, c * dt
    return np.stack([pos(a, b, c, d, 0.0), (Cn + 3 * d) / 3, (Bn + 2 * Cn + 3 * d) / 3, pos(a, b, c, d, dt)], axis=1)


def structural(p, r, n_faces):
    if int(r["solved"]) == 0:
        return abi.FH_CERT_UNSOLVED
    N, Q, fb, off = int(p["n_seg"]), int(p["n_poly"]), int(p["face_begin"]), [int(x) for x in p["face_off"]]
    if not (1 <= N <= abi.FH_MAX_SEG) or not (0 <= Q <= abi.FH_MAX_POLY) or fb < 0:
        return abi.FH_CERT_BAD_INPUT
    if off[0] != 0 or any(off[q] > off[q + 1] for q in range(Q)) or fb + off[Q] > n_faces:
        return abi.FH_CERT_BAD_INPUT
    if Q > 0 and any(not (0 <= int(r["assign"][t]) < Q) for t in range(N)):
        return abi.FH_CERT_BAD_INPUT
    dt = float(r["dt"])
    if not np.isfinite(dt) or not dt > 0 or not np.isfinite(r["coeff"][:N]).all():
        return abi.FH_CERT_NOT_FINITE
    return 0


def certify_one(p, faces, r, tol=None):
    """One fh_certificate record (abi.certificate_dtype, shape ()) of result r for problem p over the rows `faces`."""
    out = np.zeros((), dtype=abi.certificate_dtype)
    flags = structural(p, r, len(faces))
    if flags:
        out["flags"] = flags
        return out
    N, Q, fb, off = int(p["n_seg"]), int(p["n_poly"]), int(p["face_begin"]), [int(x) for x in p["face_off"]]
    dt = np.float64(r["dt"])
    co = np.array(r["coeff"][:N], dtype=np.float64)
    with np.errstate(all="ignore"):
        # corridor
        if Q == 0:
            best, assigned, worst = -INF, -INF, -1
        else:
            cp = control_points(co, dt)                       # [N][4][3]
            px, py, pz = cp[:, :, 0:1], cp[:, :, 1:2], cp[:, :, 2:3]
            e = np.full((N, Q), -INF)
            for q in range(Q):
                F = faces[fb + off[q]:fb + off[q + 1]]
                if len(F):
                    A, b = F["a"], F["b"]
                    v = ((A[:, 0] * px + A[:, 1] * py) + A[:, 2] * pz) - b   # [N][4][faces], elementwise
                    for t in range(N):
                        e[t, q] = amax(v[t])
            best_t = []
            for t in range(N):
                m = INF
                for q in range(Q):
                    m = vmin(m, float(e[t, q]))
                best_t.append(m)
            best, assigned = amax(best_t), amax([e[t, int(r["assign"][t])] for t in range(N)])
            worst = next(t for t in range(N) if best_t[t] == best)
        # the state rows, [N][3]
        a, b, c, d = co[:, 0:3], co[:, 3:6], co[:, 6:9], co[:, 9:12]
        p0, v0, a0 = pos(a, b, c, d, 0.0), vel(a, b, c, 0.0), acc(a, b, 0.0)
        p1, v1, a1 = pos(a, b, c, d, dt), vel(a, b, c, dt), acc(a, b, dt)
        jerk = 6 * a
        x0, xf = np.array(p["x0"], dtype=np.float64), np.array(p["xf"], dtype=np.float64)
        x0_defect = amax([np.abs(p0[0] - x0[0:3]), np.abs(v0[0] - x0[3:6]), np.abs(a0[0] - x0[6:9])])
        rows = [np.abs(v1[N - 1] - xf[3:6]), np.abs(a1[N - 1] - xf[6:9])]
        if int(p["force_final_pos"]) != 0:
            rows.append(np.abs(p1[N - 1] - xf[0:3]))
        xf_defect = amax(rows)
        continuity = 0.0 if N == 1 else amax([np.abs(p1[:-1] - p0[1:]), np.abs(v1[:-1] - v0[1:]), np.abs(a1[:-1] - a0[1:])])
        v_excess = amax(np.abs(v0) - np.float64(p["v_max"]))
        a_excess = amax(np.abs(a0) - np.float64(p["a_max"]))
        j_excess = amax(np.abs(jerk) - np.float64(p["j_max"]))
        a_peak = amax([np.abs(a0), np.abs(a1)])
        peaks = [np.abs(v0), np.abs(v1)]
        for t in range(N):
            for i in range(3):
                if a[t, i] != 0:
                    ts = (-b[t, i]) / (3 * a[t, i])
                    if 0 < ts < dt:
                        peaks.append(np.abs(vel(a[t, i], b[t, i], c[t, i], ts)))
        v_peak = amax(np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1) for x in peaks]))
        cost = np.float64(0.0)
        for t in range(N):
            for i in range(3):
                cost = cost + jerk[t, i] * jerk[t, i]
        cost_defect = np.abs(cost - np.float64(r["cost"]))
        vals = dict(corridor_assigned=assigned, corridor_best=best, x0_defect=x0_defect, xf_defect=xf_defect, continuity_defect=continuity,
                    v_excess=v_excess, a_excess=a_excess, j_excess=j_excess, v_peak=v_peak, a_peak=a_peak, cost=cost, cost_defect=cost_defect)
        if tol is not None:
            tc, ts_, tb, tr = (np.float64(tol[k]) for k in ("corridor", "state", "box", "cost_rel"))
            ac = np.abs(np.float64(r["cost"]))
            flags |= abi.FH_CERT_CORRIDOR if best > tc else 0
            flags |= abi.FH_CERT_ASSIGNMENT if assigned > tc else 0
            flags |= abi.FH_CERT_X0 if x0_defect > ts_ else 0
            flags |= abi.FH_CERT_XF if xf_defect > ts_ else 0
            flags |= abi.FH_CERT_CONTINUITY if continuity > ts_ else 0
            flags |= abi.FH_CERT_BOX if (v_excess > tb or a_excess > tb or j_excess > tb) else 0
            flags |= abi.FH_CERT_COST if cost_defect > tr * (ac if ac > 1 else np.float64(1.0)) else 0
    out["flags"], out["worst_seg"] = flags, worst
    for k in NUMBERS:
        out[k] = vals[k]
    return out


def certify(problems, faces, results, tol=None):
    """[n] abi.certificate_dtype."""
    out = np.zeros(len(problems), dtype=abi.certificate_dtype)
    for i in range(len(problems)):
        out[i] = certify_one(problems[i], faces, results[i], tol)
    return out


def same_bits(x, y):
    """Field by field, doubles as their 64 bits: the names of the fields that differ anywhere (empty: identical)."""
    bad = [k for k in ("flags", "worst_seg") if not np.array_equal(x[k], y[k])]
    return bad + [k for k in NUMBERS if not np.array_equal(np.ascontiguousarray(x[k]).view(np.uint64), np.ascontiguousarray(y[k]).view(np.uint64))]
