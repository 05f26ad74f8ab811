"""Moving obstacles (include/fasterhip_obstacles.h) restated in numpy: brute force over all (i, o, s, s') for the bits (one array
operation per vehicle and offset s' - s) and over all (i, j, o) for the audit, the header's model word for word.  Everything is IEEE
double and numpy fuses no multiply-add, so `obstacles()` gives the cloud tail and the mask words, and `audit()` the records, that the
device must write, byte for byte.  `variant` names one deliberate mistake (tests/test_obstacle_model.py shows which hand case each one
changes); None is the model."""
import numpy as np

import traffic_model as tm
from faster_amd import abi

VARIANTS = ("le", "no_radius", "no_tick0", "detect_at_sample", "window_unclipped", "sum_first", "ties_larger")
HULL_ORDER = ((0, 1.0), (0, -1.0), (1, 1.0), (1, -1.0), (2, 1.0), (2, -1.0))   # +x, -x, +y, -y, +z, -z after the centre


def valid(obs):
    """[m] bool: ON, seven finite doubles, radius >= 0."""
    obs = np.asarray(obs)
    with np.errstate(invalid="ignore"):
        return (((obs["flags"] & abi.FH_OBSTACLE_ON) != 0) & np.isfinite(obs["p0"]).all(axis=1) & np.isfinite(obs["v"]).all(axis=1)
                & np.isfinite(obs["radius"]) & (obs["radius"] >= 0))


def taus(tick0, instants, dc, variant=None):
    """tau = (double)(tick0 + j) * dc: the sum in integers (python's: no overflow), one conversion, one product."""
    base = 0 if variant == "no_tick0" else int(tick0)
    return np.array([float(base + int(j)) for j in instants], dtype=np.float64) * np.float64(dc)


def centres(obs, tau, variant=None):
    """[m][len(tau)][3]: c = p0 + v * tau per axis, the product rounded, then the sum (whatever the obstacle: the caller asks valid())."""
    p0, v = np.asarray(obs["p0"], dtype=np.float64)[:, None, :], np.asarray(obs["v"], dtype=np.float64)[:, None, :]
    with np.errstate(over="ignore", invalid="ignore"):
        if variant == "sum_first":
            return (p0 + v) * tau[None, :, None]
        return p0 + v * tau[None, :, None]


def d2_of(d):
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def instants(par):
    return [int(par["first_instant"]) + s * int(par["stride"]) for s in range(int(par["samples"]))]


def samples(par, obs, tick0, variant=None):
    """(show [m][S] bool, c [m][S][3] zero where the sample does not show, now [m][3], reach2 [m])."""
    obs = np.asarray(obs)
    c = centres(obs, taus(tick0, instants(par), par["dc"], variant), variant)
    show = valid(obs)[:, None] & np.isfinite(c).all(axis=2)
    c = np.where(show[:, :, None], c, 0.0)
    now = centres(obs, taus(tick0, [0], par["dc"], variant), variant)[:, 0]
    with np.errstate(over="ignore", invalid="ignore"):
        reach = np.float64(par["range"]) + (0.0 if variant == "no_radius" else obs["radius"])
        reach2 = reach * reach
    return show, c, now, np.broadcast_to(reach2, (len(obs),))


def points(par, obs, show, c):
    """[m][S][pps][3]: the points of every slot."""
    pps = int(par["points"])
    pts = np.zeros(show.shape + (pps, 3))
    pts[:, :, 0] = c
    if pps == 7:
        with np.errstate(over="ignore", invalid="ignore"):
            h = np.asarray(obs["radius"], dtype=np.float64)[:, None]
            for q, (axis, sign) in enumerate(HULL_ORDER, start=1):
                pts[:, :, q] = c
                pts[:, :, q, axis] = c[:, :, axis] + h if sign > 0 else c[:, :, axis] - h   # one add or one subtract
    pts[~show] = 0.0
    return pts


def observers(par, vehicles, plans, max_states):
    """fasterhip_traffic_timed.h's "Shows" for every vehicle: (show [n][S], c [n][S][3])."""
    return tm.samples(par, vehicles, plans, max_states, None, int(par["first_instant"]))


def detected(par, vehicles, show, c, now, variant=None):
    """[n][m][S] bool (the same for every s unless the variant asks the sample)."""
    n, (m, S) = len(vehicles), show.shape
    r = float(par["r_detect"])
    if r == 0.0:
        return np.ones((n, m, S), dtype=bool)
    pos = np.asarray(vehicles["state"]["pos"], dtype=np.float64)
    what = c if variant == "detect_at_sample" else np.broadcast_to(now[:, None, :], (m, S, 3))
    with np.errstate(over="ignore", invalid="ignore"):
        d2 = d2_of(what[None] - pos[:, None, None, :])
        near = d2 < r * r
    return near & np.isfinite(what).all(axis=2)[None] & np.isfinite(pos).all(axis=1)[:, None, None]


def decisions(par, vehicles, plans, max_states, show, c, now, reach2, variant=None):
    """[n][m][S] bool: in row i, the decision of sample (o, s)."""
    n, (m, S) = len(vehicles), show.shape
    window = int(par["window"])
    oshow, oc = observers(par, vehicles, plans, max_states)
    det = detected(par, vehicles, show, c, now, variant)
    on = np.zeros((n, m, S), dtype=bool)
    for i in range(n):
        met = np.zeros((m, S), dtype=bool)
        for s in range(S):
            if variant == "window_unclipped":
                mine = sorted(set(q % S for q in range(s - min(window, S), s + min(window, S) + 1)))   # (an index outside wraps round)
            else:
                mine = range(max(0, s - window), min(S - 1, s + window) + 1)
            for q in mine:
                if not oshow[i, q]:
                    continue
                with np.errstate(over="ignore", invalid="ignore"):
                    d2 = d2_of(c[:, s] - oc[i, q][None])
                    met[:, s] |= (d2 <= reach2) if variant == "le" else (d2 < reach2)
        on[i] = met & show & det[i]
    return on


def obstacles(par, obs, tick0, vehicles, plans, max_states, cloud, mask, variant=None):
    """(cloud [n_cloud][3], mask [n][mask_words] uint32) after the call, from those before it (copies)."""
    obs = np.asarray(obs)
    n, m, S, first, pps = len(vehicles), len(obs), int(par["samples"]), int(par["first_point"]), int(par["points"])
    assert 1 <= S <= abi.FH_OBSTACLE_MAX_SAMPLES and pps in (1, 7) and int(par["window"]) >= 0 and int(par["first_instant"]) >= 0
    assert 0 <= int(tick0) <= abi.FH_OBSTACLE_MAX_TICK
    cloud = np.array(cloud, dtype=np.float64).reshape(-1, 3)
    mask = np.array(mask, dtype=np.uint32).reshape(max(n, 1), -1)[:n]
    if n == 0 or m == 0:
        return cloud, mask
    show, c, now, reach2 = samples(par, obs, tick0, variant)
    total = m * S * pps
    assert first % 32 == 0 and first + total <= len(cloud) and first + total <= mask.shape[1] * 32
    cloud[first:first + total] = points(par, obs, show, c).reshape(-1, 3)   # every owned point is written
    on = decisions(par, vehicles, plans, max_states, show, c, now, reach2, variant)
    bits = np.repeat(on.reshape(n, m * S), pps, axis=1)   # all points of a sample share one decision
    w0, w1 = first // 32, -(-(first + total) // 32)
    padded = np.zeros((n, (w1 - w0) * 32), dtype=np.uint64)   # bits past the last owned point in the last word are zero
    padded[:, :total] = bits
    mask[:, w0:w1] = (padded.reshape(n, w1 - w0, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)   # whole words
    return cloud, mask


def obstacle_bits(par, n, m, mask):
    """[n][m S pps] bool: the owned bits of every row."""
    first, total = int(par["first_point"]), m * int(par["samples"]) * int(par["points"])
    w = np.ascontiguousarray(np.asarray(mask, dtype=np.uint32).reshape(n, -1)[:, first // 32:])
    return np.unpackbits(w.view(np.uint8), axis=1, bitorder="little")[:, :total].astype(bool)


def audit(par, obs, tick0, vehicles, plans, max_states, variant=None):
    """[n] abi.plan_obstacle_audit_dtype."""
    obs = np.asarray(obs)
    n, m = len(vehicles), len(obs)
    stride, count = int(par["stride"]), int(par["count"])
    plans = np.asarray(plans).reshape(n, max_states)
    out = np.zeros(n, dtype=abi.plan_obstacle_audit_dtype)
    ok = valid(obs) if m else np.zeros(0, dtype=bool)
    with np.errstate(over="ignore", invalid="ignore"):
        hit = np.float64(par["r"]) + (np.zeros(m) if variant == "no_radius" else np.asarray(obs["radius"], dtype=np.float64).reshape(m))
        hit2 = hit * hit
    for i in range(n):
        rec = out[i]
        rec["first"] = rec["first_obstacle"] = rec["worst"] = rec["worst_obstacle"] = -1
        rec["min_d2"] = np.inf
        head, size = int(vehicles["plan_head"][i]), int(vehicles["plan_size"][i])
        if head < 0 or size < 0 or head + size > max_states:
            rec["flags"] = abi.FH_OBSTACLE_BAD_PLAN
            continue
        mm = min(count, size) if count > 0 else size
        tested = list(range(0, mm, stride))
        rec["n_tested"] = len(tested)
        best, first, hitters = None, None, set()
        for j in tested:
            p = plans["pos"][i, head + j]
            if not np.isfinite(p).all():
                rec["flags"] |= abi.FH_OBSTACLE_NOT_FINITE
                continue
            if not m:
                continue
            c = centres(obs, taus(tick0, [j], par["dc"], variant), variant)[:, 0]
            with np.errstate(over="ignore", invalid="ignore"):
                d2 = d2_of(c - p[None])
            for o in np.nonzero(ok & np.isfinite(c).all(axis=1))[0]:
                key = (float(d2[o]), -j, -int(o)) if variant == "ties_larger" else (float(d2[o]), j, int(o))
                if d2[o] < np.inf and (best is None or key < best[0]):
                    best = (key, j, int(o))
                if (d2[o] <= hit2[o]) if variant == "le" else (d2[o] < hit2[o]):
                    hitters.add(int(o))
                    fkey = (j, -int(o)) if variant == "ties_larger" else (j, int(o))
                    if first is None or fkey < first[0]:
                        first = (fkey, j, int(o))
        if best is not None:
            rec["min_d2"], rec["worst"], rec["worst_obstacle"] = best[0][0], best[1], best[2]
        if first is not None:
            rec["first"], rec["first_obstacle"] = first[1], first[2]
            rec["flags"] |= abi.FH_OBSTACLE_HIT
        rec["n_hit"] = len(hitters)
    return out


def params(samples, stride, range, dc=0.125, r_detect=0.0, points=1, first_point=0, first_instant=0, window=0):  # noqa: A002
    return abi.default_obstacle_params(samples, stride, range, dc, r_detect, points, first_point, first_instant, window)


def layout(par, m, n_static=0):
    """(n_cloud, mask_words) that just hold the points of m obstacles behind first_point."""
    total = int(par["first_point"]) + m * int(par["samples"]) * int(par["points"])
    return max(total, n_static), abi.point_mask_words(max(total, n_static))
