"""The commit check of a fleet (include/fasterhip_check.h) restated in numpy: brute force over all pairs and all instants, the header's
model word for word.  Everything is IEEE double and numpy fuses no multiply-add, so `check()` is what the device must return in every
byte; `backup()` and `revert()` are the two copies on byte arrays.  There is no cell grid here: no field of a record depends on it.
`variant` names one deliberate mistake (tests/test_check_model.py shows which hand case each one changes); None is the model."""
import numpy as np

from faster_amd import abi

VARIANTS = ("le", "from_zero", "own_size_only", "no_kind1", "kind1_of_higher", "larger_k_on_ties", "bad_as_other")
INF = float("inf")
POISON = 0xA5


def bad_extent(head, size, max_states):
    return head < 0 or size < 0 or head + size > max_states


def params(r, stride=1, count=0):
    p = np.zeros((), dtype=abi.check_params_dtype)
    p["r"], p["stride"], p["count"] = r, stride, count
    return p


def candidates(vehicles, backup_vehicles, max_states):
    """(candidate [n] bool, old_ok [n] bool): who is checked, and whose old plan is an other of everyone else."""
    n = len(vehicles)
    cand, old_ok = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    for k in range(n):
        c, o = vehicles[k], backup_vehicles[k]
        bad_o = bad_extent(int(o["plan_head"]), int(o["plan_size"]), max_states)
        bad_c = bad_extent(int(c["plan_head"]), int(c["plan_size"]), max_states)
        old_ok[k] = not bad_o and int(o["plan_size"]) >= 1
        cand[k] = int(c["stage"]) == abi.FH_FLEET_STAGE_COMMITTED and int(c["active"]) != 0 and not bad_o and not bad_c
    return cand, old_ok


def check(par, vehicles, plans, backup_vehicles, backup_plans, max_states, variant=None):
    """[n] abi.plan_check_dtype.  plans, backup_plans: [n][max_states] abi.state_dtype."""
    n = len(vehicles)
    out = np.zeros(n, dtype=abi.plan_check_dtype)
    out["first"] = out["first_other"] = out["first_kind"] = -1
    out["d2"] = INF
    r, stride, count = float(par["r"]), int(par["stride"]), int(par["count"])
    r2 = r * r
    pos = (np.asarray(backup_plans).reshape(n, max_states)["pos"], np.asarray(plans).reshape(n, max_states)["pos"])   # [kind]
    cur = pos[1]
    cand, old_ok = candidates(vehicles, backup_vehicles, max_states)
    for i in range(n):
        if not cand[i]:
            continue
        o = out[i]
        hi, si = int(vehicles["plan_head"][i]), int(vehicles["plan_size"][i])
        so = int(backup_vehicles["plan_size"][i])
        kept = so - int(backup_vehicles["k_end_whole"][i]) - 1
        flags = abi.FH_CHECK_CANDIDATE
        if kept < 0 or kept > min(so, si):
            flags |= abi.FH_CHECK_BAD_PLAN
            kept = min(max(kept, 0), min(so, si))
        if variant == "from_zero":
            kept = 0
        m_own = min(count, si) if count > 0 else si
        own = np.arange(kept, m_own, stride, dtype=np.int64)
        o["n_tested"] = len(own)
        read = cur[i, hi + own]
        if si >= 1 and (count == 0 or si < count):
            read = np.concatenate([read, cur[i, hi + si - 1][None, :]])
        if not np.isfinite(read).all():
            flags |= abi.FH_CHECK_NOT_FINITE
        others = []   # (k, kind, head, size), sorted by (k, kind)
        for k in range(n):
            if k == i:
                continue
            hk, sk = int(backup_vehicles["plan_head"][k]), int(backup_vehicles["plan_size"][k])
            if old_ok[k]:
                others.append((k, 0, hk, sk))
            elif variant == "bad_as_other":   # (a bad record read as if it were good: one state, clipped into the array)
                others.append((k, 0, min(max(hk, 0), max_states - 1), 1))
            if (k < i or variant == "kind1_of_higher") and cand[k] and int(vehicles["plan_size"][k]) >= 1 and variant != "no_kind1":
                others.append((k, 1, int(vehicles["plan_head"][k]), int(vehicles["plan_size"][k])))
        if si >= 1 and others:
            ks, kinds, hs, ss = (np.array(c, dtype=np.int64) for c in zip(*others))
            M = np.full(len(ks), si) if variant == "own_size_only" else np.maximum(si, ss)
            if count > 0:
                M = np.minimum(M, count)
            js = np.arange(kept, int(M.max()), stride, dtype=np.int64)
            if len(js):
                p = cur[i, hi + np.minimum(js, si - 1)]                                  # [T, 3]
                idx = hs[:, None] + np.minimum(js[None, :], ss[:, None] - 1)             # [K, T]
                q = np.where((kinds == 1)[:, None, None], pos[1][ks[:, None], idx], pos[0][ks[:, None], idx])
                with np.errstate(over="ignore", invalid="ignore"):
                    d = q - p[None, :, :]
                    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                    hit = ((d2 <= r2) if variant == "le" else (d2 < r2)) & (js[None, :] < M[:, None])
                if hit.any():
                    t = int(np.argmax(hit.any(axis=0)))   # the smallest j, then the smallest k at that j, then the smaller kind
                    rows = np.nonzero(hit[:, t])[0]
                    e = int(rows[0])
                    if variant == "larger_k_on_ties":
                        e = int(rows[ks[rows] == ks[rows].max()][0])
                    o["first"], o["first_other"], o["first_kind"], o["d2"] = int(js[t]), int(ks[e]), int(kinds[e]), d2[e, t]
                    flags |= abi.FH_CHECK_CONFLICT
        o["flags"] = flags
    return out


def backup(vehicles, plans, max_states, backup_vehicles, backup_plans):
    """fh_fleet_backup_device on host arrays, in place: every record, and the live extent of every good one."""
    n = len(vehicles)
    backup_vehicles[:] = vehicles
    plans, backup_plans = np.asarray(plans).reshape(n, max_states), backup_plans.reshape(n, max_states)
    for k in range(n):
        h, s = int(vehicles["plan_head"][k]), int(vehicles["plan_size"][k])
        if not bad_extent(h, s, max_states):
            backup_plans[k, h:h + s] = plans[k, h:h + s]


def revert(records, backup_vehicles, backup_plans, max_states, vehicles, plans):
    """fh_fleet_revert_device on host arrays, in place.  Returns [n][max_states] bool: the states whose bytes are unspecified afterwards
    (those of a reverted plan outside the restored extent)."""
    n = len(vehicles)
    plans, backup_plans = plans.reshape(n, max_states), np.asarray(backup_plans).reshape(n, max_states)
    loose = np.zeros((n, max_states), dtype=bool)
    for k in range(n):
        if not int(records["flags"][k]) & abi.FH_CHECK_CONFLICT:
            continue
        vehicles[k] = backup_vehicles[k]
        vehicles["stage"][k] = abi.FH_FLEET_STAGE_CONFLICT
        h, s = int(backup_vehicles["plan_head"][k]), int(backup_vehicles["plan_size"][k])
        loose[k] = True
        if not bad_extent(h, s, max_states):
            plans[k, h:h + s] = backup_plans[k, h:h + s]
            loose[k, h:h + s] = False
    return loose


def scene(old_positions, commits, max_states=None, heads=None):
    """(vehicles, plans, backup_vehicles, backup_plans) of one cycle.  old_positions: a list of [size][3] arrays, the plans before the
    cycle; commits: {i: (k_end_whole, new positions)}: vehicle i is active, and its commit is laid out as fh_fleet_commit_device does it:
    the first kept = size - k_end_whole - 1 states of its old plan move to index 0 and the new ones follow them."""
    heads = [0] * len(old_positions) if heads is None else list(heads)
    sizes = [len(np.asarray(p, dtype=np.float64).reshape(-1, 3)) for p in old_positions]
    need = [h + s for h, s in zip(heads, sizes)]
    for i, (k_end, new) in commits.items():
        need.append(max(sizes[i] - k_end - 1, 0) + len(np.asarray(new, dtype=np.float64).reshape(-1, 3)))
    old_v, old_pl = fleet(old_positions, max_states or max(max(need), 1), heads)
    for i, (k_end, _) in commits.items():
        old_v["k_end_whole"][i], old_v["active"][i] = k_end, 1
    v, pl = old_v.copy(), old_pl.copy()
    for i, (k_end, new) in commits.items():
        new = np.asarray(new, dtype=np.float64).reshape(-1, 3)
        kept = min(max(sizes[i] - k_end - 1, 0), sizes[i])
        keep = old_pl[i, heads[i]:heads[i] + kept].copy()
        pl["pos"][i] = 1e6   # (what lies outside the plan is far from everything)
        pl[i, :kept] = keep
        pl["pos"][i, kept:kept + len(new)] = new
        v["plan_head"][i], v["plan_size"][i], v["stage"][i] = 0, kept + len(new), abi.FH_FLEET_STAGE_COMMITTED
    return v, pl, old_v, old_pl


def fleet(plan_positions, max_states=None, heads=None, k_end_whole=None):
    """(vehicles [n], plans [n][max_states]) from a list of [size][3] position arrays: the old side of a check, nobody active."""
    n = len(plan_positions)
    heads = [0] * n if heads is None else list(heads)
    ps = [np.asarray(p, dtype=np.float64).reshape(-1, 3) for p in plan_positions]
    max_states = max_states or max(max(len(p) + h for p, h in zip(ps, heads)), 1)
    v = np.zeros(n, dtype=abi.vehicle_dtype)
    pl = np.zeros((n, max_states), dtype=abi.state_dtype)
    pl["pos"] = 1e6
    for i, (p, h) in enumerate(zip(ps, heads)):
        v["plan_head"][i], v["plan_size"][i] = h, len(p)
        pl["pos"][i, h:h + len(p)] = p
    if k_end_whole is not None:
        v["k_end_whole"] = k_end_whole
    return v, pl


def near_pairs(r, vehicles, plans, max_states, separation=None):
    """The set of unordered pairs (i, k), i < k, that the separation's model (tests/separation_model.py, the judge of the invariant)
    calls near at radius r over whole plans: either record of the pair says so, asked on the fleet of those two alone.  `separation`
    replaces the model's function by another with its signature (the device's)."""
    import separation_model as sm

    separation = separation or sm.separation
    n = len(vehicles)
    plans = np.asarray(plans).reshape(n, max_states)
    par = sm.params(r, r)
    whole = separation(par, vehicles, plans, max_states)
    flagged = (whole["flags"] & abi.FH_SEP_NEAR) != 0
    pairs = set()
    for i in range(n):
        for k in range(i + 1, n):
            if flagged[i] or flagged[k]:   # (a pair is near iff one of its two records is near because of the other)
                two = separation(par, vehicles[[i, k]], plans[[i, k]], max_states)
                if (two["flags"] & abi.FH_SEP_NEAR).any():
                    pairs.add((i, k))
    return pairs


def assert_equal_records(got, want, what=""):
    """Every byte of every record: field by field for the message (the doubles as their 64-bit patterns), then the raw bytes."""
    assert got.dtype == want.dtype == abi.plan_check_dtype and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    if not len(got):
        return
    for k in abi.plan_check_dtype.names:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.dtype.kind == "f":
            a, b = a.view(np.uint64), b.view(np.uint64)
        bad = np.nonzero(a != b)[0]
        assert not len(bad), "%s field %s differs at records %s: device %s, model %s" % (what, k, bad[:8], got[k][bad[:8]], want[k][bad[:8]])
    assert got.tobytes() == want.tobytes(), what
