"""The separation of committed plans (include/fasterhip_separation.h) restated in numpy: brute force over all pairs of vehicles, the
header's model word for word.  Everything is IEEE double and numpy fuses no multiply-add, so `separation()` is what the device must
return bit for bit.  There is no cell grid here: no field of a record depends on it.  `variant` names one deliberate mistake
(tests/test_separation_model.py shows which hand case each one changes); None is the model."""
import numpy as np

from faster_amd import abi

VARIANTS = ("no_hover", "le", "larger_k_on_ties", "self_pair", "bad_as_other")
INF = float("inf")


def tested_indexes(plan_size, stride, count):
    m = min(count, plan_size) if count > 0 else plan_size
    n = -(-m // stride)
    return np.arange(n, dtype=np.int64) * stride, n


def _bad(head, size, max_states):
    return head < 0 or size < 0 or head + size > max_states


def separation(par, vehicles, plans, max_states, variant=None):
    """[n] abi.plan_separation_dtype.  plans: [n][max_states] abi.state_dtype."""
    n = len(vehicles)
    out = np.zeros(n, dtype=abi.plan_separation_dtype)
    out["first"] = out["first_other"] = out["worst"] = out["worst_other"] = -1
    out["min_d2"] = INF
    r, cap, stride, count = float(par["r"]), float(par["cap"]), int(par["stride"]), int(par["count"])
    r2, cap2 = r * r, cap * cap
    plans = np.asarray(plans).reshape(n, max_states)
    heads, sizes = vehicles["plan_head"].astype(np.int64), vehicles["plan_size"].astype(np.int64)
    bad = np.array([_bad(int(heads[k]), int(sizes[k]), max_states) for k in range(n)], dtype=bool)
    for i in range(n):
        o = out[i]
        if bad[i]:
            o["flags"] = abi.FH_SEP_BAD_PLAN
            continue
        js, o["n_tested"] = tested_indexes(int(sizes[i]), stride, count)
        pos = plans[i, heads[i] + js]["pos"] if len(js) else np.zeros((0, 3))
        ok = np.isfinite(pos).all(axis=1)
        fl = 0 if ok.all() else abi.FH_SEP_NOT_FINITE
        pos, js = pos[ok], js[ok]
        ks = np.array([k for k in range(n) if (k != i or variant == "self_pair") and (sizes[k] >= 1 if not bad[k] else variant == "bad_as_other")],
                      dtype=np.int64)
        best, first, n_near = (INF, -1, -1), (-1, -1), 0   # (d2, j, k); (j, k)
        if len(js) and len(ks):
            # (variant bad_as_other only: a bad record is read as if it were good, one state, clipped to the array)
            hk = np.where(bad[ks], np.clip(heads[ks], 0, max_states - 1), heads[ks])
            sk = np.where(bad[ks], 1, sizes[ks])
            idx = np.minimum(js[None, :], sk[:, None] - 1)   # [K, T]: a vehicle whose plan has ended stands at its last state
            q = plans["pos"][ks[:, None], hk[:, None] + idx]  # [K, T, 3]
            if variant == "no_hover":
                q = np.where((js[None, :] < sk[:, None])[..., None], q, np.nan)
            with np.errstate(over="ignore", invalid="ignore"):
                d = q - pos[None, :, :]
                d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                seen = (d2 <= cap2) if variant == "le" else (d2 < cap2)
                near = ((d2 <= r2) if variant == "le" else (d2 < r2)) & seen
            pick = (lambda col: int(ks[np.nonzero(col)[0][-1 if variant == "larger_k_on_ties" else 0]]))  # noqa: E731
            if seen.any():
                d2s = np.where(seen, d2, INF)
                attains = d2s == d2s.min()
                t = int(np.argmax(attains.any(axis=0)))   # the smallest j that attains the minimum, then the smallest k at that j
                best = (float(d2s.min()), int(js[t]), pick(attains[:, t]))
            if near.any():
                t = int(np.argmax(near.any(axis=0)))
                first = (int(js[t]), pick(near[:, t]))
                n_near = int(near.any(axis=1).sum())
        o["min_d2"], o["worst"], o["worst_other"] = best
        o["first"], o["first_other"] = first
        o["n_near"] = n_near
        o["flags"] = fl | (abi.FH_SEP_NEAR if first[0] >= 0 else 0)
    return out


def fleet(plan_positions, max_states=None, heads=None):
    """(vehicles [n], plans [n][max_states]) from a list of [size][3] position arrays (an empty list: an empty plan)."""
    n = len(plan_positions)
    heads = [0] * n if heads is None else list(heads)
    ps = [np.asarray(p, dtype=np.float64).reshape(-1, 3) for p in plan_positions]
    max_states = max_states or max(max(len(p) + h for p, h in zip(ps, heads)), 1)
    v = np.zeros(n, dtype=abi.vehicle_dtype)
    pl = np.zeros((n, max_states), dtype=abi.state_dtype)
    pl["pos"] = 1e6   # (what lies outside the plans is far from everything: reading it shows)
    for i, (p, h) in enumerate(zip(ps, heads)):
        v["plan_head"][i], v["plan_size"][i] = h, len(p)
        pl["pos"][i, h:h + len(p)] = p
    return v, pl


def params(r, cap, stride=1, count=0):
    p = np.zeros((), dtype=abi.separation_params_dtype)
    p["r"], p["cap"], p["stride"], p["count"] = r, cap, stride, count
    return p


def assert_equal_records(got, want, what=""):
    """Every byte of every record: field by field for the message (the doubles as their 64-bit patterns), then the raw bytes."""
    assert got.dtype == want.dtype == abi.plan_separation_dtype and got.shape == want.shape
    if not len(got):
        return
    for k in abi.plan_separation_dtype.names:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.dtype.kind == "f":
            a, b = a.view(np.uint64), b.view(np.uint64)
        bad = np.nonzero((a != b).reshape(len(got), -1).any(axis=1))[0]
        assert not len(bad), "%s field %s differs at records %s: device %s, model %s" % (what, k, bad[:8], got[k][bad[:8]], want[k][bad[:8]])
    assert got.tobytes() == want.tobytes(), what
