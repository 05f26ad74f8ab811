"""The priority rounds of a fleet (include/fasterhip_rounds.h) restated in numpy: brute force over all pairs and all instants, the header's
model word for word.  Everything is IEEE double and numpy fuses no multiply-add, so `classes()` is what the device must return in every
byte, and `gate()` what fh_fleet_round_gate_device writes.  There is no cell grid here: no field of a record depends on it.
`variant` names one deliberate mistake (tests/test_rounds_model.py shows which hand case each one changes); None is the model."""
import numpy as np

from faster_amd import abi

VARIANTS = ("min_size", "le", "from_stride", "vanish", "any_index", "no_clip", "same_pass", "overflow_ge")
POISON = 0xA5


def bad_extent(head, size, max_states):
    return head < 0 or size < 0 or head + size > max_states


def params(reach, rounds, passes=32, stride=1, count=0):
    p = np.zeros((), dtype=abi.round_params_dtype)
    p["reach"], p["rounds"], p["passes"], p["stride"], p["count"] = reach, rounds, passes, stride, count
    return p


def neighbours(par, vehicles, plans, max_states, variant=None):
    """(adj [n][n] bool, symmetric, False on the diagonal; flags [n]: FH_ROUND_BAD_PLAN and FH_ROUND_NOT_FINITE)."""
    n = len(vehicles)
    reach, stride, count = float(par["reach"]), int(par["stride"]), int(par["count"])
    r2 = reach * reach
    pos = np.asarray(plans).reshape(n, max_states)["pos"]
    heads, sizes = vehicles["plan_head"].astype(np.int64), vehicles["plan_size"].astype(np.int64)
    flags = np.zeros(n, dtype=np.int32)
    ok = np.zeros(n, dtype=bool)
    for i in range(n):
        h, s = int(heads[i]), int(sizes[i])
        if bad_extent(h, s, max_states):
            flags[i] |= abi.FH_ROUND_BAD_PLAN
            continue
        ok[i] = s >= 1
        m = min(count, s) if count > 0 else s
        read = pos[i, h + np.arange(0, m, stride, dtype=np.int64)]
        if s >= 1 and (count == 0 or s < count):
            read = np.concatenate([read, pos[i, h + s - 1][None, :]])
        if not np.isfinite(read).all():
            flags[i] |= abi.FH_ROUND_NOT_FINITE
    adj = np.zeros((n, n), dtype=bool)
    for i in range(n):
        for k in range(i):
            if not (ok[i] and ok[k]):
                continue
            si, sk = int(sizes[i]), int(sizes[k])
            M = min(si, sk) if variant == "min_size" else max(si, sk)
            if count > 0:
                M = min(M, count)
            js = np.arange(stride if variant == "from_stride" else 0, M, stride, dtype=np.int64)
            if variant == "vanish":
                js = js[js < min(si, sk)]   # (a plan that has ended is nowhere)
            if not len(js):
                continue
            p = pos[i, heads[i] + np.minimum(js, si - 1)]
            q = pos[k, heads[k] + np.minimum(js, sk - 1)]
            with np.errstate(over="ignore", invalid="ignore"):
                d = q - p
                d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                hit = (d2 <= r2) if variant == "le" else (d2 < r2)
            adj[i, k] = adj[k, i] = bool(hit.any())
    return adj, flags


def classes_from(adj, flags, rounds, passes, variant=None):
    """[n] abi.plan_round_dtype from the neighbour matrix: pass 0, the passes, the rest."""
    n = len(adj)
    out = np.zeros(n, dtype=abi.plan_round_dtype)
    out["flags"] = flags
    lower = [np.nonzero(adj[i, :n if variant == "any_index" else i])[0] for i in range(n)]
    clip = (lambda c: c) if variant == "no_clip" else (lambda c: min(c, rounds - 1))
    for i in range(n):
        out["n_lower"][i] = len(lower[i])
        over = len(lower[i]) >= abi.FH_ROUNDS_LIST if variant == "overflow_ge" else len(lower[i]) > abi.FH_ROUNDS_LIST
        if len(lower[i]) == 0:
            out["round_class"][i], out["decided_pass"][i] = 0, 0
        elif over:
            out["round_class"][i], out["decided_pass"][i] = rounds - 1, 0
            out["flags"][i] |= abi.FH_ROUND_OVERFLOW
        else:
            out["round_class"][i], out["decided_pass"][i] = -1, -1
    for p in range(1, passes + 1):
        seen = out if variant == "same_pass" else out.copy()   # (the model: nothing a pass decides is seen by that pass)
        for i in range(n):
            if out["decided_pass"][i] >= 0:
                continue
            dp = seen["decided_pass"][lower[i]]
            if ((dp >= 0) & ((dp <= p) if variant == "same_pass" else (dp < p))).all():
                taken = set(int(c) for c in seen["round_class"][lower[i]])
                mex = 0
                while mex in taken:
                    mex += 1
                out["round_class"][i], out["decided_pass"][i] = clip(mex), p
    rest = out["decided_pass"] < 0
    out["round_class"][rest], out["decided_pass"][rest] = rounds - 1, -1
    out["flags"][rest] |= abi.FH_ROUND_UNSETTLED
    return out


def classes(par, vehicles, plans, max_states, variant=None):
    """[n] abi.plan_round_dtype.  plans: [n][max_states] abi.state_dtype."""
    adj, flags = neighbours(par, vehicles, plans, max_states, variant)
    return classes_from(adj, flags, int(par["rounds"]), int(par["passes"]), variant)


def greedy(adj, rounds):
    """Sequential greedy colouring in index order, clipped at rounds - 1: what the passes settle to."""
    n = len(adj)
    c = np.zeros(n, dtype=np.int32)
    for i in range(n):
        taken = set(int(c[k]) for k in np.nonzero(adj[i, :i])[0])
        mex = 0
        while mex in taken:
            mex += 1
        c[i] = min(mex, rounds - 1)
    return c


def gate(records, round, active_begin, vehicles):  # noqa: A002  (the header's word)
    """fh_fleet_round_gate_device on host arrays: (vehicles with `active` rewritten, d_active [n] int32)."""
    on = np.asarray(active_begin) != 0
    if round >= 0:
        on = on & (records["round_class"] == round)
    elif round == abi.FH_ROUND_RETRY:
        on = on & (vehicles["stage"] == abi.FH_FLEET_STAGE_CONFLICT)
    else:
        assert round == abi.FH_ROUND_RESTORE
    v = vehicles.copy()
    v["active"] = on.astype(np.int32)
    return v, on.astype(np.int32)


def fixed_records(cls):
    """The records of a fleet whose classes are given (Fleet.enable_rounds(classes=...)): decided in pass 0, nothing measured."""
    out = np.zeros(len(cls), dtype=abi.plan_round_dtype)
    out["round_class"] = cls
    return out


def fleet(plan_positions, max_states=None, heads=None):
    """(vehicles [n], plans [n][max_states]) from a list of [size][3] position arrays; what lies outside a plan is far from everything."""
    n = len(plan_positions)
    heads = [0] * n if heads is None else list(heads)
    ps = [np.asarray(p, dtype=np.float64).reshape(-1, 3) for p in plan_positions]
    max_states = max_states or max([len(p) + h for p, h in zip(ps, heads)] + [1])
    v = np.zeros(n, dtype=abi.vehicle_dtype)
    pl = np.zeros((n, max_states), dtype=abi.state_dtype)
    pl["pos"] = 1e6
    for i, (p, h) in enumerate(zip(ps, heads)):
        v["plan_head"][i], v["plan_size"][i] = h, len(p)
        pl["pos"][i, h:h + len(p)] = p
    return v, pl


def assert_equal_records(got, want, what=""):
    """Every byte of every record: field by field for the message, then the raw bytes."""
    assert got.dtype == want.dtype == abi.plan_round_dtype and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    for k in abi.plan_round_dtype.names:
        bad = np.nonzero(got[k] != want[k])[0]
        assert not len(bad), "%s field %s differs at records %s: device %s, model %s" % (what, k, bad[:8], got[k][bad[:8]], want[k][bad[:8]])
    assert got.tobytes() == want.tobytes(), what
