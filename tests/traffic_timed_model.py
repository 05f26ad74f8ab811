"""Time-aware traffic (include/fasterhip_traffic_timed.h) restated in numpy: brute force over all (i, k, s, s') with s' inside the
window (one array operation per offset s' - s), the header's model word for word.  Points and the comparison of results are tests/traffic_model.py's.  Everything is IEEE double and numpy fuses no
multiply-add, so `traffic_timed()` gives the cloud tail and the mask words the device must write, byte for byte.  `variant` names one
deliberate mistake (tests/test_traffic_timed_model.py shows which hand case each one changes); None is the model."""
import numpy as np

import traffic_model as tm
from faster_amd import abi

VARIANTS = ("le", "no_clamp", "self", "window_instants", "window_one_sided", "observer_unshown_matches", "ignores_first_instant", "state_pos")
assert_equal, fleet, layout, bit = tm.assert_equal, tm.fleet, tm.layout, tm.bit


def samples(par, vehicles, plans, max_states, variant=None):
    """tests/traffic_model.py's samples from the record's first_instant on."""
    first = 0 if variant == "ignores_first_instant" else int(par["first_instant"])
    return tm.samples(par, vehicles, plans, max_states, variant, first)


def decisions(par, vehicles, show, c, variant=None):
    """[n][n][S] bool: in row i, the decision of sample (k, s)."""
    n, S = show.shape
    rule, window, stride = int(par["rule"]), int(par["window"]), int(par["stride"])
    r2 = float(par["range"]) * float(par["range"])
    ks = np.arange(n)
    if variant == "window_instants":
        window = window // stride   # (the window counted in states)
    window = min(window, S - 1)       # (s' lies in [0, S - 1]: a larger window holds no more)
    on = np.zeros((n, n, S), dtype=bool)
    for i in range(n):
        if variant == "state_pos":   # (fasterhip_traffic.h's rule: one position, every instant)
            p = vehicles["state"]["pos"][i]
            finite = bool(np.isfinite(p).all())
            ci, showi = np.broadcast_to(p if finite else np.zeros(3), (S, 3)), np.full(S, finite)
        else:
            ci, showi = c[i], show[i]
        if variant == "observer_unshown_matches":
            showi = np.ones(S, dtype=bool)   # (c is zero where a sample does not show)
        met = np.zeros((n, S), dtype=bool)   # [k][s]: is there an s' = s + o inside the window and inside [0, S - 1] that is near?
        for o in range(0 if variant == "window_one_sided" else -window, window + 1):
            s0, s1 = max(0, -o), min(S, S - o)
            with np.errstate(over="ignore", invalid="ignore"):
                d = c[:, s0:s1] - ci[None, s0 + o:s1 + o]
                d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                near = (d2 <= r2) if variant == "le" else (d2 < r2)
            met[:, s0:s1] |= near & showi[None, s0 + o:s1 + o]
        seen = (ks != i) | (variant == "self")
        if rule == abi.FH_TRAFFIC_YIELD_TO_LOWER:
            seen = seen & (ks < i)
        on[i] = met & show & seen[:, None]
    return on


def traffic_timed(par, vehicles, plans, max_states, cloud, mask, variant=None):
    """(cloud [n_cloud][3], mask [n][mask_words] uint32) after the call, from those before it (copies)."""
    n, S, first = len(vehicles), int(par["samples"]), int(par["first_point"])
    assert 1 <= S <= abi.FH_TRAFFIC_TIMED_MAX_SAMPLES and int(par["window"]) >= 0 and int(par["first_instant"]) >= 0
    cloud = np.array(cloud, dtype=np.float64).reshape(-1, 3)
    mask = np.array(mask, dtype=np.uint32).reshape(max(n, 1), -1)[:n]
    if n == 0:
        return cloud, mask
    show, c = samples(par, vehicles, plans, max_states, variant)
    pts = tm.points(par, show, c)
    pps = pts.shape[2]
    total = n * S * pps
    assert first % 32 == 0 and first + total <= len(cloud) and first + total <= mask.shape[1] * 32
    cloud[first:first + total] = pts.reshape(-1, 3)   # every traffic point is written
    on = decisions(par, vehicles, show, c, variant)
    bits = np.repeat(on.reshape(n, n * S), pps, axis=1)   # all points of a sample share one decision
    w0, w1 = first // 32, -(-(first + total) // 32)
    padded = np.zeros((n, (w1 - w0) * 32), dtype=np.uint64)   # bits past the last traffic point in the last word are zero
    padded[:, :total] = bits
    mask[:, w0:w1] = (padded.reshape(n, w1 - w0, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)   # whole words
    return cloud, mask


def params(samples, stride, range, hull=0.0, rule=abi.FH_TRAFFIC_ALL, first_point=0, first_instant=0, window=0):  # noqa: A002
    return abi.default_traffic_timed_params(samples, stride, range, hull, rule, first_point, first_instant, window)


def untimed(par):
    """fh_traffic_params with the range, hull, samples, stride, rule and first_point of a timed record."""
    return abi.default_traffic_params(int(par["samples"]), int(par["stride"]), float(par["range"]), float(par["hull"]), int(par["rule"]),
                                      int(par["first_point"]))


def traffic_bits(par, n, mask):
    """[n][n S pps] bool: the traffic bits of every row."""
    first, total = int(par["first_point"]), n * int(par["samples"]) * abi.traffic_points_per_sample(par["hull"])
    m = np.ascontiguousarray(np.asarray(mask, dtype=np.uint32).reshape(n, -1)[:, first // 32:])
    return np.unpackbits(m.view(np.uint8), axis=1, bitorder="little")[:, :total].astype(bool)
