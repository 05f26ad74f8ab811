"""The radio link of a fleet (include/fasterhip_link.h) restated in numpy: brute force over all pairs of vehicles, the header's model word
for word.  Everything is IEEE double and numpy fuses no multiply-add, so `groups()` is what fh_fleet_link_groups_device must return in
every byte and `merge()` what fh_fleet_link_merge_device leaves in the two tables.  There is no cell grid and no neighbour list here: no
output byte depends on either.  `variant` names one deliberate mistake (tests/test_link_model.py shows which hand case each one changes);
None is the model."""
import numpy as np

from faster_amd import abi

VARIANTS = ("le", "same_pass", "no_jump", "or_traffic", "non_root_sends")


def params(range_, passes=None):
    p = abi.default_link_params(range_)
    if passes is not None:
        p["passes"] = passes
    return p


def fleet(positions, view_of=None):
    """([n] abi.vehicle_dtype with state.pos = positions, view_of as int32 or None)."""
    pos = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    v = np.zeros(len(pos), dtype=abi.vehicle_dtype)
    v["state"]["pos"] = pos
    return v, (None if view_of is None else np.asarray(view_of, dtype=np.int32).reshape(-1))


def views_of(n, view_of):
    return np.arange(n, dtype=np.int64) if view_of is None else np.asarray(view_of, dtype=np.int64).reshape(-1)


def speaks(vehicles, view_of, n_views):
    n = len(vehicles)
    view = views_of(n, view_of)
    pos = vehicles["state"]["pos"].reshape(n, 3)
    return (view >= 0) & (view < n_views) & np.isfinite(pos).all(axis=1)


def linked(par, vehicles, view_of, n_views, variant=None):
    """[n][n] bool, symmetric, False on the diagonal."""
    n = len(vehicles)
    r = float(par["range"])
    r2 = r * r
    pos = vehicles["state"]["pos"].reshape(n, 3)
    ok = speaks(vehicles, view_of, n_views)
    adj = np.zeros((n, n), dtype=bool)
    for i in range(n):
        if not ok[i]:
            continue
        with np.errstate(over="ignore", invalid="ignore"):
            d = pos - pos[i]
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            hit = (d2 <= r2) if variant == "le" else (d2 < r2)
        adj[i] = hit & ok
        adj[i, i] = False
    assert np.array_equal(adj, adj.T)
    return adj


def edges(adj, view):
    """The edges between views as a set of (view(i), view(k)), both directions."""
    ii, kk = np.nonzero(adj)
    return sorted(set(zip(view[ii].tolist(), view[kk].tolist())))


def one_pass(L, edge_list, variant=None):
    """Labels after one pass: the hook reads only the labels of the pass before, then the jump."""
    seen = L if variant == "same_pass" else L.copy()
    H = L if variant == "same_pass" else L.copy()
    for a, b in edge_list:
        H[a] = min(H[a], seen[b])
    if variant == "no_jump":
        return H.copy()
    return H[H]


def groups(par, vehicles, view_of, n_views, variant=None, history=None):
    """(labels [n_views] int32, info [4] int64).  history: a list that receives the labels after every pass, L0 first."""
    n = len(vehicles)
    view = views_of(n, view_of)
    adj = linked(par, vehicles, view_of, n_views, variant)
    e = edges(adj, view)
    L = np.arange(n_views, dtype=np.int64)
    if history is not None:
        history.append(L.copy())
    changed = 0
    for _ in range(int(par["passes"])):
        new = one_pass(L.copy(), e, variant)
        changed = int((new != L).sum())
        L = new
        if history is not None:
            history.append(L.copy())
    info = np.array([changed, int((L == np.arange(n_views)).sum()), int(np.triu(adj, 1).sum()), 0], dtype=np.int64)
    return L.astype(np.int32), info


def passes_needed(adj_views_edges, n_views, limit=None):
    """The first pass after which the labels no longer change (0: identity is settled)."""
    L = np.arange(n_views, dtype=np.int64)
    p = 0
    while True:
        new = one_pass(L.copy(), adj_views_edges)
        if np.array_equal(new, L):
            return p
        L, p = new, p + 1
        assert limit is None or p <= limit


def components(n_views, edge_list):
    """The smallest view of the connected component of every view, by an independent union-find."""
    parent = list(range(n_views))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in edge_list:
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(v) for v in range(n_views)], dtype=np.int32)


def senders(labels, n_views, variant=None):
    """[n_views] the root every view sends to, -1 for a view that is alone or a root."""
    lab = np.asarray(labels, dtype=np.int64).reshape(-1)
    to = np.full(n_views, -1, dtype=np.int64)
    for v in range(n_views):
        r = int(lab[v])
        if 0 <= r < n_views and r != v and (variant == "non_root_sends" or lab[r] == r):
            to[v] = r
    return to


def merge(labels, flags, view_stride, view_bytes, mask, shared_words, variant=None):
    """The two tables after fh_fleet_link_merge_device, as copies: flags a flat uint8 array of n_views rows view_stride apart (or None),
    mask [n_views][mask_words] uint32 (or None)."""
    n_views = len(labels)
    to = senders(labels, n_views, variant)
    members = {}
    for v in range(n_views):
        if to[v] >= 0:
            members.setdefault(int(to[v]), [int(to[v])]).append(v)
    out_f = None if flags is None else np.array(flags, dtype=np.uint8).reshape(-1).copy()
    out_m = None if mask is None else np.array(mask, dtype=np.uint32).copy()
    for r, group in members.items():
        if out_f is not None and view_bytes:
            rows = np.stack([np.asarray(flags).reshape(-1)[v * view_stride:v * view_stride + view_bytes] for v in group])
            zero = (rows == 0).any(axis=0)
            for v in group:
                out_f[v * view_stride:v * view_stride + view_bytes][zero] = 0
        if out_m is not None:
            words = out_m.shape[1] if variant == "or_traffic" else shared_words
            both = np.bitwise_or.reduce(np.asarray(mask, dtype=np.uint32)[group, :words], axis=0)
            for v in group:
                out_m[v, :words] = both
    return out_f, out_m
