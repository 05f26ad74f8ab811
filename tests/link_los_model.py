"""The radio link with a line of sight (include/fasterhip_link_los.h) restated in numpy: brute force over all pairs of vehicles, the
header's model word for word, on tests/link_model.py's views, edges and passes.  Everything is IEEE double and numpy fuses no
multiply-add, so `groups_los()` is what fh_fleet_link_groups_los_device must return in every byte.  There is no cell grid and no neighbour
list here: no output byte depends on either.  occ is the grid fh_map_occupancy returns ([mz][my][mx], non-zero = occupied), m_origin and
m_res its lattice.  `variant` names one deliberate mistake (tests/test_link_los_model.py shows which hand case each one changes); None is
the model.  Not a test file."""
import numpy as np

import link_model as lm

VARIANTS = ("from_observer", "ends_tested", "q_only", "full_cell_step", "outside_blocks", "le", "blocked_counts_twice")


def cell_of(x, m_origin, m_res):
    """The map cell of a point as three floored doubles (never converted: the ends of a ray are compared as the sensor compares them)."""
    return tuple(np.floor((np.float64(x[a]) - np.float64(m_origin[a])) / np.float64(m_res)) for a in range(3))


def sampled_cells(p, q, m_origin, m_res, variant=None):
    """The cells of the samples j = 1 .. K - 1 of the ray from p to q: ([K - 1] fx, fy, fz as floored doubles)."""
    p, q = np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)
    m_res = np.float64(m_res)
    d = q - p
    d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    dist = np.sqrt(d2)
    step = m_res if variant == "full_cell_step" else 0.5 * m_res
    K = max(1.0, float(np.ceil(dist / step)))
    j = np.arange(1, int(K), dtype=np.float64)
    t = j / np.float64(K)
    return tuple(np.floor((p[a] + d[a] * t - np.float64(m_origin[a])) / m_res) for a in range(3))


def blocked(p, q, occ, m_origin, m_res, variant=None):
    """Is the ray from p (the vehicle with the smaller index) to q blocked?"""
    fx, fy, fz = sampled_cells(p, q, m_origin, m_res, variant)
    if not len(fx):
        return False
    mz, my, mx = occ.shape
    pc, qc = cell_of(p, m_origin, m_res), cell_of(q, m_origin, m_res)
    at_p = (fx == pc[0]) & (fy == pc[1]) & (fz == pc[2])
    at_q = (fx == qc[0]) & (fy == qc[1]) & (fz == qc[2])
    if variant == "ends_tested":
        tested = np.ones(len(fx), dtype=bool)
    elif variant == "q_only":
        tested = ~at_q
    else:
        tested = ~at_p & ~at_q
    inside = (fx >= 0) & (fx < mx) & (fy >= 0) & (fy < my) & (fz >= 0) & (fz < mz)
    if variant == "outside_blocks" and (tested & ~inside).any():
        return True
    look = tested & inside
    return bool((occ[fz[look].astype(np.int64), fy[look].astype(np.int64), fx[look].astype(np.int64)] != 0).any())


def linked_los(par, vehicles, view_of, n_views, occ, m_origin, m_res, variant=None):
    """([n][n] bool linked, [n][n] bool blocked): entry [i][k] is what vehicle i finds about k; both are symmetric in the model (one
    orientation per pair) and False on the diagonal.  blocked: both speak, in range, and the ray is blocked."""
    n = len(vehicles)
    pos = vehicles["state"]["pos"].reshape(n, 3)
    near = lm.linked(par, vehicles, view_of, n_views, "le" if variant == "le" else None)   # both speak and in range
    adj = np.zeros((n, n), dtype=bool)
    blk = np.zeros((n, n), dtype=bool)
    for i in range(n):
        for k in range(n):
            if not near[i, k]:
                continue
            if variant == "from_observer":
                a, b = i, k
            else:
                a, b = min(i, k), max(i, k)
                if i > k:   # the same orientation whoever asks
                    adj[i, k], blk[i, k] = adj[k, i], blk[k, i]
                    continue
            blk[i, k] = blocked(pos[a], pos[b], occ, m_origin, m_res, variant)
            adj[i, k] = not blk[i, k]
    if variant != "from_observer":
        assert np.array_equal(adj, adj.T) and np.array_equal(blk, blk.T)
    return adj, blk


def groups_los(par, vehicles, view_of, n_views, occ, m_origin, m_res, variant=None, history=None):
    """(labels [n_views] int32, info [4] int64): link_model.groups on the pairs that are linked in line of sight."""
    n = len(vehicles)
    view = lm.views_of(n, view_of)
    adj, blk = linked_los(par, vehicles, view_of, n_views, occ, m_origin, m_res, variant)
    e = lm.edges(adj, view)
    L = np.arange(n_views, dtype=np.int64)
    if history is not None:
        history.append(L.copy())
    changed = 0
    for _ in range(int(par["passes"])):
        new = lm.one_pass(L.copy(), e)
        changed = int((new != L).sum())
        L = new
        if history is not None:
            history.append(L.copy())
    n_blocked = int(blk.sum()) if variant == "blocked_counts_twice" else int(np.triu(blk, 1).sum())
    info = np.array([changed, int((L == np.arange(n_views)).sum()), int(np.triu(adj, 1).sum()), n_blocked], dtype=np.int64)
    return L.astype(np.int32), info
