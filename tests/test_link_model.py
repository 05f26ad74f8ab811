"""The model of the radio link (tests/link_model.py, include/fasterhip_link.h) on the CPU: hand cases of the groups and of the merge,
settled labels against an independent union-find on random fleets, the header's three consequences after every pass, what the worst
arrangements need, and five wrong variants of the model, each of which changes a named hand case."""
import numpy as np
import pytest

from faster_amd import abi

import link_model as lm


def labels_of(positions, range_, view_of=None, n_views=None, passes=8, variant=None, history=None):
    v, vo = lm.fleet(positions, view_of)
    n_views = len(v) if n_views is None else n_views
    return lm.groups(lm.params(range_, passes), v, vo, n_views, variant, history)


# ---- hand cases of the groups ---------------------------------------------------------------------------------------------------------------
def test_two_vehicles_exactly_at_range_are_not_linked():
    L, info = labels_of([[0, 0, 0], [1.5, 0, 0]], 1.5)
    assert L.tolist() == [0, 1] and info.tolist() == [0, 2, 0, 0]
    L, info = labels_of([[0, 0, 0], [np.nextafter(1.5, 0), 0, 0]], 1.5)
    assert L.tolist() == [0, 0] and info.tolist() == [0, 1, 1, 0]
    # d2 is the sum of three products from left to right, compared with range * range rounded once
    p = np.array([0.1, 0.2, 0.3])
    d2 = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]
    r = float(np.sqrt(d2))
    want = d2 < r * r
    L, _ = labels_of([[0, 0, 0], p], r)
    assert (L[1] == 0) == want


def test_a_position_that_is_not_finite_does_not_speak():
    for bad in (np.nan, np.inf, -np.inf):
        L, info = labels_of([[0, 0, 0], [0.1, bad, 0], [0.2, 0, 0]], 1.0)
        assert L.tolist() == [0, 1, 0] and info.tolist() == [0, 2, 1, 0], bad


def test_a_view_number_out_of_range_does_not_speak():
    L, info = labels_of([[0, 0, 0], [0.1, 0, 0], [0.2, 0, 0], [0.3, 0, 0]], 1.0, view_of=[2, -1, 3, 1], n_views=3)
    assert L.tolist() == [0, 1, 1] and info.tolist() == [0, 2, 1, 0]   # vehicles 0 and 3 are linked: views 2 and 1; -1 and 3 are no views
    L, info = labels_of([[0, 0, 0], [0.1, 0, 0], [0.2, 0, 0]], 1.0, n_views=2)   # no view_of: vehicle 2 would be view 2 of 2
    assert L.tolist() == [0, 0] and info[2] == 1


def test_two_vehicles_of_one_view_and_a_view_with_no_vehicle():
    L, info = labels_of([[0, 0, 0], [0.1, 0, 0], [5, 0, 0]], 1.0, view_of=[3, 3, 0], n_views=5)
    assert L.tolist() == [0, 1, 2, 3, 4] and info.tolist() == [0, 5, 1, 0]   # the pair is counted; its edge 3 - 3 changes nothing
    L, info = labels_of([[0, 0, 0], [0.1, 0, 0], [0.2, 0, 0]], 1.0, view_of=[3, 3, 1], n_views=5)
    assert L.tolist() == [0, 1, 2, 1, 4] and info.tolist() == [0, 4, 3, 0]


def test_teams_bridged_by_one_pair():
    # team A (view 1) at x = 0 and 10, team B (view 2) at x = 10.5 and 30, a loner (view 0) far away
    L, info = labels_of([[0, 0, 0], [10, 0, 0], [10.5, 0, 0], [30, 0, 0], [0, 50, 0]], 1.0, view_of=[1, 1, 2, 2, 0], n_views=3)
    assert L.tolist() == [0, 1, 1] and info.tolist() == [0, 2, 1, 0]
    L, _ = labels_of([[0, 0, 0], [10, 0, 0], [10.5, 0, 0], [30, 0, 0], [0, 50, 0]], 0.4, view_of=[1, 1, 2, 2, 0], n_views=3)
    assert L.tolist() == [0, 1, 2]


# ---- the consequences -------------------------------------------------------------------------------------------------------------------------
def random_fleet(rng, n, n_views, box):
    pos = rng.uniform(0.0, box, size=(n, 3))
    view_of = rng.integers(-1, n_views + 1, size=n).astype(np.int32)   # some views out of range, some views with no vehicle
    pos[rng.integers(0, n)] = np.nan
    return pos, view_of


@pytest.mark.parametrize("seed", range(6))
def test_invariants_after_every_pass_and_settled_labels_are_component_minima(seed):
    rng = np.random.default_rng(seed)
    n, n_views = 70, 40
    pos, view_of = random_fleet(rng, n, n_views, box=(3.0, 5.0, 8.0)[seed % 3])
    v, vo = lm.fleet(pos, view_of)
    par = lm.params(1.0, n_views - 1)
    history = []
    L, info = lm.groups(par, v, vo, n_views, history=history)
    e = lm.edges(lm.linked(par, v, vo, n_views), lm.views_of(n, vo))
    comp = lm.components(n_views, e)
    for p, Lp in enumerate(history):
        assert (Lp <= np.arange(n_views)).all(), p                      # L[v] <= v
        assert np.array_equal(comp[Lp], comp), p                        # L[v] is a view of v's component
        if p:
            assert (Lp <= history[p - 1]).all(), p                      # (labels only fall)
    assert np.array_equal(L, comp) and info[0] == 0                     # n_views - 1 passes always suffice
    assert info[1] == len(set(comp.tolist())) and info[3] == 0
    adj = lm.linked(par, v, vo, n_views)
    assert info[2] == sum(1 for i in range(n) for k in range(i + 1, n) if adj[i, k]) > 0
    # the last pass that changes a label reports it, the pass after it reports 0
    need = lm.passes_needed(e, n_views)
    assert 1 <= need <= n_views - 1
    L_need, last = lm.groups(lm.params(1.0, need), v, vo, n_views)
    assert np.array_equal(L_need, comp) and last[0] != 0
    _, settled = lm.groups(lm.params(1.0, need + 1), v, vo, n_views)
    assert settled[0] == 0


def chain_edges(order):
    e = []
    for a, b in zip(order[:-1], order[1:]):
        e += [(int(a), int(b)), (int(b), int(a))]
    return e


@pytest.mark.parametrize("n,descending,far_end", ((64, 6, 63), (1024, 10, 1023)))
def test_what_the_worst_arrangements_need(n, descending, far_end):
    """The numbers the header states next to FH_LINK_DEFAULT_PASSES: a chain in descending index order doubles its reach per pass; an
    ascending chain whose minimum sits at the far end needs every one of the n_views - 1 passes that always suffice."""
    assert lm.passes_needed(chain_edges(range(n - 1, -1, -1)), n) == descending
    assert lm.passes_needed(chain_edges(list(range(1, n)) + [0]), n, limit=n - 1) == far_end == n - 1
    assert descending <= abi.FH_LINK_DEFAULT_PASSES == 32 <= abi.FH_LINK_MAX_PASSES == 1024
    p = abi.default_link_params(2.5)
    assert (float(p["range"]), int(p["passes"])) == (2.5, 32) and not p["reserved"].any()


# ---- the merge, hand labels ---------------------------------------------------------------------------------------------------------------------
HAND_LABELS = np.array([0, 0, 1, -1, 9, 5, 0, 7], dtype=np.int32)
# view 1 and 6 send to root 0; view 2's label 1 is not a root: alone; 3: negative; 4: >= n_views; 5 and 7: roots without senders


def hand_tables(stride=7, view_bytes=5, mask_words=3):
    rng = np.random.default_rng(3)
    flags = rng.integers(0, 6, size=len(HAND_LABELS) * stride).astype(np.uint8)
    mask = rng.integers(0, 1 << 32, size=(len(HAND_LABELS), mask_words), dtype=np.uint64).astype(np.uint32)
    return flags, mask


def test_merge_with_hand_labels():
    stride, vb, words = 7, 5, 3
    flags, mask = hand_tables(stride, vb, words)
    assert lm.senders(HAND_LABELS, 8).tolist() == [-1, 0, -1, -1, -1, -1, 0, -1]
    for shared in (0, 2, words):
        f, m = lm.merge(HAND_LABELS, flags, stride, vb, mask, shared)
        rows, before = f.reshape(8, stride), flags.reshape(8, stride)
        group = [0, 1, 6]
        zero = (before[group, :vb] == 0).any(axis=0)
        for v in group:
            assert (rows[v, :vb][zero] == 0).all() and np.array_equal(rows[v, :vb][~zero], before[v, :vb][~zero])
            assert np.array_equal(m[v, :shared], mask[0, :shared] | mask[1, :shared] | mask[6, :shared])
            assert np.array_equal(m[v, shared:], mask[v, shared:])                 # the traffic words are per observer
        assert np.array_equal(rows[:, vb:], before[:, vb:])                         # the padding
        for v in (2, 3, 4, 5, 7):                                                   # alone this call
            assert np.array_equal(rows[v], before[v]) and np.array_equal(m[v], mask[v])
        # a second merge changes nothing
        f2, m2 = lm.merge(HAND_LABELS, f, stride, vb, m, shared)
        assert np.array_equal(f2, f) and np.array_equal(m2, m)
    assert zero.any() and not zero.all()
    f, m = lm.merge(HAND_LABELS, None, stride, vb, mask, words)
    assert f is None and m is not None
    f, m = lm.merge(HAND_LABELS, flags, stride, vb, None, 0)
    assert m is None and f is not None


# ---- wrong variants: each changes a named hand case -------------------------------------------------------------------------------------------------
def test_variant_le_links_two_vehicles_exactly_at_range():
    L, _ = labels_of([[0, 0, 0], [1.5, 0, 0]], 1.5, variant="le")
    assert L.tolist() == [0, 0]


def test_variant_same_pass_settles_a_chain_in_fewer_passes():
    pos = [[float(i), 0, 0] for i in range(8)]
    view_of = [1, 2, 3, 4, 5, 6, 7, 0]    # the ascending chain with the minimum at the far end
    model, _ = labels_of(pos, 1.2, view_of, 8, passes=1)
    wrong, _ = labels_of(pos, 1.2, view_of, 8, passes=1, variant="same_pass")
    assert model.tolist() == [0, 1, 1, 1, 2, 3, 4, 0]
    assert wrong.tolist() != model.tolist() and (wrong <= model).all()


def test_variant_no_jump_leaves_a_descending_chain_one_hop_per_pass():
    pos = [[float(i), 0, 0] for i in range(8)]
    view_of = [7, 6, 5, 4, 3, 2, 1, 0]
    model, info = labels_of(pos, 1.2, view_of, 8, passes=3)
    wrong, _ = labels_of(pos, 1.2, view_of, 8, passes=3, variant="no_jump")
    assert model.tolist() == [0] * 8 and info[0] != 0      # pass 3 still changed labels; a fourth finds them settled
    assert wrong.tolist() == [0, 0, 0, 0, 1, 2, 3, 4]
    _, info = labels_of(pos, 1.2, view_of, 8, passes=4)
    assert info[0] == 0


def test_variant_or_traffic_merges_the_words_of_the_observers():
    flags, mask = hand_tables()
    _, model = lm.merge(HAND_LABELS, None, 7, 5, mask, 2)
    _, wrong = lm.merge(HAND_LABELS, None, 7, 5, mask, 2, variant="or_traffic")
    assert np.array_equal(model[:, :2], wrong[:, :2]) and not np.array_equal(model[[0, 1, 6], 2], wrong[[0, 1, 6], 2])


def test_variant_non_root_sends():
    flags, mask = hand_tables()
    model_f, model_m = lm.merge(HAND_LABELS, flags, 7, 5, mask, 3)
    wrong_f, wrong_m = lm.merge(HAND_LABELS, flags, 7, 5, mask, 3, variant="non_root_sends")
    assert np.array_equal(model_m[2], mask[2]) and not np.array_equal(wrong_m[2], mask[2])   # view 2, whose label 1 is no root
    assert not np.array_equal(model_f, wrong_f) or not np.array_equal(model_m, wrong_m)


def test_every_variant_is_named():
    assert set(lm.VARIANTS) == {"le", "same_pass", "no_jump", "or_traffic", "non_root_sends"}
