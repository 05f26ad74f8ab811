"""The model of the radio link with a line of sight (include/fasterhip_link_los.h; tests/link_los_model.py) on the hand cases of
tests/link_los_cases.py and on random fleets, without a device: every hand case gives the labels and info written next to it; every
variant of the model (one deliberate mistake each) changes a named hand case; a seeded search finds a pair whose answer depends on the
orientation of the ray; and the header's three consequences and the info[2] + info[3] identity hold against tests/link_model.py.
The occupancy comes from the map read on the host (tests/map_read_model.py); tests/test_gpu_link_los.py holds the device's
fh_map_occupancy to the same grid."""
import numpy as np
import pytest

import link_los_cases as lc
import link_los_model as ll
import link_model as lm
import map_read_model as mr


@pytest.fixture(scope="module")
def scene():
    occ, dims, origin = mr.occupancy(lc.cloud(), **lc.READ)
    assert tuple(dims) == lc.DIMS and tuple(float(o) for o in origin) == lc.ORIGIN   # exactly: boundaries at multiples of 0.2
    assert np.array_equal(occ, lc.expected_occupancy())
    return occ, np.asarray(origin, dtype=np.float64)


@pytest.fixture(scope="module")
def forest():
    occ, dims, origin = mr.occupancy(lc.forest_cloud(), **lc.READ)
    assert tuple(dims) == lc.DIMS and 0 < (occ != 0).sum() < occ.size // 2
    return occ, np.asarray(origin, dtype=np.float64)


@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_hand_case(scene, name):
    occ, origin = scene
    par, v, vo, n_views, want_l, want_i = lc.case(name)
    got_l, got_i = ll.groups_los(par, v, vo, n_views, occ, origin, lc.RES)
    assert got_l.tolist() == want_l.tolist() and got_i.tolist() == want_i.tolist(), name
    plain_l, plain_i = lm.groups(par, v, vo, n_views)
    assert got_i[2] + got_i[3] == plain_i[2] and plain_i[3] == 0


def test_the_hand_cases_are_what_their_names_say(scene):
    occ, origin = scene
    pos = lambda name: np.array(lc.CASES[name][0], dtype=np.float64)   # noqa: E731
    cells = lambda p, q: ll.sampled_cells(p, q, origin, lc.RES)        # noqa: E731
    # the door is one cell wide and the ray through it is tested there (not exempt, not outside)
    p, q = pos("through_the_door")
    fx, fy, fz = cells(p, q)
    assert set(fy.tolist()) == {14.0} and {9.0, 10.0, 11.0} <= set(fx.tolist()) and (occ[2, 14, 9:12] == 0).all() and (occ[2, 13, 9:12] != 0).all()
    p, q = pos("clips_the_jamb")
    fx, fy, fz = cells(p, q)
    assert ((fy == 15.0) & (fx == 11.0)).any() and not ((fy == 15.0) & (fx < 11.0)).any()
    # the vehicle in the wall stands in an occupied cell, and the samples in that cell are the only occupied ones of its ray
    p, q = pos("inside_an_inflated_cell")
    pc = ll.cell_of(p, origin, lc.RES)
    assert pc == (9.0, 5.0, 2.0) and occ[2, 5, 9] != 0
    fx, fy, fz = cells(p, q)
    hit = occ[fz.astype(int), fy.astype(int), fx.astype(int)] != 0
    assert hit.any() and (fx[hit] == 9.0).all()
    p, q = pos("two_in_one_cell")
    assert ll.cell_of(p, origin, lc.RES) == ll.cell_of(q, origin, lc.RES) == (10.0, 4.0, 2.0) and len(cells(p, q)[0]) == 1
    p, q = pos("nearer_than_half_a_cell")
    assert len(cells(p, q)[0]) == 0 and ll.cell_of(p, origin, lc.RES) != ll.cell_of(q, origin, lc.RES)
    p = pos("outside_the_map")
    fx, fy, fz = cells(p[0], p[1])
    assert (fz >= 10.0).all() and len(fz) > 5                       # wholly outside
    fx, fy, fz = cells(p[2], p[3])
    assert (fz >= 10.0).any() and (fz < 10.0).any()                 # outside, then inside
    fx, fy, fz = cells(p[4], p[5])
    assert (fy < 0.0).any() and (fy >= 0.0).any()
    p = pos("exactly_at_range")
    d = p[1] - p[0]
    assert (d * d).sum() == 1.5 * 1.5


@pytest.mark.parametrize("variant", sorted(lc.TELLS))
def test_every_variant_changes_its_hand_case(scene, variant):
    occ, origin = scene
    name = lc.TELLS[variant]
    par, v, vo, n_views, want_l, want_i = lc.case(name)
    got_l, got_i = ll.groups_los(par, v, vo, n_views, occ, origin, lc.RES, variant)
    assert got_l.tolist() != want_l.tolist() or got_i.tolist() != want_i.tolist(), (variant, name)


def test_the_variants_are_those_of_the_model():
    assert sorted(ll.VARIANTS) == sorted(list(lc.TELLS) + ["from_observer"])


def test_a_pair_whose_answer_depends_on_the_orientation(scene):
    """The seeded search of tests/link_los_cases.py (seed 2027) must find a pair on the 0.1 m grid whose ray is free from one end and
    blocked from the other.  The model takes the ray from the vehicle with the smaller index: the same two positions are linked in one
    index order and blocked in the other, and both vehicles agree in each.  `from_observer` makes the two ends disagree."""
    occ, origin = scene
    found = lc.orientation_pair(occ, origin, lc.RES, ll.blocked)
    assert found is not None, "no pair in %d tries of seed %d" % (lc.SEARCH_TRIES, lc.SEARCH_SEED)
    p, q, tries = found
    assert tries == 836 and p.tolist() == [-1.3, -1.3, 0.2] and q.tolist() == [-1.8, -0.9, 0.5]
    a, b = ll.sampled_cells(p, q, origin, lc.RES), ll.sampled_cells(q, p, origin, lc.RES)
    assert set(zip(*[c.tolist() for c in a])) != set(zip(*[c.tolist() for c in b]))   # the two rays sample different cells
    par = lm.params(3.0, 2)
    v, _ = lm.fleet([p, q])
    got = ll.groups_los(par, v, None, 2, occ, origin, lc.RES)
    assert got[0].tolist() == [0, 0] and got[1].tolist() == [0, 1, 1, 0]
    v_rev, _ = lm.fleet([q, p])
    got = ll.groups_los(par, v_rev, None, 2, occ, origin, lc.RES)
    assert got[0].tolist() == [0, 1] and got[1].tolist() == [0, 2, 0, 1]
    adj, blk = ll.linked_los(par, v, None, 2, occ, origin, lc.RES, "from_observer")
    assert adj[0, 1] and not adj[1, 0] and blk[1, 0] and not blk[0, 1]
    wrong = ll.groups_los(par, v, None, 2, occ, origin, lc.RES, "from_observer")
    assert wrong[0].tolist() == [0, 1]   # vehicle 1 does not hear vehicle 0


@pytest.mark.parametrize("range_", (0.8, 1.5, 3.0))
def test_three_consequences_and_the_identity_on_random_fleets(forest, range_):
    occ, origin = forest
    relays = 0
    for seed in (3, 4):
        pos, view_of = lc.forest_fleet(seed)
        v, vo = lm.fleet(pos, view_of)
        par = lm.params(range_, 32)
        plain_l, plain_i = lm.groups(par, v, vo, 24)
        # 1. an empty map: the plain link, byte for byte
        l0, i0 = ll.groups_los(par, v, vo, 24, np.zeros_like(occ), origin, lc.RES)
        assert np.array_equal(l0, plain_l) and i0.tolist() == plain_i.tolist() and i0[3] == 0
        # 2. a subset of the plain pairs; every group inside one plain group; the identity
        adj, blk = ll.linked_los(par, v, vo, 24, occ, origin, lc.RES)
        plain = lm.linked(par, v, vo, 24)
        assert not (adj & ~plain).any() and not (blk & ~plain).any() and not (adj & blk).any() and np.array_equal(adj | blk, plain)
        los_l, los_i = ll.groups_los(par, v, vo, 24, occ, origin, lc.RES)
        assert los_i[2] + los_i[3] == plain_i[2] and los_i[3] > 0 and los_i[0] == 0 and plain_i[0] == 0
        for g in np.unique(los_l):
            assert len(set(plain_l[los_l == g].tolist())) == 1
        assert los_i[1] >= plain_i[1]
        assert np.array_equal(los_l, lm.components(24, lm.edges(adj, lm.views_of(len(v), vo))))
        # 3. relays: a blocked pair in one group all the same
        view = lm.views_of(len(v), vo)
        ii, kk = np.nonzero(np.triu(blk, 1))
        relays += int((los_l[view[ii]] == los_l[view[kk]]).sum())
    assert relays > 0 or range_ < 1.0
