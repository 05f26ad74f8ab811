"""The inputs of tests/test_gpu_decomp_edges.py proved on the CPU against the host restatement (frontend.decompose): if a builder of
tests/decomp_edge_cases.py is off, it fails here and not as a puzzling difference on the device."""
import numpy as np
import pytest

import decomp_edge_cases as dec
from faster_amd import frontend


@pytest.fixture(scope="module", autouse=True)
def built():
    from faster_amd import build as fb

    fb.build_frontend()


def host_rows(segment, cloud):
    (A, b), = frontend.decompose(np.asarray(segment).reshape(2, 3), cloud, drone_radius=dec.DRONE_RADIUS, bbox=dec.BBOX)[0]
    return np.column_stack([A, b])


def test_caps_are_read_from_the_kernel_header():
    assert dec.CAP % 64 == 0 and dec.CAP_IDS % 64 == 0 and dec.CAP < dec.CAP_IDS < dec.CAP_GLOBAL
    assert dec.BLIST >= 64 and dec.MAX_FACES_POLY >= 16 and dec.CORRIDOR_MAX_POLY <= dec.MAX_POLY
    assert dec.BLOCK_EDGE_SIZES[1] == (dec.MIN_BLOCKS - 1) * 64 and dec.BLOCK_EDGE_SIZES[2] == (dec.MIN_BLOCKS - 1) * 64 + 1


@pytest.mark.parametrize("name", sorted(dec.EXACT_CASES))
def test_exact_clouds_hold_their_margins_and_give_usable_polytopes(name):
    """Every segment's list is exactly as long as the case says (margins by the builder's own dot products, over the merged cloud), and the
    host polytope has 7 rows for an empty list, 8 for one point, and between 9 and 511 otherwise: the rows fit max_faces = 512 and the
    separating planes are really exercised."""
    segs, cloud, ks = dec.EXACT_CASES[name]()
    for s, k in zip(segs, ks):
        inside = dec.assert_exact(s, cloud, k)
        assert int(inside.sum()) == k
        rows = len(host_rows(s, cloud))
        if k <= 1:
            assert rows == 7 + k, (name, k, rows)
        else:
            assert 9 <= rows < 512, (name, k, rows)


def test_compaction_clouds_keep_the_near_points_in_the_tail():
    segs, cloud, ks = dec.compaction_case()
    for s, k, near in zip(segs, ks, (False, False, True, True)):
        d = dec.segment_dist(s, cloud[dec.plane_depth(s, cloud) >= dec.MARGIN_IN])
        assert len(d) == k
        if near:
            assert d[dec.CAP_IDS:].max() <= d[:dec.CAP_IDS].min()
        else:
            assert abs(d[dec.CAP_IDS:].mean() - d[:dec.CAP_IDS].mean()) < 0.05
        # the first separating plane (0.1 m: more than the inflation moves a point) puts entries in front of position CAP_IDS away and keeps
        # entries behind it: the compaction moves entries of the HBM tail into LDS; of the longer lists more than CAP_IDS entries stay, so
        # the compacted list still straddles the border
        pts, r0 = cloud[dec.plane_depth(s, cloud) >= dec.MARGIN_IN], host_rows(s, cloud)[0]
        stay, go = pts @ r0[:3] < r0[3] - 0.1, pts @ r0[:3] > r0[3] + 0.1
        assert go[:dec.CAP_IDS].sum() > 100 and stay[dec.CAP_IDS:].sum() > 100
        if k == 6000:
            assert int(stay.sum()) > dec.CAP_IDS


@pytest.mark.parametrize("j", range(len(dec.TIE_CASES)))
def test_tie_clouds_are_sensitive_to_which_index_wins(j):
    """The two mirror points sit at the list positions the case names, and swapping them in the cloud changes the host's rows: the first
    separating plane passes through whichever comes first."""
    a, b, k = dec.TIE_CASES[j]
    c0, c1 = dec.tie_case(j, False), dec.tie_case(j, True)
    inside = dec.plane_depth(dec.TIE_SEGMENT, c0) >= dec.MARGIN_IN
    assert int(inside.sum()) == k
    lst0, lst1 = c0[inside], c1[inside]
    assert np.array_equal(lst0[a], dec.TIE_PAIR[0]) and np.array_equal(lst0[b], dec.TIE_PAIR[1])
    assert np.array_equal(lst1[a], dec.TIE_PAIR[1]) and np.array_equal(lst1[b], dec.TIE_PAIR[0])
    differ = np.any(c0 != c1, axis=1)
    assert int(differ.sum()) == 2
    r0, r1 = host_rows(dec.TIE_SEGMENT, c0), host_rows(dec.TIE_SEGMENT, c1)
    assert 9 <= len(r0) < 512 and len(r0) == len(r1)
    assert not np.array_equal(r0, r1)
    # the winner's plane is the first row: y <= 0.7 for (1, +0.75, 1), -y <= 0.7 for its mirror image
    assert np.array_equal(r0[0, :3], [0.0, 1.0, 0.0]) and np.array_equal(r1[0, :3], [0.0, -1.0, 0.0]) and r0[0, 3] == r1[0, 3]


@pytest.mark.parametrize("c", [dec.BLIST - 1, dec.BLIST, dec.BLIST + 1])
def test_block_clouds_hit_exactly_the_blocks_they_name(c):
    cloud = dec.block_list_cloud(c)
    assert len(cloud) % 64 != 0 and (len(cloud) + 63) // 64 >= c
    assert dec.blocks_meeting_box(dec.BLOCK_SEGMENT, cloud) == c
    dec.assert_exact(dec.BLOCK_SEGMENT, cloud, c)
    last = cloud[len(cloud) // 64 * 64:]
    assert int((dec.plane_depth(dec.BLOCK_SEGMENT, last) >= dec.MARGIN_IN).sum()) == 1   # one list point in the partial block
    assert 9 <= len(host_rows(dec.BLOCK_SEGMENT, cloud)) < 512


def test_block_edge_clouds():
    for n in dec.BLOCK_EDGE_SIZES:
        cloud = dec.block_edge_cloud(n)
        assert len(cloud) == n
        dec.assert_exact(dec.BLOCK_SEGMENT, cloud, 100)
        assert 9 <= len(host_rows(dec.BLOCK_SEGMENT, cloud)) < 512
    assert [(n + 63) // 64 >= dec.MIN_BLOCKS for n in dec.BLOCK_EDGE_SIZES] == [False, False, True, True]


def test_max_faces_segment_has_enough_rows():
    segs, cloud, _ = dec.max_faces_case()
    assert len(host_rows(segs[0], cloud)) >= 10 and len(host_rows(segs[1], cloud)) == 7


def test_corridor_case_on_the_host():
    """n_points covers -2 .. 4; the many-faces leg has more than FH_MAX_FACES_POLY rows on the host and every other leg at most that many
    (and at least 8: a real polytope); several pairs share no row total with the largest, so that faces_per_problem = T - 1 fails some
    pairs and keeps others."""
    case = dec.corridor_case()
    assert set(case["n_points"].tolist()) == {-2, -1, 0, 1, 2, 3, 4}
    many = case["many"]
    totals = {}
    for i in range(len(case["paths"])):
        v = dec.legs_of(case, i)
        if v is None:
            continue
        rows = [len(b) for _, b in frontend.decompose(v, case["cloud"], drone_radius=dec.DRONE_RADIUS, bbox=dec.BBOX)[0]]
        for leg, r in enumerate(rows):
            if (i, leg) == many:
                assert r > dec.MAX_FACES_POLY, r
            else:
                assert 8 <= r <= dec.MAX_FACES_POLY, (i, leg, r)
        if i != many[0]:
            totals[i] = sum(rows)
    T = max(totals.values())
    assert 0 < many[0] < len(case["paths"]) - 1 and len(totals) >= 20
    assert 1 <= sum(t == T for t in totals.values()) < len(totals)
