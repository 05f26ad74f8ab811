"""fh::decomp_kernel where a segment's point list changes home (coordinates in LDS up to FH_DECOMP_CAP points, ids in LDS up to
FH_DECOMP_CAP_IDS, LDS + the workgroup's HBM workspace up to FH_DECOMP_CAP_GLOBAL, -1 beyond), where the candidate-block list switches on
and overflows, at rows == max_faces, and corridor_assemble_kernel's failure clauses — through fh_decompose_batch_device and
fh_corridor_batch_device.

Every comparison is exact: device rows against the host restatement (frontend.decompose) by np.array_equal, same rows, same order.  Every
output buffer is one slot longer than the batch and starts as the byte 0xA5: the guard slot and the rows [count, max_faces) of every
segment must still be 0xA5 after the launch.  The inputs come from tests/decomp_edge_cases.py and are proved on the CPU in
tests/test_decomp_edge_cases.py (list lengths exact, ties sensitive to the winner, block counts exact)."""
import numpy as np
import pytest
import torch  # noqa: F401  (before libfasterhip.so is loaded: one HIP runtime per process)

import decomp_edge_cases as dec
from faster_amd import abi, capi, frontend

pytestmark = pytest.mark.gpu

FS = abi.face_dtype.itemsize
POISON = 0xA5
DEV = "cuda:0"
MAX_FACES = 512


@pytest.fixture(scope="module", autouse=True)
def built():
    from faster_amd import build as fb

    fb.build_frontend()


@pytest.fixture(scope="module")
def c():
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def poisoned(nbytes):
    return torch.full((nbytes,), POISON, dtype=torch.uint8, device=DEV)


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


_HOST = {}


def host_rows(segment, cloud, key=None):
    """the host restatement's rows [r][4] of one segment (computed once per key)"""
    if key is not None and key in _HOST:
        return _HOST[key]
    (A, b), = frontend.decompose(np.asarray(segment).reshape(2, 3), cloud, drone_radius=dec.DRONE_RADIUS, bbox=dec.BBOX)[0]
    rows = np.column_stack([A, b])
    if key is not None:
        _HOST[key] = rows
    return rows


def launch(ctx, d_cloud, n_cloud, segments, max_faces=MAX_FACES):
    """fh_decompose_batch_device into poisoned buffers with one guard slot; checks the guard and the rows behind every count.
    -> (d_faces [n + 1][max_faces][FS] bytes, counts [n] numpy)"""
    n = len(segments)
    d_seg = to_dev(np.asarray(segments, dtype=np.float64).reshape(n, 6))
    d_faces, d_counts = poisoned((n + 1) * max_faces * FS), poisoned((n + 1) * 4)
    ctx.decompose_batch_device(d_cloud.data_ptr() if n_cloud else None, n_cloud, d_seg.data_ptr(), n, max_faces, d_faces.data_ptr(),
                               d_counts.data_ptr(), drone_radius=dec.DRONE_RADIUS, bbox=dec.BBOX)
    ctx.sync()
    f = d_faces.view(n + 1, max_faces, FS)
    cnt = d_counts.view(torch.int32)
    assert bool((f[n] == POISON).all()) and bool((d_counts[4 * n:] == POISON).all()), "the guard slot was written"
    counts = cnt[:n].cpu().numpy().copy()
    assert np.all((counts >= -1) & (counts <= max_faces)), counts[(counts < -1) | (counts > max_faces)][:8]
    live = cnt[:n].to(torch.int64)[:, None]
    dead = (torch.arange(max_faces, device=DEV)[None, :] >= live) & (live >= 0)   # (a -1 segment's rows are not looked at)
    assert bool((f[:n][dead] == POISON).all()), "rows behind a segment's count were written"
    return f, counts


def rows_of(f, i, count):
    r = f[i, :count].cpu().numpy().view(abi.face_dtype).reshape(count)
    return np.column_stack([r["a"], r["b"]])


def assert_equals_host(f, counts, i, ref, what):
    print("%s: segment %d device count %d host rows %d" % (what, i, counts[i], len(ref)))
    assert counts[i] == len(ref), (what, i, int(counts[i]), len(ref))
    assert np.array_equal(rows_of(f, i, len(ref)), ref), (what, i)


def run_case(ctx, name, segments, cloud, ks, max_faces=MAX_FACES):
    d_cloud = to_dev(cloud)
    f, counts = launch(ctx, d_cloud, len(cloud), segments, max_faces)
    for i, (s, k) in enumerate(zip(segments, ks)):
        if k > dec.CAP_GLOBAL:
            print("%s: segment %d (%d points) device count %d" % (name, i, k, counts[i]))
            assert counts[i] == -1, (name, i, k, int(counts[i]))
        else:
            assert_equals_host(f, counts, i, host_rows(s, cloud), "%s k=%d" % (name, k))
    return f, counts


# ---- list length at every switch ---------------------------------------------------------------------------------------------------------
def test_list_length_at_every_switch(c):
    """A list of 0, 1, 63, 64, 65 points (lanes, one block of 64), CAP - 1 / CAP / CAP + 1 (coordinates -> ids), CAP_IDS - 1 / CAP_IDS /
    CAP_IDS + 1 (LDS -> LDS + HBM tail), CAP_IDS + 63 / + 64 / + 65 (the first block of the tail); CAP and CAP_IDS also on a horizontal and a
    vertical segment.  One launch, one cloud.  Mutations this catches: a home switch one entry late (a list of CAP + 1 points
    converted to coordinates runs over the end of its arrays; a list of CAP_IDS + 1 ids kept in LDS alone runs into the flag bytes), a
    tail index that forgets `- FH_DECOMP_CAP_IDS`, a sweep that drops the entry at position CAP_IDS."""
    segs, cloud, ks = dec.list_length_case()
    assert {dec.CAP, dec.CAP + 1, dec.CAP_IDS, dec.CAP_IDS + 1} <= set(ks)
    run_case(c, "list_length", segs, cloud, ks)


def test_list_length_at_the_global_cap(c):
    """CAP_GLOBAL - 1 and CAP_GLOBAL points are decomposed (the workspace holds them to its last id and flag byte), CAP_GLOBAL + 1 reports
    -1 and leaves its rows alone; the segments on either side of it keep theirs."""
    segs, cloud, ks = dec.list_cap_case()
    order = [0, 2, 1]  # the failing segment in the middle
    f, counts = run_case(c, "list_cap", segs[order], cloud, [ks[j] for j in order])
    assert counts[1] == -1 and bool((f[1] == POISON).all())


# ---- compaction across the LDS / HBM border ----------------------------------------------------------------------------------------------------
def test_compaction_across_the_lds_border(c):
    """Lists of 3000 and 6000 points: after every separating plane the survivors move to the front, from the HBM tail across position
    CAP_IDS into LDS; in the second pair of clouds the points nearest the segment all start in the tail, so the survivors come mostly from
    there.  An entry lost, duplicated or reordered at the border changes a later arg-min and with it a row."""
    segs, cloud, ks = dec.compaction_case()
    run_case(c, "compaction", segs, cloud, ks)


# ---- exact ties across lane, block and home borders -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("j", range(len(dec.TIE_CASES)))
def test_ties_across_boundaries(c, j):
    """Two mirror-image points with bit-equal ellipsoid distances, closest of all, at list positions on either side of a lane, a block of
    64, the LDS / HBM border: the lowest list index must win every arg-min, as in the host's sequential scan — in both cloud orders (the
    host's rows differ between them, tests/test_decomp_edge_cases.py)."""
    a, b, k = dec.TIE_CASES[j]
    got = []
    for swap in (False, True):
        cloud = dec.tie_case(j, swap)
        f, counts = launch(c, to_dev(cloud), len(cloud), dec.TIE_SEGMENT[None, :])
        ref = host_rows(dec.TIE_SEGMENT, cloud)
        assert_equals_host(f, counts, 0, ref, "tie (%d, %d) of %d swap=%d" % (a, b, k, swap))
        got.append(ref)
    assert not np.array_equal(got[0], got[1])


# ---- the candidate-block list ----------------------------------------------------------------------------------------------------------------
def both_block_settings(cloud, what):
    """the cloud under fh_sched.cloud_blocks 1 and 0: byte-equal outputs, both equal to the host"""
    segs = dec.BLOCK_SEGMENT[None, :]
    ref = host_rows(dec.BLOCK_SEGMENT, cloud)
    d_cloud = to_dev(cloud) if len(cloud) else None
    outs = []
    for blocks in (1, 0):
        ctx = capi.Context(0)
        try:
            ctx.set_sched(cloud_blocks=blocks)
            f, counts = launch(ctx, d_cloud, len(cloud), segs)
            assert_equals_host(f, counts, 0, ref, "%s cloud_blocks=%d" % (what, blocks))
            outs.append((f.clone(), counts))
        finally:
            ctx.close()
    assert torch.equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]), what


@pytest.mark.parametrize("n_cloud", dec.BLOCK_EDGE_SIZES)
def test_block_boxes_switch_on_at_eight_blocks(n_cloud):
    """7 blocks (447 points: the last partial; 448: all full) sweep the whole cloud, 8 blocks (449: a block of one point; 512) go through
    the block boxes: the same rows."""
    both_block_settings(dec.block_edge_cloud(n_cloud), "n_cloud=%d" % n_cloud)


@pytest.mark.parametrize("hits", [dec.BLIST - 1, dec.BLIST, dec.BLIST + 1])
def test_block_list_at_its_capacity(hits):
    """BLIST - 1 and BLIST candidate blocks fill the list (to its last entry), one more falls back to the full sweep; the last block of
    the cloud is partial and holds a point of the list.  Mutations this catches: BLIST + 1 candidates written into a list of BLIST, a
    partial last block whose box takes in lanes past n_cloud, a candidate list that drops its last entry (the list point of the partial
    block), a sweep that visits the candidates out of cloud order."""
    both_block_settings(dec.block_list_cloud(hits), "hit blocks=%d" % hits)


def test_empty_and_single_point_clouds():
    both_block_settings(np.zeros((0, 3)), "empty cloud")
    p1, _, dh, d, dv, _ = dec.frame(dec.BLOCK_SEGMENT)
    both_block_settings((p1 + 0.9 * dh + 0.5 * d + 0.3 * dv)[None, :], "one point")


# ---- rows == max_faces ---------------------------------------------------------------------------------------------------------------------
def test_max_faces_edge(c):
    """A polytope of r rows fits max_faces = r exactly; with max_faces = r - 1 it reports -1, writes no row of the next segment, and that
    segment still gets its own rows.  An empty cloud with max_faces = 8 gives the 6 box rows and the ground plane."""
    segs, cloud, _ = dec.max_faces_case()
    ref0, ref1 = host_rows(segs[0], cloud), host_rows(segs[1], cloud)
    r = len(ref0)
    assert r >= 10 and len(ref1) == 7
    d_cloud = to_dev(cloud)
    f, counts = launch(c, d_cloud, len(cloud), segs, max_faces=r)
    assert_equals_host(f, counts, 0, ref0, "max_faces = r")
    assert_equals_host(f, counts, 1, ref1, "max_faces = r, next")
    f, counts = launch(c, d_cloud, len(cloud), segs, max_faces=r - 1)
    print("max_faces = r - 1: device count %d (r = %d)" % (counts[0], r))
    assert counts[0] == -1
    assert_equals_host(f, counts, 1, ref1, "max_faces = r - 1, next")
    f, counts = launch(c, None, 0, segs, max_faces=8)
    assert list(counts) == [7, 7]
    for i in range(2):
        assert_equals_host(f, counts, i, host_rows(segs[i], np.zeros((0, 3))), "empty cloud, max_faces = 8")


# ---- one workgroup, all three homes in turn -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grids", [1, 3])
def test_one_workgroup_all_three_homes_in_turn(c, grids):
    """A launch larger than the resident grid (12 workgroups per CU): a workgroup decomposes a long list (ids, HBM tail), a short one as
    coordinates in the same LDS bytes, a long one again, in a shuffled order, with NaN slots in between.  Every copy of a segment equals the
    host rows of that segment; a NaN slot reports 0 and keeps its rows; a second launch on the same context — workspace and LDS reused —
    gives the same bytes.  (grids = 3: three rounds of the grid, so that most workgroups take several segments.)"""
    segs, cloud, ks = dec.homes_case()
    n = 12 * grids * n_cu() + 500
    kinds = len(ks) + 1   # the last kind is the NaN slot
    kind = np.zeros(n, dtype=np.int64)
    longest = np.argsort(ks)[-2:]
    fixed = np.concatenate([np.repeat(longest, 64), np.full(100, kinds - 1)])
    others = [k for k in range(kinds - 1) if k not in longest]
    kind[:len(fixed)] = fixed
    kind[len(fixed):] = np.array(others)[np.arange(n - len(fixed)) % len(others)]
    kind = kind[np.random.default_rng(23).permutation(n)]
    table = np.vstack([segs, np.full((1, 6), np.nan)])
    d_cloud = to_dev(cloud)
    f, counts = launch(c, d_cloud, len(cloud), table[kind])
    for k in range(kinds):
        idx = np.nonzero(kind == k)[0]
        assert len(idx) >= 64
        t_idx = torch.from_numpy(idx).to(DEV)
        if k == kinds - 1:
            assert np.all(counts[idx] == 0) and bool((f[t_idx] == POISON).all()), "NaN slot"
            continue
        assert_equals_host(f, counts, idx[0], host_rows(segs[k], cloud, key=("homes", k)), "homes k=%d" % ks[k])
        assert np.all(counts[idx] == counts[idx[0]]), (ks[k], np.unique(counts[idx]))
        same = (f[t_idx] == f[idx[0]][None]).flatten(1).all(dim=1)
        assert bool(same.all()), ("copies of one segment differ", ks[k], idx[~same.cpu().numpy()][:8])
    if grids == 1:
        f2, counts2 = launch(c, d_cloud, len(cloud), table[kind])
        assert torch.equal(f, f2) and np.array_equal(counts, counts2)


# ---- corridor assembly ---------------------------------------------------------------------------------------------------------------------------
def corridor_launch(ctx, case, d_cloud, fpp):
    n, mp = len(case["paths"]), case["max_poly"] + 1
    d_paths, d_np = to_dev(case["paths"]), to_dev(case["n_points"])
    d_faces, d_off, d_npoly, d_goal = poisoned((n + 1) * fpp * FS), poisoned((n + 1) * 9 * 4), poisoned((n + 1) * 4), poisoned((n + 1) * 24)
    ctx.corridor_batch_device(d_cloud.data_ptr(), len(case["cloud"]), d_paths.data_ptr(), d_np.data_ptr(), n, mp, case["max_poly"], fpp,
                              d_faces.data_ptr(), d_off.data_ptr(), d_npoly.data_ptr(), d_goal.data_ptr(), drone_radius=dec.DRONE_RADIUS,
                              bbox=dec.BBOX)
    ctx.sync()
    for d, per in ((d_faces, fpp * FS), (d_off, 36), (d_npoly, 4), (d_goal, 24)):
        assert bool((d[n * per:] == POISON).all()), "the guard pair was written"
        if d is not d_faces:  # (a pair without legs gets no rows)
            assert not bool((d[:n * per].view(n, per) == POISON).all(dim=1).any()), "a pair's output was never written"
    faces = d_faces.cpu().numpy()[:n * fpp * FS].reshape(n, fpp, FS)
    return (faces, d_off.cpu().numpy().view(np.int32)[:n * 9].reshape(n, 9).copy(), d_npoly.cpu().numpy().view(np.int32)[:n].copy(),
            d_goal.cpu().numpy().view(np.float64)[:n * 3].reshape(n, 3).copy())


def pair_rows(faces, i, total):
    r = np.ascontiguousarray(faces[i, :total]).view(abi.face_dtype).reshape(total)
    return np.column_stack([r["a"], r["b"]])


def test_corridor_assembly(c):
    """64 paths with max_poly = 3 and n_points over -2 .. 4.  A usable path: n_poly, all nine face_off entries, the rows back to back and
    the goal are what frontend.decompose of its kept vertices gives; the rows behind its total stay 0xA5.  An unusable path (n_points < 2):
    n_poly 0, nine zero offsets, a NaN goal, no row written.  The pair with a leg of more than FH_MAX_FACES_POLY rows: n_poly 0 and zeroed
    offsets, its neighbours as expected.  faces_per_problem = T (the largest row total): every pair fits; T - 1: exactly the pairs with
    total T get n_poly 0 and every other pair's outputs are the same bytes."""
    case = dec.corridor_case()
    n, many = len(case["paths"]), case["many"][0]
    d_cloud = to_dev(case["cloud"])
    expect = {}
    for i in range(n):
        v = dec.legs_of(case, i)
        if v is not None:
            expect[i] = [np.column_stack([A, b]) for A, b in frontend.decompose(v, case["cloud"], drone_radius=dec.DRONE_RADIUS, bbox=dec.BBOX)[0]]
    assert max(len(r) for r in expect[many]) > dec.MAX_FACES_POLY
    totals = {i: sum(len(r) for r in rows) for i, rows in expect.items() if i != many}
    T = max(totals.values())

    def check(fpp, failing):
        faces, off, npoly, goal = corridor_launch(c, case, d_cloud, fpp)
        for i in range(n):
            v = dec.legs_of(case, i)
            if v is None:
                assert npoly[i] == 0 and not off[i].any() and np.isnan(goal[i]).all(), (fpp, i, npoly[i], off[i], goal[i])
                assert np.all(faces[i] == POISON), (fpp, i)
                continue
            assert np.array_equal(goal[i], v[-1]), (fpp, i)
            if i in failing:
                print("faces_per_problem %d: pair %d n_poly %d (host legs %s)" % (fpp, i, npoly[i], [len(r) for r in expect[i]]))
                assert npoly[i] == 0 and not off[i].any(), (fpp, i, npoly[i], off[i])
                continue
            rows = np.vstack(expect[i])
            ends = np.cumsum([len(r) for r in expect[i]])
            want_off = np.concatenate([[0], ends, np.full(8 - len(ends), ends[-1])]).astype(np.int32)
            assert npoly[i] == len(expect[i]), (fpp, i, npoly[i])
            assert np.array_equal(off[i], want_off), (fpp, i, off[i], want_off)
            assert np.array_equal(pair_rows(faces, i, len(rows)), rows), (fpp, i)
            assert np.all(faces[i, len(rows):] == POISON), (fpp, i)
        return faces, off, npoly, goal

    full = check(T, {many})
    assert full[2][many - 1] > 0 and full[2][many + 1] > 0   # (the pairs before and after it are usable, and were compared above)
    at_T = {i for i, t in totals.items() if t == T}
    assert 1 <= len(at_T) < len(totals)
    less = check(T - 1, {many} | at_T)
    for i in set(totals) - at_T:
        assert np.array_equal(less[0][i, :totals[i]], full[0][i, :totals[i]]) and np.array_equal(less[1][i], full[1][i])
        assert less[2][i] == full[2][i] and np.array_equal(less[3][i], full[3][i])
