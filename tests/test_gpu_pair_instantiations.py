"""Every instantiation of the fused pair kernel (`solve_kernel<NSEG, true, WPS, UNK>`: NSEG 6 / 10 / 15 / 16, the three-wavefront
build, the two-wavefront build, and the two-wavefront build whose hand-off asks unknown space as an input — rule mode 2) against the
oracle with complete pair outputs, and in the library's default mode — lazy pair outputs (fh_sched.pair_outputs = 0: the safe
problem is built in LDS and written to memory only when it is first handed to another workgroup, which then stages it from there)
with compact results — against the complete outputs, bit for bit.  A launch whose scheduling makes safe problems change hands
checks the take-from-memory path of every instantiation."""
import numpy as np
import pytest
import torch

from faster_amd import abi, capi, corridor
from test_gpu_pair_interrupts import HEAD, TEMPLATE, _bytes, _dev, launch_pairs, same_records
from test_gpu_round3 import check_pairs_against_oracle, compare

pytestmark = pytest.mark.gpu

INSTANTIATIONS = [(n, w, u) for n in (6, 10, 15, 16) for w, u in ((3, False), (2, False), (2, True))]
# per kernel size: the segment counts mixed in one batch (all <= NSEG) and the polytope counts of the corridors
SHAPES = {6: ((3, 5, 6), (1, 2, 3)), 10: ((6, 8, 10), (2, 3, 4, 5, 6)), 15: ((11, 13, 15), (4, 5, 6, 7, 8)), 16: ((12, 14, 16), (6, 7, 8))}
SHARING = dict(publish_factor=1, min_nodes=1, backlog=256, waiting_workgroups=64)   # frames change hands early and often


def mixed_batch(nseg, seed):
    """Three segment counts up to NSEG, plus corridors pulled in by 0.3 m (more trials, larger trees), interleaved."""
    segs, polys = SHAPES[nseg]
    parts = [corridor.whole_batch(160, seed=seed + k, n_seg=n, p_choices=polys)[:2] for k, n in enumerate(segs)]
    tight, tfaces, _ = corridor.whole_batch(192, seed=seed + 7, n_seg=nseg, p_choices=polys)
    tfaces = tfaces.copy()
    tfaces["b"] -= 0.3
    whole, faces = corridor.concat(parts + [(tight, tfaces)])
    whole = whole[np.random.default_rng(seed).permutation(len(whole))]
    return whole, faces


def unknown_grid(whole, seed):
    """A sparse grid of unknown voxels over the starts of the batch (as in test_gpu_round5's pool test)."""
    res, dims = 0.25, (96, 96, 16)
    origin = np.array([whole["x0"][:, 0].min() - 2.0, whole["x0"][:, 1].min() - 2.0, -0.5])
    flags = (np.random.default_rng(seed).random(dims[::-1]) < 0.0008).astype(np.uint8)
    return torch.from_numpy(flags.reshape(-1).copy()).cuda(), origin, res, dims


def context(pair_outputs, wpc, unk, grid, **sched):
    c = capi.Context(0, pair_outputs=pair_outputs, compact_results=not pair_outputs)
    c.set_sched(workgroups_per_cu=wpc, **sched)
    c.set_pair_margin(0.05)
    if unk:
        c.set_pair_rule(mode=2, drone_radius=0.3, delta_h=1.0, delta_a=0.5)
        c.set_unknown_grid_device(grid[0].data_ptr(), grid[1], grid[2], grid[3])
    return c


def check_against_staged_hand_off(c, oracle, whole, faces, tmpl, idx, full):
    """Rule mode 2 (oracle/pair_glue.py has no unknown grid): whole results against the oracle, the safe problems record for record and
    row for row against the staged hand-off (fh_pair_glue_device, same rule and grid) of the fused whole results, and the safe results
    against the oracle on the device-written safe problems."""
    w, s, safe, sfaces = full
    B = len(whole)
    compare(w[idx], oracle.solve_batch(whole[idx], faces))
    d_whole, d_faces, d_safe, d_wr = _dev(whole), _dev(faces), _dev(tmpl), _dev(w)
    d_sf = torch.zeros_like(d_faces)
    c.pair_glue_device(d_whole.data_ptr(), d_wr.data_ptr(), d_faces.data_ptr(), B, 0.5, 0.2, 3, d_safe.data_ptr(), d_sf.data_ptr())
    c.sync()
    safe_ref, sf_ref = d_safe.cpu().numpy().view(abi.problem_dtype), d_sf.cpu().numpy().view(abi.face_dtype)
    for f in abi.problem_dtype.names:
        assert (_bytes(safe[f]) == _bytes(safe_ref[f])).all(), f
    live = np.flatnonzero(safe_ref["n_seg"] > 0)
    assert 0 < len(live) < B                   # some trajectories come near an unknown voxel, some do not
    for i in live:
        f0, n = int(safe_ref["face_begin"][i]), int(safe_ref["face_off"][i][safe_ref["n_poly"][i]])
        assert np.array_equal(_bytes(sfaces[f0:f0 + n]), _bytes(sf_ref[f0:f0 + n])), i
    li = idx[safe_ref["n_seg"][idx] > 0]
    compare(s[li], oracle.solve_batch(safe[li], sfaces))


def lazy_equals_complete(lazy, full, tmpl, nseg):
    """Lazy outputs with compact results (buffers filled with 0xCD) against complete outputs: every result field but the work counters
    bit for bit, rows < NSEG equal, rows >= NSEG untouched, the template fields of the safe records never written; a safe record that
    WAS written (its problem was handed to another workgroup) equals the complete one, and so do its rows.  Returns those pairs."""
    (w0, s0, safe0, sf0), (w1, s1, safe1, sf1) = lazy, full
    for a, b, what in ((w0, w1, "whole"), (s0, s1, "safe")):
        eq = same_records(a, b, nseg)
        assert eq.all(), (what, np.flatnonzero(~eq)[:8])
        assert (a["coeff"][:, nseg:].view(np.uint8) == 0xCD).all(), what
        assert not b["coeff"][:, nseg:].any(), what
    for f in TEMPLATE:
        assert (_bytes(safe0[f]) == _bytes(tmpl[f])).all(), f
    written = np.flatnonzero((_bytes(safe0) != _bytes(tmpl)).any(axis=1))
    for i in written:
        for f in abi.problem_dtype.names:
            assert np.array_equal(_bytes(safe0[f][i:i + 1]), _bytes(safe1[f][i:i + 1])), (i, f)
        f0, n = int(safe1["face_begin"][i]), int(safe1["face_off"][i][safe1["n_poly"][i]])
        assert np.array_equal(_bytes(sf0[f0:f0 + n]), _bytes(sf1[f0:f0 + n])), i
    return written


@pytest.mark.parametrize("nseg,waves,unk", INSTANTIATIONS, ids=["%d-%dw%s" % (n, w, "-unk" if u else "") for n, w, u in INSTANTIATIONS])
def test_pair_instantiation_complete_against_oracle_and_lazy_bit_for_bit(oracle, nseg, waves, unk):
    """One instantiation, forced with fh_sched.workgroups_per_cu (12: three wavefronts per SIMD, 8: two; rule mode 2 has two only) and
    confirmed with fh_last_launch.  (1) complete outputs against the oracle on 96 pairs of a batch of mixed segment counts (rule mode 2:
    against the staged hand-off); (2) lazy outputs with compact results against the complete outputs on the whole batch; (3) the 96
    pairs with the largest safe trees, alone on the device with scheduling that hands frames to idle workgroups early (no result may
    depend on it): the same bits again, safe problems handed over (donations > 0), and at least one lazy safe record written — a safe
    problem that another workgroup staged from memory.
    Not at NSEG = 6 (all three builds): nothing changes hands there with this scheduling (measured: 0 frames donated).  The trees are
    small — the largest of the 96 picked pairs has 7 (rule mode 2: 23) whole and 15 safe branch-and-bound nodes over ALL its factor
    trials, and a tree first looks for idle workgroups at its 8th node (fh_sched.look_every at its default).  Its sharing launch is still
    checked bit for bit against the complete outputs."""
    wpc = 12 if waves == 3 else 8
    name = "fh::solve_kernel<%d, true, %d, %s>" % (nseg, waves, "true" if unk else "false")
    whole, faces = mixed_batch(nseg, seed=700 + 10 * nseg + (1 if unk else 0))
    tmpl = corridor.safe_templates(whole)
    B = len(whole)
    idx = np.sort(np.random.default_rng(nseg).choice(B, 96, replace=False))
    grid = unknown_grid(whole, seed=nseg) if unk else None
    full_c, lazy_c = context(True, wpc, unk, grid), context(False, wpc, unk, grid)
    try:
        # (1) complete outputs against the oracle
        if unk:
            full = launch_pairs(full_c, whole, faces, tmpl, nseg, fill=0xAB)
            assert full_c.last_launch()[1] == name
            check_against_staged_hand_off(full_c, oracle, whole, faces, tmpl, idx, full)
        else:
            wref, oks = check_pairs_against_oracle(full_c, oracle, whole, faces, nseg, idx)
            assert full_c.last_launch()[1] == name
            assert wref["solved"].mean() > 0.5 and oks.sum() > 0
            full_c.set_pair_margin(0.05)       # (check_pairs_against_oracle leaves the context at the default margin)
            full = launch_pairs(full_c, whole, faces, tmpl, nseg, fill=0xAB)
        assert full[0]["solved"].mean() > 0.5 and full[1]["solved"].sum() > 0
        # (2) lazy outputs, compact results
        lazy = launch_pairs(lazy_c, whole, faces, tmpl, nseg, fill=0xCD)
        assert lazy_c.last_launch()[1] == name
        lazy_equals_complete(lazy, full, tmpl, nseg)
        # (3) safe problems that change hands
        live = np.flatnonzero(full[2]["n_seg"] > 0)
        pick = np.sort(live[np.argsort(-full[1]["nodes"][live], kind="stable")[:96]])
        sw, sfc = whole[pick], faces
        stmpl = tmpl[pick]
        for c in (full_c, lazy_c):
            c.set_sched(workgroups_per_cu=wpc, **SHARING)
        sfull = launch_pairs(full_c, sw, sfc, stmpl, nseg, fill=0xAB)
        slazy = launch_pairs(lazy_c, sw, sfc, stmpl, nseg, fill=0xCD)
        st = lazy_c.share_stats()
        assert lazy_c.last_launch()[1] == name and full_c.last_launch()[1] == name
        for got, ref in ((sfull[0], full[0][pick]), (sfull[1], full[1][pick])):
            assert same_records(got, ref, nseg).all()
        written = lazy_equals_complete(slazy, sfull, stmpl, nseg)
        print("%s: %d pairs, %d / %d whole / safe solved; sharing launch: %d frames donated, %d taken, %d of %d lazy safe records written "
              "(most nodes of a picked pair: whole %d, safe %d)" % (name, B, full[0]["solved"].sum(), full[1]["solved"].sum(), st["donated"],
                                                                   st["stolen"], len(written), len(pick), full[0]["nodes"][pick].max(),
                                                                   full[1]["nodes"][pick].max()))
        assert st["error"] == 0
        if nseg != 6:
            assert st["donated"] > 0 and len(written) > 0
    finally:
        full_c.close()
        lazy_c.close()
