"""The host layer's device buffers under reuse (faster_amd/csrc/fh_host.hpp: DeviceBuffer, the named buffers of a context, of a map and
of the pool): one handle is taken through calls whose buffers stay, grow past the 4096-byte floor, stay again and grow past the earlier
capacity, and every output equals what a fresh handle gives for the same call.  A buffer under a wrong name, two entry points sharing a
buffer that a launch still reads, or a buffer freed before the stream was waited for shows as a difference.

What tests/test_gpu_solve_edges.py and tests/test_gpu_parity.py already hold is not repeated: batch sizes of ONE entry point on one
context, the refusal of rows outside the face array, and the pool's shards against a one-way run."""
import numpy as np
import pytest
import torch  # noqa: F401  (before libfasterhip.so is loaded: one HIP runtime per process)

from faster_amd import abi, capi, corridor, frontend

pytestmark = pytest.mark.gpu

# 1; the smallest count whose problem records (264 B each) exceed the 4096-byte floor of a buffer; 1 again; a count above every earlier
# capacity, the floor of the 4-byte counts included
SIZES = (1, 16, 1, 1025)
WORK_COUNTERS = ("nodes", "qp_iters", "kflops")   # who helped whom decides them when work is shared: every other byte of a result is fixed


def context(share):
    c = capi.Context(0)
    par = abi.default_params()
    par["share"] = share
    c.set_params(par)
    return c


def host_calls(n):
    """The five host-pointer entry points on a batch of n: name -> (context -> tuple of output arrays)."""
    pr, faces, _ = corridor.whole_batch(n, seed=40 + n, n_seg=6, p_choices=(1, 2))
    rng = np.random.default_rng(n)
    cloud = rng.uniform(-3.0, 3.0, size=(200, 3))
    a = rng.uniform(-2.0, 2.0, size=(n, 3))
    segments = np.concatenate([a, a + rng.uniform(0.3, 1.0, size=(n, 3))], axis=1)
    solved = {}

    def solve(c):
        solved["res"] = c.solve_batch(pr, faces)
        return (solved["res"],)

    return [("fh_solve_batch", solve),
            ("fh_sample_batch", lambda c: c.sample_batch(pr, solved["res"], 12)),
            ("fh_dt_initial_batch", lambda c: (c.dt_initial_batch(pr),)),
            ("fh_decompose_batch", lambda c: c.decompose_batch(cloud, segments, max_faces=32)),
            ("fh_solve_batch_speculative", lambda c: (c.solve_batch_speculative(pr, faces, 4),))]


def as_bytes(arr, share):
    arr = np.ascontiguousarray(arr).copy()
    if share and arr.dtype == abi.result_dtype:
        for f in WORK_COUNTERS:
            arr[f] = 0
    return arr.tobytes()


@pytest.mark.parametrize("share", [0, 1], ids=["alone", "shared"])
def test_host_pointer_entry_points_interleaved_on_one_context(share):
    """share = 0: every byte of every output.  share = 1 (the default): every byte but the three work counters of a result."""
    reused = context(share)
    solved_any = False
    for step, n in enumerate(SIZES):
        for name, call in host_calls(n):
            fresh = context(share)
            want = call(fresh)
            fresh.close()
            got = call(reused)
            assert len(got) == len(want)
            for k, (g, w) in enumerate(zip(got, want)):
                assert as_bytes(g, share) == as_bytes(w, share), (step, n, name, k)
            if name == "fh_solve_batch":
                solved_any |= bool(got[0]["solved"].all())
    reused.close()
    assert solved_any


def test_one_map_through_a_small_a_larger_and_the_small_grid_again():
    """The bits, the jump tables and the order buffer of a map regrow with the larger grid (more queries than wavefronts: the launch order
    is on) and are reused, larger than needed, by the small grid after it; both searches each time."""
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    small = frontend.forest_queries(8, 5, size=(8.0, 8.0, 3.0), min_goal_dist=3.0)
    large = frontend.forest_queries(cu + 44, 6, size=(20.0, 20.0, 3.0))

    def plan(vmap, world, mode):
        cloud, cells, center, starts, goals = world
        vmap.read(cloud, cells, 0.2, center, 0.0, 3.0, 0.3)
        vmap.set_search(mode)
        paths, npts, ex = vmap.plan_batch(starts, goals)
        paths[np.arange(paths.shape[1])[None, :] >= np.maximum(npts, 0)[:, None]] = 0.0   # (the rows beyond a path's vertices are not outputs)
        return vmap.dims()[0].tobytes(), vmap.occupancy().tobytes(), paths.tobytes(), npts.tobytes(), ex.tobytes(), int((npts > 0).sum())

    def new_map():
        vmap = capi.Map(0)
        vmap.set_sched(waves_per_cu=1)   # one wavefront per CU: cu + 44 queries are more than the wavefronts
        return vmap

    reused = new_map()
    for step, world in enumerate((small, large, small)):
        for mode in ("astar", "jps"):
            fresh = new_map()
            want = plan(fresh, world, mode)
            fresh.close()
            got = plan(reused, world, mode)
            assert got == want, (step, mode)
            assert got[-1] >= len(world[3]) // 2, (step, mode, got[-1])   # (the comparison is about paths, not about "no path")
    reused.close()


def test_pool_on_one_device_equals_one_context_around_a_negative_face_begin():
    """Both scan the batch with the same rule (fhh::scan_batch): a record with face_begin < 0 between good neighbours is the kernel's to
    report, and no reason to refuse or to change anything else — record for record, the bad one included."""
    pr, faces, _ = corridor.whole_batch(6, seed=3, n_seg=6, p_choices=(1, 2))
    pr["face_begin"][2] = -1
    c = context(0)
    pool = capi.Pool([0])
    par = abi.default_params()
    par["share"] = 0
    pool.set_params(par)
    one = c.solve_batch(pr, faces)
    many = pool.solve_batch(pr, faces)
    pool.close()
    c.close()
    assert one["status"][2] == abi.FH_ST_BAD_INPUT and one["solved"][2] == 0
    assert np.delete(one["solved"], 2).all()
    assert many.tobytes() == one.tobytes()
