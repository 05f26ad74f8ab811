"""The third regime of a solve launch on the GPU (faster_amd/csrc/fh_policy.hpp, launch_solve in fh_capi.hip): a launch issued while
more solve launches of the process are outstanding on the device than the runtime has hardware queues runs with the queued regime's
look period, and computes what a launch alone computes, bit for bit.  FASTERHIP_HW_QUEUES = 2 states the queue count for the contexts
of this test only (read once per context, in fh_create): with launches in flight on two other contexts a third one is queued."""
import os

import numpy as np
import pytest

from faster_amd import abi, capi, corridor

pytestmark = pytest.mark.gpu

FIELDS = ("solved", "trials", "status", "factor", "dt", "cost", "coeff", "assign")
LOOK_ALONE, LOOK_BESIDE, LOOK_QUEUED = 8, 16, 16  # FH_LOOK_EVERY, FH_LOOK_EVERY_BUSY, fhp::LOOK_EVERY_QUEUED (fh_policy.hpp)
N = 10


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


@pytest.fixture()
def three_contexts_two_queues():
    import torch  # noqa: F401  (torch first: one HIP runtime in the process)

    before = os.environ.get("FASTERHIP_HW_QUEUES")
    os.environ["FASTERHIP_HW_QUEUES"] = "2"
    ctxs = []
    try:
        for _ in range(3):
            ctxs.append(capi.Context(0))
        yield ctxs
    finally:
        for c in ctxs:
            c.close()
        if before is None:
            del os.environ["FASTERHIP_HW_QUEUES"]
        else:
            os.environ["FASTERHIP_HW_QUEUES"] = before


def _same(got, ref, what):
    for f in FIELDS:
        a, b = (got[f][:, :N], ref[f][:, :N]) if f in ("coeff", "assign") else (got[f], ref[f])
        assert np.array_equal(a, b), (what, f)


def _queue_up(ctxs, launch):
    """launch(k) issues one launch on context k.  One launch alone on the third context; then four launches on each of the first two
    (milliseconds of work on two streams, so that a stall of this host thread cannot let them finish first) and one on the third."""
    a, b, c = ctxs
    launch(2)
    c.sync()
    assert c.last_launch()[0]["look_every"] == LOOK_ALONE
    yield "alone"
    for _ in range(4):
        launch(0)
    assert a.last_launch()[0]["look_every"] == LOOK_ALONE  # (launches of its own stream do not count)
    for _ in range(4):
        launch(1)
    assert b.last_launch()[0]["look_every"] == LOOK_BESIDE  # one other, two queues
    launch(2)
    assert c.last_launch()[0]["look_every"] == LOOK_QUEUED  # two others, two queues: this one waits behind another launch's tail
    for x in ctxs:
        x.sync()
        assert x.share_stats()["error"] == 0
    yield "queued"


def test_a_queued_launch_of_whole_problems_gives_the_bits_of_a_launch_alone(three_contexts_two_queues):
    import torch

    ctxs = three_contexts_two_queues
    B = 16384
    whole, faces, _ = corridor.whole_batch(B, seed=91, n_seg=N, p_choices=(2, 3, 4, 5, 6))
    mf = int(whole["face_off"][np.arange(B), whole["n_poly"]].max())
    d_whole, d_faces = _dev(whole), _dev(faces)
    outs = [torch.zeros(B * abi.result_dtype.itemsize, dtype=torch.uint8, device="cuda:0") for _ in range(3)]

    def launch(k):
        ctxs[k].solve_batch_device(d_whole.data_ptr(), d_faces.data_ptr(), B, N, mf, outs[k].data_ptr())

    steps = _queue_up(ctxs, launch)
    next(steps)
    alone = outs[2].cpu().numpy().view(abi.result_dtype).copy()
    assert alone["solved"].mean() > 0.99
    outs[2].zero_()
    torch.cuda.synchronize()
    next(steps)
    for k in range(3):
        _same(outs[k].cpu().numpy().view(abi.result_dtype), alone, "context %d" % k)


def test_a_context_gives_its_own_stream_back_and_takes_a_new_one():
    """fh_set_stream: a context that is given its caller's stream destroys its own (an idle stream would hold a place on the runtime's
    hardware queues), and NULL creates one again.  Launches before, between and after give the same bits, the launch events of the
    destroyed stream can still be read, and a second switch to the same stream is harmless."""
    import torch

    B = 512
    whole, faces, _ = corridor.whole_batch(B, seed=93, n_seg=N, p_choices=(2, 3, 4, 5, 6))
    mf = int(whole["face_off"][np.arange(B), whole["n_poly"]].max())
    d_whole, d_faces = _dev(whole), _dev(faces)
    out = torch.zeros(B * abi.result_dtype.itemsize, dtype=torch.uint8, device="cuda:0")
    c = capi.Context(0)
    try:
        c.timing_reset()
        results = []
        s = torch.cuda.Stream()
        for stream in (None, s.cuda_stream, s.cuda_stream, 0, s.cuda_stream, 0):
            if stream is not None:
                c.set_stream(stream)
            out.zero_()
            torch.cuda.synchronize()
            c.solve_batch_device(d_whole.data_ptr(), d_faces.data_ptr(), B, N, mf, out.data_ptr())
            c.sync()
            results.append(out.cpu().numpy().view(abi.result_dtype).copy())
        assert results[0]["solved"].mean() > 0.99
        for r in results[1:]:
            _same(r, results[0], "after a change of stream")
        ms = c.timing_read()
        assert len(ms) == len(results) and (np.asarray(ms) > 0).all()
    finally:
        c.close()


def test_a_queued_launch_of_fused_pairs_gives_the_bits_of_a_launch_alone(three_contexts_two_queues):
    """The path the benchmark runs: fh_solve_pairs_device with lazy pair outputs (the safe problem of a pair stays on chip), 2048 pairs —
    the smallest batch that is sorted when it is alone."""
    import torch

    ctxs = three_contexts_two_queues
    B = 2048
    whole, faces, _ = corridor.whole_batch(B, seed=92, n_seg=N, p_choices=(2, 3, 4, 5, 6))
    tmpl = corridor.safe_templates(whole)
    mf = int(whole["face_off"][np.arange(B), whole["n_poly"]].max())
    d_whole, d_faces = _dev(whole), _dev(faces)
    RS = abi.result_dtype.itemsize
    bufs = []
    for c in ctxs:
        c.set_pair_margin(0.05)
        c.set_sched(pair_outputs=0, compact_results=1)
        bufs.append((_dev(tmpl), torch.zeros_like(d_faces), torch.zeros(B * RS, dtype=torch.uint8, device="cuda:0"), torch.zeros(B * RS, dtype=torch.uint8, device="cuda:0")))

    def launch(k):
        ds, dsf, dwr, dsr = bufs[k]
        ctxs[k].solve_pairs_device(d_whole.data_ptr(), d_faces.data_ptr(), B, N, mf, 0.5, 0.2, 3, dwr.data_ptr(), ds.data_ptr(), dsf.data_ptr(), dsr.data_ptr())

    steps = _queue_up(ctxs, launch)
    next(steps)
    alone_w = bufs[2][2].cpu().numpy().view(abi.result_dtype).copy()
    alone_s = bufs[2][3].cpu().numpy().view(abi.result_dtype).copy()
    assert alone_w["solved"].mean() > 0.99 and 0.5 < alone_s["solved"].mean() < 1.0
    bufs[2][2].zero_()
    bufs[2][3].zero_()
    torch.cuda.synchronize()
    next(steps)
    for k in range(3):
        _same(bufs[k][2].cpu().numpy().view(abi.result_dtype), alone_w, "whole, context %d" % k)
        _same(bufs[k][3].cpu().numpy().view(abi.result_dtype), alone_s, "safe, context %d" % k)
