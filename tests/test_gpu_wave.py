"""Every primitive of faster_amd/csrc/fh_wave.hip.hpp on a wavefront of the device, lane by lane, and fhu::div (fh_udiv.hpp) on the
device, against the contracts of tests/wave_model.py: min, max, math.fsum, the bits of pairwise summation in lane order, n // d.  The
device is never compared with the model's emulation of the DPP network.

tests/hip/wave_probe.hip holds one probe per primitive (built by `python -m faster_amd.build` into tests/hip/libwaveprobe.so): block b
runs case b on one wavefront and every lane writes what it got.  One launch per probe over all of its cases.  Every output buffer
starts as the byte 0xA5 with a guard row in front and behind; the guards, and the lanes a probe must not write, are looked at after
the launch.  A failure names primitive, case and lane."""
import ctypes
import os

import numpy as np
import pytest
import torch  # before the probe library is loaded: one HIP runtime per process

import wave_model as wm

pytestmark = pytest.mark.gpu

SO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hip", "libwaveprobe.so")
ROW = {"f64": 8 * wm.W, "i32": 4 * wm.W, "u32": 4 * wm.W}  # bytes of one row of 64 lanes


@pytest.fixture(scope="module")
def probe():
    assert os.path.exists(SO), "%s is missing: run `python -m faster_amd.build` (build_wave_probe: hipcc --offload-arch=gfx950)" % SO
    return ctypes.CDLL(SO)


def run_on_device(lib):
    def run(prim, ins):
        n = len(ins[0])
        assert 0 < n < 4096 and all(len(a) == n for a in ins), prim.name
        for a, k in zip(ins, prim.ins):  # what the probe reads is what the launch covers: n rows of 64 lanes, or n words
            assert a.dtype == wm.DTYPE[k] and a.shape == ((n,) if k.endswith("s") else (n, wm.W)) and a.flags.c_contiguous, (prim.name, k)
        if prim.name.startswith("gather") or prim.name == "readlane_f64":
            assert ins[1].min() >= 0 and ins[1].max() < wm.W, prim.name  # lane numbers
        d_ins = [torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda() for a in ins]
        d_outs = [torch.full(((n + 2) * ROW[k],), wm.POISON_BYTE, dtype=torch.uint8, device="cuda") for k in prim.outs]
        fn = getattr(lib, "wp_" + prim.name)
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p] * (len(d_ins) + len(d_outs)) + [ctypes.c_int, ctypes.c_void_p]
        rc = fn(*[t.data_ptr() for t in d_ins], *[t.data_ptr() + ROW[k] for t, k in zip(d_outs, prim.outs)], n,
                torch.cuda.current_stream().cuda_stream)
        assert rc == 0, "%s: the launch returned HIP error %d" % (prim.name, rc)
        torch.cuda.synchronize()
        outs = []
        for t, k in zip(d_outs, prim.outs):
            raw = t.cpu().numpy()
            assert (raw[:ROW[k]] == wm.POISON_BYTE).all() and (raw[-ROW[k]:] == wm.POISON_BYTE).all(), "%s wrote into a guard row" % prim.name
            outs.append(raw[ROW[k]:-ROW[k]].view(wm.DTYPE[k]).reshape(n, wm.W).copy())
        return outs
    return run


@pytest.fixture(scope="module")
def measured(probe):
    """All probes once; the tests below read the failures of their primitives."""
    return wm.verify(run_on_device(probe))


def _of(failures, *prefixes):
    return [f for f in failures if f.startswith(prefixes)]


def _none(failures):
    assert not failures, "%d failures, the first of them:\n%s" % (len(failures), "\n".join(failures[:8]))


def test_every_probe_ran(measured):
    _, results = measured
    assert set(results) == set(wm.PRIMS)
    assert all(len(results[p][0]) == len(results[p][1][0]) > 0 for p in results)


def test_floating_sums(measured):
    _none(_of(measured[0], "wave_sum [", "half_sum [", "half_sum2 [", "halves_sum [", "half_sum(x * y)", "half_sum2(x * y, z * w) ["))


def test_integer_reductions(measured):
    _none(_of(measured[0], "wave_sum_i32 [", "wave_or [", "wave_min_i32 [", "wave_min_i32_xor [", "rows3_sum_i32 ["))


def test_minima_and_maxima(measured):
    _none(_of(measured[0], "wave_min [", "wave_max [", "half_min [", "vmax_f64 [", "vmin_f64 ["))


def test_nonneg_maxima(measured):
    """Positive iff some lane is positive, the maximum itself when it is >= +0.  All-negative input: the header said "max(0, ...)"; the
    device returns the negative maximum (the lane that is read never takes a filled value), which is what the header now says."""
    failures, results = measured
    _none(_of(failures, "wave_max_nonneg [", "half_max_nonneg ["))
    for prim, covered in (("wave_max_nonneg", 64), ("half_max_nonneg", 32)):
        names, outs, ins = results[prim]
        for case in ("all_negative", "all_negative_down", "all_negative_tiny"):
            c = names.index(case if covered == 64 else case + "/nan")
            want = np.full(wm.W, ins[0][c][:covered].max())
            print("%s [%s]: lanes all negative, returns %r (the maximum is %r)" % (prim, names[c], outs[0][c][0], want[0]))
            assert np.array_equal(wm.bits(outs[0][c]), wm.bits(want)), (prim, names[c], outs[0][c][0], want[0])


def test_results_per_lane(measured):
    _none(_of(measured[0], "quad_max [", "slices_max [", "group_max_nonneg<", "quad_argmax [", "gather_f64 [", "gather_i32 [", "readlane_f64 ["))


def test_ballots_and_uniform_values(measured):
    _none(_of(measured[0], "rank_in [", "first_lane [", "wave_any [", "lane_id [", "uniform_i32 [", "uniform_f64 ["))


def test_division_by_a_fixed_divisor(measured):
    _none(_of(measured[0], "fhu::"))


def test_bit_identities_of_the_comments(measured):
    _none(_of(measured[0], "half_sum2(a, b) ==", "half_sum2(x * y, z * w) ==", "half_sum ==", "half_min ==", "half_max_nonneg ==", "wave_min_i32 =="))


def test_nothing_else_failed(measured):
    _none(measured[0])
