"""The cases of tests/wave_model.py are sharp: the emulation of the DPP controls, with every primitive of fh_wave.hip.hpp written in it
the way the header writes it, meets every contract on every case, and each planted mutant of it fails at least one.  No GPU: this
proves the cases and the contracts, not the device (tests/test_gpu_wave.py holds the device to the same contracts).

Three changes that the eye takes for mutants cannot fail any case, and the test says so instead of pretending (the reasons stand beside
`EQUIVALENT` in tests/wave_model.py): in `wave_min`, zero fill in place of INFINITY changes lanes that lane 63, the lane which is
read, never depends on, and a row mask 0xf in place of 0xa or 0xc changes no lane of the final vector at all.  The test holds exactly
that: for the fill the lane vector does change and lane 63 does not; for the masks the whole vector keeps its bits."""
import numpy as np
import pytest

import wave_model as wm


@pytest.fixture(scope="module")
def emulated():
    return wm.verify(wm.run_emulation)


def test_the_emulation_meets_every_contract_on_every_case(emulated):
    failures, results = emulated
    assert set(results) == set(wm.PRIMS) and len(results) >= 30
    assert not failures, "%d failures, the first: %s" % (len(failures), failures[:5])


def test_the_cases_where_a_lane_network_goes_wrong_are_there():
    names = {p: [n for n, _ in prim.cases()] for p, prim in wm.PRIMS.items()}
    for p in ("wave_sum", "wave_min", "wave_max", "wave_max_nonneg", "wave_sum_i32", "wave_or", "wave_min_i32", "wave_min_i32_xor"):
        for l in range(wm.W):
            assert "onehot%d" % l in names[p], (p, l)
        for a, b in wm.BOUNDARY_PAIRS:
            assert "twohot%d_%d" % (a, b) in names[p], (p, a, b)
        for l in wm.EXTREME_LANES:
            assert "extreme%d" % l in names[p], (p, l)
        assert {"ramp_up", "ramp_down", "all_equal"} <= set(names[p]), p
    for p in ("half_sum", "half_min", "half_max_nonneg"):
        assert sum(n.endswith("/nan") for n in names[p]) > 90 and "onehot31/nan" in names[p] and "twohot31_32/full" in names[p], p
    assert "all_int_max" in names["wave_min_i32"] and "wrap_int_max" in names["wave_sum_i32"] and "onehot3/garbage" in names["rows3_sum_i32"]
    assert "all_negative" in names["wave_max_nonneg"] and "all_negative/nan" in names["half_max_nonneg"]
    assert {"sh0", "sh1", "sh2"} == {n.rsplit("/", 1)[1] for n in names["quad_argmax"]}
    n, d = (np.concatenate([c[1][j] for c in wm.PRIMS["udiv"].cases()]) for j in (0, 1))
    assert set(d.tolist()) == set(wm.UDIV_D) and n.min() == 0 and n.max() == 2 ** 28 - 1 and len(n) > 500


@pytest.mark.parametrize("name", sorted(wm.MUTANTS))
def test_each_mutant_fails_a_case(name):
    prim = wm.PRIMS[wm.MUTANTS[name][0]]
    ins = prim.stacked()
    failures = wm.check_cases(prim, ins, wm.run_emulation(prim, ins, wm.MUTANTS[name][1]))
    assert failures, "no case of %s tells '%s' from the header's form" % (prim.name, name)
    assert not wm.check_cases(prim, ins, wm.run_emulation(prim, ins)), "the unmutated form fails too: the mutant proves nothing"


def test_enough_mutants():
    assert len(wm.MUTANTS) >= 8


@pytest.mark.parametrize("name", sorted(wm.EQUIVALENT))
def test_changes_that_no_caller_can_see(name):
    """(module docstring) Lane 63, the lane that is read, has the same bits on every case; the lane vector before the read changes where
    the change reaches other lanes (the change is really planted) and keeps every bit where it reaches none."""
    prim_name, mutant, lanes, vector_changes = wm.EQUIVALENT[name]
    prim = wm.PRIMS[prim_name]
    ins = prim.stacked()
    plain = [wm.lanes_after(v, np.minimum, wm.SIX, wm.INF) for v in ins[0]]
    changed = [lanes(v) for v in ins[0]]
    assert any(not np.array_equal(wm.bits(a), wm.bits(b)) for a, b in zip(plain, changed)) == vector_changes, name
    assert all(wm.bits(a)[63] == wm.bits(b)[63] for a, b in zip(plain, changed)), name
    assert not wm.check_cases(prim, ins, wm.run_emulation(prim, ins, mutant))


def test_the_dpp_emulation_itself():
    """The controls on a vector of lane numbers: what each lane reads, what a lane without a source gets, what a row mask leaves alone."""
    v, old = np.arange(100, 164), np.full(64, -7)
    assert wm.dpp0(v, 0x111).tolist() == [0 if l % 16 == 0 else 99 + l for l in range(64)]
    assert wm.dpp(v, 0x118, 0xf, old, False).tolist() == [-7 if l % 16 < 8 else 92 + l for l in range(64)]
    assert wm.dpp(v, 0x142, 0xa, old, False).tolist() == [-7] * 16 + [115] * 16 + [-7] * 16 + [147] * 16
    assert wm.dpp(v, 0x143, 0xc, old, False).tolist() == [-7] * 32 + [131] * 32
    assert wm.dpp0(v, 0x143).tolist() == [0] * 32 + [131] * 32
    assert wm.dpp0(v, 0xB1)[:4].tolist() == [101, 100, 103, 102] and wm.dpp0(v, 0x4E)[60:].tolist() == [162, 163, 160, 161]
    assert wm.dpp0(v, 0x140)[16:32].tolist() == list(range(131, 115, -1)) and wm.dpp0(v, 0x141)[8:16].tolist() == list(range(115, 107, -1))
    a, b = wm.swap32(v, v + 1000)
    assert a.tolist() == list(range(100, 132)) + list(range(1100, 1132)) and b.tolist() == list(range(132, 164)) + list(range(1132, 1164))


def test_the_bars_of_a_sum():
    """The two bars bite: one ulp off the pairwise bits is caught, and so is an error above the fsum bound."""
    v = wm.binades(np.random.default_rng(5))
    good = np.full(64, wm.pairwise(v))
    wm.check_sum("t", "c", "sum", v, good, 6)
    with pytest.raises(wm.Mismatch, match=r"t \[c\] .* lane 0"):
        wm.check_sum("t", "c", "sum", v, np.nextafter(good, np.inf), 6)
    with pytest.raises(wm.Mismatch, match="above the bound"):
        wm.check_sum("t", "c", "sum", v, good + 1e-9 * np.abs(v).sum(), 6, tree=False)
    with pytest.raises(wm.Mismatch, match="lane 63"):
        wm.check_sum("t", "c", "sum", v, np.where(wm.LANE == 63, np.nextafter(good, np.inf), good), 6)
