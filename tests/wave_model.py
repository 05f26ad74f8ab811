"""What a caller of `faster_amd/csrc/fh_wave.hip.hpp` (and of `fhu::div`, `fh_udiv.hpp`) is promised, lane by lane, and the cases that
hold the device to it.  Three parts:

(a) CONTRACTS.  For each primitive a check in plain numpy / Python of what comes back in EVERY lane: `min`, `max`, `math.fsum`,
    `n // d`.  A contract does not restate the DPP steps.  Floating sums have two bars: |got - fsum| <= k u S / (1 - k u) with
    u = 2^-53, S = sum |v| and k the depth of the summation tree (6 for 64 lanes, 5 for 32, 1 for halves_sum) — the textbook bound
    of a tree of that depth, not tuned — and the bits of pairwise summation in lane order (`v = v[0::2] + v[1::2]` until one is left),
    which is the tree that row_shr 1/2/4/8, row_bcast:15, row_bcast:31 build: lane 15 of a row holds the balanced tree of its 16
    lanes, lane 63 holds (r3 + r2) + (r1 + r0).
(b) CASES, chosen for where a lane network goes wrong: one-hot in each lane, two-hot across the row and half boundaries, ramps,
    the extreme in the first and last lane of every row, infinities, denormals, cancellation, 40 binades of random values, INT_MIN /
    INT_MAX, wrapping sums, NaN or garbage in the lanes a primitive must not read.
(c) An EMULATION of the DPP controls the header uses (row_shr n, row_bcast:15, row_bcast:31 with row masks and zero or identity fill,
    quad_perm, row_mirror, row_half_mirror, the 32-lane swap) with every primitive written in it the way the header writes it, and
    MUTANTS of those.  tests/test_wave_model.py holds that the emulation meets (a) on (b) and that the mutants do not: the cases are
    sharp.  The device is never compared with the emulation, only with the contracts (tests/test_gpu_wave.py).

Both tests go through `verify(run)`: `run(prim, ins)` is the emulation or the probe library, everything else is shared.
"""
import math
from fractions import Fraction

import numpy as np

W = 64
INF = float("inf")
NAN = float("nan")
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
U = 2.0 ** -53
POISON_BYTE = 0xA5  # output buffers start as this byte: a lane that must not be written still holds it afterwards
POISON = {"f64": np.frombuffer(bytes([POISON_BYTE]) * 8, dtype=np.float64)[0], "i32": np.frombuffer(bytes([POISON_BYTE]) * 4, dtype=np.int32)[0],
          "u32": np.frombuffer(bytes([POISON_BYTE]) * 4, dtype=np.uint32)[0]}
DTYPE = {"f64": np.float64, "i32": np.int32, "u32": np.uint32, "i32s": np.int32, "u64s": np.uint64}
BOUNDARY_PAIRS = ((15, 16), (31, 32), (47, 48), (0, 63), (31, 63))
EXTREME_LANES = (0, 15, 16, 31, 32, 47, 48, 63)
LANE = np.arange(W)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a.view(np.uint32)


class Mismatch(AssertionError):
    pass


def _same(prim, case, what, got, want):
    """Bit for bit in every lane; the message names primitive, case and the first lane that differs."""
    got, want = np.asarray(got), np.asarray(want, dtype=np.asarray(got).dtype)
    g, w = bits(got), bits(want)
    bad = np.nonzero(g != w)[0]
    if len(bad):
        l = int(bad[0])
        raise Mismatch("%s [%s] %s, lane %d: got %r (%#x), want %r (%#x); %d lanes differ"
                       % (prim, case, what, l, got[l], int(g[l]), want[l], int(w[l]), len(bad)))


def _full(x, dtype=np.float64):
    return np.full(W, x, dtype=dtype)


# ------------------------------------------------------------------------------------------------------------ (a) contracts

def pairwise(x):
    v = np.array(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        while len(v) > 1:
            v = v[0::2] + v[1::2]
    return v[0]


def sum_bar(x, k):
    """(fsum, bound): the exact sum rounded once and k u S / (1 - k u).  With an infinity among the summands the sum is that infinity
    and the bound 0 (no case holds both signs)."""
    x = np.asarray(x, dtype=np.float64)
    if not np.all(np.isfinite(x)):
        return float(np.sum(x[~np.isfinite(x)])), 0.0
    return math.fsum(x.tolist()), k * U * math.fsum(np.abs(x).tolist()) / (1.0 - k * U)


def check_sum(prim, case, what, x, out, k, tree=True):
    """x: the covered lanes in lane order; out: what all 64 lanes got (the sum is wave-uniform)."""
    ref, bound = sum_bar(x, k)
    for l in range(W):
        g = float(out[l])
        if not (g == ref or abs(g - ref) <= bound):
            raise Mismatch("%s [%s] %s, lane %d: got %r, fsum %r, |difference| %r above the bound %r of a tree of depth %d"
                           % (prim, case, what, l, g, ref, abs(g - ref), bound, k))
    if tree:
        _same(prim, case, what + " (bits of pairwise summation in lane order)", out, _full(pairwise(x)))


def check_sum_of_products(prim, case, what, x, y, out, k):
    """out = sum of x[l] y[l]: against the exact sum of the exact products (rationals), one more rounding than the tree's depth for
    the products (a contracted first stage rounds less, never more)."""
    exact = sum((Fraction(float(a)) * Fraction(float(b)) for a, b in zip(x, y)), Fraction(0))
    mag = sum((abs(Fraction(float(a)) * Fraction(float(b))) for a, b in zip(x, y)), Fraction(0))
    bound = Fraction((k + 1) * U) * mag / (1 - Fraction((k + 1) * U))
    for l in range(W):
        if not abs(Fraction(float(out[l])) - exact) <= bound:
            raise Mismatch("%s [%s] %s, lane %d: got %r, exact %r, bound %r" % (prim, case, what, l, out[l], float(exact), float(bound)))


def check_nonneg_max(prim, case, x, out):
    """What `wave_max_nonneg` / `half_max_nonneg` promise: positive iff some covered lane is positive, and the maximum itself when it is
    >= +0.  On all-negative input only "not positive, no NaN, uniform" is promised (what comes back is recorded by the GPU test)."""
    m = float(np.max(x))
    if m >= 0.0:
        _same(prim, case, "maximum >= +0", out, _full(m))
    else:
        _same(prim, case, "uniform", out, _full(out[0]))
        if not float(out[0]) <= 0.0:
            raise Mismatch("%s [%s] all lanes negative, lane 0: got %r, not positive was promised" % (prim, case, out[0]))


def group_max(v, group):
    return np.repeat(np.max(np.asarray(v).reshape(-1, group), axis=1), group)


def argmax_contract(v, i, group):
    """The pair that wins each aligned group in the order "greater v first, then the smaller i as an unsigned number"."""
    ov, oi = np.empty(W), np.empty(W, dtype=np.int32)
    for g in range(0, W, group):
        best = min(range(g, g + group), key=lambda l: (-float(v[l]), int(i[l]) & 0xffffffff))
        ov[g:g + group], oi[g:g + group] = v[best], i[best]
    return ov, oi


def popcount_below(m, l):
    return bin(int(m) & ((1 << l) - 1)).count("1")


# --------------------------------------------------------------------------------------------------------------- (b) cases

def _rng(tag):
    return np.random.default_rng([ord(c) for c in tag])


def base_rows(identity, hot, extreme, dtype=np.float64, tag="rows"):
    """The cases every reduction gets.  hot(l): the value a hot lane l holds (distinct per lane); extreme: beyond a background in [1, 2)."""
    rng, rows = _rng(tag), []
    for l in range(W):
        r = np.full(W, identity, dtype=dtype)
        r[l] = hot(l)
        rows.append(("onehot%d" % l, r))
    for a, b in BOUNDARY_PAIRS:
        r = np.full(W, identity, dtype=dtype)
        r[a], r[b] = hot(a), hot(b)
        rows.append(("twohot%d_%d" % (a, b), r))
    rows.append(("ramp_up", np.arange(1, W + 1).astype(dtype)))
    rows.append(("ramp_down", np.arange(W, 0, -1).astype(dtype)))
    rows.append(("all_equal", np.full(W, 3, dtype=dtype)))
    for l in EXTREME_LANES:
        r = (rng.uniform(1.0, 2.0, W) if dtype == np.float64 else rng.integers(1000, 2000, W)).astype(dtype)
        r[l] = extreme
        rows.append(("extreme%d" % l, r))
    return rows


def binades(rng, signed=True):
    v = rng.uniform(1.0, 2.0, W) * 2.0 ** rng.integers(-20, 21, W)
    return v * rng.choice([-1.0, 1.0], W) if signed else v


def _with(row, **at):
    r = np.array(row)
    for k, x in at.items():
        r[int(k[1:])] = x
    return r


DENORMAL = 5e-324


def f64_rows(kind):
    """kind: 'sum', 'min', 'max' (any sign), 'nonneg' (wave / half_max_nonneg: any sign in, maximum >= +0), 'group' (values >= +0)."""
    rng = _rng("f64" + kind)
    hot = lambda l: 1.0 + l / 64.0  # noqa: E731
    if kind == "sum":
        rows = base_rows(0.0, hot, 1e10, tag="sum")
        rows += [("inf_pos", _with(binades(rng), l5=INF)), ("inf_neg", _with(binades(rng), l40=-INF)), ("inf_lane63", _with(binades(rng), l63=INF)),
                 ("denormals", DENORMAL * np.arange(1, W + 1)), ("denormals_signed", DENORMAL * np.arange(1, W + 1) * np.where(LANE % 3 == 0, -1.0, 1.0)),
                 ("denormal_beside_one", _with(_full(DENORMAL), l16=1.0, l47=-1.0)),
                 ("cancel_alternating", np.where(LANE % 2 == 0, 1e300, -1e300)),
                 ("cancel_ends", _with(_full(1.0), l0=1e300, l63=-1e300)),
                 ("cancel_rows", _with(binades(rng), l15=1e300, l16=-1e300, l31=1e300, l32=-1e300)),
                 ("cancel_low_half", _with(binades(rng), l3=1e300, l28=-1e300)),
                 ("big_same_sign", _full(1e300))]
    elif kind == "min":
        rows = base_rows(INF, hot, -100.0, tag="min")
        rows += [("all_identity", _full(INF)), ("neg_inf", _with(binades(rng), l33=-INF)), ("neg_inf_low", _with(binades(rng), l7=-INF)),
                 ("some_inf", _with(binades(rng), l0=INF, l15=INF, l31=INF, l63=INF)),
                 ("denormals", DENORMAL * np.arange(W, 0, -1)), ("denormals_neg", -DENORMAL * np.arange(1, W + 1)),
                 ("big", _with(_full(1e300), l20=-1e300, l52=-1e300)), ("ramp_negative", -np.arange(1.0, W + 1))]
    elif kind == "max":
        rows = base_rows(-INF, hot, 100.0, tag="max")
        rows += [("all_identity", _full(-INF)), ("pos_inf", _with(binades(rng), l33=INF)), ("pos_inf_low", _with(binades(rng), l7=INF)),
                 ("some_neg_inf", _with(binades(rng), l0=-INF, l15=-INF, l31=-INF, l63=-INF)),
                 ("denormals", DENORMAL * np.arange(1, W + 1)), ("denormals_neg", -DENORMAL * np.arange(1, W + 1)),
                 ("big", _with(_full(-1e300), l20=1e300, l52=1e300)), ("ramp_negative", -np.arange(1.0, W + 1)),
                 ("negative_down", -np.arange(float(W), 0.0, -1.0))]
    elif kind == "nonneg":
        rows = base_rows(0.0, hot, 100.0, tag="nonneg")
        rows += [("all_zero", _full(0.0)), ("pos_inf", _with(binades(rng), l33=INF)), ("pos_inf_low", _with(binades(rng), l7=INF)),
                 ("neg_inf_beside_positive", _with(_full(-INF), l9=2.0, l41=3.0)),
                 ("denormals", DENORMAL * np.arange(1, W + 1)), ("one_denormal", _with(_full(0.0), l31=DENORMAL, l63=DENORMAL)),
                 ("big", _with(_full(-1e300), l20=1e300, l52=1e300)),
                 ("negative_but_one_low", _with(-np.arange(1.0, W + 1), l16=0.5)), ("negative_but_one_high", _with(-np.arange(1.0, W + 1), l48=0.5)),
                 # outside "max(0, ...)" as a value, inside the contract "positive iff some lane is positive"
                 ("all_negative", -np.arange(1.0, W + 1)), ("all_negative_down", -np.arange(float(W), 0.0, -1.0)),
                 ("all_negative_tiny", _full(-DENORMAL))]
    else:
        rows = base_rows(0.0, hot, 100.0, tag="group")
        rows += [("all_zero", _full(0.0)), ("pos_inf", _with(binades(rng, False), l33=INF, l7=INF)), ("denormals", DENORMAL * np.arange(1, W + 1)),
                 ("big", _with(_full(1.0), l20=1e300, l52=1e300))]
    for s in range(8):
        v = binades(rng, signed=kind != "group")
        if kind == "nonneg":
            v[rng.integers(0, 32)] = abs(v[0]) + 1.0  # some lane of the low half is positive
        rows.append(("random40_%d" % s, v))
    return rows


def half_rows(rows, identity):
    """The 32-lane forms: each row as it is (whatever lanes 32..63 hold), with NaN in lanes 32..63 (not read) and with the identity there
    (where the half forms return the bits of the six-stage forms)."""
    out = []
    for name, r in rows:
        out.append((name + "/full", r))
        out.append((name + "/nan", np.concatenate([r[:32], np.full(32, NAN)])))
        out.append((name + "/id", np.concatenate([r[:32], np.full(32, identity)])))
    return out


def wave_rows(kind, identity):
    rows = f64_rows(kind)
    return rows + [(n, r) for n, r in half_rows(rows, identity) if n.endswith("/id")]


def i32_rows(kind):
    rng = _rng("i32" + kind)
    if kind == "min":
        rows = base_rows(INT_MAX, lambda l: 100 + l, -5000, np.int32, "imin")
        rows += [("all_int_max", _full(INT_MAX, np.int32)), ("int_min_lane", _with(_full(7, np.int32), l37=INT_MIN)),
                 ("int_min_low", _with(_full(INT_MAX, np.int32), l0=INT_MIN)), ("all_int_min", _full(INT_MIN, np.int32)),
                 ("negative", (-np.arange(1, W + 1)).astype(np.int32))]
    elif kind == "or":
        rows = base_rows(0, lambda l: 1 << (l % 31), 1 << 30, np.int32, "or")
        rows += [("all_ones", _full(-1, np.int32)), ("sign_bit", _with(_full(0, np.int32), l48=INT_MIN)), ("lane_bits", (1 << (LANE % 32)).astype(np.uint32).view(np.int32))]
    else:
        rows = base_rows(0, lambda l: 100 + l, 1 << 20, np.int32, "isum")
        rows += [("wrap_int_max", _full(INT_MAX, np.int32)), ("wrap_int_min", _full(INT_MIN, np.int32)),
                 ("wrap_pair", _with(_full(0, np.int32), l15=INT_MAX, l16=INT_MAX, l47=1, l63=1)),
                 ("int_min_int_max", np.where(LANE % 2 == 0, INT_MIN, INT_MAX).astype(np.int32)), ("minus_ones", _full(-1, np.int32))]
    for s in range(8):
        rows.append(("random_%d" % s, rng.integers(INT_MIN, INT_MAX, W, endpoint=True).astype(np.int32)))
    return rows


def rows3_rows():
    rng, out = _rng("rows3"), []
    for name, r in i32_rows("sum"):
        out.append((name + "/full", r))
        out.append((name + "/garbage", np.concatenate([r[:48], rng.integers(INT_MIN, INT_MAX, 16, endpoint=True).astype(np.int32)])))
    return out


def pair_up(rows, step=7):
    """Two-operand cases from a one-operand list: row j beside row j + step (named 'A + B')."""
    n = len(rows)
    return [("%s + %s" % (rows[j][0], rows[(j + step) % n][0]), (rows[j][1], rows[(j + step) % n][1])) for j in range(n)]


def product_rows():
    """(x, y) whose products are the summands of half_sum: exact products (small integers), inexact ones over 40 binades, NaN in the
    lanes that are not read."""
    rng, rows = _rng("products"), []
    rows.append(("small_integers", (rng.integers(-50, 50, W).astype(np.float64), rng.integers(-50, 50, W).astype(np.float64))))
    rows.append(("ramp_times_ramp", (np.arange(1.0, W + 1), np.arange(float(W), 0.0, -1.0))))
    for s in range(10):
        x, y = binades(rng), binades(rng)
        if s % 2:
            x[32:] = NAN
        rows.append(("random40_%d" % s, (x, y)))
    for l in (0, 15, 16, 31):
        x, y = np.zeros(W), rng.uniform(1.0, 2.0, W)
        x[l] = 1.0 / 3.0
        rows.append(("onehot%d" % l, (x, y)))
    rows.append(("cancel", (np.where(LANE % 2 == 0, 1e150, -1e150) * np.repeat(rng.uniform(1.0, 2.0, W // 2), 2), _full(1e150))))
    return rows


def argmax_cases():
    rng, out = _rng("argmax"), []
    rows = []
    idx = rng.permutation(W).astype(np.int32)
    rows.append(("all_equal_indices_decide", _full(2.5), idx))
    rows.append(("all_equal_minus_one_and_int_max", _full(2.5), _with(idx + 100, l1=-1, l6=-1, l8=INT_MAX, l13=INT_MAX, l18=-1, l19=INT_MAX,
                                                                      l32=INT_MAX, l35=-1, l60=-1, l61=-1, l62=-1, l63=5)))
    rows.append(("all_equal_high_bit", _full(-1.0), _with(idx, l0=INT_MIN, l5=INT_MIN, l10=-2, l11=-1, l50=INT_MIN + 1, l51=INT_MIN)))
    rows.append(("all_minus_one", _full(0.0), _full(-1, np.int32)))
    rows.append(("minus_one_against_zero", _full(0.0), np.where(LANE % 4 == 2, 0, -1).astype(np.int32)))
    v = np.tile([5.0, 1.0, 5.0, 1.0], 16)
    rows.append(("tie_across_pairs_02", v, np.tile(np.array([7, 0, 3, 0], np.int32), 16)))
    rows.append(("tie_across_pairs_13", np.tile([1.0, 5.0, 1.0, 5.0], 16), np.tile(np.array([0, 3, 0, 7], np.int32), 16)))
    rows.append(("tie_across_pairs_03", np.tile([5.0, 1.0, 1.0, 5.0], 16), np.tile(np.array([-1, 0, 0, 9], np.int32), 16)))
    rows.append(("tie_across_pairs_12", np.tile([1.0, 5.0, 5.0, 1.0], 16), np.tile(np.array([0, INT_MAX, INT_MIN, 0], np.int32), 16)))
    rows.append(("value_beats_index", np.tile([1.0, 2.0, 3.0, 4.0], 16), np.tile(np.array([0, 1, 2, -1], np.int32), 16)))
    rows.append(("distinct", binades(rng), idx))
    rows.append(("neg_inf", _with(_full(-INF), l2=1.0, l4=-5.0, l63=0.0), idx))
    for l in range(4):
        rows.append(("onehot_quad_lane%d" % l, np.where(LANE % 4 == l, 9.0, 1.0), idx))
    for s in range(4):
        rows.append(("random_ties_%d" % s, rng.integers(0, 3, W).astype(np.float64), rng.integers(-1, 3, W).astype(np.int32)))
    for name, v, i in rows:
        for sh in (0, 1, 2):
            out.append(("%s/sh%d" % (name, sh), (np.asarray(v, np.float64), np.asarray(i, np.int32), sh)))
    return out


def gather_sources():
    rng = _rng("gather")
    src = [("identity", LANE), ("reverse", 63 - LANE), ("rotate1", (LANE + 1) % W), ("rotate63", (LANE + 63) % W), ("rotate32", (LANE + 32) % W),
           ("all_to_0", _full(0, np.int64)), ("all_to_63", _full(63, np.int64)), ("all_to_17", _full(17, np.int64)), ("all_to_32", _full(32, np.int64)),
           ("permutation", rng.permutation(W)), ("repeats", rng.integers(0, W, W))]
    return [(n, s.astype(np.int32)) for n, s in src]


RANK_MASKS = [("zero", 0), ("all_ones", 2 ** 64 - 1), ("bit31", 1 << 31), ("bit32", 1 << 32), ("bit0", 1), ("bit63", 1 << 63),
              ("alternating_even", 0x5555555555555555), ("alternating_odd", 0xAAAAAAAAAAAAAAAA), ("low_half", 0xFFFFFFFF), ("high_half", 0xFFFFFFFF00000000)]


def predicate_rows():
    rng, rows = _rng("pred"), [("none", _full(0, np.int32)), ("all", _full(1, np.int32))]
    for l in range(W):
        rows.append(("onehot%d" % l, _with(_full(0, np.int32), **{"l%d" % l: (-1, 1, INT_MIN, 256)[l % 4]})))
    for a, b in BOUNDARY_PAIRS:
        rows.append(("twohot%d_%d" % (a, b), _with(_full(0, np.int32), **{"l%d" % a: 1, "l%d" % b: 1})))
    for s in range(4):
        rows.append(("random_%d" % s, (rng.random(W) < 0.1).astype(np.int32)))
    return rows


UNIFORM_FIRST = (0, 1, 15, 16, 31, 32, 33, 47, 48, 63)
UDIV_D = (1, 2, 3, 5, 7, 31, 32, 33, 1000, 2 ** 20 - 1, 2 ** 20)
UDIV_NMAX = 2 ** 28


def udiv_pairs():
    rng, pairs = _rng("udiv"), []
    for d in UDIV_D:
        ns = {0, 1, d - 1, d, d + 1, UDIV_NMAX - 1, (UDIV_NMAX - 1) // d * d, (UDIV_NMAX - 1) // d * d - 1}
        for k in (2, 3, 7, 100, 255, 4096):
            ns |= {k * d - 1, k * d, k * d + 1}
        ns |= set(int(x) for x in rng.integers(0, UDIV_NMAX, 24))
        pairs += [(n, d) for n in sorted(ns) if 0 <= n < UDIV_NMAX]
    return pairs


# ------------------------------------------------------------------------------------------------- (c) the DPP controls, emulated

def _source(ctrl, l):
    """The lane that lane l reads under a DPP control, None where it has none (the fill or the old value takes its place)."""
    if ctrl < 0x100:  # quad_perm
        return (l & ~3) + ((ctrl >> (2 * (l & 3))) & 3)
    if 0x111 <= ctrl <= 0x11f:  # row_shr n
        n = ctrl - 0x110
        return l - n if (l & 15) >= n else None
    if ctrl == 0x140:  # row_mirror
        return (l & ~15) + 15 - (l & 15)
    if ctrl == 0x141:  # row_half_mirror
        return (l & ~7) + 7 - (l & 7)
    if ctrl == 0x142:  # row_bcast:15: lane 15 of each row to the next row
        return (l & ~15) - 1 if l >= 16 else None
    if ctrl == 0x143:  # row_bcast:31: lane 31 to rows 2 and 3
        return 31 if l >= 32 else None
    raise ValueError(hex(ctrl))


def dpp(src, ctrl, row_mask=0xf, old=None, bound_ctrl=False):
    """update_dpp(old, src, ctrl, row_mask, 0xf, bound_ctrl): a row that the mask leaves out keeps `old`; a lane without a source takes 0
    with bound_ctrl and keeps `old` without."""
    src = np.asarray(src)
    out = np.zeros_like(src) if old is None else np.array(old, dtype=src.dtype)
    for l in range(W):
        if not (row_mask >> (l >> 4)) & 1:
            continue
        s = _source(ctrl, l)
        if s is not None:
            out[l] = src[s]
        elif bound_ctrl:
            out[l] = 0
    return out


def dpp0(v, ctrl):
    return dpp(v, ctrl, 0xf, None, True)


def swap32(vdst, src):
    """v_permlane32_swap: lanes 32..63 of vdst change places with lanes 0..31 of src.  Returns (vdst, src) afterwards."""
    return np.concatenate([vdst[:32], src[:32]]), np.concatenate([vdst[32:], src[32:]])


ROWS = (0x111, 0x112, 0x114, 0x118)
SIX = tuple((c, 0xf) for c in ROWS) + ((0x142, 0xa), (0x143, 0xc))
FIVE = SIX[:5]


def lanes_after(v, op, stages, fill=None):
    """The lane vector after the stages (ctrl, row mask).  fill None: the zero-filling form (dpp0, every row written); else `old`."""
    v = np.array(v)
    with np.errstate(all="ignore"):
        for ctrl, mask in stages:
            v = op(v, dpp0(v, ctrl) if fill is None else dpp(v, ctrl, mask, np.full(W, fill, dtype=v.dtype), False))
    return v


def _all(x, dtype=None):
    return np.full(W, x, dtype=dtype if dtype is not None else np.asarray(x).dtype)


def emu_wave_sum(v, stages=SIX, read=63):
    return _all(lanes_after(v, np.add, stages)[read])


def emu_half_sum(v, stages=FIVE, read=31):
    return _all(lanes_after(v, np.add, stages)[read])


def emu_halves_sum(v):
    a, b = swap32(v, v)
    with np.errstate(all="ignore"):
        return a + b


def emu_half_sum2(a, b, swap=True):
    with np.errstate(all="ignore"):
        a, b = a + dpp0(a, 0x111), b + dpp0(b, 0x111)
    v = swap32(a, b)[0] if swap else a
    v = lanes_after(v, np.add, ((0x112, 0xf), (0x114, 0xf), (0x118, 0xf), (0x142, 0xf)))
    return _all(v[31]), _all(v[63])


def emu_wave_sum_i32(v, stages=SIX):
    return _all(lanes_after(v, np.add, stages)[63])


def emu_wave_or(v):
    return _all(lanes_after(v, np.bitwise_or, SIX)[63])


def emu_wave_max_nonneg(v):
    return _all(lanes_after(v, np.maximum, SIX)[63])


def emu_half_max_nonneg(v):
    return _all(lanes_after(v, np.maximum, FIVE)[31])  # (what rows 2 and 3 make of a NaN does not reach lane 31)


def emu_wave_min(v, stages=SIX, fill=INF, read=63):
    return _all(lanes_after(v, np.minimum, stages, fill)[read])


def emu_wave_max(v):
    return _all(lanes_after(v, np.fmax, SIX, -INF)[63])


def emu_half_min(v):
    return _all(lanes_after(v, np.minimum, FIVE, INF)[31])


def emu_wave_min_i32(v, stages=SIX, fill=INT_MAX):
    return _all(lanes_after(v, np.minimum, stages, fill)[63])


def emu_wave_min_i32_xor(v):
    v = np.array(v)
    for o in (32, 16, 8, 4, 2, 1):
        v = np.minimum(v, v[LANE ^ o])
    return v


def emu_rows3_sum_i32(v, read=(15, 31, 47)):
    x = lanes_after(v, np.add, SIX[:4])
    with np.errstate(all="ignore"):
        return _all(np.sum(x[list(read)], dtype=np.int32))


def _greater(o, v):
    return np.where(o > v, o, v)


def emu_quad_max(v, second=0x4E):
    v = _greater(dpp0(v, 0xB1), v)
    return _greater(dpp0(v, second), v)


def emu_group_max_nonneg(v, group, mirror=True):
    for ctrl in (0xB1, 0x4E, 0x141) + ((0x140,) if group == 16 and mirror else ()):
        v = np.maximum(v, dpp0(v, ctrl))
    return v


def emu_slices_max(v, sh):
    for ctrl in (0xB1, 0x4E)[:sh]:
        v = np.maximum(v, dpp0(v, ctrl))
    return v


def emu_quad_argmax(v, i, sh, signed_tie=False):
    v, i = np.array(v), np.array(i)
    for ctrl in (0xB1, 0x4E)[:sh]:
        ov, oi = dpp0(v, ctrl), dpp0(i, ctrl)
        less = oi < i if signed_tie else oi.view(np.uint32) < i.view(np.uint32)
        take = (ov > v) | ((ov == v) & less)
        v, i = np.where(take, ov, v), np.where(take, oi, i)
    return v, i


def emu_rank_in(m, inclusive=False):
    lo, hi = int(m) & 0xffffffff, int(m) >> 32
    below = lambda word, l: bin(word & ((1 << min(max(l, 0), 32)) - 1)).count("1")  # noqa: E731  (mbcnt of one 32-bit word)
    return np.array([below(lo, l + inclusive) + below(hi, l + inclusive - 32) for l in range(W)], dtype=np.int32)


def emu_first_lane(p):
    m = sum(1 << l for l in range(W) if p[l] != 0)
    return _all((m & -m).bit_length() - 1 if m else -1, np.int32)


def emu_uniform(v, k, kind):
    out = np.full(W, POISON[kind], dtype=DTYPE[kind])
    out[k:] = v[k]
    return out


def emu_udiv(n, d):
    q, qf, inv, invf = (np.empty(W, np.int32), np.empty(W, np.int32), np.empty(W, np.uint32), np.empty(W, np.uint32))
    for l in range(W):
        nn, dd = int(n[l]), int(d[l])
        i0 = 0xffffffff if dd <= 1 else (1 << 32) // dd
        i1 = 0xffffffff if dd <= 1 else int(4294967296.0 / float(dd))
        for inverse, quot in ((i0, q), (i1, qf)):
            e = (nn * inverse) >> 32
            quot[l] = e + 1 if (nn - e * dd) % (1 << 32) >= dd else e
        inv[l], invf[l] = i0, i1
    return q, qf, inv, invf


# ----------------------------------------------------------------------------------------------------- the table of primitives

class Prim:
    def __init__(self, name, ins, outs, cases, check, emulate):
        self.name, self.ins, self.outs, self.check, self.emulate = name, tuple(ins), tuple(outs), check, emulate
        self._cases, self._made = cases, None

    def cases(self):
        """[(name, (operand, ...))], made once: rows of 64 lanes, or one word per case for the kinds that end in 's'."""
        if self._made is None:
            self._made = [(n, c if isinstance(c, tuple) else (c,)) for n, c in self._cases()]
            assert len({n for n, _ in self._made}) == len(self._made), self.name
        return self._made

    def rows(self):
        """[(name, first operand)]: the cases of a one-operand primitive, to build two-operand cases from."""
        return [(n, c[0]) for n, c in self.cases()]

    def stacked(self):
        """The operands of all cases, one array per operand: (cases, 64) for rows, (cases,) for words."""
        cs = self.cases()
        return [np.ascontiguousarray(np.array([c[1][j] for c in cs], dtype=DTYPE[k]).reshape((len(cs), W) if not k.endswith("s") else (len(cs),)))
                for j, k in enumerate(self.ins)]


PRIMS = {}


def _prim(name, ins, outs, cases, check, emulate):
    PRIMS[name] = Prim(name, ins, outs, cases, check, emulate)


def _reduction(name, kind_rows, covered, check_value, emulate, kind="f64"):
    def check(case, ins, outs):
        check_value(name, case, ins[0][:covered], outs[0])
    _prim(name, (kind,), (kind,), kind_rows, check, lambda v: (emulate(v),))


_reduction("wave_sum", lambda: wave_rows("sum", 0.0), 64, lambda p, c, x, o: check_sum(p, c, "sum of lanes 0..63", x, o, 6), emu_wave_sum)
_reduction("half_sum", lambda: half_rows(f64_rows("sum"), 0.0), 32, lambda p, c, x, o: check_sum(p, c, "sum of lanes 0..31", x, o, 5), emu_half_sum)
_reduction("wave_min", lambda: wave_rows("min", INF), 64, lambda p, c, x, o: _same(p, c, "min of lanes 0..63", o, _full(np.min(x))), emu_wave_min)
_reduction("half_min", lambda: half_rows(f64_rows("min"), INF), 32, lambda p, c, x, o: _same(p, c, "min of lanes 0..31", o, _full(np.min(x))), emu_half_min)
_reduction("wave_max_nonneg", lambda: wave_rows("nonneg", 0.0), 64, check_nonneg_max, emu_wave_max_nonneg)
_reduction("half_max_nonneg", lambda: half_rows(f64_rows("nonneg"), 0.0), 32, check_nonneg_max, emu_half_max_nonneg)
_reduction("wave_sum_i32", lambda: i32_rows("sum"), 64,
           lambda p, c, x, o: _same(p, c, "sum mod 2^32", o, _full((int(np.sum(x.astype(np.int64))) + 2 ** 31) % 2 ** 32 - 2 ** 31, np.int32)), emu_wave_sum_i32, "i32")
_reduction("rows3_sum_i32", rows3_rows, 48,
           lambda p, c, x, o: _same(p, c, "sum of lanes 0..47 mod 2^32", o, _full((int(np.sum(x.astype(np.int64))) + 2 ** 31) % 2 ** 32 - 2 ** 31, np.int32)),
           emu_rows3_sum_i32, "i32")
_reduction("wave_or", lambda: i32_rows("or"), 64, lambda p, c, x, o: _same(p, c, "or", o, _full(np.bitwise_or.reduce(x), np.int32)), emu_wave_or, "i32")
_reduction("wave_min_i32", lambda: i32_rows("min"), 64, lambda p, c, x, o: _same(p, c, "min", o, _full(np.min(x), np.int32)), emu_wave_min_i32, "i32")
_reduction("wave_min_i32_xor", lambda: i32_rows("min"), 64, lambda p, c, x, o: _same(p, c, "min", o, _full(np.min(x), np.int32)), emu_wave_min_i32_xor, "i32")


def _wave_max_rows():
    rows = wave_rows("max", -INF)
    base = binades(_rng("wavemaxnan"))
    for l in EXTREME_LANES:  # NaN lanes are ignored while some lane holds a number
        rows.append(("nan_lane%d" % l, _with(base, **{"l%d" % l: NAN})))
        rows.append(("only_number_lane%d" % l, _with(_full(NAN), **{"l%d" % l: -3.0 - l})))
    rows.append(("nan_rows_0_and_2", np.where((LANE >> 4) % 2 == 0, NAN, base)))
    return rows


_reduction("wave_max", _wave_max_rows, 64, lambda p, c, x, o: _same(p, c, "max of the lanes that hold a number", o, _full(np.nanmax(x))), emu_wave_max)


def _check_halves_sum(case, ins, outs):
    v = ins[0]
    with np.errstate(all="ignore"):
        want = np.tile(v[:32] + v[32:], 2)
    _same("halves_sum", case, "v[l % 32] + v[l % 32 + 32]", outs[0], want)
    for l in range(32):  # the first bar, k = 1 (implied by the bits; stated as for the other sums)
        check_sum("halves_sum", case, "pair %d" % l, np.array([v[l], v[l + 32]]), _full(outs[0][l]), 1, tree=False)


_prim("halves_sum", ("f64",), ("f64",), lambda: f64_rows("sum"), _check_halves_sum, lambda v: (emu_halves_sum(v),))


def _check_half_sum2(case, ins, outs):
    check_sum("half_sum2", case, "sa: sum of a in lanes 0..31", ins[0][:32], outs[0], 5)
    check_sum("half_sum2", case, "sb: sum of b in lanes 0..31", ins[1][:32], outs[1], 5)


_prim("half_sum2", ("f64", "f64"), ("f64", "f64"), lambda: pair_up(PRIMS["half_sum"].rows()), _check_half_sum2, emu_half_sum2)

_prim("half_sum_prod", ("f64", "f64"), ("f64",), product_rows,
      lambda case, ins, outs: check_sum_of_products("half_sum(x * y)", case, "lanes 0..31", ins[0][:32], ins[1][:32], outs[0], 5),
      lambda x, y: (emu_half_sum(x * y),))


def _product_pairs():
    rows = product_rows()
    return [("%s + %s" % (rows[j][0], rows[(j + 3) % len(rows)][0]), rows[j][1] + rows[(j + 3) % len(rows)][1]) for j in range(len(rows))]


def _check_half_sum2_prod(case, ins, outs):
    check_sum_of_products("half_sum2(x * y, z * w)", case, "sa", ins[0][:32], ins[1][:32], outs[0], 5)
    check_sum_of_products("half_sum2(x * y, z * w)", case, "sb", ins[2][:32], ins[3][:32], outs[1], 5)


_prim("half_sum2_prod", ("f64",) * 4, ("f64", "f64"), _product_pairs, _check_half_sum2_prod, lambda x, y, z, w: emu_half_sum2(x * y, z * w))


def _elementwise_rows():
    rng = _rng("vminmax")
    a, b = binades(rng), binades(rng)
    special = np.array([INF, -INF, DENORMAL, -DENORMAL, 1e300, -1e300, 0.0, 1.0])
    return [("random40", (a, b)), ("equal", (a, a.copy())), ("swapped", (b, a)),
            ("special_pairs", (np.repeat(special, 8), np.tile(special, 8))),  # (+0, +0) is the only zero pair: no +0 beside -0
            ("denormals", (DENORMAL * LANE, DENORMAL * (63 - LANE)))]


def _check_vminmax(case, ins, outs):
    _same("vmax_f64", case, "max(a, b)", outs[0], np.maximum(ins[0], ins[1]))
    _same("vmin_f64", case, "min(a, b)", outs[1], np.minimum(ins[0], ins[1]))


_prim("vminmax_f64", ("f64", "f64"), ("f64", "f64"), _elementwise_rows, _check_vminmax, lambda a, b: (np.maximum(a, b), np.minimum(a, b)))

_prim("quad_max", ("f64",), ("f64",), lambda: f64_rows("max"), lambda case, ins, outs: _same("quad_max", case, "max of the aligned four", outs[0], group_max(ins[0], 4)),
      lambda v: (emu_quad_max(v),))
for _g in (8, 16):
    _prim("group_max_nonneg%d" % _g, ("f64",), ("f64",), lambda: f64_rows("group"),
          lambda case, ins, outs, g=_g: _same("group_max_nonneg<%d>" % g, case, "max of the aligned %d" % g, outs[0], group_max(ins[0], g)),
          lambda v, g=_g: (emu_group_max_nonneg(v, g),))
_prim("slices_max", ("f64", "i32s"), ("f64",), lambda: [("%s/sh%d" % (n, sh), (r, sh)) for n, r in f64_rows("max") for sh in (0, 1, 2)],
      lambda case, ins, outs: _same("slices_max", case, "max of the aligned %d" % (1 << ins[1]), outs[0], group_max(ins[0], 1 << int(ins[1]))),
      lambda v, sh: (emu_slices_max(v, int(sh)),))


def _check_argmax(case, ins, outs):
    wv, wi = argmax_contract(ins[0], ins[1], 1 << int(ins[2]))
    _same("quad_argmax", case, "v of the winner", outs[0], wv)
    _same("quad_argmax", case, "i of the winner", outs[1], wi)


_prim("quad_argmax", ("f64", "i32", "i32s"), ("f64", "i32"), argmax_cases, _check_argmax, lambda v, i, sh: emu_quad_argmax(v, i, int(sh)))

_GATHER_F64 = binades(_rng("gatherv"))
_GATHER_I32 = _rng("gatheri").integers(INT_MIN, INT_MAX, W, endpoint=True).astype(np.int32)
_prim("gather_f64", ("f64", "i32"), ("f64",), lambda: [(n, (_GATHER_F64, s)) for n, s in gather_sources()],
      lambda case, ins, outs: _same("gather_f64", case, "v[src[l]]", outs[0], ins[0][ins[1]]), lambda v, s: (v[s],))
_prim("gather_i32", ("i32", "i32"), ("i32",), lambda: [(n, (_GATHER_I32, s)) for n, s in gather_sources()],
      lambda case, ins, outs: _same("gather_i32", case, "v[src[l]]", outs[0], ins[0][ins[1]]), lambda v, s: (v[s],))
_prim("readlane_f64", ("f64", "i32s"), ("f64",), lambda: [("lane%d" % l, (_GATHER_F64, l)) for l in range(W)],
      lambda case, ins, outs: _same("readlane_f64", case, "v[lane]", outs[0], _full(ins[0][int(ins[1])])), lambda v, l: (_all(v[int(l)]),))


def _rank_masks():
    rng = _rng("rank")
    return [(n, (m,)) for n, m in RANK_MASKS] + [("random_%d" % s, (int(rng.integers(0, 2 ** 64, dtype=np.uint64)),)) for s in range(8)]


_prim("rank_in", ("u64s",), ("i32",), _rank_masks,
      lambda case, ins, outs: _same("rank_in", case, "popcount(m & ((1 << l) - 1))", outs[0], np.array([popcount_below(ins[0], l) for l in range(W)], np.int32)),
      lambda m: (emu_rank_in(m),))
_prim("first_lane", ("i32",), ("i32",), predicate_rows,
      lambda case, ins, outs: _same("first_lane", case, "lowest lane with pred, -1 if none", outs[0],
                                    _full(int(np.nonzero(ins[0])[0][0]) if ins[0].any() else -1, np.int32)),
      lambda p: (emu_first_lane(p),))
_prim("wave_any", ("i32",), ("i32",), predicate_rows,
      lambda case, ins, outs: _same("wave_any", case, "any lane with pred", outs[0], _full(int(ins[0].any()), np.int32)),
      lambda p: (_all(int(emu_first_lane(p)[0] >= 0), np.int32),))
_prim("lane_id", ("i32",), ("i32",), lambda: [("zeros", _full(0, np.int32)), ("garbage", _GATHER_I32)],
      lambda case, ins, outs: _same("lane_id", case, "l", outs[0], LANE.astype(np.int32)), lambda v: (LANE.astype(np.int32),))
for _k in ("i32", "f64"):
    def _check_uniform(case, ins, outs, kind=_k):
        k = int(ins[1])
        want = np.full(W, POISON[kind], dtype=DTYPE[kind])
        want[k:] = ins[0][k]
        _same("uniform_" + kind, case, "lane %d's value in lanes %d..63, lanes below untouched" % (k, k), outs[0], want)
    _prim("uniform_" + _k, (_k, "i32s"), (_k,), lambda kind=_k: [("first_active%d" % k, ((_GATHER_I32 if kind == "i32" else _GATHER_F64), k)) for k in UNIFORM_FIRST],
          _check_uniform, lambda v, k, kind=_k: (emu_uniform(v, int(k), kind),))


def _udiv_rows():
    pairs = udiv_pairs()
    pairs += [(0, 1)] * (-len(pairs) % W)
    a = np.array(pairs, dtype=np.int32).reshape(-1, W, 2)
    return [("pairs%d_d%d_to_d%d" % (j, a[j, 0, 1], a[j, -1, 1]), (a[j, :, 0].copy(), a[j, :, 1].copy())) for j in range(len(a))]


def _check_udiv(case, ins, outs):
    n, d = ins[0].astype(np.int64), ins[1].astype(np.int64)
    inv = np.where(d == 1, 2 ** 32 - 1, 2 ** 32 // d).astype(np.uint32)
    _same("fhu::inverse", case, "2^32 // d", outs[2], inv)
    _same("fhu::inverse_fp", case, "2^32 // d", outs[3], inv)
    _same("fhu::div with inverse", case, "n // d", outs[0], (n // d).astype(np.int32))
    _same("fhu::div with inverse_fp", case, "n // d", outs[1], (n // d).astype(np.int32))


_prim("udiv", ("i32", "i32"), ("i32", "i32", "u32", "u32"), _udiv_rows, _check_udiv, emu_udiv)


# ------------------------------------------------------------------------------------------------------------------ running it

def run_emulation(prim, ins, emulate=None):
    """The emulation as a `run`: the operands of all cases in, one (cases, 64) array per result out."""
    fn = emulate or prim.emulate
    n = len(ins[0])
    outs = [np.empty((n, W), dtype=DTYPE[k]) for k in prim.outs]
    for c in range(n):
        for o, r in zip(outs, fn(*[a[c] for a in ins])):
            o[c] = r
    return outs


def check_cases(prim, ins, outs):
    """The failures ("primitive [case] what, lane: got, want") of one primitive over all its cases."""
    failures = []
    for c, (name, _) in enumerate(prim.cases()):
        try:
            prim.check(name, [a[c] for a in ins], [o[c] for o in outs])
        except Mismatch as e:
            failures.append(str(e))
    return failures


def check_identities(results):
    """The bit identities the header's comments claim, between the outputs of the probes.  results: name -> (case names, outs, ins).
    +0 is the identity of a maximum only among values >= +0: the `_nonneg` identity is asked where the low half holds such a value."""
    failures = []

    def out_of(prim, case, j=0):
        return results[prim][1][j][results[prim][0].index(case)]

    def same(what, case, a, b):
        try:
            _same(what, case, "identity", a, b)
        except Mismatch as e:
            failures.append(str(e))

    for pair, single, what in (("half_sum2", "half_sum", "half_sum2(a, b) == (half_sum(a), half_sum(b))"),
                               ("half_sum2_prod", "half_sum_prod", "half_sum2(x * y, z * w) == (half_sum(x * y), half_sum(z * w))")):
        for case in results[pair][0]:
            a, b = case.split(" + ")
            same(what, case, out_of(pair, case, 0), out_of(single, a))
            same(what, case, out_of(pair, case, 1), out_of(single, b))
    for half, wave in (("half_sum", "wave_sum"), ("half_min", "wave_min"), ("half_max_nonneg", "wave_max_nonneg")):
        ids = [c for j, c in enumerate(results[half][0]) if c.endswith("/id") and (wave != "wave_max_nonneg" or np.max(results[half][2][0][j][:32]) >= 0.0)]
        assert len(ids) > 80, half
        for case in ids:
            same("%s == %s with the identity in lanes 32..63" % (half, wave), case, out_of(half, case), out_of(wave, case))
    for case in results["wave_min_i32"][0]:
        same("wave_min_i32 == wave_min_i32_xor", case, out_of("wave_min_i32", case), out_of("wave_min_i32_xor", case))
    return failures


def verify(run, only=None):
    """Every primitive (or those named) on all its cases through `run(prim, ins) -> outs`, then the identities.  Returns
    (failures, results)."""
    failures, results = [], {}
    for name, prim in PRIMS.items():
        if only is not None and name not in only:
            continue
        ins = prim.stacked()
        outs = run(prim, ins)
        failures += check_cases(prim, ins, outs)
        results[name] = ([n for n, _ in prim.cases()], outs, ins)
    if only is None:
        failures += check_identities(results)
    return failures, results


# --------------------------------------------------------------------------------------------------------------------- mutants

# name -> (primitive, the emulation with one thing wrong).  Each must fail at least one case of its primitive.
MUTANTS = {
    "wave_sum without row_shr 8": ("wave_sum", lambda v: (emu_wave_sum(v, tuple(s for s in SIX if s[0] != 0x118)),)),
    "wave_sum without row_bcast:31": ("wave_sum", lambda v: (emu_wave_sum(v, SIX[:5]),)),
    "wave_sum_i32 without row_bcast:15": ("wave_sum_i32", lambda v: (emu_wave_sum_i32(v, SIX[:4] + SIX[5:]),)),
    "wave_sum read from lane 31": ("wave_sum", lambda v: (emu_wave_sum(v, SIX, 31),)),
    "wave_min read from lane 31": ("wave_min", lambda v: (emu_wave_min(v, read=31),)),
    "quad_argmax tie by signed comparison": ("quad_argmax", lambda v, i, sh: emu_quad_argmax(v, i, int(sh), signed_tie=True)),
    "rows3_sum_i32 reads lane 63 as well": ("rows3_sum_i32", lambda v: (emu_rows3_sum_i32(v, (15, 31, 47, 63)),)),
    "half_sum with six stages, read from lane 63": ("half_sum", lambda v: (emu_half_sum(v, SIX, 63),)),
    "half_sum2 without the move of b": ("half_sum2", lambda a, b: emu_half_sum2(a, b, swap=False)),
    "halves_sum adds a lane to itself": ("halves_sum", lambda v: (v + v,)),
    "quad_max with quad_perm [1,0,3,2] twice": ("quad_max", lambda v: (emu_quad_max(v, 0xB1),)),
    "group_max_nonneg<16> without row_mirror": ("group_max_nonneg16", lambda v: (emu_group_max_nonneg(v, 16, mirror=False),)),
    "rank_in counts its own lane": ("rank_in", lambda m: (emu_rank_in(m, inclusive=True),)),
}

# Three changes that look like mutants and are none, in `wave_min` as in every form that reads lane 63.
#  * Zero fill in place of INFINITY: a fill goes to a lane without a source, and the lane that is read never is one, nor is any lane it
#    depends on — every row_shr source of lane 15 of a row lies inside the row.  Other lanes of the vector change, lane 63 does not.
#  * Row mask 0xf in place of 0xa: row 0 has no source under row_bcast:15 and keeps `old`; row 2 takes min(., r1), which row_bcast:31
#    brings it anyway as lane 31 = min(r1, r0).  Row mask 0xf in place of 0xc: rows 0 and 1 have no source under row_bcast:31.  With an
#    idempotent operation not one lane of the final vector changes.  (The sums run unmasked for the same reason: rows 0 and 2 pick up
#    partial sums nobody reads, fh_wave.hip.hpp at dpp0_f64.)
# name -> (primitive, result, lane vector before the read, whether some lane of that vector changes).
_MIN_0xf_0xa = tuple((c, 0xf) for c in ROWS) + ((0x142, 0xf), (0x143, 0xc))
_MIN_0xf_0xc = tuple((c, 0xf) for c in ROWS) + ((0x142, 0xa), (0x143, 0xf))
EQUIVALENT = {
    "wave_min with row mask 0xf in place of 0xa": ("wave_min", lambda v: (emu_wave_min(v, _MIN_0xf_0xa),), lambda v: lanes_after(v, np.minimum, _MIN_0xf_0xa, INF), False),
    "wave_min with row mask 0xf in place of 0xc": ("wave_min", lambda v: (emu_wave_min(v, _MIN_0xf_0xc),), lambda v: lanes_after(v, np.minimum, _MIN_0xf_0xc, INF), False),
    "wave_min with zero fill in place of INFINITY": ("wave_min", lambda v: (emu_wave_min(v, fill=0.0),), lambda v: lanes_after(v, np.minimum, SIX, 0.0), True),
}
