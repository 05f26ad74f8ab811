"""CPU-side checks of include/fasterhip_gain.h: its entry point is declared there and in no other header, the header compiles alone as
C99 and C++11, the struct layouts and constants equal faster_amd/abi.py, FH_ABI_VERSION stays, the symbol is exported and bound in a
list of its own, the device code lives in fh_gain.hip.hpp which fh_reach.hip alone includes, the files the feature must not touch do
not name it, every clause of the prologue answers FH_ERR_ARG in the stated order (all of them come before the first call of the
runtime, so host pointers stand in for device pointers), and Fleet.explore_gain raises explore_reachable()'s errors before any launch."""
import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from faster_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "faster_amd", "csrc")
HDR = os.path.join(INC, "fasterhip.h")
NEW_HDR = os.path.join(INC, "fasterhip_gain.h")
NEW = ["fh_gain_goals_device"]
NAMES = r"fh_gain|fasterhip_gain|FH_GAIN|gain_goals|gain_record|gain_params|explore_gain"
OK, ARG, DEVICE = 0, -1, -2


@pytest.fixture(scope="module")
def built():
    from faster_amd import build as fb

    fb.build_all()
    return fb


def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(fh_[a-z_0-9]+)\s*\(", text))


def test_the_entry_point_is_declared_in_its_own_header_which_compiles_alone(tmp_path):
    assert set(NEW) == _declared(NEW_HDR)
    for other in glob.glob(os.path.join(INC, "*.h")):
        if other != NEW_HDR:
            assert not set(NEW) & _declared(other), other
            assert not re.search(NAMES, open(other).read()), other
    for untouched in ("fh_map.hip", "fh_capi.hip", "fh_pool.hip"):
        assert not re.search(NAMES, open(os.path.join(CSRC, untouched)).read()), untouched
    for other in glob.glob(os.path.join(CSRC, "*.hpp")):
        if os.path.basename(other) != "fh_gain.hip.hpp":
            assert not re.search(NAMES, open(other).read()), other
    assert int(re.search(r"#define FH_ABI_VERSION (\d+)", open(HDR).read()).group(1)) == abi.FH_ABI_VERSION == 9
    text = open(NEW_HDR).read()
    for inc in ("fasterhip.h", "fasterhip_frontier.h", "fasterhip_reach.h"):
        assert '#include "%s"' % inc in text
    assert not re.search(r"fh_spread|fasterhip_spread|FH_SPREAD", text)
    src = "#include \"fasterhip_gain.h\"\nint main(void) {\n" + "".join("  (void)%s;\n" % n for n in NEW) + "  return 0;\n}\n"
    for lang, std, comp in (("c", "-std=c99", "gcc"), ("c++", "-std=c++11", "g++")):
        f = tmp_path / ("probe." + ("c" if lang == "c" else "cpp"))
        f.write_text(src)
        r = subprocess.run([comp, "-fsyntax-only", "-x", lang, std, "-Wall", "-pedantic", "-I", INC, str(f)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr.strip(), (lang, r.stderr[-2000:])


def test_struct_layouts_and_constants_of_the_header_equal_abi_py(tmp_path):
    """sizeof and every offsetof of the two structs, printed by a C program compiled against the header."""
    structs = (("fh_gain_params", abi.gain_params_dtype, 64), ("fh_gain_record", abi.gain_record_dtype, 64))
    consts = ["FH_GAIN_MAX_RADIUS", "FH_GAIN_MAX_HOP_COST", "FH_GAIN_ALL_POOR"]
    kept = ["FH_FRONTIER_WANTED", "FH_FRONTIER_FOUND", "FH_FRONTIER_NO_VIEW", "FH_FRONTIER_BAD_POS", "FH_REACH_START_OUTSIDE", "FH_REACH_BOX_TOO_LARGE",
            "FH_REACH_CUT"]
    lines = []
    for name, dt, _ in structs:
        lines.append('  printf("%s.size %%d\\n", (int)sizeof(%s));' % (name, name))
        lines += ['  printf("%s.%s %%d\\n", (int)offsetof(%s, %s));' % (name, k, name, k) for k in dt.names]
    lines += ['  printf("%s %%d\\n", (int)%s);' % (k, k) for k in consts + kept]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"fasterhip_gain.h\"\nint main(void) {\n" + "\n".join(lines)
                   + "\n  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", INC, str(src), "-o", str(exe)])
    got = dict((k, int(v)) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()))
    for name, dt, size in structs:
        assert got[name + ".size"] == dt.itemsize == size, name
        for k in dt.names:
            assert got[name + "." + k] == dt.fields[k][1], (name, k)
    for k in consts + kept:
        assert got[k] == getattr(abi, k), k
    assert [getattr(abi, k) for k in consts] == [31, 16384, 128]
    # the flag sits beside the bits of the two headers before it, which keep their values
    assert [got[k] for k in kept] == [1, 2, 4, 8, 16, 32, 64] and not got["FH_GAIN_ALL_POOR"] & sum(got[k] for k in kept)
    # the params begin as fh_reach_params does (40 bytes), and the first 40 bytes of the record are fh_reach_record's
    for k in ("r_max", "r_avoid", "z_lo", "z_hi", "want", "max_hops"):
        assert abi.gain_params_dtype.fields[k] == abi.reach_params_dtype.fields[k], k
    assert abi.gain_params_dtype.fields["gain_radius"][1] == 40 == abi.reach_params_dtype.fields["reserved"][1]
    for k in ("flags", "view", "cell", "hops", "candidates", "reachable", "reached", "levels", "d2"):
        assert abi.gain_record_dtype.fields[k] == abi.reach_record_dtype.fields[k], k
    assert abi.gain_record_dtype.fields["gain"][1] == 40 == abi.reach_record_dtype.fields["reserved"][1]
    p = abi.default_gain_params(2.5, 7)
    assert (float(p["r_max"]), float(p["r_avoid"]), float(p["z_lo"]), float(p["z_hi"]), int(p["want"]), int(p["max_hops"]), int(p["gain_radius"]),
            int(p["hop_cost"]), int(p["min_gain"])) == (2.5, 0.0, -np.inf, np.inf, abi.FH_FRONTIER_WANT_REACHED, 0, 7, 1, 0) and not p["reserved"].any()
    r = abi.default_reach_params(2.5)
    assert p.tobytes()[:40] == r.tobytes()[:40]


def test_the_symbol_is_exported_and_bound_and_the_device_code_is_included_by_fh_reach_hip_alone(built):
    from faster_amd import capi
    from faster_amd.fleet import Fleet

    L = ctypes.CDLL(built.SO)
    for name in NEW:
        assert hasattr(L, name), name
    assert capi.GAIN_SYMBOLS == NEW
    lists = [k for k in dir(capi) if k.endswith("SYMBOLS") and k != "GAIN_SYMBOLS"]
    assert len(lists) >= 14 and "SYMBOLS" in lists and "REACH_SYMBOLS" in lists and "SPREAD_SYMBOLS" in lists
    for k in lists:
        assert not set(NEW) & set(getattr(capi, k)), k
    assert len(capi.lib().fh_gain_goals_device.argtypes) == 14
    assert hasattr(capi.Map, "gain_goals_device")
    for name in ("explore_gain", "explore_gain_stages", "gain_records"):
        assert hasattr(Fleet, name), name
    assert NEW_HDR in built.DEPS and os.path.join(CSRC, "fh_gain.hip.hpp") in built.DEPS
    assert built.SOURCES[-1] == os.path.join(CSRC, "fh_reach.hip") and len(built.SOURCES) == 4
    assert "capi.GAIN_SYMBOLS" in open(os.path.join(ROOT, "__graft_entry__.py")).read()   # build() touches the new symbol
    assert capi.lib().fh_abi_version() == 9
    strip = lambda path: re.sub(r"//[^\n]*", "", open(path).read())   # noqa: E731
    for other in glob.glob(os.path.join(CSRC, "*")):
        if os.path.basename(other) != "fh_reach.hip":
            assert "fh_gain.hip.hpp" not in strip(other), other
    includes = re.findall(r'#include "([^"]+)"', strip(os.path.join(CSRC, "fh_reach.hip")))
    assert includes.index("fh_gain.hip.hpp") > includes.index("fh_spread.hip.hpp") == includes.index("fh_reach.hip.hpp") + 1
    body = strip(os.path.join(CSRC, "fh_gain.hip.hpp"))
    assert sorted(set(re.findall(r"\b(\w+_kernel)\s*\(", body))) == ["gain_goals_kernel"]
    assert "#pragma clang fp contract(off)" in body and "atomic" not in body.lower()
    with pytest.raises(capi.FasterHipError):
        capi.Map.gain_goals_device(None, abi.default_reach_params(1.0), None, None, 0, None, 1, None, 0, None, None, None, None)   # not a gain record


def test_every_argument_rule_in_the_stated_order(built):
    """Case k breaks clause k and every clause after it, and keeps every clause before it: FH_ERR_ARG.  Nothing but the last clauses
    passing gives anything else: FH_OK for n == 0 without any pointer, and with host memory for d_records the runtime is asked whose
    it is and the answer is FH_ERR_DEVICE, with or without a device."""
    from faster_amd import capi

    L = capi.lib()
    buf = np.zeros(1 << 16, dtype=np.uint8)
    d = buf.ctypes.data
    nan, inf = float("nan"), float("inf")

    def grid(res=0.5, dims=(8, 8, 4)):
        g = np.zeros(1, dtype=abi.voxel_grid_dtype)
        g["origin"], g["res"], g["dims"] = (0.1, 0.2, 0.3), res, dims
        return g

    def par(**kw):
        p = np.ascontiguousarray(abi.default_gain_params(1.5, 3)).reshape(1).copy()
        for k, v in kw.items():
            p[k] = v
        return p

    good = dict(p=par(), mg=grid(res=0.3, dims=(9, 9, 5)), bits=d + 20480, g=grid(), flags=d, stride=256, view_of=None, n_views=2, veh=d + 1024, n=1,
                goals=d + 4096, mask=d + 8192, rec=d + 12288)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        ptr = lambda x: None if x is None else abi.ptr(x)   # noqa: E731
        return L.fh_gain_goals_device(None, ptr(a["p"]), ptr(a["mg"]), a["bits"], ptr(a["g"]), a["flags"], a["stride"], a["view_of"], a["n_views"],
                                      a["veh"], a["n"], a["goals"], a["mask"], a["rec"])

    # the header's order.  (name, what breaks it)
    grids = [None] + [grid(res=r) for r in (0.0, -0.5, nan)] + [grid(dims=dm) for dm in ((0, 8, 4), (8, 0, 4), (8, 8, -1))]
    many = [grid(dims=dm) for dm in ((1 << 16, 1 << 15, 1), (1 << 16, 1 << 16, 1 << 16), (2, 1 << 30, 1))]
    clauses = [
        ("par", [dict(p=None)]),
        ("r_max", [dict(r_max=v) for v in (nan, inf, -inf, 0.0, -0.0, -1.0)]),
        ("r_avoid", [dict(r_avoid=v) for v in (nan, inf, -inf, -1e-300, -1.0)]),
        ("z", [dict(z_lo=lo, z_hi=hi) for lo, hi in ((nan, 1.0), (0.0, nan), (nan, nan), (1.0, 0.5), (inf, -inf))]),
        ("want", [dict(want=v) for v in (0, 8, 9, 16, -1, 1 << 30)]),
        ("max_hops", [dict(max_hops=v) for v in (-1, -(1 << 31))]),
        ("gain_radius", [dict(gain_radius=v) for v in (-1, 32, 1 << 30, -(1 << 31))]),
        ("hop_cost", [dict(hop_cost=v) for v in (-1, 16385, (1 << 31) - 1, -(1 << 31))]),
        ("min_gain", [dict(min_gain=v) for v in (-1, -(1 << 31))]),
        ("map_grid", [dict(mg=v) for v in grids]),
        ("map cells", [dict(mg=v) for v in many]),
        ("d_map_bits", [dict(bits=None)]),
        ("grid", [dict(g=v) for v in grids]),
        ("cells", [dict(g=v, stride=1 << 62) for v in many]),
        ("view_stride", [dict(stride=v) for v in (255, 0)]),
        ("n_views", [dict(n_views=v) for v in (0, -3)]),
        ("n", [dict(n=v) for v in (-1, -(1 << 31))]),
    ]
    fields = ("r_max", "r_avoid", "z_lo", "z_hi", "want", "max_hops", "gain_radius", "hop_cost", "min_gain")
    # what breaks each clause together with every later one: the value of the argument, or of the field of par
    worst = dict(r_max=nan, r_avoid=-1.0, z_lo=nan, want=0, max_hops=-1, gain_radius=-1, hop_cost=-1, min_gain=-1, mg=None, bits=None, g=None, stride=0,
                 n_views=0, n=-1)
    order = ["r_max", "r_avoid", "z_lo", "want", "max_hops", "gain_radius", "hop_cost", "min_gain", "mg", "mg", "bits", "g", "g", "stride", "n_views", "n"]
    assert len(order) == len(clauses) - 1
    nothing = dict(flags=None, veh=None, goals=None, mask=None, rec=None)

    def build(kw, extra):
        """The call's arguments from a mix of arguments and fields of par."""
        kw = dict(kw, **extra)
        if "p" in kw:
            return kw
        f = {k: kw.pop(k) for k in list(kw) if k in fields}
        if f:
            kw["p"] = par(**f)
        return kw

    for k, (name, breaks) in enumerate(clauses):
        after = {key: worst[key] for key in order[k:]}   # (clause k + 1 is about order[k]; without par its fields are not read)
        for kw in breaks:
            assert call(**build(kw, {})) == ARG, (name, kw)                                                    # the clause alone
            later = {key: v for key, v in after.items() if key not in kw}
            assert call(**build(kw, dict(later, **nothing))) == ARG, (name, kw)                                # and with everything after it broken too
            if "n" not in kw:
                assert call(**build(kw, dict(nothing, n=0))) == ARG, (name, kw)                                # n == 0 does not turn it into FH_OK
    # the order itself: with clause k and everything BEFORE it fine and everything after it broken the answer is still ARG (above); a
    # clause is not skipped either: each one alone, with everything else fine, says ARG, and with all of them fine the call goes on
    assert call(n=0, **nothing) == OK and call(n=0) == OK
    for key in nothing:
        assert call(**{key: None}) == ARG, key
    assert call(view_of=d + 40000) == DEVICE    # may be given, may be NULL
    # the edges of the rules that pass: n == 0, so nothing is launched
    for p in (par(gain_radius=0), par(gain_radius=31), par(hop_cost=0), par(hop_cost=16384), par(min_gain=0), par(min_gain=(1 << 31) - 1),
              par(max_hops=(1 << 31) - 1), par(z_lo=inf, z_hi=inf), par(r_max=1e-300), par(r_avoid=0.0)):
        assert call(p=p, n=0) == OK
    # host memory is no place for the records: the device that owns them is asked for before anything is launched
    assert call() == DEVICE
    assert L.fh_abi_version() == 9


def test_the_two_entry_points_before_it_answer_what_they_answered(built):
    """Their clauses are now two functions called in a row: the order of fh_reach_goals_device across the seam (max_hops, then
    map_grid), with a params record that fh_gain_goals_device would refuse."""
    from faster_amd import capi

    L = capi.lib()
    buf = np.zeros(1 << 16, dtype=np.uint8)
    d = buf.ctypes.data
    g = np.zeros(1, dtype=abi.voxel_grid_dtype)
    g["origin"], g["res"], g["dims"] = (0.1, 0.2, 0.3), 0.5, (8, 8, 4)
    p = np.ascontiguousarray(abi.default_reach_params(1.5)).reshape(1).copy()
    p["reserved"] = -1   # (where gain_radius, hop_cost and min_gain are: fh_reach_params does not read them)
    args = lambda par, mg, n: (None, abi.ptr(par), None if mg is None else abi.ptr(mg), d + 20480, abi.ptr(g), d, 256, None, 2, d + 1024, n,   # noqa: E731
                               d + 4096, d + 8192, d + 12288)
    assert L.fh_reach_goals_device(*args(p, g, 0)) == OK and L.fh_reach_goals_device(*args(p, g, 1)) == DEVICE
    assert L.fh_reach_goals_device(*args(p, None, 0)) == ARG
    bad = p.copy()
    bad["max_hops"] = -1
    assert L.fh_reach_goals_device(*args(bad, g, 0)) == ARG and L.fh_reach_goals_device(*args(bad, None, 0)) == ARG


def test_fleet_explore_gain_raises_what_explore_reachable_raises_before_any_launch():
    from faster_amd import capi
    from faster_amd.fleet import Fleet

    f = Fleet.__new__(Fleet)   # (no device here: only the checks that come before the first launch are reached)
    f.cloud = f.map_args = f.view_flags = f.flags = f.view_of = f.d_headings = f.grid = None
    f.d_reach_goals = f.d_reach_mask = f.d_reach_records = f.d_reach_view_of = None
    f.d_gain_goals = f.d_gain_mask = f.d_gain_records = None
    f.map = f.ctx = None

    def both(match, *args, **kw):
        said = []
        for method, name, more in ((f.explore_reachable, "Fleet.explore_reachable:", ()), (f.explore_gain, "Fleet.explore_gain:", (5,)),
                                   (f.explore_gain_stages, "Fleet.explore_gain:", (5,))):
            with pytest.raises(capi.FasterHipError, match=match) as e:
                method(args[0], *more, *args[1:], **kw)
            assert str(e.value).startswith(name), str(e.value)
            said.append(str(e.value).replace(name, ""))
        assert said[0] == said[1] == said[2]   # the same words, but for the name

    both("set_map", 2.0)
    f.cloud, f.map_args = object(), ((10, 10, 4), 0.2, (0.0, 0.0, 1.0), 2.0, 0.0)
    both("set_unknown_views", 2.0, want="all")
    with pytest.raises(capi.FasterHipError, match="explore_gain first"):
        f.gain_records()

    class Flags:   # stands in for the tensor of the views
        shape = (3, 100)

    f.view_flags, f.n_views, f.n = Flags(), 3, 3
    f.grid = ((0.0, 0.0, 0.0), 0.5, (5, 5, 4))
    both("enable_heading", 2.0)
    both("enable_heading", 2.0, want=("no_path", "reached"))
    for bad in ("arrived", (), ("all", "none")):
        both("want", 2.0, want=bad)
    assert "at most 31" in Fleet.explore_gain.__doc__ and "rounded down" in Fleet.explore_gain.__doc__
