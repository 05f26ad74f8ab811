"""CPU-side checks of fh_reach_goals_device: declared in include/fasterhip_reach.h and in no other header, the header compiles alone
as C99 and C++11, exported, bound in faster_amd/capi.py on Map and on Fleet, the struct layouts and the constants of the header equal
faster_amd/abi.py, FH_ABI_VERSION stays, the code lives in a translation unit of its own of which fh_map.hip, fh_capi.hip, fasterhip.h
and fasterhip_frontier.h know nothing, every clause of the prologue answers FH_ERR_ARG in the stated order (all of them come before
the first call of the runtime, so host pointers stand in for device pointers), and Fleet.explore_reachable raises explore()'s errors
before any launch."""
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
NEW_HDR = os.path.join(INC, "fasterhip_reach.h")
NEW = ["fh_reach_goals_device"]
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
    for untouched in (HDR, os.path.join(INC, "fasterhip_frontier.h"), os.path.join(CSRC, "fh_map.hip"), os.path.join(CSRC, "fh_capi.hip")):
        # (the word itself is everywhere in them: FH_VEHICLE_GOAL_REACHED, "as far as the sensor reaches"; the names of this feature are not)
        assert not re.search(r"fh_reach|fasterhip_reach|reach_goals|reach_record|reach_params|explore_reachable", open(untouched).read(), flags=re.I), untouched
    assert int(re.search(r"#define FH_ABI_VERSION (\d+)", open(HDR).read()).group(1)) == abi.FH_ABI_VERSION == 9
    text = open(NEW_HDR).read()
    assert '#include "fasterhip.h"' in text and '#include "fasterhip_frontier.h"' in text
    src = "#include \"fasterhip_reach.h\"\nint main(void) {\n" + "".join("  (void)%s;\n" % n for n in NEW) + "  return 0;\n}\n"
    for lang, std, comp in (("c", "-std=c99", "gcc"), ("c++", "-std=c++11", "g++")):
        f = tmp_path / ("probe." + ("c" if lang == "c" else "cpp"))
        f.write_text(src)
        r = subprocess.run([comp, "-fsyntax-only", "-x", lang, std, "-Wall", "-pedantic", "-I", INC, str(f)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr.strip(), (lang, r.stderr[-2000:])


def test_struct_layouts_and_constants_of_the_header_equal_abi_py(tmp_path):
    """sizeof and every offsetof of the two structs, printed by a C program compiled against the header."""
    structs = (("fh_reach_params", abi.reach_params_dtype, 64), ("fh_reach_record", abi.reach_record_dtype, 48))
    consts = ["FH_REACH_START_OUTSIDE", "FH_REACH_BOX_TOO_LARGE", "FH_REACH_CUT", "FH_REACH_MAX_WORDS"]
    lines = []
    for name, dt, _ in structs:
        lines.append('  printf("%s.size %%d\\n", (int)sizeof(%s));' % (name, name))
        lines += ['  printf("%s.%s %%d\\n", (int)offsetof(%s, %s));' % (name, k, name, k) for k in dt.names]
    lines += ['  printf("%s %%d\\n", (int)%s);' % (k, k) for k in consts]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"fasterhip_reach.h\"\nint main(void) {\n" + "\n".join(lines)
                   + "\n  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", INC, str(src), "-o", str(exe)])
    got = dict((k, int(v)) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()))
    for name, dt, size in structs:
        assert got[name + ".size"] == dt.itemsize == size, name
        for k in dt.names:
            assert got[name + "." + k] == dt.fields[k][1], (name, k)
    for k in consts:
        assert got[k] == getattr(abi, k), k
    assert [getattr(abi, k) for k in consts] == [16, 32, 64, 1024]
    # fh_reach_params is fh_frontier_params with max_hops in its first reserved word
    for k in ("r_max", "r_avoid", "z_lo", "z_hi", "want"):
        assert abi.reach_params_dtype.fields[k][1] == abi.frontier_params_dtype.fields[k][1], k
    assert abi.reach_params_dtype.fields["max_hops"][1] == abi.frontier_params_dtype.fields["reserved"][1]
    p = abi.default_reach_params(2.5)
    assert (float(p["r_max"]), float(p["r_avoid"]), float(p["z_lo"]), float(p["z_hi"]), int(p["want"]), int(p["max_hops"])) == \
        (2.5, 0.0, -np.inf, np.inf, abi.FH_FRONTIER_WANT_REACHED, 0) and not p["reserved"].any()


def test_the_symbol_is_exported_and_bound_and_the_code_has_a_translation_unit_of_its_own(built):
    from faster_amd import capi
    from faster_amd.fleet import Fleet

    L = ctypes.CDLL(built.SO)
    for name in NEW:
        assert hasattr(L, name), name
    assert capi.REACH_SYMBOLS == NEW
    lists = [k for k in dir(capi) if k.endswith("SYMBOLS") and k != "REACH_SYMBOLS"]
    assert len(lists) >= 12 and "SYMBOLS" in lists and "FRONTIER_SYMBOLS" in lists
    for k in lists:
        assert not set(NEW) & set(getattr(capi, k)), k
    assert capi.lib().fh_reach_goals_device.argtypes is not None and len(capi.lib().fh_reach_goals_device.argtypes) == 14
    assert hasattr(capi.Map, "reach_goals_device")
    for name in ("explore_reachable", "explore_reachable_stages", "reach_records"):
        assert hasattr(Fleet, name), name
    assert NEW_HDR in built.DEPS and os.path.join(CSRC, "fh_reach.hip.hpp") in built.DEPS
    assert built.SOURCES[-1] == os.path.join(CSRC, "fh_reach.hip") and len(built.SOURCES) == 4
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "capi.REACH_SYMBOLS" in entry   # build() touches the new symbol
    assert capi.lib().fh_abi_version() == 9
    # the kernel's header is included by fh_reach.hip only, and holds one kernel, under fp contract(off)
    for other in glob.glob(os.path.join(CSRC, "*")):
        if os.path.basename(other) != "fh_reach.hip":
            assert "fh_reach.hip.hpp" not in re.sub(r"//[^\n]*", "", open(other).read()), other
    body = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "fh_reach.hip.hpp")).read())
    assert sorted(set(re.findall(r"\b(\w+_kernel)\s*\(", body))) == ["reach_goals_kernel"]
    assert "#pragma clang fp contract(off)" in body
    with pytest.raises(capi.FasterHipError):
        capi.Map.reach_goals_device(None, abi.default_frontier_params(1.0), None, None, 0, None, 1, None, 0, None, None, None, None)   # not a reach record


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
        p = np.ascontiguousarray(abi.default_reach_params(1.5)).reshape(1).copy()
        for k, v in kw.items():
            p[k] = v
        return p

    good = dict(p=par(), mg=grid(res=0.3, dims=(9, 9, 5)), bits=d + 20480, g=grid(), flags=d, stride=256, view_of=None, n_views=2, veh=d + 1024, n=1,
                goals=d + 4096, mask=d + 8192, rec=d + 12288)
    # clause by clause, in the header's order: (name, the argument it is about, values that break it)
    clauses = [
        ("par", "p", [None]),
        ("r_max", "p", [par(r_max=v) for v in (nan, inf, -inf, 0.0, -0.0, -1.0)]),
        ("r_avoid", "p", [par(r_avoid=v) for v in (nan, inf, -inf, -1e-300, -1.0)]),
        ("z", "p", [par(z_lo=lo, z_hi=hi) for lo, hi in ((nan, 1.0), (0.0, nan), (nan, nan), (1.0, 0.5), (inf, -inf))]),
        ("want", "p", [par(want=v) for v in (0, 8, 9, 16, -1, 1 << 30)]),
        ("max_hops", "p", [par(max_hops=v) for v in (-1, -(1 << 31))]),
        ("map_grid", "mg", [None] + [grid(res=r) for r in (0.0, -0.5, nan)] + [grid(dims=dm) for dm in ((0, 8, 4), (8, 0, 4), (8, 8, -1))]),
        ("map cells", "mg", [grid(dims=dm) for dm in ((1 << 16, 1 << 15, 1), (1 << 16, 1 << 16, 1 << 16), (2, 1 << 30, 1),
                                                      ((1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1))]),
        ("d_map_bits", "bits", [None]),
        ("grid", "g", [None] + [grid(res=r) for r in (0.0, -0.5, nan)] + [grid(dims=dm) for dm in ((0, 8, 4), (8, 0, 4), (8, 8, -1))]),
        ("cells", "g", [grid(dims=dm) for dm in ((1 << 16, 1 << 15, 1), (1 << 16, 1 << 16, 1 << 16), (2, 1 << 30, 1))]),
        ("view_stride", "stride", [255, 0]),
        ("n_views", "n_views", [0, -3]),
        ("n", "n", [-1, -(1 << 31)]),
    ]
    # what breaks a clause together with every clause after it (the params record carries five clauses: the later fields broken too)
    broken_after = {"p": None, "mg": None, "bits": None, "g": None, "stride": 0, "n_views": 0, "n": -1}
    later_fields = {"r_max": dict(r_avoid=-1.0, z_lo=nan, want=0, max_hops=-1), "r_avoid": dict(z_lo=nan, want=0, max_hops=-1),
                    "z": dict(want=0, max_hops=-1), "want": dict(max_hops=-1), "max_hops": {}}
    nothing = dict(flags=None, veh=None, goals=None, mask=None, rec=None)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        ptr = lambda x: None if x is None else abi.ptr(x)   # noqa: E731
        return L.fh_reach_goals_device(None, ptr(a["p"]), ptr(a["mg"]), a["bits"], ptr(a["g"]), a["flags"], a["stride"], a["view_of"], a["n_views"],
                                       a["veh"], a["n"], a["goals"], a["mask"], a["rec"])

    order = ["p", "mg", "bits", "g", "stride", "n_views", "n"]
    for name, key, values in clauses:
        after = {k: broken_after[k] for k in order[order.index(key) + 1:]}
        for v in values:
            if key == "p" and v is not None:
                v = v.copy()
                for f, x in later_fields[name].items():
                    v[f] = x
            if key == "g" and name == "grid":
                after["stride"] = 0
            if name == "cells":
                after["stride"] = 0   # (smaller than any number of cells)
            alone = dict(stride=1 << 62) if name == "cells" else {}
            assert call(**{key: v}, **alone) == ARG, (name, v)             # the clause alone
            assert call(**{key: v}, **after, **nothing) == ARG, (name, v)   # and with everything after it broken as well
            if key != "n":
                assert call(**{key: v}, n=0, **nothing) == ARG, (name, v)   # n == 0 does not turn it into FH_OK
    # every rule passes: n == 0 is fine without any pointer, then the pointers
    assert call(n=0, **nothing) == OK and call(n=0) == OK
    for k in nothing:
        assert call(**{k: None}) == ARG, k
    # the edges of the rules that pass: n == 0, so nothing is launched
    for p in (par(r_max=1e-300), par(r_max=1e300), par(r_avoid=0.0), par(z_lo=-inf, z_hi=inf), par(z_lo=1.0, z_hi=1.0), par(z_lo=inf, z_hi=inf),
              par(max_hops=0), par(max_hops=(1 << 31) - 1)):
        assert call(p=p, n=0) == OK
    for v in (1, 2, 3, 4, 5, 6, 7):
        assert call(p=par(want=v), n=0) == OK, v
    assert call(stride=256, n=0) == OK and call(g=grid(dims=(1, 1, 1)), stride=1, n=0) == OK
    assert call(mg=grid(dims=(1, 1, 1)), n=0) == OK and call(mg=grid(dims=(1 << 15, 1 << 15, 1)), n=0) == OK
    # host memory is no place for the records: the device that owns them is asked for before anything is launched
    assert call() == DEVICE
    assert L.fh_abi_version() == 9


def test_fleet_explore_reachable_raises_what_explore_raises_before_any_launch():
    from faster_amd import capi
    from faster_amd.fleet import Fleet

    f = Fleet.__new__(Fleet)   # (no device here: only the checks that come before the first launch are reached)
    f.cloud = f.map_args = f.view_flags = f.flags = f.view_of = f.d_headings = f.grid = None
    f.d_explore_goals = f.d_explore_view_of = f.d_coverage = None
    f.d_reach_goals = f.d_reach_mask = f.d_reach_records = f.d_reach_view_of = None
    f.map = f.ctx = None

    def both(match, *args, **kw):
        for method, name in ((f.explore, "Fleet.explore:"), (f.explore_reachable, "Fleet.explore_reachable:")):
            with pytest.raises(capi.FasterHipError, match=match) as e:
                method(*args, **kw)
            assert str(e.value).startswith(name), str(e.value)
        return str(e.value)

    both("set_map", 2.0)
    f.cloud, f.map_args = object(), ((10, 10, 4), 0.2, (0.0, 0.0, 1.0), 2.0, 0.0)
    both("set_unknown_views", 2.0, want="all")
    with pytest.raises(capi.FasterHipError, match="explore_reachable first"):
        f.reach_records()

    class Flags:   # stands in for the tensor of the views
        shape = (3, 100)

    f.view_flags, f.n_views, f.n = Flags(), 3, 3
    f.grid = ((0.0, 0.0, 0.0), 0.5, (5, 5, 4))
    both("enable_heading", 2.0)
    both("enable_heading", 2.0, want=("no_path", "reached"))
    for bad in ("arrived", (), ("all", "none")):
        both("want", 2.0, want=bad)
    # the same words, but for the name
    with pytest.raises(capi.FasterHipError) as a:
        f.explore(2.0, want="arrived")
    with pytest.raises(capi.FasterHipError) as b:
        f.explore_reachable(2.0, want="arrived")
    assert str(b.value) == str(a.value).replace("Fleet.explore:", "Fleet.explore_reachable:")
