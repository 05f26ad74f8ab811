"""CPU-side checks of include/fasterhip_sight.h: its entry point is declared there and in no other header, the header compiles alone as
C99 and C++11 and includes the three headers it may, the struct layouts and constants equal faster_amd/abi.py and, compiled together
with the header of the gain chooser, that header's, FH_ABI_VERSION stays, the symbol is exported and bound in a list of its own, the
device code lives in fh_sight.hip.hpp which fh_reach.hip alone includes, after fh_team.hip.hpp, with one kernel, no atomics and the
gain chooser's helpers called and not defined, every clause of the prologue answers FH_ERR_ARG in the gain chooser's order (all of
them come before the first call of the runtime, so host pointers stand in for device pointers), and Fleet.explore_sight raises
explore_reachable()'s errors before any launch."""
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
NEW_HDR = os.path.join(INC, "fasterhip_sight.h")
NEW = ["fh_sight_goals_device"]
NAMES = r"fh_sight|fasterhip_sight|FH_SIGHT|sight_goals|sight_record|sight_params|explore_sight"
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
            assert not re.search(NAMES, open(other).read()), other            # no existing public header has a word about it
    for untouched in ("fh_map.hip", "fh_capi.hip", "fh_pool.hip", "fh_spread.hip.hpp", "fh_gain.hip.hpp", "fh_reach.hip.hpp", "fh_team.hip.hpp"):
        assert not re.search(NAMES, open(os.path.join(CSRC, untouched)).read()), untouched
    assert int(re.search(r"#define FH_ABI_VERSION (\d+)", open(HDR).read()).group(1)) == abi.FH_ABI_VERSION == 9
    text = open(NEW_HDR).read()
    assert sorted(re.findall(r'#include "([^"]+)"', text)) == ["fasterhip.h", "fasterhip_frontier.h", "fasterhip_reach.h"]   # these three only
    src = "#include \"fasterhip_sight.h\"\nint main(void) {\n" + "".join("  (void)%s;\n" % n for n in NEW) + "  return 0;\n}\n"
    for lang, std, comp in (("c", "-std=c99", "gcc"), ("c++", "-std=c++11", "g++")):
        f = tmp_path / ("probe." + ("c" if lang == "c" else "cpp"))
        f.write_text(src)
        r = subprocess.run([comp, "-fsyntax-only", "-x", lang, std, "-Wall", "-pedantic", "-I", INC, str(f)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr.strip(), (lang, r.stderr[-2000:])
    for limit in ("diagonally", "inflated", "stop at the box", "no field of view", "team"):    # the known limits are stated
        assert limit in text, limit


def test_struct_layouts_and_constants_of_the_header_equal_abi_py_and_the_gain_choosers(tmp_path):
    """sizeof and every offsetof of the two structs and every constant, printed by a C program compiled against the header together
    with the header of the gain chooser."""
    structs = (("fh_sight_params", abi.sight_params_dtype, 64), ("fh_sight_record", abi.sight_record_dtype, 64),
               ("fh_gain_params", abi.gain_params_dtype, 64), ("fh_gain_record", abi.gain_record_dtype, 64))
    consts = ["FH_SIGHT_MAX_RADIUS", "FH_SIGHT_MAX_HOP_COST", "FH_SIGHT_ALL_POOR"]
    theirs = ["FH_GAIN_MAX_RADIUS", "FH_GAIN_MAX_HOP_COST", "FH_GAIN_ALL_POOR"]
    kept = ["FH_FRONTIER_WANTED", "FH_FRONTIER_FOUND", "FH_FRONTIER_NO_VIEW", "FH_FRONTIER_BAD_POS", "FH_REACH_START_OUTSIDE", "FH_REACH_BOX_TOO_LARGE",
            "FH_REACH_CUT"]
    lines = []
    for name, dt, _ in structs:
        lines.append('  printf("%s.size %%d\\n", (int)sizeof(%s));' % (name, name))
        lines += ['  printf("%s.%s %%d\\n", (int)offsetof(%s, %s));' % (name, k, name, k) for k in dt.names]
    lines += ['  printf("%s %%d\\n", (int)%s);' % (k, k) for k in consts + theirs + kept]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"fasterhip_gain.h\"\n#include \"fasterhip_sight.h\"\nint main(void) {\n"
                   + "\n".join(lines) + "\n  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", INC, str(src), "-o", str(exe)])
    got = dict((k, int(v)) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()))
    for name, dt, size in structs:
        assert got[name + ".size"] == dt.itemsize == size, name
        for k in dt.names:
            assert got[name + "." + k] == dt.fields[k][1], (name, k)
    for k in consts + theirs + kept:
        assert got[k] == getattr(abi, k), k
    assert [got[k] for k in consts] == [31, 16384, 128] == [got[k] for k in theirs]
    assert not got["FH_SIGHT_ALL_POOR"] & sum(got[k] for k in kept)
    # the params: the gain chooser's, field by field; the record: its first 56 bytes, then ball_gain and walls
    assert abi.sight_params_dtype.names == abi.gain_params_dtype.names
    for k in abi.gain_params_dtype.names:
        assert abi.sight_params_dtype.fields[k] == abi.gain_params_dtype.fields[k] and got["fh_sight_params." + k] == got["fh_gain_params." + k], k
    assert abi.sight_record_dtype.names[:13] == abi.gain_record_dtype.names[:13] and abi.gain_record_dtype.names[13:] == ("reserved",)
    for k in abi.gain_record_dtype.names[:13]:
        assert abi.sight_record_dtype.fields[k] == abi.gain_record_dtype.fields[k] and got["fh_sight_record." + k] == got["fh_gain_record." + k], k
    assert (got["fh_gain_record.best_gain"], got["fh_gain_record.reserved"], got["fh_sight_record.ball_gain"], got["fh_sight_record.walls"]) == (52, 56, 56, 60)
    assert abi.sight_record_dtype.names[13:] == ("ball_gain", "walls")
    p = abi.default_sight_params(2.5, 7)
    assert (float(p["r_max"]), float(p["r_avoid"]), float(p["z_lo"]), float(p["z_hi"]), int(p["want"]), int(p["max_hops"]), int(p["gain_radius"]),
            int(p["hop_cost"]), int(p["min_gain"])) == (2.5, 0.0, -np.inf, np.inf, abi.FH_FRONTIER_WANT_REACHED, 0, 7, 1, 0) and not p["reserved"].any()
    assert p.tobytes() == abi.default_gain_params(2.5, 7).tobytes()


def test_the_symbol_is_exported_and_bound_and_the_device_code_is_included_by_fh_reach_hip_alone(built):
    from faster_amd import capi
    from faster_amd.fleet import Fleet

    L = ctypes.CDLL(built.SO)
    for name in NEW:
        assert hasattr(L, name), name
    assert capi.SIGHT_SYMBOLS == NEW
    lists = [k for k in dir(capi) if k.endswith("SYMBOLS") and k != "SIGHT_SYMBOLS"]
    assert len(lists) >= 16 and "SYMBOLS" in lists and "GAIN_SYMBOLS" in lists and "TEAM_SYMBOLS" in lists
    for k in lists:
        assert not set(NEW) & set(getattr(capi, k)), k
    assert len(capi.lib().fh_sight_goals_device.argtypes) == 14 == len(capi.lib().fh_gain_goals_device.argtypes)
    assert hasattr(capi.Map, "sight_goals_device")
    for name in ("explore_sight", "explore_sight_stages", "sight_records"):
        assert hasattr(Fleet, name), name
    assert NEW_HDR in built.DEPS and os.path.join(CSRC, "fh_sight.hip.hpp") in built.DEPS
    assert built.SOURCES[-1] == os.path.join(CSRC, "fh_reach.hip") and len(built.SOURCES) == 4
    assert "capi.SIGHT_SYMBOLS" in open(os.path.join(ROOT, "__graft_entry__.py")).read()   # build() touches the new symbol
    assert capi.lib().fh_abi_version() == 9
    strip = lambda path: re.sub(r"//[^\n]*", "", open(path).read())   # noqa: E731
    for other in glob.glob(os.path.join(CSRC, "*")):
        if os.path.basename(other) != "fh_reach.hip":
            assert "fh_sight.hip.hpp" not in strip(other), other
    host = strip(os.path.join(CSRC, "fh_reach.hip"))
    includes = re.findall(r'#include "([^"]+)"', host)
    assert includes.index("fh_sight.hip.hpp") == includes.index("fh_team.hip.hpp") + 1 == includes.index("fh_gain.hip.hpp") + 2
    body = strip(os.path.join(CSRC, "fh_sight.hip.hpp"))
    assert sorted(set(re.findall(r"\b(\w+_kernel)\s*\(", body))) == ["sight_goals_kernel"]
    assert "#pragma clang fp contract(off)" in body and "atomic" not in body.lower()
    assert body.count("#pragma clang fp contract(off)") == strip(os.path.join(CSRC, "fh_gain.hip.hpp")).count("#pragma clang fp contract(off)")
    assert body.count("__syncthreads()") == strip(os.path.join(CSRC, "fh_gain.hip.hpp")).count("__syncthreads()")        # the barriers stay
    for called in ("gain_ball(", "gain_take(", "GainBest", "gain_key_hops(", "gain_key_utility(", "gain_before("):   # called, not copied
        assert called in body, called
    assert not re.search(r"__device__[^\n;{]*\b(gain_ball|gain_take|gain_key|gain_key_hops|gain_key_utility|gain_before)\s*\(", body)
    assert re.search(r"__device__[^\n;{]*\bsight_gain\s*\(", body)             # the per-candidate evaluation is a function of its own
    entry = host[host.index("int fh_sight_goals_device"):host.index("int fh_team_goals_device")]
    assert re.findall(r"hipLaunchKernelGGL\(fhp::(\w+)", entry) == ["sight_goals_kernel"]
    for tie in ("FH_SIGHT_MAX_RADIUS == FH_GAIN_MAX_RADIUS", "FH_SIGHT_MAX_HOP_COST == FH_GAIN_MAX_HOP_COST", "FH_SIGHT_ALL_POOR == FH_GAIN_ALL_POOR"):
        assert tie in host, tie
    with pytest.raises(capi.FasterHipError):
        capi.Map.sight_goals_device(None, abi.default_reach_params(1.0), None, None, 0, None, 1, None, 0, None, None, None, None)   # not a sight record


def test_every_argument_rule_in_the_order_of_the_gain_chooser(built):
    """Case k breaks clause k and every clause after it, and keeps every clause before it: FH_ERR_ARG.  Nothing but the last clauses
    passing gives anything else: FH_OK for n == 0 without any pointer, and with host memory for d_records the runtime is asked whose
    it is and the answer is FH_ERR_DEVICE, with or without a device.  Every call is made to the gain chooser's entry point too: the
    two answer alike."""
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
        p = np.ascontiguousarray(abi.default_sight_params(1.5, 3)).reshape(1).copy()
        for k, v in kw.items():
            p[k] = v
        return p

    good = dict(p=par(), mg=grid(res=0.3, dims=(9, 9, 5)), bits=d + 20480, g=grid(), flags=d, stride=256, view_of=None, n_views=2, veh=d + 1024, n=1,
                goals=d + 4096, mask=d + 8192, rec=d + 12288)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        ptr = lambda x: None if x is None else abi.ptr(x)   # noqa: E731
        args = (None, ptr(a["p"]), ptr(a["mg"]), a["bits"], ptr(a["g"]), a["flags"], a["stride"], a["view_of"], a["n_views"], a["veh"], a["n"],
                a["goals"], a["mask"], a["rec"])
        rc = L.fh_sight_goals_device(*args)
        assert rc == L.fh_gain_goals_device(*args), kw
        return rc

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
    worst = dict(r_max=nan, r_avoid=-1.0, z_lo=nan, want=0, max_hops=-1, gain_radius=-1, hop_cost=-1, min_gain=-1, mg=None, bits=None, g=None, stride=0,
                 n_views=0, n=-1)
    order = ["r_max", "r_avoid", "z_lo", "want", "max_hops", "gain_radius", "hop_cost", "min_gain", "mg", "mg", "bits", "g", "g", "stride", "n_views", "n"]
    assert len(order) == len(clauses) - 1
    nothing = dict(flags=None, veh=None, goals=None, mask=None, rec=None)

    def build(kw, extra):
        kw = dict(kw, **extra)
        if "p" in kw:
            return kw
        f = {k: kw.pop(k) for k in list(kw) if k in fields}
        if f:
            kw["p"] = par(**f)
        return kw

    for k, (name, breaks) in enumerate(clauses):
        after = {key: worst[key] for key in order[k:]}
        for kw in breaks:
            assert call(**build(kw, {})) == ARG, (name, kw)
            later = {key: v for key, v in after.items() if key not in kw}
            assert call(**build(kw, dict(later, **nothing))) == ARG, (name, kw)
            if "n" not in kw:
                assert call(**build(kw, dict(nothing, n=0))) == ARG, (name, kw)
    assert call(n=0, **nothing) == OK and call(n=0) == OK
    for key in nothing:
        assert call(**{key: None}) == ARG, key
    assert call(view_of=d + 40000) == DEVICE    # may be given, may be NULL
    for p in (par(gain_radius=0), par(gain_radius=31), par(hop_cost=0), par(hop_cost=16384), par(min_gain=0), par(min_gain=(1 << 31) - 1),
              par(max_hops=(1 << 31) - 1), par(z_lo=inf, z_hi=inf), par(r_max=1e-300), par(r_avoid=0.0), par(reserved=-7)):
        assert call(p=p, n=0) == OK
    assert call() == DEVICE
    assert L.fh_abi_version() == 9


def test_fleet_explore_sight_raises_what_explore_reachable_raises_before_any_launch():
    from faster_amd import capi
    from faster_amd.fleet import Fleet

    f = Fleet.__new__(Fleet)   # (no device here: only the checks that come before the first launch are reached)
    f.cloud = f.map_args = f.view_flags = f.flags = f.view_of = f.d_headings = f.grid = None
    f.d_reach_goals = f.d_reach_mask = f.d_reach_records = f.d_reach_view_of = None
    f.d_sight_goals = f.d_sight_mask = f.d_sight_records = None
    f.map = f.ctx = None

    def both(match, *args, **kw):
        said = []
        for method, name, more in ((f.explore_reachable, "Fleet.explore_reachable:", ()), (f.explore_sight, "Fleet.explore_sight:", (5,)),
                                   (f.explore_sight_stages, "Fleet.explore_sight:", (5,))):
            with pytest.raises(capi.FasterHipError, match=match) as e:
                method(args[0], *more, *args[1:], **kw)
            assert str(e.value).startswith(name), str(e.value)
            said.append(str(e.value).replace(name, ""))
        assert said[0] == said[1] == said[2]   # the same words, but for the name

    both("set_map", 2.0)
    f.cloud, f.map_args = object(), ((10, 10, 4), 0.2, (0.0, 0.0, 1.0), 2.0, 0.0)
    both("set_unknown_views", 2.0, want="all")
    with pytest.raises(capi.FasterHipError, match="explore_sight first"):
        f.sight_records()

    class Flags:   # stands in for the tensor of the views
        shape = (3, 100)

    f.view_flags, f.n_views, f.n = Flags(), 3, 3
    f.grid = ((0.0, 0.0, 0.0), 0.5, (5, 5, 4))
    both("enable_heading", 2.0)
    for bad in ("arrived", (), ("all", "none")):
        both("want", 2.0, want=bad)
    assert "at most 31" in Fleet.explore_sight.__doc__ and "rounded down" in Fleet.explore_sight.__doc__
