"""CPU-side checks of include/fasterhip_bid.h: its two entry points are declared there and in no other header, the header compiles alone
as C99 and C++11 and names no header of another chooser, the struct layouts and constants equal faster_amd/abi.py and, offset by offset,
those of the chooser it stands beside, FH_ABI_VERSION stays, the symbols are exported and bound in a list of their own, the device code
lives in fh_bid.hip.hpp which fh_reach.hip alone includes, after fh_sight.hip.hpp, with exactly three kernels that call K17's helpers,
the entry points stand before fh_sight_goals_device, every clause of the prologue answers FH_ERR_ARG in the stated order (all of them
come before the first call of the runtime, so host pointers stand in for device pointers), and Fleet.explore_bid raises explore_team()'s
errors before any launch."""
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
NEW_HDR = os.path.join(INC, "fasterhip_bid.h")
NEW = ["fh_bid_work_bytes", "fh_bid_goals_device"]
NAMES = r"fh_bid|fasterhip_bid|FH_BID|bid_goals|bid_record|bid_params|explore_bid"
OK, ARG, DEVICE = 0, -1, -2


@pytest.fixture(scope="module")
def built():
    from faster_amd import build as fb

    fb.build_all()
    return fb


def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(fh_[a-z_0-9]+)\s*\(", text))


def test_the_entry_points_are_declared_in_their_own_header_which_compiles_alone(tmp_path):
    assert set(NEW) == _declared(NEW_HDR)
    for other in glob.glob(os.path.join(INC, "*.h")):
        if other != NEW_HDR:
            assert not set(NEW) & _declared(other), other
            assert not re.search(NAMES, open(other).read()), other            # no existing public header has a word about it
    for untouched in ("fh_map.hip", "fh_capi.hip", "fh_pool.hip", "fh_spread.hip.hpp", "fh_gain.hip.hpp", "fh_reach.hip.hpp", "fh_team.hip.hpp",
                      "fh_sight.hip.hpp"):
        assert not re.search(NAMES, open(os.path.join(CSRC, untouched)).read()), untouched
    assert int(re.search(r"#define FH_ABI_VERSION (\d+)", open(HDR).read()).group(1)) == abi.FH_ABI_VERSION == 9
    text = open(NEW_HDR).read()
    assert re.findall(r'#include "([^"]+)"', text) == ["fasterhip.h", "fasterhip_frontier.h", "fasterhip_reach.h"]
    # it names no header of another chooser, and none of their identifiers
    assert not re.search(r"fasterhip_(spread|gain|team|sight)|fh_(spread|gain|team|sight)|FH_(SPREAD|GAIN|TEAM|SIGHT)", text)
    assert "((n + 63) & ~63) + n * FH_BID_LIST * 4 + n * 8 + 2 * n * 4" in text   # the work-bytes formula, exactly
    src = "#include \"fasterhip_bid.h\"\nint main(void) {\n" + "".join("  (void)%s;\n" % n for n in NEW) + "  return 0;\n}\n"
    for lang, std, comp in (("c", "-std=c99", "gcc"), ("c++", "-std=c++11", "g++")):
        f = tmp_path / ("probe." + ("c" if lang == "c" else "cpp"))
        f.write_text(src)
        r = subprocess.run([comp, "-fsyntax-only", "-x", lang, std, "-Wall", "-pedantic", "-I", INC, str(f)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr.strip(), (lang, r.stderr[-2000:])


def test_struct_layouts_and_constants_against_the_chooser_it_stands_beside(tmp_path):
    """sizeof and every offsetof of the two structs and every constant, printed by a C program compiled against this header together
    with the headers of the other choosers for a team: the constants it carries under its own names have their values."""
    structs = (("fh_bid_params", abi.bid_params_dtype, 80), ("fh_bid_record", abi.bid_record_dtype, 96),
               ("fh_team_params", abi.team_params_dtype, 80), ("fh_team_record", abi.team_record_dtype, 96))
    consts = ["FH_BID_OVERFLOW", "FH_BID_UNSETTLED", "FH_BID_CLAIMED", "FH_BID_ALL_POOR", "FH_BID_MAX_PASSES", "FH_BID_DEFAULT_PASSES",
              "FH_BID_MAX_RADIUS", "FH_BID_MAX_HOP_COST", "FH_BID_LIST"]
    theirs = ["FH_TEAM_OVERFLOW", "FH_TEAM_UNSETTLED", "FH_TEAM_CLAIMED", "FH_TEAM_ALL_POOR", "FH_TEAM_MAX_PASSES", "FH_TEAM_DEFAULT_PASSES",
              "FH_TEAM_MAX_RADIUS", "FH_TEAM_MAX_HOP_COST", "FH_TEAM_LIST"]
    more = ["FH_SPREAD_OVERFLOW", "FH_SPREAD_UNSETTLED", "FH_SPREAD_CLAIMED", "FH_SPREAD_MAX_PASSES", "FH_SPREAD_DEFAULT_PASSES", "FH_GAIN_MAX_RADIUS",
            "FH_GAIN_MAX_HOP_COST", "FH_SIGHT_MAX_RADIUS", "FH_SIGHT_MAX_HOP_COST"]
    lines = []
    for name, dt, _ in structs:
        lines.append('  printf("%s.size %%d\\n", (int)sizeof(%s));' % (name, name))
        lines += ['  printf("%s.%s %%d\\n", (int)offsetof(%s, %s));' % (name, k, name, k) for k in dt.names]
    lines += ['  printf("%s %%d\\n", (int)%s);' % (k, k) for k in consts + theirs + more]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"fasterhip_spread.h\"\n#include \"fasterhip_gain.h\"\n#include \"fasterhip_team.h\"\n"
                   "#include \"fasterhip_sight.h\"\n#include \"fasterhip_bid.h\"\nint main(void) {\n" + "\n".join(lines) + "\n  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", INC, str(src), "-o", str(exe)])
    got = dict((k, int(v)) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()))
    for name, dt, size in structs:
        assert got[name + ".size"] == dt.itemsize == size, name
        for k in dt.names:
            assert got[name + "." + k] == dt.fields[k][1], (name, k)
    for k in consts + theirs + more:
        assert got[k] == getattr(abi, k), k
    assert [got[k] for k in consts] == [128, 256, 512, 1024, 64, 8, 31, 16384, 64]
    assert [got[k] for k in consts[:8]] == [got[k] for k in theirs[:8]] and got["FH_BID_LIST"] == 2 * got["FH_TEAM_LIST"]
    assert [got[k] for k in consts[:3] + consts[4:8]] == [got[k] for k in more[:7]] and [got[k] for k in consts[6:8]] == [got[k] for k in more[7:]]
    # the params: field by field; the record: word by word, `lower` read as `rivals` and `reserved0` as `searches`
    assert abi.bid_params_dtype.names == abi.team_params_dtype.names
    for k in abi.team_params_dtype.names:
        assert abi.bid_params_dtype.fields[k] == abi.team_params_dtype.fields[k], k
    renamed = {"lower": "rivals", "reserved0": "searches"}
    assert [renamed.get(k, k) for k in abi.team_record_dtype.names] == list(abi.bid_record_dtype.names)
    for k in abi.team_record_dtype.names:
        assert abi.bid_record_dtype.fields[renamed.get(k, k)] == abi.team_record_dtype.fields[k], k
    assert (abi.bid_record_dtype.fields["rivals"][1], abi.bid_record_dtype.fields["searches"][1]) == (48, 60)
    for args in ((2.5, 1.5, 7), (2.5, 1.5, 7, 3), (2.5, 1.5, 7, -1)):
        assert abi.default_bid_params(*args).tobytes() == abi.default_team_params(*args).tobytes()   # the same defaults
    p = abi.default_bid_params(2.5, 1.5, 7)
    assert (int(p["passes"]), int(p["hop_cost"]), int(p["min_gain"]), int(p["claim_radius"])) == (8, 1, 0, 7)


def test_the_symbols_are_exported_and_bound_and_the_device_code_is_included_by_fh_reach_hip_alone(built):
    from faster_amd import capi
    from faster_amd.fleet import Fleet

    L = ctypes.CDLL(built.SO)
    for name in NEW:
        assert hasattr(L, name), name
    assert capi.BID_SYMBOLS == NEW
    lists = [k for k in dir(capi) if k.endswith("SYMBOLS") and k != "BID_SYMBOLS"]
    assert len(lists) >= 17 and "SYMBOLS" in lists and "TEAM_SYMBOLS" in lists and "SIGHT_SYMBOLS" in lists
    for k in lists:
        assert not set(NEW) & set(getattr(capi, k)), k
    assert len(capi.lib().fh_bid_goals_device.argtypes) == 17 and capi.lib().fh_bid_goals_device.argtypes == capi.lib().fh_team_goals_device.argtypes
    assert capi.lib().fh_bid_work_bytes.restype == ctypes.c_size_t
    assert hasattr(capi.Map, "bid_goals_device")
    for name in ("explore_bid", "explore_bid_stages", "bid_records"):
        assert hasattr(Fleet, name), name
    assert NEW_HDR in built.DEPS and os.path.join(CSRC, "fh_bid.hip.hpp") in built.DEPS
    assert built.SOURCES[-1] == os.path.join(CSRC, "fh_reach.hip") and len(built.SOURCES) == 4
    assert "capi.BID_SYMBOLS" in open(os.path.join(ROOT, "__graft_entry__.py")).read()   # build() touches the new symbols
    assert capi.lib().fh_abi_version() == 9
    strip = lambda path: re.sub(r"//[^\n]*", "", open(path).read())   # noqa: E731
    for other in glob.glob(os.path.join(CSRC, "*")):
        if os.path.basename(other) != "fh_reach.hip":
            assert "fh_bid.hip.hpp" not in strip(other), other
    includes = re.findall(r'#include "([^"]+)"', strip(os.path.join(CSRC, "fh_reach.hip")))
    assert includes.index("fh_bid.hip.hpp") == includes.index("fh_sight.hip.hpp") + 1 == includes.index("fh_team.hip.hpp") + 2
    body = strip(os.path.join(CSRC, "fh_bid.hip.hpp"))
    assert sorted(set(re.findall(r"\b(\w+_kernel)\s*\(", body))) == ["bid_goals_kernel", "bid_peers_kernel", "bid_settle_kernel"]
    assert "#pragma clang fp contract(off)" in body and "atomic" not in body.lower()
    assert re.findall(r'#include "([^"]+)"', body) == ["../../include/fasterhip_bid.h", "fh_wave.hip.hpp"]
    for called in ("gain_ball(", "gain_take(", "GainBest", "gain_key_hops(", "gain_key_utility(", "gain_before("):   # called, not copied
        assert called in body, called
    assert not re.search(r"__device__[^\n;{]*\b(gain_ball|gain_take|gain_key|gain_key_hops|gain_key_utility|gain_before)\s*\(", body)
    # the entry points stand before fh_sight_goals_device; 2 + 2 passes launches: the class kernel as it is, the scan, and the two
    # kernels of a round in the loop over the rounds
    host = strip(os.path.join(CSRC, "fh_reach.hip"))
    at = [host.index("size_t fh_bid_work_bytes"), host.index("int fh_bid_goals_device"), host.index("int fh_sight_goals_device"),
          host.index("int fh_team_goals_device")]
    assert at == sorted(at) and host.index("int fh_gain_goals_device") < at[0]
    entry = host[at[1]:at[2]]
    assert re.findall(r"hipLaunchKernelGGL\(fhp::(\w+)", entry) == ["spread_class_kernel", "bid_peers_kernel", "bid_goals_kernel", "bid_settle_kernel"]
    loop = entry[entry.index("for (int p = 1; p <= par->passes; p++)"):]
    assert re.findall(r"hipLaunchKernelGGL\(fhp::(\w+)", loop) == ["bid_goals_kernel", "bid_settle_kernel"]
    assert entry.count("static_assert") >= 3 and "FH_TEAM_LIST" in entry and "offsetof(fh_team_record, lower)" in entry
    for n in (1, 2, 63, 64, 65, 1000):
        assert int(capi.lib().fh_bid_work_bytes(n)) == ((n + 63) & ~63) + n * abi.FH_BID_LIST * 4 + n * 8 + 2 * n * 4
    assert int(capi.lib().fh_bid_work_bytes(0)) == 0 == int(capi.lib().fh_bid_work_bytes(-5))
    with pytest.raises(capi.FasterHipError):
        capi.Map.bid_goals_device(None, abi.default_spread_params(1.0, 1.0), None, None, 0, None, 1, None, None, 0, None, 0, None, None, None, None)


def test_every_argument_rule_in_the_stated_order(built):
    """Case k breaks clause k and every clause after it, and keeps every clause before it: FH_ERR_ARG.  Nothing but the last clauses
    passing gives anything else: FH_OK for n == 0 without any pointer, and with host memory for d_records the runtime is asked whose
    it is and the answer is FH_ERR_DEVICE, with or without a device.  Every call is made to the other chooser's entry point too: the
    same clauses, the same order, the same answers."""
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
        p = np.ascontiguousarray(abi.default_bid_params(1.5, 1.0, 3)).reshape(1).copy()
        for k, v in kw.items():
            p[k] = v
        return p

    work = int(L.fh_bid_work_bytes(1))
    assert work == 64 + 256 + 8 + 8 and work > int(L.fh_spread_work_bytes(1))
    good = dict(p=par(), mg=grid(res=0.3, dims=(9, 9, 5)), bits=d + 20480, g=grid(), flags=d, stride=256, view_of=None, n_views=2, group=None,
                veh=d + 1024, n=1, work=d + 24576, work_bytes=work, goals=d + 4096, mask=d + 8192, rec=d + 12288)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        ptr = lambda x: None if x is None else abi.ptr(x)   # noqa: E731
        args = (None, ptr(a["p"]), ptr(a["mg"]), a["bits"], ptr(a["g"]), a["flags"], a["stride"], a["view_of"], a["n_views"], a["group"], a["veh"],
                a["n"], a["work"], a["work_bytes"], a["goals"], a["mask"], a["rec"])
        rc = L.fh_bid_goals_device(*args)
        if a["work_bytes"] >= work or rc == ARG and a["work_bytes"] == 0:
            assert L.fh_team_goals_device(*args) == rc, kw   # K18's answer (the same bytes are its params; its workspace is the smaller)
        return rc

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
        ("map_grid", [dict(mg=v) for v in grids]),
        ("map cells", [dict(mg=v) for v in many]),
        ("d_map_bits", [dict(bits=None)]),
        ("grid", [dict(g=v) for v in grids]),
        ("cells", [dict(g=v, stride=1 << 62) for v in many]),
        ("view_stride", [dict(stride=v) for v in (255, 0)]),
        ("n_views", [dict(n_views=v) for v in (0, -3)]),
        ("n", [dict(n=v) for v in (-1, -(1 << 31))]),
        ("r_spread", [dict(r_spread=v) for v in (nan, inf, -inf, 0.0, -0.0, -1.0)]),
        ("passes", [dict(passes=v) for v in (0, -1, 65, 1 << 30, -(1 << 31))]),
        ("gain_radius", [dict(gain_radius=v) for v in (-1, 32, 1 << 30, -(1 << 31))]),
        ("hop_cost", [dict(hop_cost=v) for v in (-1, 16385, (1 << 31) - 1, -(1 << 31))]),
        ("min_gain", [dict(min_gain=v) for v in (-1, -(1 << 31))]),
        ("claim_radius", [dict(claim_radius=v) for v in (-2, 32, 1 << 30, -(1 << 31))]),
    ]
    fields = ("r_max", "r_avoid", "z_lo", "z_hi", "want", "max_hops", "r_spread", "passes", "gain_radius", "hop_cost", "min_gain", "claim_radius")
    # what breaks each clause together with every later one: the value of the argument, or of the field of par
    worst = dict(r_max=nan, r_avoid=-1.0, z_lo=nan, want=0, max_hops=-1, mg=None, bits=None, g=None, stride=0, n_views=0, n=-1, r_spread=nan, passes=0,
                 gain_radius=-1, hop_cost=-1, min_gain=-1, claim_radius=-2)
    order = ["r_max", "r_avoid", "z_lo", "want", "max_hops", "mg", "mg", "bits", "g", "g", "stride", "n_views", "n", "r_spread", "passes", "gain_radius",
             "hop_cost", "min_gain", "claim_radius"]
    assert len(order) == len(clauses) - 1
    nothing = dict(flags=None, veh=None, goals=None, mask=None, rec=None, work=None, work_bytes=0)

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
            if "n" not in kw and name != "n":
                # n == 0 does not turn it into FH_OK: every clause comes before that answer
                assert call(**build(kw, dict(nothing, n=0))) == ARG, (name, kw)
    # all clauses fine: the call goes on to n == 0, then to the pointers, the workspace and its size
    assert call(n=0, **nothing) == OK and call(n=0) == OK
    for key in ("flags", "veh", "goals", "mask", "rec", "work"):
        assert call(**{key: None}) == ARG, key
    assert call(work_bytes=work - 1) == ARG and call(work_bytes=0) == ARG      # one byte short is refused
    assert call(work_bytes=int(L.fh_spread_work_bytes(1))) == ARG             # and so is the other choosers' workspace
    assert call(view_of=d + 40000) == DEVICE and call(group=d + 40000) == DEVICE    # may be given, may be NULL
    # the edges of the rules that pass: n == 0, so nothing is launched
    for p in (par(claim_radius=-1), par(claim_radius=0), par(claim_radius=31), par(gain_radius=0), par(gain_radius=31), par(hop_cost=0),
              par(hop_cost=16384), par(min_gain=(1 << 31) - 1), par(passes=1), par(passes=64), par(r_spread=1e-300), par(max_hops=(1 << 31) - 1)):
        assert call(p=p, n=0) == OK
    # host memory is no place for the records: the device that owns them is asked for before anything is launched
    assert call() == DEVICE
    assert L.fh_abi_version() == 9


def test_fleet_explore_bid_raises_what_explore_team_raises_before_any_launch():
    from faster_amd import capi
    from faster_amd.fleet import Fleet

    f = Fleet.__new__(Fleet)   # (no device here: only the checks that come before the first launch are reached)
    f.cloud = f.map_args = f.view_flags = f.flags = f.view_of = f.d_headings = f.grid = None
    f.d_reach_goals = f.d_reach_mask = f.d_reach_records = f.d_reach_view_of = None
    f.d_team_goals = f.d_team_mask = f.d_team_records = f.d_team_work = f.d_link_labels = None
    f.d_bid_goals = f.d_bid_mask = f.d_bid_records = f.d_bid_work = None
    f.map = f.ctx = None

    def both(match, *args, **kw):
        said = []
        for method, name in ((f.explore_team, "Fleet.explore_team:"), (f.explore_team_stages, "Fleet.explore_team:"), (f.explore_bid, "Fleet.explore_bid:"),
                             (f.explore_bid_stages, "Fleet.explore_bid:")):
            with pytest.raises(capi.FasterHipError, match=match) as e:
                method(args[0], 1.0, 5, *args[1:], **kw)
            assert str(e.value).startswith(name), str(e.value)
            said.append(str(e.value).replace(name, ""))
        assert said[0] == said[1] == said[2] == said[3]   # the same words, but for the name

    both("set_map", 2.0)
    f.cloud, f.map_args = object(), ((10, 10, 4), 0.2, (0.0, 0.0, 1.0), 2.0, 0.0)
    both("set_unknown_views", 2.0, want="all")
    with pytest.raises(capi.FasterHipError, match="explore_bid first"):
        f.bid_records()
    both("groups", 2.0, groups="team")

    class Flags:   # stands in for the tensor of the views
        shape = (3, 100)

    f.view_flags, f.n_views, f.n = Flags(), 3, 3
    f.grid = ((0.0, 0.0, 0.0), 0.5, (5, 5, 4))
    both("enable_heading", 2.0)
    for bad in ("arrived", (), ("all", "none")):
        both("want", 2.0, want=bad)
    import inspect

    assert inspect.signature(Fleet.explore_bid) == inspect.signature(Fleet.explore_team) == inspect.signature(Fleet.explore_bid_stages)
    assert inspect.signature(Fleet.bid_records) == inspect.signature(Fleet.team_records)
    assert "claim_radius" in Fleet.explore_bid.__doc__ and "at most 31" in Fleet.explore_bid.__doc__
