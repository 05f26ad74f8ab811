"""CPU-side checks of fh_prospect_goals_device: declared in include/fasterhip_prospect.h and in no other header, the header compiles
alone as C99 and C++11, exported, bound in faster_amd/capi.py on Map and on Fleet, the struct layouts and the constants of the header
equal faster_amd/abi.py, FH_ABI_VERSION stays, the device code lives in fh_prospect.hpp which fh_reach.hip alone includes, between the
far chooser's device header and the team's, with two kernels and no atomics, every clause of the prologue answers FH_ERR_ARG in the
stated order (all of them come before the first call of the runtime, so host pointers stand in for device pointers),
fh_prospect_work_bytes is the formula, a workspace one byte short is refused, and Fleet.explore_far_gain raises explore_far()'s errors
before any launch."""
import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from faster_amd import abi

import far_gain_model as fg
import far_model as fa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "faster_amd", "csrc")
HDR = os.path.join(INC, "fasterhip.h")
NEW_HDR = os.path.join(INC, "fasterhip_prospect.h")
NEW = ["fh_prospect_work_bytes", "fh_prospect_goals_device"]
NAMES = r"fh_prospect|fasterhip_prospect|FH_PROSPECT|far_gain_goals|far_gain_record|far_gain_params|explore_far_gain"
OTHERS = (r"fh_far|fasterhip_far|FH_FAR|far_goals|far_record|far_params|explore_far|fh_gain|fasterhip_gain|FH_GAIN|gain_goals|gain_record|"
          r"gain_params|explore_gain|fh_team|fasterhip_team|FH_TEAM|team_goals|team_record|team_params|explore_team|fh_sight|fasterhip_sight|"
          r"FH_SIGHT|sight_goals|sight_record|sight_params|explore_sight|fh_bid|fasterhip_bid|FH_BID|bid_goals|bid_record|bid_params|explore_bid|"
          r"fh_apart|fasterhip_apart|FH_APART|far_spread_goals|far_spread_record|far_spread_params|explore_far_spread|fh_spread|"
          r"fasterhip_spread|FH_SPREAD|spread_goals|spread_record|spread_params|explore_spread")
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
    for untouched in glob.glob(os.path.join(CSRC, "*")):
        if os.path.basename(untouched) not in ("fh_reach.hip", "fh_prospect.hpp"):
            assert not re.search(NAMES, open(untouched).read()), untouched    # nor has any other file of the device code
    assert int(re.search(r"#define FH_ABI_VERSION (\d+)", open(HDR).read()).group(1)) == abi.FH_ABI_VERSION == 9
    text = open(NEW_HDR).read()
    assert re.findall(r'#include "([^"]+)"', text) == ["fasterhip.h", "fasterhip_frontier.h", "fasterhip_reach.h"]
    assert not re.search(OTHERS, text)   # the other choosers keep their names to themselves
    assert "n_views * 4 * W * 8 + ((n_views + 63) & ~63) + n_views * 64 * W * 2" in text
    src = "#include \"fasterhip_prospect.h\"\nint main(void) {\n" + "".join("  (void)%s;\n" % n for n in NEW) + "  return 0;\n}\n"
    for lang, std, comp in (("c", "-std=c99", "gcc"), ("c++", "-std=c++11", "g++")):
        f = tmp_path / ("probe." + ("c" if lang == "c" else "cpp"))
        f.write_text(src)
        r = subprocess.run([comp, "-fsyntax-only", "-x", lang, std, "-Wall", "-pedantic", "-I", INC, str(f)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr.strip(), (lang, r.stderr[-2000:])


def test_struct_layouts_and_constants_of_the_header_equal_abi_py(tmp_path):
    """sizeof and every offsetof of the two structs, printed by a C program compiled against the header."""
    structs = (("fh_prospect_params", abi.far_gain_params_dtype, 64), ("fh_prospect_record", abi.far_gain_record_dtype, 80),
               ("fh_far_params", abi.far_params_dtype, 64), ("fh_far_record", abi.far_record_dtype, 64))
    consts = ["FH_PROSPECT_SKIPPED", "FH_PROSPECT_MAX_WORDS", "FH_PROSPECT_ALL_POOR", "FH_PROSPECT_MAX_BLOCKS", "FH_PROSPECT_MAX_HOP_COST",
              "FH_FAR_SKIPPED", "FH_FAR_MAX_WORDS", "FH_APART_UNSETTLED", "FH_APART_CLAIMED", "FH_REACH_START_OUTSIDE", "FH_REACH_CUT",
              "FH_FRONTIER_WANTED", "FH_FRONTIER_FOUND", "FH_FRONTIER_NO_VIEW", "FH_FRONTIER_BAD_POS"]
    lines = []
    for name, dt, _ in structs:
        lines.append('  printf("%s.size %%d\\n", (int)sizeof(%s));' % (name, name))
        lines += ['  printf("%s.%s %%d\\n", (int)offsetof(%s, %s));' % (name, k, name, k) for k in dt.names]
    lines += ['  printf("%s %%d\\n", (int)%s);' % (k, k) for k in consts]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"fasterhip_far.h\"\n#include \"fasterhip_apart.h\"\n"
                   "#include \"fasterhip_prospect.h\"\nint main(void) {\n" + "\n".join(lines) + "\n  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", INC, str(src), "-o", str(exe)])
    got = dict((k, int(v)) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()))
    for name, dt, size in structs:
        assert got[name + ".size"] == dt.itemsize == size, name
        for k in dt.names:
            assert got[name + "." + k] == dt.fields[k][1], (name, k)
    for k in consts:
        assert got[k] == getattr(abi, k), k
    assert [got[k] for k in consts[:5]] == [128, 512, 1024, 5, 16384]
    assert (got["FH_PROSPECT_SKIPPED"], got["FH_PROSPECT_MAX_WORDS"]) == (got["FH_FAR_SKIPPED"], got["FH_FAR_MAX_WORDS"])
    # the params are the far chooser's with three of its reserved words in use; the first 64 bytes of the record are its record
    fp, gp = abi.far_params_dtype, abi.far_gain_params_dtype
    assert gp.names == fp.names[:-1] + ("gain_blocks", "hop_cost", "min_gain", "reserved")
    assert all(gp.fields[k][:2] == fp.fields[k][:2] for k in fp.names[:-1])
    assert [gp.fields[k][1] for k in ("gain_blocks", "hop_cost", "min_gain", "reserved")] == [fp.fields["reserved"][1] + 4 * j for j in range(4)]
    fr, gr = abi.far_record_dtype, abi.far_gain_record_dtype
    assert gr.names == fr.names + ("gain", "utility", "poor", "best_gain") and all(gr.fields[k][:2] == fr.fields[k][:2] for k in fr.names)
    assert [gr.fields[k][1] for k in ("gain", "utility", "poor", "best_gain")] == [64, 68, 72, 76]
    # the new flag is a bit of its own beside the ones it stands with, the team's far chooser's two included
    others = [got[k] for k in consts[7:]] + [got["FH_FAR_SKIPPED"], abi.FH_REACH_BOX_TOO_LARGE]
    assert all(got["FH_PROSPECT_ALL_POOR"] & o == 0 for o in others)
    p = abi.default_far_gain_params(8, 2)
    assert (float(p["r_avoid"]), float(p["z_lo"]), float(p["z_hi"]), float(p["reserved_d"]), int(p["want"]), int(p["max_hops"]), int(p["block"]),
            int(p["gain_blocks"]), int(p["hop_cost"]), int(p["min_gain"])) == (0.0, -np.inf, np.inf, 0.0, abi.FH_FRONTIER_WANT_REACHED, 0, 8, 2, 64, 0)
    assert not p["reserved"].any()


def test_the_symbols_are_exported_and_bound_and_the_device_code_is_included_by_fh_reach_hip_alone(built):
    from faster_amd import capi
    from faster_amd.fleet import Fleet

    L = ctypes.CDLL(built.SO)
    for name in NEW:
        assert hasattr(L, name), name
    assert capi.FAR_GAIN_SYMBOLS == NEW
    lists = [k for k in dir(capi) if k.endswith("SYMBOLS") and k != "FAR_GAIN_SYMBOLS"]
    assert len(lists) >= 20 and "SYMBOLS" in lists and "FAR_SYMBOLS" in lists and "FAR_SPREAD_SYMBOLS" in lists and "GAIN_SYMBOLS" in lists
    for k in lists:
        assert not set(NEW) & set(getattr(capi, k)), k
    assert len(capi.lib().fh_prospect_goals_device.argtypes) == 17 and capi.lib().fh_prospect_goals_device.restype == ctypes.c_int32
    assert capi.lib().fh_prospect_goals_device.argtypes == capi.lib().fh_far_goals_device.argtypes
    assert capi.lib().fh_prospect_work_bytes.restype == ctypes.c_size_t and len(capi.lib().fh_prospect_work_bytes.argtypes) == 3
    assert hasattr(capi.Map, "far_gain_goals_device")
    for name in ("explore_far_gain", "explore_far_gain_stages", "far_gain_records"):
        assert hasattr(Fleet, name), name
    assert NEW_HDR in built.DEPS and os.path.join(CSRC, "fh_prospect.hpp") in built.DEPS
    assert built.SOURCES[-1] == os.path.join(CSRC, "fh_reach.hip") and len(built.SOURCES) == 4
    assert "capi.FAR_GAIN_SYMBOLS" in open(os.path.join(ROOT, "__graft_entry__.py")).read()   # build() touches the new symbols
    assert capi.lib().fh_abi_version() == 9
    strip = lambda path: re.sub(r"//[^\n]*", "", open(path).read())   # noqa: E731
    for other in glob.glob(os.path.join(CSRC, "*")):
        if os.path.basename(other) != "fh_reach.hip":
            assert "fh_prospect.hpp" not in strip(other), other
    host = strip(os.path.join(CSRC, "fh_reach.hip"))
    includes = re.findall(r'#include "([^"]+)"', host)
    assert includes.index("fh_far.hip.hpp") < includes.index("fh_prospect.hpp") < includes.index("fh_apart.hpp") == len(includes) - 1
    assert [i for i in includes if i.endswith(".hip.hpp")][-1] == "fh_far.hip.hpp"
    raw = open(os.path.join(CSRC, "fh_prospect.hpp")).read()
    body = strip(os.path.join(CSRC, "fh_prospect.hpp"))
    assert sorted(set(re.findall(r"\b(\w+_kernel)\s*\(", body))) == ["prospect_blocks_kernel", "prospect_goals_kernel"]
    assert "#pragma clang fp contract(off)" in body and "atomic" not in raw.lower()
    assert re.findall(r'#include "([^"]+)"', body) == ["../../include/fasterhip_prospect.h"]
    assert "fh_far.hip.hpp" not in body and "fh_apart.hpp" not in body and not re.search(OTHERS, raw)
    for called in ("far_start(", "far_summary<false>(", "far_expand(", "far_level_any(", "far_scan_block(", "far_put_goal(", "far_head(",
                   "far_passable(", "far_target(", "far_block_d2(", "reach_before(", "FAR_WORDS", "FarArgs"):   # the far chooser's own, called
        assert called in body, called
    assert not re.search(r"__device__[^\n;{]*\b(far_judge|far_gap2|far_body|far_block_d2|far_passable|far_target|reach_before|far_start|far_summary|"
                         r"far_expand|far_level_any|far_scan_block|far_put_goal|far_head|far_claim_scan)\s*\(", body)   # not copied
    assert "prospect_goals_kernel(ProspectArgs p) { prospect_body<false>(p, ProspectNoClaims()); }" in body
    far = strip(os.path.join(CSRC, "fh_far.hip.hpp"))
    assert "far_goals_kernel(FarArgs a) { far_body<false>(a, FarNoClaims()); }" in far and "far_body<true>(" in strip(os.path.join(CSRC, "fh_apart.hpp"))
    assert sorted(set(re.findall(r"\b(\w+_kernel)\s*\(", far))) == ["far_blocks_kernel", "far_goals_kernel", "far_need_kernel"]
    # the entry points stand outside the spans the other choosers' tests cut out; a memset of the need bytes, then three launches
    at = [host.index("static size_t bid_offers_offset"), host.index("size_t fh_prospect_work_bytes"), host.index("int fh_prospect_goals_device"),
          host.index("int fh_apart_goals_device")]
    assert at == sorted(at)
    entry = host[at[2]:at[3]]
    assert re.findall(r"hipLaunchKernelGGL\(fhp::(\w+)", entry) == ["far_need_kernel", "prospect_blocks_kernel", "prospect_goals_kernel"]
    assert entry.count("hipMemsetAsync(") == 1 and entry.index("hipMemsetAsync(") < entry.index("hipLaunchKernelGGL")
    assert "reach_table_clauses(" in entry and "reach_field_clauses(" in entry and "far_words(" in entry
    assert "static_assert" in entry and "offsetof(fh_prospect_record, block_d2) == offsetof(fh_far_record, block_d2)" in entry
    with pytest.raises(capi.FasterHipError):
        capi.Map.far_gain_goals_device(None, abi.default_far_params(8), None, None, 0, None, 1, None, None, 0, None, 0, None, None, None, None)


def grid(res=0.5, dims=(8, 8, 4)):
    g = np.zeros(1, dtype=abi.voxel_grid_dtype)
    g["origin"], g["res"], g["dims"] = (0.1, 0.2, 0.3), res, dims
    return g


def test_work_bytes_is_the_formula_and_zero_for_each_bad_argument(built):
    from faster_amd import capi

    wb, far = capi.lib().fh_prospect_work_bytes, capi.lib().fh_far_work_bytes
    for dims in ((8, 8, 4), (13, 7, 3), (65, 1, 2), (64, 64, 8), (1, 1, 1), (1000, 900, 40), fa.OVER_CAP):
        for B in (1, 2, 3, 8, 16):
            for n_views in (1, 2, 63, 64, 65, 1000):
                W = fa.blocks_of(dims, B)[2]
                want = 0 if W > 512 else n_views * 4 * W * 8 + ((n_views + 63) & ~63) + n_views * 64 * W * 2
                got = int(wb(abi.ptr(grid(dims=dims)), B, n_views))
                assert got == want == fg.work_bytes(dims, B, n_views), (dims, B, n_views)
                assert want == 0 or (want - n_views * 64 * W * 2 == int(far(abi.ptr(grid(dims=dims)), B, n_views)) and (want - n_views * 128 * W) % 8 == 0)
    assert int(wb(abi.ptr(grid(dims=(64, 64, 8))), 1, 1)) == 4 * 512 * 8 + 64 + 64 * 512 * 2 and int(wb(abi.ptr(grid(dims=fa.OVER_CAP)), 1, 1)) == 0
    assert int(wb(None, 8, 1)) == 0
    for dims in ((0, 8, 4), (8, 0, 4), (8, 8, 0), (-1, 8, 4)):
        assert int(wb(abi.ptr(grid(dims=dims)), 8, 1)) == 0, dims
    for B in (0, -1, 17, 1 << 30, -(1 << 31)):
        assert int(wb(abi.ptr(grid()), B, 1)) == 0, B
    for n_views in (0, -1, -(1 << 31)):
        assert int(wb(abi.ptr(grid()), 8, n_views)) == 0, n_views
    big = (1 << 31) - 1
    assert int(wb(abi.ptr(grid(dims=(big, big, big))), 1, 1)) == 0 and int(wb(abi.ptr(grid(dims=(big, big, big))), 16, big)) == 0
    assert int(wb(abi.ptr(grid()), 8, big)) == big * 4 * 8 + ((big + 63) & ~63) + big * 128   # nothing overflows


def test_every_argument_rule_in_the_stated_order(built):
    """Case k breaks clause k and every clause after it, and keeps every clause before it: FH_ERR_ARG.  Nothing but the last clauses
    passing gives anything else: FH_OK for n == 0 without any pointer, and with host memory for d_records the runtime is asked whose
    it is and the answer is FH_ERR_DEVICE, with or without a device."""
    from faster_amd import capi

    L = capi.lib()
    buf = np.zeros(1 << 16, dtype=np.uint8)
    d = buf.ctypes.data
    nan, inf = float("nan"), float("inf")

    def par(**kw):
        p = np.ascontiguousarray(abi.default_far_gain_params(8, 2)).reshape(1).copy()
        for k, v in kw.items():
            p[k] = v
        return p

    need = 2 * 4 * 1 * 8 + 64 + 2 * 64 * 2   # n_views 2, W 1
    assert int(L.fh_prospect_work_bytes(abi.ptr(grid()), 8, 2)) == need
    good = dict(p=par(), mg=grid(res=0.3, dims=(9, 9, 5)), bits=d + 20480, g=grid(), flags=d, stride=256, view_of=None, n_views=2, skip=None,
                veh=d + 1024, n=1, work=d + 24576, work_bytes=need, goals=d + 4096, mask=d + 8192, rec=d + 12288)
    clauses = [
        ("par", "p", [None]),
        ("r_avoid", "p", [par(r_avoid=v) for v in (nan, inf, -inf, -1e-300, -1.0)]),
        ("z", "p", [par(z_lo=lo, z_hi=hi) for lo, hi in ((nan, 1.0), (0.0, nan), (nan, nan), (1.0, 0.5), (inf, -inf))]),
        ("want", "p", [par(want=v) for v in (0, 8, 9, 16, -1, 1 << 30)]),
        ("max_hops", "p", [par(max_hops=v) for v in (-1, -(1 << 31))]),
        ("block", "p", [par(block=v) for v in (0, -1, 17, 1 << 30, -(1 << 31))]),
        ("gain_blocks", "p", [par(gain_blocks=v) for v in (-1, 6, 1 << 30, -(1 << 31))]),
        ("hop_cost", "p", [par(hop_cost=v) for v in (-1, 16385, (1 << 31) - 1, -(1 << 31))]),
        ("min_gain", "p", [par(min_gain=v) for v in (-1, -(1 << 31))]),
        ("map_grid", "mg", [None] + [grid(res=r) for r in (0.0, -0.5, nan)] + [grid(dims=dm) for dm in ((0, 8, 4), (8, 0, 4), (8, 8, -1))]),
        ("map cells", "mg", [grid(dims=dm) for dm in ((1 << 16, 1 << 15, 1), (1 << 16, 1 << 16, 1 << 16), (2, 1 << 30, 1),
                                                      ((1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1))]),
        ("d_map_bits", "bits", [None]),
        ("grid", "g", [None] + [grid(res=r) for r in (0.0, -0.5, nan)] + [grid(dims=dm) for dm in ((0, 8, 4), (8, 0, 4), (8, 8, -1))]),
        ("cells", "g", [grid(dims=dm) for dm in ((1 << 16, 1 << 15, 1), (1 << 16, 1 << 16, 1 << 16), (2, 1 << 30, 1))]),
        ("view_stride", "stride", [255, 0]),
        ("n_views", "n_views", [0, -3]),
        ("n", "n", [-1, -(1 << 31)]),
        ("words", "g", [grid(dims=fa.OVER_CAP), grid(dims=(1 << 15, 1 << 15, 1)), grid(dims=(64 * 512 + 1, 1, 1)), grid(dims=(64, 1, 513))]),
        ("work_bytes", "work_bytes", [need - 1, 0]),
    ]
    # what breaks a clause together with every clause after it (the params record carries eight clauses: the later fields broken too)
    broken_after = {"p": None, "mg": None, "bits": None, "g": None, "stride": 0, "n_views": 0, "n": -1, "work_bytes": 0}
    later_fields = {"r_avoid": dict(z_lo=nan, want=0, max_hops=-1, block=0, gain_blocks=-1, hop_cost=-1, min_gain=-1),
                    "z": dict(want=0, max_hops=-1, block=0, gain_blocks=-1, hop_cost=-1, min_gain=-1),
                    "want": dict(max_hops=-1, block=0, gain_blocks=-1, hop_cost=-1, min_gain=-1),
                    "max_hops": dict(block=0, gain_blocks=-1, hop_cost=-1, min_gain=-1), "block": dict(gain_blocks=-1, hop_cost=-1, min_gain=-1),
                    "gain_blocks": dict(hop_cost=-1, min_gain=-1), "hop_cost": dict(min_gain=-1), "min_gain": {}}
    nothing = dict(flags=None, veh=None, goals=None, mask=None, rec=None, work=None)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        ptr = lambda x: None if x is None else abi.ptr(x)   # noqa: E731
        return L.fh_prospect_goals_device(None, ptr(a["p"]), ptr(a["mg"]), a["bits"], ptr(a["g"]), a["flags"], a["stride"], a["view_of"],
                                          a["n_views"], a["skip"], a["veh"], a["n"], a["work"], a["work_bytes"], a["goals"], a["mask"], a["rec"])

    order = ["p", "mg", "bits", "g", "stride", "n_views", "n", "work_bytes"]
    for name, key, values in clauses:
        after = {k: broken_after[k] for k in order[order.index(key) + 1:]}
        for v in values:
            alone = {}
            if key == "p" and v is not None:
                v = v.copy()
                for f, x in later_fields[name].items():
                    v[f] = x
            if name in ("grid", "cells"):
                after["stride"] = 0   # (smaller than any number of cells)
            if name == "cells":
                alone = dict(stride=1 << 62)
            if name == "words":   # every clause before it holds: a stride that covers the cells, and blocks of one voxel
                alone = dict(stride=1 << 40, p=par(block=1), work_bytes=1 << 40)
                after = dict(stride=1 << 40, work_bytes=0)
            assert call(**{**alone, key: v}) == ARG, (name, v)                           # the clause alone
            assert call(**{**alone, **after, **nothing, key: v}) == ARG, (name, v)        # and with everything after it broken as well
            if key != "n":
                assert call(**{**alone, **nothing, key: v, "n": 0}) == ARG, (name, v)    # n == 0 does not turn it into FH_OK
    # the order itself: a broken clause hides every later one but none before it — the three new fields stand between block and the
    # tables: with a null map_grid each of them still answers, and none of them hides a bad block
    for p in (par(gain_blocks=6), par(hop_cost=16385), par(min_gain=-1), par(block=0, gain_blocks=2)):
        assert call(p=p, mg=None, n=0) == ARG
    assert call(g=grid(dims=fa.OVER_CAP), stride=1 << 40, p=par(block=2), work_bytes=1 << 40, n=0) == OK
    assert call(work_bytes=need - 1) == ARG and call(work_bytes=need - 1, n=0, **nothing) == ARG   # (the bytes do not depend on n)
    # a workspace one byte short, at the cap
    full = 2 * 4 * 512 * 8 + 64 + 2 * 64 * 512 * 2
    assert call(g=grid(dims=(64, 64, 8)), stride=1 << 40, p=par(block=1), work_bytes=full, **nothing) == ARG           # (the pointers come last)
    assert call(g=grid(dims=(64, 64, 8)), stride=1 << 40, p=par(block=1), work_bytes=full) == DEVICE
    assert call(g=grid(dims=(64, 64, 8)), stride=1 << 40, p=par(block=1), work_bytes=full - 1) == ARG                  # one byte short
    assert call(g=grid(dims=(64, 64, 8)), stride=1 << 40, p=par(block=1), work_bytes=full - 1, n=0) == ARG
    assert call(g=grid(dims=(64, 64, 8)), stride=1 << 40, p=par(block=1), work_bytes=2 * 4 * 512 * 8 + 64, n=0) == ARG   # the far chooser's bytes are not enough
    # every rule passes: n == 0 is fine without any pointer, then the pointers
    assert call(n=0, **nothing) == OK and call(n=0) == OK
    for k in nothing:
        assert call(**{k: None}) == ARG, k
    assert call(work_bytes=need + 1, n=0) == OK
    # the edges of the rules that pass: n == 0, so nothing is launched
    for p in (par(gain_blocks=0), par(gain_blocks=5), par(hop_cost=0), par(hop_cost=16384), par(min_gain=(1 << 31) - 1), par(r_avoid=1e300),
              par(z_lo=inf, z_hi=inf), par(block=16), par(block=1), par(reserved_d=nan)):
        assert call(p=p, n=0, work_bytes=1 << 20) == OK
    # d_view_of and d_skip may be null or not; host memory is no place for the records
    assert call() == DEVICE and call(view_of=d + 16384, skip=d + 16640) == DEVICE
    assert L.fh_abi_version() == 9


def test_fleet_explore_far_gain_raises_what_explore_far_raises_before_any_launch(built):
    from faster_amd import capi
    from faster_amd.fleet import Fleet

    f = Fleet.__new__(Fleet)   # (no device here: only the checks that come before the first launch are reached)
    f.cloud = f.map_args = f.view_flags = f.flags = f.view_of = f.d_headings = f.grid = None
    f.d_reach_view_of = None
    f.d_far_goals = f.d_far_mask = f.d_far_records = f.d_far_work = f._far_work_key = None
    f.d_far_gain_goals = f.d_far_gain_mask = f.d_far_gain_records = f.d_far_gain_work = f._far_gain_work_key = None
    f.d_explore_mask = f.d_reach_mask = f.d_spread_mask = f.d_gain_mask = f.d_sight_mask = f.d_team_mask = f.d_bid_mask = None
    f.d_link_labels = None
    f.map = f.ctx = None

    def both(match, *args, **kw):
        """explore_far(block, ...) and explore_far_gain(block, gain_blocks, ...): the same words, but for the name."""
        said = []
        for method, name, first in ((f.explore_far, "Fleet.explore_far:", (8,)), (f.explore_far_gain, "Fleet.explore_far_gain:", (8, 2, None, 0))):
            with pytest.raises(capi.FasterHipError, match=match) as e:
                method(*first, *args, **kw)
            assert str(e.value).startswith(name), str(e.value)
            said.append(str(e.value).replace(name, ""))
        assert said[0] == said[1]

    both("set_map")
    f.cloud, f.map_args = object(), ((10, 10, 4), 0.2, (0.0, 0.0, 1.0), 2.0, 0.0)
    both("set_unknown_views", want="all")
    with pytest.raises(capi.FasterHipError, match="explore_far_gain first"):
        f.far_gain_records()

    class Flags:   # stands in for the tensor of the views
        shape = (3, 100)

    f.view_flags, f.n_views, f.n = Flags(), 3, 3
    f.grid = ((0.0, 0.0, 0.0), 0.5, (5, 5, 4))
    both("enable_heading")
    for bad in ("arrived", (), ("all", "none")):
        both("want", want=bad)
    f.params, f.z_ground = abi.default_fleet_params(), 0.0
    both("after is None or one of", want="all", after="nearest")
    for name in ("explore", "reachable", "spread", "gain", "sight", "team", "bid"):
        both("has not run", want="all", after=name)
    for kw, match in ((dict(gain_blocks=6), "gain_blocks must be 0 .. 5"), (dict(gain_blocks=-1), "gain_blocks must be"),
                      (dict(hop_cost=16385), "hop_cost must be None or 0 .. 16384"), (dict(hop_cost=-1), "hop_cost must be"),
                      (dict(min_gain=-1), "min_gain must be >= 0")):
        with pytest.raises(capi.FasterHipError, match=match):
            f.explore_far_gain(8, want="all", **kw)
    f.grid = ((0.0, 0.0, 0.0), 0.5, fa.OVER_CAP)
    for block in (1, 0, 17):
        with pytest.raises(capi.FasterHipError, match="Fleet.explore_far_gain: block must be"):
            f.explore_far_gain(block, want="all")
