"""CPU-side checks of fh_stake_goals_device: declared in include/fasterhip_stake.h and in no other header, the header compiles alone as C99
and C++11, the names of the other choosers and its own are kept apart both ways, exported, bound in faster_amd/capi.py on Map and on Fleet
with the far chooser for a team's eighteen argument types, the struct layouts and the constants of the header equal faster_amd/abi.py and
begin as that chooser's and the far chooser by gain's do, FH_ABI_VERSION stays, the device code lives in fh_stake.hpp which fh_reach.hip
alone includes, between the device headers of those two, with two kernels and no read-modify-write, the entry point launches the chain
the header states after one memset, every clause of the prologue answers FH_ERR_ARG in the stated order (all of them come before the
first call of the runtime, so host pointers stand in for device pointers), fh_stake_work_bytes is the formula, a workspace one byte
short is refused, and Fleet.explore_far_team raises explore_far_spread()'s errors before any launch."""
import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from faster_amd import abi

import far_model as fa
import far_team_model as ft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "faster_amd", "csrc")
HDR = os.path.join(INC, "fasterhip.h")
NEW_HDR = os.path.join(INC, "fasterhip_stake.h")
NEW_DEV = os.path.join(CSRC, "fh_stake.hpp")
NEW = ["fh_stake_work_bytes", "fh_stake_goals_device"]
NAMES = r"fh_stake|fasterhip_stake|FH_STAKE|far_team_goals|far_team_record|far_team_params|explore_far_team"
OTHERS = (r"fh_far|fasterhip_far|FH_FAR|far_goals|far_record|far_params|explore_far|fh_gain|fasterhip_gain|FH_GAIN|gain_goals|gain_record|"
          r"gain_params|explore_gain|fh_team|fasterhip_team|FH_TEAM|team_goals|team_record|team_params|explore_team|fh_sight|fasterhip_sight|"
          r"FH_SIGHT|sight_goals|sight_record|sight_params|explore_sight|fh_bid|fasterhip_bid|FH_BID|bid_goals|bid_record|bid_params|explore_bid|"
          r"fh_apart|fasterhip_apart|FH_APART|far_spread_goals|far_spread_record|far_spread_params|explore_far_spread|fh_spread|"
          r"fasterhip_spread|FH_SPREAD|spread_goals|spread_record|spread_params|explore_spread|fh_prospect|fasterhip_prospect|FH_PROSPECT|"
          r"far_gain_goals|far_gain_record|far_gain_params|explore_far_gain")
FORMULA = "n_views * 4 * W * 8 + ((n_views + 63) & ~63) + n_views * 64 * W * 2 + ((n + 63) & ~63) + n * 4 + n * 4"
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
        if os.path.basename(untouched) not in ("fh_reach.hip", "fh_stake.hpp"):
            assert not re.search(NAMES, open(untouched).read()), untouched    # nor has any other file of the device code
    assert int(re.search(r"#define FH_ABI_VERSION (\d+)", open(HDR).read()).group(1)) == abi.FH_ABI_VERSION == 9
    text = open(NEW_HDR).read()
    assert re.findall(r'#include "([^"]+)"', text) == ["fasterhip.h", "fasterhip_frontier.h", "fasterhip_reach.h"]
    assert not re.search(OTHERS, text)                  # the other choosers keep their names to themselves
    assert not re.search(OTHERS, open(NEW_DEV).read())  # in the device file too
    assert FORMULA in text
    for said in ("K21", "K22", "K23", "(a)", "(b)", "(c)", "(d)", "(e)"):
        assert said in text, said
    src = "#include \"fasterhip_stake.h\"\nint main(void) {\n" + "".join("  (void)%s;\n" % n for n in NEW) + "  return 0;\n}\n"
    for lang, std, comp in (("c", "-std=c99", "gcc"), ("c++", "-std=c++11", "g++")):
        f = tmp_path / ("probe." + ("c" if lang == "c" else "cpp"))
        f.write_text(src)
        r = subprocess.run([comp, "-fsyntax-only", "-x", lang, std, "-Wall", "-pedantic", "-I", INC, str(f)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr.strip(), (lang, r.stderr[-2000:])


def test_struct_layouts_and_constants_of_the_header_equal_abi_py(tmp_path):
    """sizeof and every offsetof of the two structs, printed by a C program compiled against the header."""
    structs = (("fh_stake_params", abi.far_team_params_dtype, 96), ("fh_stake_record", abi.far_team_record_dtype, 128),
               ("fh_apart_params", abi.far_spread_params_dtype, 96), ("fh_apart_record", abi.far_spread_record_dtype, 96),
               ("fh_prospect_params", abi.far_gain_params_dtype, 64), ("fh_prospect_record", abi.far_gain_record_dtype, 80))
    consts = ["FH_STAKE_SKIPPED", "FH_STAKE_UNSETTLED", "FH_STAKE_CLAIMED", "FH_STAKE_ALL_POOR", "FH_STAKE_MAX_WORDS", "FH_STAKE_MAX_PASSES",
              "FH_STAKE_DEFAULT_PASSES", "FH_STAKE_MAX_BLOCKS", "FH_STAKE_MAX_HOP_COST", "FH_STAKE_MAX_CLAIM_BLOCKS",
              "FH_FAR_SKIPPED", "FH_APART_UNSETTLED", "FH_APART_CLAIMED", "FH_PROSPECT_ALL_POOR", "FH_FAR_MAX_WORDS", "FH_APART_MAX_PASSES",
              "FH_APART_DEFAULT_PASSES", "FH_PROSPECT_MAX_BLOCKS", "FH_PROSPECT_MAX_HOP_COST",
              "FH_REACH_START_OUTSIDE", "FH_REACH_CUT", "FH_FRONTIER_WANTED", "FH_FRONTIER_FOUND", "FH_FRONTIER_NO_VIEW", "FH_FRONTIER_BAD_POS"]
    lines = []
    for name, dt, _ in structs:
        lines.append('  printf("%s.size %%d\\n", (int)sizeof(%s));' % (name, name))
        lines += ['  printf("%s.%s %%d\\n", (int)offsetof(%s, %s));' % (name, k, name, k) for k in dt.names]
    lines += ['  printf("%s %%d\\n", (int)%s);' % (k, k) for k in consts]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"fasterhip_far.h\"\n#include \"fasterhip_apart.h\"\n"
                   "#include \"fasterhip_prospect.h\"\n#include \"fasterhip_stake.h\"\nint main(void) {\n" + "\n".join(lines) + "\n  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", INC, str(src), "-o", str(exe)])
    got = dict((k, int(v)) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()))
    for name, dt, size in structs:
        assert got[name + ".size"] == dt.itemsize == size, name
        for k in dt.names:
            assert got[name + "." + k] == dt.fields[k][1], (name, k)
    for k in consts:
        assert got[k] == getattr(abi, k), k
    assert [got[k] for k in consts[:10]] == [128, 256, 512, 1024, 512, 64, 8, 5, 16384, 5]
    assert [got[k] for k in consts[:9]] == [got[k] for k in consts[10:19]]   # equal values under its own names
    # the params: the team's far chooser's, with the gain chooser's three words in its reserved words and claim_blocks first in its tail
    sp, gp, tp = abi.far_spread_params_dtype, abi.far_gain_params_dtype, abi.far_team_params_dtype
    assert tp.names == gp.names + ("r_spread", "passes", "claim_blocks", "reserved_tail")
    assert all(tp.fields[k][:2] == gp.fields[k][:2] for k in gp.names)
    assert all(tp.fields[k][:2] == sp.fields[k][:2] for k in sp.names if k not in ("reserved", "reserved_tail"))
    assert [tp.fields[k][1] for k in ("gain_blocks", "hop_cost", "min_gain", "reserved")] == [sp.fields["reserved"][1] + 4 * j for j in range(4)]
    assert (tp.fields["r_spread"][1], tp.fields["passes"][1], tp.fields["claim_blocks"][1], tp.fields["reserved_tail"][1]) == (64, 72, 76, 80)
    assert tp.fields["claim_blocks"][1] == sp.fields["reserved_tail"][1]
    # the record: the team's far chooser's 96 bytes, the gain chooser's four, covered, removed
    sr, gr, tr = abi.far_spread_record_dtype, abi.far_gain_record_dtype, abi.far_team_record_dtype
    assert tr.names == sr.names + ("gain", "utility", "poor", "best_gain", "covered", "removed", "reserved_end")
    assert all(tr.fields[k][:2] == sr.fields[k][:2] for k in sr.names)
    assert [tr.fields[k][1] - 96 for k in ("gain", "utility", "poor", "best_gain")] == [gr.fields[k][1] - 64 for k in ("gain", "utility", "poor", "best_gain")]
    assert [tr.fields[k][1] for k in ("gain", "utility", "poor", "best_gain", "covered", "removed", "reserved_end")] == [96, 100, 104, 108, 112, 116, 120]
    p = abi.default_far_team_params(8, 2.5, 2)
    assert (float(p["r_avoid"]), float(p["z_lo"]), float(p["z_hi"]), float(p["reserved_d"]), int(p["want"]), int(p["max_hops"]), int(p["block"]),
            int(p["gain_blocks"]), int(p["hop_cost"]), int(p["min_gain"]), float(p["r_spread"]), int(p["passes"]), int(p["claim_blocks"])) == \
        (0.0, -np.inf, np.inf, 0.0, abi.FH_FRONTIER_WANT_REACHED, 0, 8, 2, 64, 0, 2.5, 8, 2)
    assert not p["reserved"].any() and not p["reserved_tail"].any()


def test_the_symbols_are_exported_and_bound_and_the_device_code_is_included_by_fh_reach_hip_alone(built):
    from faster_amd import capi
    from faster_amd.fleet import Fleet

    L = ctypes.CDLL(built.SO)
    for name in NEW:
        assert hasattr(L, name), name
    assert capi.FAR_TEAM_SYMBOLS == NEW
    lists = [k for k in dir(capi) if k.endswith("SYMBOLS") and k != "FAR_TEAM_SYMBOLS"]
    assert len(lists) >= 21 and "SYMBOLS" in lists and "FAR_SYMBOLS" in lists and "FAR_SPREAD_SYMBOLS" in lists and "FAR_GAIN_SYMBOLS" in lists
    for k in lists:
        assert not set(NEW) & set(getattr(capi, k)), k
    assert len(capi.lib().fh_stake_goals_device.argtypes) == 18 and capi.lib().fh_stake_goals_device.restype == ctypes.c_int32
    assert capi.lib().fh_stake_goals_device.argtypes == capi.lib().fh_apart_goals_device.argtypes
    assert capi.lib().fh_stake_work_bytes.restype == ctypes.c_size_t and capi.lib().fh_stake_work_bytes.argtypes == capi.lib().fh_apart_work_bytes.argtypes
    assert hasattr(capi.Map, "far_team_goals_device")
    for name in ("explore_far_team", "explore_far_team_stages", "far_team_records"):
        assert hasattr(Fleet, name), name
    assert NEW_HDR in built.DEPS and NEW_DEV in built.DEPS
    assert built.SOURCES[-1] == os.path.join(CSRC, "fh_reach.hip") and len(built.SOURCES) == 4
    assert "capi.FAR_TEAM_SYMBOLS" in open(os.path.join(ROOT, "__graft_entry__.py")).read()   # build() touches the new symbols
    assert capi.lib().fh_abi_version() == 9
    strip = lambda path: re.sub(r"//[^\n]*", "", open(path).read())   # noqa: E731
    for other in glob.glob(os.path.join(CSRC, "*")):
        if os.path.basename(other) != "fh_reach.hip":
            assert "fh_stake.hpp" not in strip(other), other
    host = strip(os.path.join(CSRC, "fh_reach.hip"))
    includes = re.findall(r'#include "([^"]+)"', host)
    assert includes.index("fh_far.hip.hpp") < includes.index("fh_prospect.hpp") < includes.index("fh_stake.hpp") < includes.index("fh_apart.hpp")
    assert includes.index("fh_apart.hpp") == len(includes) - 1 and [i for i in includes if i.endswith(".hip.hpp")][-1] == "fh_far.hip.hpp"
    raw = open(NEW_DEV).read()
    body = strip(NEW_DEV)
    assert sorted(set(re.findall(r"\b(\w+_kernel)\s*\(", body))) == ["stake_count_kernel", "stake_goals_kernel"]
    assert "#pragma clang fp contract(off)" in body and "atomic" not in raw.lower()
    assert re.findall(r'#include "([^"]+)"', body) == ["../../include/fasterhip_stake.h"]
    for called in ("far_count_body(", "far_put_goal(", "far_head(", "far_team_words(", "prospect_words(", "prospect_body<true>(",
                   "FAR_WORDS", "ProspectArgs"):   # the far choosers' own, called
        assert called in body, called
    assert not re.search(r"__device__[^\n;{]*\b(far_judge|far_gap2|far_body|far_block_d2|far_passable|far_target|reach_before|prospect_weigh|"
                         r"prospect_before|prospect_store)\s*\(", body)   # not copied
    # the claim scan is the far chooser's, called by the gain chooser's body, and no loop of it stands here; the covered set is a seventh
    # bitmap, which this file holds
    shared = [strip(os.path.join(CSRC, f)) for f in ("fh_far.hip.hpp", "fh_prospect.hpp")]
    assert len(re.findall(r"\bfar_claim_scan\s*\(", shared[0])) == 1 and "far_claim_scan<true>(" in shared[1] and "far_claim_scan<false>(" in shared[0]
    assert not re.search(r"far_claim_scan|FarClaims|__ballot|rank_in|s_pts|s_cnt|s_cb|far_expand|far_summary|far_scan_block", body)
    assert "s_c[FAR_WORDS]" in body
    # what the far chooser's and the gain chooser's device headers define, no other file of the device code defines
    defined = lambda text: set(re.findall(r"__device__ __forceinline__ [^\n;{(]*?(\w+)\s*\(", text))   # noqa: E731
    helpers = defined(shared[0]) | defined(shared[1])
    assert {"far_start", "far_summary", "far_expand", "far_level_any", "far_scan_block", "far_put_goal", "far_head", "far_team_words",
            "far_count_body", "far_claim_scan", "far_body", "prospect_words", "prospect_weigh", "prospect_body"} <= helpers
    assert not defined(shared[0]) & defined(shared[1])
    for other in glob.glob(os.path.join(CSRC, "*")):
        if os.path.basename(other) not in ("fh_far.hip.hpp", "fh_prospect.hpp"):
            assert not helpers & defined(strip(other)), other
    # the entry points stand outside the spans the other choosers' tests cut out
    at = [host.index("static size_t bid_offers_offset"), host.index("size_t fh_prospect_work_bytes"), host.index("size_t fh_stake_work_bytes"),
          host.index("int fh_stake_goals_device"), host.index("int fh_prospect_goals_device"), host.index("int fh_apart_goals_device")]
    assert at == sorted(at)
    entry = host[at[3]:at[4]]
    launches = re.findall(r"hipLaunchKernelGGL\(fhp::(\w+)", entry)
    assert launches == ["far_need_kernel", "prospect_blocks_kernel", "far_spread_class_kernel", "stake_count_kernel", "stake_goals_kernel"]
    assert entry.count("hipMemsetAsync(") == 1 and entry.index("hipMemsetAsync(") < entry.index("hipLaunchKernelGGL")
    assert re.search(r"for \(int p = 1; p <= par->passes; p\+\+\) \{\s*k\.pass = p;\s*hipLaunchKernelGGL\(fhp::stake_goals_kernel", entry)
    assert "reach_table_clauses(" in entry and "reach_field_clauses(" in entry and "far_words(" in entry
    assert "static_assert" in entry and "offsetof(fh_stake_record, claimed) == offsetof(fh_apart_record, claimed)" in entry
    assert "offsetof(fh_stake_params, min_gain) == offsetof(fh_prospect_params, min_gain)" in entry
    with pytest.raises(capi.FasterHipError):
        capi.Map.far_team_goals_device(None, abi.default_far_spread_params(8, 2.0), None, None, 0, None, 1, None, None, None, 0, None, 0, None, None,
                                       None, None)


def grid(res=0.5, dims=(8, 8, 4)):
    g = np.zeros(1, dtype=abi.voxel_grid_dtype)
    g["origin"], g["res"], g["dims"] = (0.1, 0.2, 0.3), res, dims
    return g


def test_work_bytes_is_the_formula_and_zero_for_each_bad_argument(built):
    from faster_amd import capi

    wb, pro, apart = capi.lib().fh_stake_work_bytes, capi.lib().fh_prospect_work_bytes, capi.lib().fh_apart_work_bytes
    for dims in ((8, 8, 4), (13, 7, 3), (65, 1, 2), (64, 64, 8), (1, 1, 1), (1000, 900, 40), fa.OVER_CAP):
        for B in (1, 2, 3, 8, 16):
            for n_views in (1, 2, 63, 64, 65, 1000):
                for n in (0, 1, 63, 64, 65, 300):
                    W = fa.blocks_of(dims, B)[2]
                    want = 0 if W > 512 else n_views * 4 * W * 8 + ((n_views + 63) & ~63) + n_views * 64 * W * 2 + ((n + 63) & ~63) + n * 4 + n * 4
                    got = int(wb(abi.ptr(grid(dims=dims)), B, n_views, n))
                    assert got == want == ft.work_bytes(dims, B, n_views, n), (dims, B, n_views, n)
                    if want:
                        g = abi.ptr(grid(dims=dims))
                        assert want - int(pro(g, B, n_views)) == int(apart(g, B, n_views, n)) - int(capi.lib().fh_far_work_bytes(g, B, n_views))
                        assert int(pro(g, B, n_views)) % 8 == 0
    assert int(wb(None, 8, 1, 1)) == 0
    for dims in ((0, 8, 4), (8, 0, 4), (8, 8, 0), (-1, 8, 4)):
        assert int(wb(abi.ptr(grid(dims=dims)), 8, 1, 1)) == 0, dims
    for B in (0, -1, 17, 1 << 30, -(1 << 31)):
        assert int(wb(abi.ptr(grid()), B, 1, 1)) == 0, B
    for n_views in (0, -1, -(1 << 31)):
        assert int(wb(abi.ptr(grid()), 8, n_views, 1)) == 0, n_views
    for n in (-1, -(1 << 31)):
        assert int(wb(abi.ptr(grid()), 8, 1, n)) == 0, n
    big = (1 << 31) - 1
    assert int(wb(abi.ptr(grid(dims=(big, big, big))), 1, 1, 1)) == 0 and int(wb(abi.ptr(grid(dims=fa.OVER_CAP)), 1, 1, 1)) == 0
    assert int(wb(abi.ptr(grid()), 8, big, big)) == big * 4 * 8 + ((big + 63) & ~63) + big * 128 + ((big + 63) & ~63) + 8 * big   # nothing overflows


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
        p = np.ascontiguousarray(abi.default_far_team_params(8, 2.0, 2)).reshape(1).copy()
        for k, v in kw.items():
            p[k] = v
        return p

    need = 2 * 4 * 1 * 8 + 64 + 2 * 64 * 2 + 64 + 4 + 4   # n_views 2, W 1, n 1
    assert int(L.fh_stake_work_bytes(abi.ptr(grid()), 8, 2, 1)) == need
    good = dict(p=par(), mg=grid(res=0.3, dims=(9, 9, 5)), bits=d + 20480, g=grid(), flags=d, stride=256, view_of=None, n_views=2, skip=None,
                group=None, veh=d + 1024, n=1, work=d + 24576, work_bytes=need, goals=d + 4096, mask=d + 8192, rec=d + 12288)
    # the clauses in the stated order; `key` is the argument a clause reads, `tail` the fields of the params that LATER clauses read
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
        ("r_spread", "p", [par(r_spread=v) for v in (nan, inf, -inf, 0.0, -0.0, -1.0)]),
        ("passes", "p", [par(passes=v) for v in (0, -1, 65, 1 << 30, -(1 << 31))]),
        ("claim_blocks", "p", [par(claim_blocks=v) for v in (-1, 6, 1 << 30, -(1 << 31))]),
        ("work_bytes", "work_bytes", [need - 1, 0]),
    ]
    # the fields of the params that later clauses read, broken: the three tail fields come after the tables
    head = ["r_avoid", "z", "want", "max_hops", "block", "gain_blocks", "hop_cost", "min_gain"]
    head_break = dict(r_avoid=dict(r_avoid=nan), z=dict(z_lo=nan), want=dict(want=0), max_hops=dict(max_hops=-1), block=dict(block=0),
                      gain_blocks=dict(gain_blocks=-1), hop_cost=dict(hop_cost=-1), min_gain=dict(min_gain=-1))
    tail = ["r_spread", "passes", "claim_blocks"]
    tail_break = dict(r_spread=dict(r_spread=nan), passes=dict(passes=0), claim_blocks=dict(claim_blocks=-1))
    table_break = dict(mg=None, bits=None, g=None, stride=0, n_views=0, n=-1)
    table_order = ["mg", "bits", "g", "stride", "n_views", "n"]
    nothing = dict(flags=None, veh=None, goals=None, mask=None, rec=None, work=None)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        ptr = lambda x: None if x is None else abi.ptr(x)   # noqa: E731
        return L.fh_stake_goals_device(None, ptr(a["p"]), ptr(a["mg"]), a["bits"], ptr(a["g"]), a["flags"], a["stride"], a["view_of"],
                                       a["n_views"], a["skip"], a["group"], a["veh"], a["n"], a["work"], a["work_bytes"], a["goals"], a["mask"],
                                       a["rec"])

    for name, key, values in clauses:
        for v in values:
            alone, after = {}, {"work_bytes": 0}
            if key == "p" and v is not None:
                v = v.copy()
                later = (head[head.index(name) + 1:] + tail) if name in head else tail[tail.index(name) + 1:]
                for f in later:
                    for field, x in {**head_break, **tail_break}[f].items():
                        v[field] = x
            if name in head or name == "par":
                after.update(table_break)
            elif key in table_order:
                after.update({k: table_break[k] for k in table_order[table_order.index(key) + 1:]})
                after["p"] = par(r_spread=nan, passes=0, claim_blocks=-1)
            if name in ("grid", "cells"):
                after["stride"] = 0   # (smaller than any number of cells)
            if name == "cells":
                alone = dict(stride=1 << 62)
            if name == "words":   # every clause before it holds: a stride that covers the cells, and blocks of one voxel
                alone = dict(stride=1 << 40, p=par(block=1), work_bytes=1 << 40)
                after = dict(stride=1 << 40, work_bytes=0, p=par(block=1, r_spread=nan, passes=0, claim_blocks=-1))
            if name == "work_bytes":
                after = {}
            assert call(**{**alone, key: v}) == ARG, (name, v)                           # the clause alone
            assert call(**{**alone, **after, **nothing, key: v}) == ARG, (name, v)        # and with everything after it broken as well
            if key != "n" and not (name == "work_bytes" and v >= need - 72):   # (the workspace of n == 0 is 72 bytes smaller)
                assert call(**{**alone, **nothing, key: v, "n": 0}) == ARG, (name, v)    # n == 0 does not turn it into FH_OK
    # the order itself, seen from outside: what a broken clause hides.  With more words than the cap (clause "words") the tail fields
    # are not reached and FH_ERR_ARG stands whatever they hold; with the words in range each of them answers, also for n == 0
    for p in (par(r_spread=nan), par(passes=65), par(claim_blocks=6)):
        assert call(p=p, n=0) == ARG and call(p=p) == ARG
    for p in (par(gain_blocks=6), par(hop_cost=16385), par(min_gain=-1), par(block=0, gain_blocks=2)):
        assert call(p=p, mg=None, n=0) == ARG
    assert call(g=grid(dims=fa.OVER_CAP), stride=1 << 40, p=par(block=2), work_bytes=1 << 40, n=0) == OK
    assert call(work_bytes=need - 1) == ARG and call(work_bytes=need - 1, **nothing) == ARG
    assert call(work_bytes=need - 72, n=0, **nothing) == OK   # (the bytes depend on n: 64 class bytes and two words less for n == 0)
    assert call(work_bytes=need - 73, n=0, **nothing) == ARG
    # a workspace one byte short, at the cap
    full = 2 * 4 * 512 * 8 + 64 + 2 * 64 * 512 * 2 + 64 + 8
    assert call(g=grid(dims=(64, 64, 8)), stride=1 << 40, p=par(block=1), work_bytes=full, **nothing) == ARG           # (the pointers come last)
    assert call(g=grid(dims=(64, 64, 8)), stride=1 << 40, p=par(block=1), work_bytes=full) == DEVICE
    assert call(g=grid(dims=(64, 64, 8)), stride=1 << 40, p=par(block=1), work_bytes=full - 1) == ARG                  # one byte short
    assert call(g=grid(dims=(64, 64, 8)), stride=1 << 40, p=par(block=1), work_bytes=full - 72, n=0) == OK
    assert call(g=grid(dims=(64, 64, 8)), stride=1 << 40, p=par(block=1), work_bytes=full - 73, n=0) == ARG
    # every rule passes: n == 0 is fine without any pointer, then the pointers
    assert call(n=0, **nothing) == OK and call(n=0) == OK
    for k in nothing:
        assert call(**{k: None}) == ARG, k
    assert call(work_bytes=need + 1, n=0) == OK
    # the edges of the rules that pass: n == 0, so nothing is launched
    for p in (par(gain_blocks=0), par(gain_blocks=5), par(hop_cost=0), par(hop_cost=16384), par(min_gain=(1 << 31) - 1), par(r_avoid=1e300),
              par(z_lo=inf, z_hi=inf), par(block=16), par(block=1), par(reserved_d=nan), par(r_spread=1e-300), par(r_spread=1e300), par(passes=1),
              par(passes=64), par(claim_blocks=0), par(claim_blocks=5)):
        assert call(p=p, n=0, work_bytes=1 << 20) == OK
    # d_view_of, d_skip and d_group may be null or not; host memory is no place for the records
    assert call() == DEVICE and call(view_of=d + 16384, skip=d + 16640, group=d + 16896) == DEVICE
    assert L.fh_abi_version() == 9


def test_fleet_explore_far_team_raises_what_explore_far_spread_raises_before_any_launch(built):
    from faster_amd import capi
    from faster_amd.fleet import Fleet

    f = Fleet.__new__(Fleet)   # (no device here: only the checks that come before the first launch are reached)
    f.cloud = f.map_args = f.view_flags = f.flags = f.view_of = f.d_headings = f.grid = None
    f.d_reach_view_of = None
    f.d_far_goals = f.d_far_mask = f.d_far_records = f.d_far_work = f._far_work_key = None
    f.d_far_spread_goals = f.d_far_spread_mask = f.d_far_spread_records = f.d_far_spread_work = f._far_spread_work_key = None
    f.d_far_team_goals = f.d_far_team_mask = f.d_far_team_records = f.d_far_team_work = f._far_team_work_key = None
    f.d_explore_mask = f.d_reach_mask = f.d_spread_mask = f.d_gain_mask = f.d_sight_mask = f.d_team_mask = f.d_bid_mask = None
    f.d_link_labels = None
    f.map = f.ctx = None

    def both(match, *args, **kw):
        """explore_far_spread(block, r_spread, ...) and explore_far_team(block, r_spread, ...): the same words, but for the name."""
        said = []
        for method, name in ((f.explore_far_spread, "Fleet.explore_far_spread:"), (f.explore_far_team, "Fleet.explore_far_team:")):
            with pytest.raises(capi.FasterHipError, match=match) as e:
                method(8, 2.0, *args, **kw)
            assert str(e.value).startswith(name), str(e.value)
            said.append(str(e.value).replace(name, ""))
        assert said[0] == said[1]

    both("set_map")
    f.cloud, f.map_args = object(), ((10, 10, 4), 0.2, (0.0, 0.0, 1.0), 2.0, 0.0)
    both("set_unknown_views", want="all")
    with pytest.raises(capi.FasterHipError, match="explore_far_team first"):
        f.far_team_records()

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
    both("groups is", want="all", groups="team")
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(capi.FasterHipError, match="r_spread must be finite and > 0"):
            f.explore_far_team(8, bad, want="all")
    for bad in (0, -1, 65):
        with pytest.raises(capi.FasterHipError, match="passes must be None or 1 .. 64"):
            f.explore_far_team(8, 2.0, want="all", passes=bad)
    for kw, match in ((dict(gain_blocks=6), "gain_blocks must be 0 .. 5"), (dict(gain_blocks=-1), "gain_blocks must be"),
                      (dict(hop_cost=16385), "hop_cost must be None or 0 .. 16384"), (dict(hop_cost=-1), "hop_cost must be"),
                      (dict(min_gain=-1), "min_gain must be >= 0"), (dict(claim_blocks=6), "claim_blocks must be None or 0 .. 5"),
                      (dict(claim_blocks=-1), "claim_blocks must be")):
        with pytest.raises(capi.FasterHipError, match=match):
            f.explore_far_team(8, 2.0, want="all", **kw)
    f.grid = ((0.0, 0.0, 0.0), 0.5, fa.OVER_CAP)
    for block in (1, 0, 17):
        with pytest.raises(capi.FasterHipError, match="Fleet.explore_far_team: block must be"):
            f.explore_far_team(block, 2.0, want="all")
