"""CPU-side checks of fh_apart_goals_device: declared in include/fasterhip_apart.h and in no other header, the header compiles
alone as C99 and C++11, exported, bound in faster_amd/capi.py on Map and on Fleet, the struct layouts and the constants of the header
equal faster_amd/abi.py, FH_ABI_VERSION stays, the device code lives in fh_apart.hpp which fh_reach.hip alone includes, last,
with three kernels and no atomics, every clause of the prologue answers FH_ERR_ARG in the stated order (all of them come before the
first call of the runtime, so host pointers stand in for device pointers), fh_apart_work_bytes is the formula, a workspace one byte
short is refused, and Fleet.explore_far_spread raises explore_far()'s errors before any launch."""
import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from faster_amd import abi

import far_model as fa
import far_spread_model as fs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "faster_amd", "csrc")
HDR = os.path.join(INC, "fasterhip.h")
NEW_HDR = os.path.join(INC, "fasterhip_apart.h")
NEW = ["fh_apart_work_bytes", "fh_apart_goals_device"]
NAMES = r"fh_apart|fasterhip_apart|FH_APART|far_spread_goals|far_spread_record|far_spread_params|explore_far_spread"
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
        if os.path.basename(untouched) not in ("fh_reach.hip", "fh_far.hip.hpp", "fh_apart.hpp"):
            assert not re.search(NAMES, open(untouched).read()), untouched    # nor has any other file of the device code
    assert int(re.search(r"#define FH_ABI_VERSION (\d+)", open(HDR).read()).group(1)) == abi.FH_ABI_VERSION == 9
    text = open(NEW_HDR).read()
    assert re.findall(r'#include "([^"]+)"', text) == ["fasterhip.h", "fasterhip_frontier.h", "fasterhip_reach.h"]
    # (K21's header and the team chooser's keep their names to themselves: tests/test_far_abi.py and tests/test_spread_abi.py)
    assert not re.search(r"fh_spread|fasterhip_spread|FH_SPREAD|fh_far|fasterhip_far|FH_FAR|far_goals|far_record|far_params|explore_far", text)
    assert "n_views * 4 * W * 8 + ((n_views + 63) & ~63)" in text and "((n + 63) & ~63) class bytes + n int32 groups + n int32 `lower`" in text
    src = "#include \"fasterhip_apart.h\"\nint main(void) {\n" + "".join("  (void)%s;\n" % n for n in NEW) + "  return 0;\n}\n"
    for lang, std, comp in (("c", "-std=c99", "gcc"), ("c++", "-std=c++11", "g++")):
        f = tmp_path / ("probe." + ("c" if lang == "c" else "cpp"))
        f.write_text(src)
        r = subprocess.run([comp, "-fsyntax-only", "-x", lang, std, "-Wall", "-pedantic", "-I", INC, str(f)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr.strip(), (lang, r.stderr[-2000:])


def test_struct_layouts_and_constants_of_the_header_equal_abi_py(tmp_path):
    """sizeof and every offsetof of the two structs, printed by a C program compiled against the header."""
    structs = (("fh_apart_params", abi.far_spread_params_dtype, 96), ("fh_apart_record", abi.far_spread_record_dtype, 96),
               ("fh_far_params", abi.far_params_dtype, 64), ("fh_far_record", abi.far_record_dtype, 64))
    consts = ["FH_APART_UNSETTLED", "FH_APART_CLAIMED", "FH_APART_MAX_PASSES", "FH_APART_DEFAULT_PASSES", "FH_APART_SKIPPED", "FH_APART_MAX_WORDS", "FH_FAR_SKIPPED",
              "FH_FAR_MAX_WORDS", "FH_REACH_START_OUTSIDE", "FH_REACH_CUT", "FH_FRONTIER_WANTED", "FH_FRONTIER_FOUND", "FH_FRONTIER_NO_VIEW",
              "FH_FRONTIER_BAD_POS"]
    lines = []
    for name, dt, _ in structs:
        lines.append('  printf("%s.size %%d\\n", (int)sizeof(%s));' % (name, name))
        lines += ['  printf("%s.%s %%d\\n", (int)offsetof(%s, %s));' % (name, k, name, k) for k in dt.names]
    lines += ['  printf("%s %%d\\n", (int)%s);' % (k, k) for k in consts]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"fasterhip_far.h\"\n#include \"fasterhip_apart.h\"\nint main(void) {\n" + "\n".join(lines)
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
    assert [got[k] for k in consts[:6]] == [256, 512, 64, 8, 128, 512]
    assert [got[k] for k in consts[:6]] == [abi.FH_SPREAD_UNSETTLED, abi.FH_SPREAD_CLAIMED, abi.FH_SPREAD_MAX_PASSES, abi.FH_SPREAD_DEFAULT_PASSES,
                                            abi.FH_FAR_SKIPPED, abi.FH_FAR_MAX_WORDS]
    # the first 64 bytes of both are the structs of the chooser without claims, field for field
    for long, short in ((abi.far_spread_params_dtype, abi.far_params_dtype), (abi.far_spread_record_dtype, abi.far_record_dtype)):
        assert long.names[:len(short.names)] == short.names
        assert all(long.fields[k][:2] == short.fields[k][:2] for k in short.names)
    assert abi.far_spread_params_dtype.names[len(abi.far_params_dtype.names):] == ("r_spread", "passes", "reserved_tail")
    assert abi.far_spread_record_dtype.names[len(abi.far_record_dtype.names):] == ("group", "decided_pass", "lower", "standing", "claims", "claimed",
                                                                                  "reserved_tail")
    assert abi.far_spread_params_dtype.fields["r_spread"][1] == 64 and abi.far_spread_record_dtype.fields["group"][1] == 64
    # the new flags are bits of their own beside the ones they stand with
    others = [got[k] for k in consts[6:] if k != "FH_FAR_MAX_WORDS"] + [abi.FH_REACH_BOX_TOO_LARGE]
    assert all(got[f] & o == 0 for f in consts[:2] for o in others) and got[consts[0]] & got[consts[1]] == 0
    p = abi.default_far_spread_params(8, 2.5)
    assert (float(p["r_avoid"]), float(p["z_lo"]), float(p["z_hi"]), float(p["reserved_d"]), int(p["want"]), int(p["max_hops"]), int(p["block"]),
            float(p["r_spread"]), int(p["passes"])) == (0.0, -np.inf, np.inf, 0.0, abi.FH_FRONTIER_WANT_REACHED, 0, 8, 2.5, abi.FH_APART_DEFAULT_PASSES)
    assert not p["reserved"].any() and not p["reserved_tail"].any()


def test_the_symbols_are_exported_and_bound_and_the_device_code_is_included_by_fh_reach_hip_alone(built):
    from faster_amd import capi
    from faster_amd.fleet import Fleet

    L = ctypes.CDLL(built.SO)
    for name in NEW:
        assert hasattr(L, name), name
    assert capi.FAR_SPREAD_SYMBOLS == NEW
    lists = [k for k in dir(capi) if k.endswith("SYMBOLS") and k != "FAR_SPREAD_SYMBOLS"]
    assert len(lists) >= 19 and "SYMBOLS" in lists and "FAR_SYMBOLS" in lists and "SPREAD_SYMBOLS" in lists
    for k in lists:
        assert not set(NEW) & set(getattr(capi, k)), k
    assert len(capi.lib().fh_apart_goals_device.argtypes) == 18 and capi.lib().fh_apart_goals_device.restype == ctypes.c_int32
    assert capi.lib().fh_apart_work_bytes.restype == ctypes.c_size_t and len(capi.lib().fh_apart_work_bytes.argtypes) == 4
    assert hasattr(capi.Map, "far_spread_goals_device")
    for name in ("explore_far_spread", "explore_far_spread_stages", "far_spread_records"):
        assert hasattr(Fleet, name), name
    assert os.path.join(CSRC, "fh_apart.hpp") in built.DEPS
    assert built.SOURCES[-1] == os.path.join(CSRC, "fh_reach.hip") and len(built.SOURCES) == 4
    assert "capi.FAR_SPREAD_SYMBOLS" in open(os.path.join(ROOT, "__graft_entry__.py")).read()   # build() touches the new symbols
    assert capi.lib().fh_abi_version() == 9
    strip = lambda path: re.sub(r"//[^\n]*", "", open(path).read())   # noqa: E731
    for other in glob.glob(os.path.join(CSRC, "*")):
        if os.path.basename(other) != "fh_reach.hip":
            assert "fh_apart.hpp" not in strip(other), other
    host = strip(os.path.join(CSRC, "fh_reach.hip"))
    includes = re.findall(r'#include "([^"]+)"', host)
    assert includes[-1] == "fh_apart.hpp" and includes.index("fh_far.hip.hpp") < len(includes) - 1   # last, behind the body it calls
    body = strip(os.path.join(CSRC, "fh_apart.hpp"))
    assert sorted(set(re.findall(r"\b(\w+_kernel)\s*\(", body))) == ["far_spread_class_kernel", "far_spread_count_kernel", "far_spread_goals_kernel"]
    assert "#pragma clang fp contract(off)" in body and "atomic" not in body.lower()
    assert re.findall(r'#include "([^"]+)"', body) == ["../../include/fasterhip_apart.h"]
    for called in ("far_body<true>(", "far_judge(", "far_count_body(", "far_put_goal(", "far_head(", "far_team_words("):   # the chooser's own, called
        assert called in body, called
    assert not re.search(r"__device__[^\n;{]*\b(far_judge|far_gap2|far_body|far_block_d2|far_count_body|far_claim_scan|far_put_goal|far_head|"
                         r"far_team_words)\s*\(", body)   # not copied
    assert not re.search(r"far_gap2|__ballot|rank_in|s_pts|s_cnt", body)   # the claim scan stands in the chooser's device header, behind far_body<true>
    assert "far_claim_scan<false>(" in strip(os.path.join(CSRC, "fh_far.hip.hpp"))
    far = strip(os.path.join(CSRC, "fh_far.hip.hpp"))
    assert "far_goals_kernel(FarArgs a) { far_body<false>(a, FarNoClaims()); }" in far
    # the entry points stand behind fh_far_goals_device; the summary stage is that chooser's: its memset and its two launches
    at = [host.index("int fh_far_goals_device"), host.index("size_t fh_apart_work_bytes"), host.index("int fh_apart_goals_device"),
          host.index("int fh_bid_goals_device")]
    assert at == sorted(at)
    entry = host[at[2]:at[3]]
    assert re.findall(r"hipLaunchKernelGGL\(fhp::(\w+)", entry) == ["far_need_kernel", "far_blocks_kernel", "far_spread_class_kernel",
                                                                     "far_spread_count_kernel", "far_spread_goals_kernel"]
    assert entry.count("hipMemsetAsync(") == 1 and entry.index("hipMemsetAsync(") < entry.index("hipLaunchKernelGGL")
    assert "reach_table_clauses(" in entry and "reach_field_clauses(" in entry
    with pytest.raises(capi.FasterHipError):
        capi.Map.far_spread_goals_device(None, abi.default_far_params(8), None, None, 0, None, 1, None, None, None, 0, None, 0, None, None, None, None)


def grid(res=0.5, dims=(8, 8, 4)):
    g = np.zeros(1, dtype=abi.voxel_grid_dtype)
    g["origin"], g["res"], g["dims"] = (0.1, 0.2, 0.3), res, dims
    return g


def test_work_bytes_is_the_formula_and_zero_for_each_bad_argument(built):
    from faster_amd import capi

    wb, far = capi.lib().fh_apart_work_bytes, capi.lib().fh_far_work_bytes
    for dims in ((8, 8, 4), (13, 7, 3), (65, 1, 2), (64, 64, 8), (1, 1, 1), fa.OVER_CAP):
        for B in (1, 2, 8, 16):
            for n_views in (1, 64, 65):
                for n in (0, 1, 63, 64, 65, 1000):
                    base = int(far(abi.ptr(grid(dims=dims)), B, n_views))
                    want = 0 if base == 0 else base + ((n + 63) & ~63) + 4 * n + 4 * n
                    assert int(wb(abi.ptr(grid(dims=dims)), B, n_views, n)) == want == fs.work_bytes(dims, B, n_views, n), (dims, B, n_views, n)
    assert int(wb(abi.ptr(grid(dims=(64, 64, 8))), 1, 1, 3)) == 4 * 512 * 8 + 64 + 64 + 12 + 12
    assert int(wb(abi.ptr(grid()), 8, 1, 0)) == 4 * 8 + 64 and int(wb(abi.ptr(grid()), 8, 1, 0)) % 8 == 0
    assert int(wb(abi.ptr(grid(dims=fa.OVER_CAP)), 1, 1, 3)) == 0   # W = 513
    assert int(wb(None, 8, 1, 3)) == 0
    for dims in ((0, 8, 4), (8, 0, 4), (8, 8, 0), (-1, 8, 4)):
        assert int(wb(abi.ptr(grid(dims=dims)), 8, 1, 3)) == 0, dims
    for B in (0, -1, 17, 1 << 30, -(1 << 31)):
        assert int(wb(abi.ptr(grid()), B, 1, 3)) == 0, B
    for n_views in (0, -1, -(1 << 31)):
        assert int(wb(abi.ptr(grid()), 8, n_views, 3)) == 0, n_views
    for n in (-1, -(1 << 31)):
        assert int(wb(abi.ptr(grid()), 8, 1, n)) == 0, n
    big = (1 << 31) - 1
    assert int(wb(abi.ptr(grid(dims=(big, big, big))), 1, 1, big)) == 0
    assert int(wb(abi.ptr(grid()), 8, big, big)) == big * 4 * 8 + ((big + 63) & ~63) + ((big + 63) & ~63) + 8 * big   # nothing overflows


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
        p = np.ascontiguousarray(abi.default_far_spread_params(8, 2.0)).reshape(1).copy()
        for k, v in kw.items():
            p[k] = v
        return p

    need = 2 * 4 * 1 * 8 + 64 + 64 + 4 + 4   # n_views 2, W 1, n 1
    assert int(L.fh_apart_work_bytes(abi.ptr(grid()), 8, 2, 1)) == need
    good = dict(p=par(), mg=grid(res=0.3, dims=(9, 9, 5)), bits=d + 20480, g=grid(), flags=d, stride=256, view_of=None, n_views=2, skip=None,
                group=None, veh=d + 1024, n=1, work=d + 24576, work_bytes=need, goals=d + 4096, mask=d + 8192, rec=d + 12288)
    clauses = [
        ("par", "p", [None]),
        ("r_avoid", "p", [par(r_avoid=v) for v in (nan, inf, -inf, -1e-300, -1.0)]),
        ("z", "p", [par(z_lo=lo, z_hi=hi) for lo, hi in ((nan, 1.0), (0.0, nan), (nan, nan), (1.0, 0.5), (inf, -inf))]),
        ("want", "p", [par(want=v) for v in (0, 8, 9, 16, -1, 1 << 30)]),
        ("max_hops", "p", [par(max_hops=v) for v in (-1, -(1 << 31))]),
        ("block", "p", [par(block=v) for v in (0, -1, 17, 1 << 30, -(1 << 31))]),
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
        ("r_spread", "p2", [dict(r_spread=v) for v in (nan, inf, -inf, 0.0, -0.0, -1.0)]),
        ("passes", "p2", [dict(passes=v) for v in (0, -1, 65, 1 << 30, -(1 << 31))]),
        ("work_bytes", "work_bytes", [need - 1, 0]),
    ]
    # what breaks a clause together with every clause after it (the params record carries seven clauses: the later fields broken too)
    broken_after = {"p": None, "mg": None, "bits": None, "g": None, "stride": 0, "n_views": 0, "n": -1, "p2": None, "work_bytes": 0}
    tail = dict(r_spread=nan, passes=0)
    later_fields = {"r_avoid": dict(z_lo=nan, want=0, max_hops=-1, block=0, **tail), "z": dict(want=0, max_hops=-1, block=0, **tail),
                    "want": dict(max_hops=-1, block=0, **tail), "max_hops": dict(block=0, **tail), "block": dict(**tail), "r_spread": dict(passes=0),
                    "passes": {}}
    nothing = dict(flags=None, veh=None, goals=None, mask=None, rec=None, work=None)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        a.pop("p2", None)
        ptr = lambda x: None if x is None else abi.ptr(x)   # noqa: E731
        return L.fh_apart_goals_device(None, ptr(a["p"]), ptr(a["mg"]), a["bits"], ptr(a["g"]), a["flags"], a["stride"], a["view_of"],
                                            a["n_views"], a["skip"], a["group"], a["veh"], a["n"], a["work"], a["work_bytes"], a["goals"], a["mask"],
                                            a["rec"])

    order = ["p", "mg", "bits", "g", "stride", "n_views", "n", "p2", "work_bytes"]
    for name, key, values in clauses:
        after = {k: broken_after[k] for k in order[order.index(key) + 1:] if k != "p2"}
        for v in values:
            alone = {}
            base = par(block=1) if name == "words" else par()
            if key == "p2":   # the tail of the params record: every clause of its head, and of the tables, holds
                v, key_ = par(**v, **later_fields[name]), "p"
            else:
                key_ = key
                if key == "p" and v is not None:
                    v = v.copy()
                    for f, x in later_fields[name].items():
                        v[f] = x
                elif key != "p" and order.index(key) < order.index("p2"):   # a clause of the tables: the record's tail is broken with what follows
                    broken = base.copy()
                    broken["r_spread"], broken["passes"] = nan, 0
                    after["p"] = broken
            if name in ("grid", "cells"):
                after["stride"] = 0   # (smaller than any number of cells)
            if name == "cells":
                alone = dict(stride=1 << 62)
            if name == "words":   # every clause before it holds: a stride that covers the cells, and blocks of one voxel
                alone = dict(stride=1 << 40, p=par(block=1), work_bytes=1 << 40)
                after = dict(stride=1 << 40, p=after["p"], work_bytes=0)
            assert call(**{**alone, key_: v}) == ARG, (name, v)                           # the clause alone
            assert call(**{**alone, **after, **nothing, key_: v}) == ARG, (name, v)        # and with everything after it broken as well
            if key != "n" and not (key == "work_bytes" and v >= 128):   # (the bytes depend on n: 128 are enough for n == 0)
                assert call(**{**alone, **nothing, key_: v, "n": 0}) == ARG, (name, v)    # n == 0 does not turn it into FH_OK
    # the order itself: a broken clause hides every later one but none before it — W > FH_FAR_MAX_WORDS comes before r_spread, r_spread
    # before passes, passes before work_bytes, work_bytes before n == 0, n == 0 before the pointers
    assert call(g=grid(dims=fa.OVER_CAP), stride=1 << 40, p=par(block=2, r_spread=nan), work_bytes=1 << 40, n=0) == ARG
    assert call(g=grid(dims=fa.OVER_CAP), stride=1 << 40, p=par(block=2), work_bytes=1 << 40, n=0) == OK
    assert call(work_bytes=need - 1) == ARG and call(work_bytes=need - 1, n=0, **nothing) == OK   # (n == 0 needs no class byte)
    assert call(work_bytes=127, n=0) == ARG and call(work_bytes=128, n=0, **nothing) == OK
    # a workspace one byte short, at the cap
    full = 2 * 4 * 512 * 8 + 64 + 64 + 8
    assert call(g=grid(dims=(64, 64, 8)), stride=1 << 40, p=par(block=1), work_bytes=full, **nothing) == ARG           # (the pointers come last)
    assert call(g=grid(dims=(64, 64, 8)), stride=1 << 40, p=par(block=1), work_bytes=full) == DEVICE
    assert call(g=grid(dims=(64, 64, 8)), stride=1 << 40, p=par(block=1), work_bytes=full - 1) == ARG                  # one byte short
    assert call(g=grid(dims=(64, 64, 8)), stride=1 << 40, p=par(block=1), work_bytes=full - 1, n=0) == OK              # (n == 0: no class bytes)
    assert call(g=grid(dims=(64, 64, 8)), stride=1 << 40, p=par(block=1), work_bytes=2 * 4 * 512 * 8 + 63, n=0) == ARG
    # every rule passes: n == 0 is fine without any pointer, then the pointers
    assert call(n=0, **nothing) == OK and call(n=0) == OK
    for k in nothing:
        assert call(**{k: None}) == ARG, k
    assert call(work_bytes=need + 1, n=0) == OK
    # the edges of the rules that pass: n == 0, so nothing is launched
    for p in (par(r_spread=5e-324), par(r_spread=1e300), par(passes=1), par(passes=64), par(r_avoid=1e300), par(z_lo=inf, z_hi=inf),
              par(block=16), par(reserved_d=nan)):
        assert call(p=p, n=0, work_bytes=1 << 20) == OK
    # d_view_of, d_skip and d_group may be null or not; host memory is no place for the records
    assert call() == DEVICE and call(view_of=d + 16384, skip=d + 16640, group=d + 16896) == DEVICE
    assert L.fh_abi_version() == 9


def test_fleet_explore_far_spread_raises_what_explore_far_raises_before_any_launch(built):
    from faster_amd import capi
    from faster_amd.fleet import Fleet

    f = Fleet.__new__(Fleet)   # (no device here: only the checks that come before the first launch are reached)
    f.cloud = f.map_args = f.view_flags = f.flags = f.view_of = f.d_headings = f.grid = None
    f.d_reach_view_of = None
    f.d_far_goals = f.d_far_mask = f.d_far_records = f.d_far_work = f._far_work_key = None
    f.d_far_spread_goals = f.d_far_spread_mask = f.d_far_spread_records = f.d_far_spread_work = f._far_spread_work_key = None
    f.d_explore_mask = f.d_reach_mask = f.d_spread_mask = f.d_gain_mask = f.d_sight_mask = f.d_team_mask = f.d_bid_mask = None
    f.d_link_labels = None
    f.map = f.ctx = None

    def both(match, *args, **kw):
        """explore_far(block, ...) and explore_far_spread(block, r_spread, ...): the same words, but for the name."""
        said = []
        for method, name, first in ((f.explore_far, "Fleet.explore_far:", (8,)), (f.explore_far_spread, "Fleet.explore_far_spread:", (8, 2.0))):
            with pytest.raises(capi.FasterHipError, match=match) as e:
                method(*first, *args, **kw)
            assert str(e.value).startswith(name), str(e.value)
            said.append(str(e.value).replace(name, ""))
        assert said[0] == said[1]

    both("set_map")
    f.cloud, f.map_args = object(), ((10, 10, 4), 0.2, (0.0, 0.0, 1.0), 2.0, 0.0)
    both("set_unknown_views", want="all")
    with pytest.raises(capi.FasterHipError, match="explore_far_spread first"):
        f.far_spread_records()

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
    with pytest.raises(capi.FasterHipError, match="groups is"):
        f.explore_far_spread(8, 2.0, want="all", groups="team")
    f.grid = ((0.0, 0.0, 0.0), 0.5, fa.OVER_CAP)
    for block in (1, 0, 17):
        with pytest.raises(capi.FasterHipError, match="Fleet.explore_far_spread: block must be"):
            f.explore_far_spread(block, 2.0, want="all")
