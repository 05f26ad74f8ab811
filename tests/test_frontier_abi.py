"""CPU-side checks of the frontier entry points (fh_map_frontier_goals_device, fh_map_view_coverage_device): declared in
include/fasterhip_frontier.h and in no other header, the header compiles alone as C99 and C++11, exported, bound in faster_amd/capi.py
on Map and on Fleet, the struct layouts and the constants of the header equal faster_amd/abi.py, FH_ABI_VERSION stays, fh_capi.hip and
fasterhip.h know nothing of it, the kernels come last in fh_map.hip's code object, and a null map is an argument error (a map cannot be
created without a device: the other clauses of the prologues are tested in tests/test_gpu_frontier.py)."""
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
NEW_HDR = os.path.join(INC, "fasterhip_frontier.h")
NEW = ["fh_map_frontier_goals_device", "fh_map_view_coverage_device"]
ARG = -1


@pytest.fixture(scope="module")
def built():
    from faster_amd import build as fb

    fb.build_all()
    return fb


def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(fh_[a-z_0-9]+)\s*\(", text))


def test_entry_points_are_declared_in_their_own_header_which_compiles_alone(tmp_path):
    assert set(NEW) == _declared(NEW_HDR)
    for other in glob.glob(os.path.join(INC, "*.h")):
        if other != NEW_HDR:
            assert not set(NEW) & _declared(other), other
    assert "frontier" not in open(HDR).read().lower()                              # nothing was added to fasterhip.h, not even a comment
    assert "frontier" not in open(os.path.join(CSRC, "fh_capi.hip")).read().lower()   # and fh_capi.hip is not touched
    assert int(re.search(r"#define FH_ABI_VERSION (\d+)", open(HDR).read()).group(1)) == abi.FH_ABI_VERSION == 9
    src = "#include \"fasterhip_frontier.h\"\nint main(void) {\n" + "".join("  (void)%s;\n" % n for n in NEW) + "  return 0;\n}\n"
    for lang, std, comp in (("c", "-std=c99", "gcc"), ("c++", "-std=c++11", "g++")):
        f = tmp_path / ("probe." + ("c" if lang == "c" else "cpp"))
        f.write_text(src)
        r = subprocess.run([comp, "-fsyntax-only", "-x", lang, std, "-Wall", "-pedantic", "-I", INC, str(f)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr.strip(), (lang, r.stderr[-2000:])


def test_struct_layouts_and_constants_of_the_header_equal_abi_py(tmp_path):
    """sizeof and every offsetof of the three structs, printed by a C program compiled against the header."""
    structs = (("fh_frontier_params", abi.frontier_params_dtype, 64), ("fh_frontier_record", abi.frontier_record_dtype, 32),
               ("fh_view_coverage", abi.view_coverage_dtype, 16))
    consts = ["FH_FRONTIER_WANT_REACHED", "FH_FRONTIER_WANT_NO_PATH", "FH_FRONTIER_WANT_ALL", "FH_FRONTIER_WANTED", "FH_FRONTIER_FOUND",
              "FH_FRONTIER_NO_VIEW", "FH_FRONTIER_BAD_POS"]
    lines = []
    for name, dt, _ in structs:
        lines.append('  printf("%s.size %%d\\n", (int)sizeof(%s));' % (name, name))
        lines += ['  printf("%s.%s %%d\\n", (int)offsetof(%s, %s));' % (name, k, name, k) for k in dt.names]
    lines += ['  printf("%s %%d\\n", (int)%s);' % (k, k) for k in consts]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"fasterhip_frontier.h\"\nint main(void) {\n" + "\n".join(lines)
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
    assert [getattr(abi, k) for k in consts] == [1, 2, 4, 1, 2, 4, 8]
    p = abi.default_frontier_params(2.5)
    assert (float(p["r_max"]), float(p["r_avoid"]), float(p["z_lo"]), float(p["z_hi"]), int(p["want"])) == \
        (2.5, 0.0, -np.inf, np.inf, abi.FH_FRONTIER_WANT_REACHED) and not p["reserved"].any()


def test_symbols_are_exported_and_bound(built):
    from faster_amd import capi
    from faster_amd.fleet import Fleet

    L = ctypes.CDLL(built.SO)
    for name in NEW:
        assert hasattr(L, name), name
    assert sorted(capi.FRONTIER_SYMBOLS) == sorted(NEW)
    lists = [k for k in dir(capi) if k.endswith("SYMBOLS") and k != "FRONTIER_SYMBOLS"]
    assert len(lists) >= 11 and "SYMBOLS" in lists and "LINK_SYMBOLS" in lists
    for k in lists:
        assert not set(NEW) & set(getattr(capi, k)), k
    for name in ("frontier_goals_device", "view_coverage_device"):
        assert hasattr(capi.Map, name), name
    for name in ("explore", "explore_stages", "explore_records", "coverage"):
        assert hasattr(Fleet, name), name
    assert NEW_HDR in built.DEPS   # (a change of the header rebuilds the library)
    assert os.path.join(CSRC, "fh_frontier.hip.hpp") in built.DEPS
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "capi.FRONTIER_SYMBOLS" in entry   # build() touches the new symbols
    assert capi.lib().fh_abi_version() == 9


def test_the_kernels_come_last_in_the_maps_code_object():
    """fh_frontier.hip.hpp is included by fh_map.hip only, after fh_view_subset.hip.hpp, and defines no kernel of the headers before it."""
    text = open(os.path.join(CSRC, "fh_map.hip")).read()
    device = re.findall(r'#include "(fh_\w+\.hip\.hpp)"', text)
    assert device == ["fh_path.hip.hpp", "fh_view_subset.hip.hpp", "fh_frontier.hip.hpp"]
    for other in glob.glob(os.path.join(CSRC, "*")):
        if os.path.basename(other) != "fh_map.hip":
            assert "fh_frontier.hip.hpp" not in re.sub(r"//[^\n]*", "", open(other).read()), other
    body = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "fh_frontier.hip.hpp")).read())
    kernels = sorted(set(re.findall(r"\b(\w+_kernel)\s*\(", body)))
    assert kernels == ["frontier_goals_kernel", "view_coverage_kernel"]
    for other in ("fh_path.hip.hpp", "fh_view_subset.hip.hpp"):
        theirs = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, other)).read())
        assert not set(kernels) & set(re.findall(r"\b(\w+_kernel)\s*\(", theirs)), other
    assert "#pragma clang fp contract(off)" in body


def test_a_null_map_is_an_argument_error(built):
    from faster_amd import capi

    L = capi.lib()
    buf = np.zeros(4096, dtype=np.uint8)
    d = abi.ptr(buf)
    par = np.ascontiguousarray(abi.default_frontier_params(1.0)).reshape(1)
    g = np.zeros(1, dtype=abi.voxel_grid_dtype)
    g["origin"], g["res"], g["dims"] = (0.0, 0.0, 0.0), 0.5, (4, 4, 4)
    assert L.fh_map_frontier_goals_device(None, abi.ptr(par), abi.ptr(g), d, 64, None, 1, d, 1, d, d, d) == ARG
    assert L.fh_map_frontier_goals_device(None, None, None, None, 0, None, 0, None, -1, None, None, None) == ARG
    assert L.fh_map_view_coverage_device(None, abi.ptr(g), d, 64, 1, d) == ARG
    assert L.fh_map_view_coverage_device(None, None, None, 0, 0, None) == ARG
    with pytest.raises(capi.FasterHipError):
        capi.Map.frontier_goals_device(None, np.zeros(4), None, None, 0, None, 1, None, 0, None, None, None)   # not a params record


def test_fleet_explore_without_views_raises():
    """Before any launch: explore needs a map and views (or set_unknown's one grid), "reached" needs headings, want must be known."""
    from faster_amd import capi
    from faster_amd.fleet import Fleet

    f = Fleet.__new__(Fleet)   # (no device here: only the checks that come before the first launch are reached)
    f.cloud = f.map_args = f.view_flags = f.flags = f.view_of = f.d_headings = f.grid = None
    f.d_explore_goals = f.d_explore_view_of = f.d_coverage = None
    f.map = f.ctx = None
    with pytest.raises(capi.FasterHipError, match="set_map"):
        f.explore(2.0)
    f.cloud, f.map_args = object(), ((10, 10, 4), 0.2, (0.0, 0.0, 1.0), 2.0, 0.0)
    with pytest.raises(capi.FasterHipError, match="set_unknown_views"):
        f.explore(2.0, want="all")
    with pytest.raises(capi.FasterHipError, match="set_unknown_views"):
        f.coverage()
    with pytest.raises(capi.FasterHipError, match="explore first"):
        f.explore_records()

    class Flags:   # stands in for the tensor of the views
        shape = (3, 100)

    f.view_flags, f.n_views, f.n = Flags(), 3, 3
    f.grid = ((0.0, 0.0, 0.0), 0.5, (5, 5, 4))
    with pytest.raises(capi.FasterHipError, match="enable_heading"):
        f.explore(2.0)
    with pytest.raises(capi.FasterHipError, match="enable_heading"):
        f.explore(2.0, want=("no_path", "reached"))
    for bad in ("arrived", (), ("all", "none")):
        with pytest.raises(capi.FasterHipError, match="want"):
            f.explore(2.0, want=bad)
