"""CPU-side checks of the listed views' entry points (fh_map_view_list_device, fh_map_read_views_listed_device): declared in
include/fasterhip_view_subset.h and not in fasterhip.h, the header compiles alone as C99 and C++11, exported, bound in
faster_amd/capi.py and on Fleet, FH_ABI_VERSION stays, and a null map is an argument error (there is no CPU path)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from faster_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "fasterhip.h")
SUBSET_HDR = os.path.join(INC, "fasterhip_view_subset.h")
NEW = ["fh_map_view_list_device", "fh_map_read_views_listed_device"]
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
    assert set(NEW) == _declared(SUBSET_HDR)
    assert not set(NEW) & _declared(HDR)   # fasterhip.h is pinned to capi.SYMBOLS (tests/test_abi.py): the new ones stay out of it
    assert int(re.search(r"#define FH_ABI_VERSION (\d+)", open(HDR).read()).group(1)) == abi.FH_ABI_VERSION == 9
    src = "#include \"fasterhip_view_subset.h\"\nint main(void) {\n" + "".join("  (void)%s;\n" % n for n in NEW) + "  return 0;\n}\n"
    for lang, std, comp in (("c", "-std=c99", "gcc"), ("c++", "-std=c++11", "g++")):
        f = tmp_path / ("probe." + ("c" if lang == "c" else "cpp"))
        f.write_text(src)
        r = subprocess.run([comp, "-fsyntax-only", "-x", lang, std, "-Wall", "-pedantic", "-I", INC, str(f)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr.strip(), (lang, r.stderr[-2000:])


def test_symbols_are_exported_and_bound(built):
    from faster_amd import capi
    from faster_amd.fleet import Fleet

    L = ctypes.CDLL(built.SO)
    for name in NEW:
        assert hasattr(L, name), name
    assert sorted(capi.VIEW_SUBSET_SYMBOLS) == sorted(NEW)
    others = (set(capi.SYMBOLS) | set(capi.OCCUPANCY_SYMBOLS) | set(capi.CERTIFY_SYMBOLS) | set(capi.AUDIT_SYMBOLS) | set(capi.SEPARATION_SYMBOLS)
              | set(capi.TRAFFIC_SYMBOLS) | set(capi.TRAFFIC_TIMED_SYMBOLS) | set(capi.CHECK_SYMBOLS) | set(capi.ROUNDS_SYMBOLS))
    assert not set(NEW) & others
    for name in ("view_list_device", "read_views_listed_device"):
        assert hasattr(capi.Map, name), name
    for name in ("enable_listed_views", "view_lists"):
        assert hasattr(Fleet, name), name
    assert SUBSET_HDR in built.DEPS   # (a change of the header rebuilds the library)
    assert os.path.join(ROOT, "faster_amd", "csrc", "fh_view_subset.hip.hpp") in built.DEPS


def test_a_null_map_is_an_argument_error(built):
    from faster_amd import capi

    L = capi.lib()
    buf = np.zeros(64, dtype=np.int32)
    cells, center = np.array([4, 4, 4], dtype=np.int32), np.zeros(3)
    d = abi.ptr(buf)
    assert L.fh_map_view_list_device(None, None, None, 1, 1, d, d) == ARG
    assert L.fh_map_read_views_listed_device(None, None, 0, None, 0, 1, abi.ptr(cells), 0.5, abi.ptr(center), 0.0, 3.0, 0.5, d, d) == ARG
    assert L.fh_abi_version() == 9


def test_the_kernels_come_last_in_the_map_code_object():
    """fh_view_subset.hip.hpp is included after fh_path.hip.hpp and defines no kernel of another header again."""
    text = open(os.path.join(ROOT, "faster_amd", "csrc", "fh_map.hip")).read()
    assert text.index('#include "fh_path.hip.hpp"') < text.index('#include "fh_view_subset.hip.hpp"')
    sub = open(os.path.join(ROOT, "faster_amd", "csrc", "fh_view_subset.hip.hpp")).read()
    kernels = re.findall(r"\b(\w+_kernel)\s*\(", sub)
    assert sorted(kernels) == ["clear_views_listed_kernel", "jps_table_views_listed_kernel", "mark_views_listed_kernel", "view_compact_kernel",
                               "view_flag_kernel"]
    path = open(os.path.join(ROOT, "faster_amd", "csrc", "fh_path.hip.hpp")).read()
    assert not set(kernels) & set(re.findall(r"\b(\w+_kernel)\s*\(", path))
