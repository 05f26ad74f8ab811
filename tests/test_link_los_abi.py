"""CPU-side checks of fh_fleet_link_groups_los_device: declared in include/fasterhip_link_los.h and in no other header, the header compiles
alone as C99 and C++11 and adds no struct or constant, exported, bound in faster_amd/capi.py and on Fleet, FH_ABI_VERSION stays, the two
new kernels lie behind every kernel of before, and every FH_ERR_ARG clause that can be reached without a device in the stated order (a
map that holds no grid and a range of more than 4096 cells need a map, which needs a device: tests/test_gpu_link_los.py)."""
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
LINK_HDR = os.path.join(INC, "fasterhip_link.h")
NEW_HDR = os.path.join(INC, "fasterhip_link_los.h")
NEW = ["fh_fleet_link_groups_los_device"]
OK, ARG, DEV = 0, -1, -2


@pytest.fixture(scope="module")
def built():
    from faster_amd import build as fb

    fb.build_all()
    return fb


def _code(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def _declared(path):
    return set(re.findall(r"\b(fh_[a-z_0-9]+)\s*\(", _code(path)))


def test_the_entry_point_is_declared_in_its_own_header_which_compiles_alone(tmp_path):
    assert set(NEW) == _declared(NEW_HDR)
    for other in sorted(os.listdir(INC)):
        if other != "fasterhip_link_los.h":
            assert not set(NEW) & _declared(os.path.join(INC, other)), other
    code = _code(NEW_HDR)
    assert re.findall(r'#include "([^"]+)"', code) == ["fasterhip_link.h"]
    assert "struct fh_" not in code.replace("struct fh_voxel_grid", "") and "enum" not in code and "typedef" not in code   # fh_link_params is reused
    assert int(re.search(r"#define FH_ABI_VERSION (\d+)", open(HDR).read()).group(1)) == abi.FH_ABI_VERSION == 9
    src = "#include \"fasterhip_link_los.h\"\nint main(void) {\n" + "".join("  (void)%s;\n" % n for n in NEW) + "  (void)fh_fleet_link_merge_device;\n  return 0;\n}\n"
    for lang, std, comp in (("c", "-std=c99", "gcc"), ("c++", "-std=c++11", "g++")):
        f = tmp_path / ("probe." + ("c" if lang == "c" else "cpp"))
        f.write_text(src)
        r = subprocess.run([comp, "-fsyntax-only", "-x", lang, std, "-Wall", "-pedantic", "-I", INC, str(f)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr.strip(), (lang, r.stderr[-2000:])


def test_the_symbol_is_exported_and_bound(built):
    import inspect

    from faster_amd import capi
    from faster_amd.fleet import Fleet

    L = ctypes.CDLL(built.SO)
    for name in NEW:
        assert hasattr(L, name), name
    assert capi.LINK_LOS_SYMBOLS == NEW
    lists = [k for k in dir(capi) if k.endswith("SYMBOLS") and k != "LINK_LOS_SYMBOLS"]
    assert len(lists) >= 22 and "LINK_SYMBOLS" in lists
    for k in lists:
        assert not set(NEW) & set(getattr(capi, k)), k
    assert hasattr(capi.Context, "fleet_link_groups_los_device")
    for f in (Fleet.link, Fleet.link_stages):
        assert inspect.signature(f).parameters["los"].default is False
    assert NEW_HDR in built.DEPS and os.path.join(ROOT, "faster_amd", "csrc", "fh_link_los.hip.hpp") in built.DEPS
    assert "capi.LINK_LOS_SYMBOLS" in open(os.path.join(ROOT, "__graft_entry__.py")).read()   # build() touches the new symbol


def test_the_two_kernels_lie_behind_every_kernel_of_before():
    """fh_capi.hip reaches the new device header through the last line of fh_link.hip.hpp, the last device header it names: nothing of
    before moves in the code object.  The new header defines its two kernels and no kernel of another header again."""
    csrc = os.path.join(ROOT, "faster_amd", "csrc")
    strip = lambda text: re.sub(r"//[^\n]*", "", text)   # noqa: E731
    capi_text = open(os.path.join(csrc, "fh_capi.hip")).read()
    device = re.findall(r'#include "(fh_\w+\.hip\.hpp)"', capi_text)
    assert device[-1] == "fh_link.hip.hpp" and "fh_link_los.hip.hpp" not in device
    link = strip(open(os.path.join(csrc, "fh_link.hip.hpp")).read())
    assert link.rstrip().endswith('#include "fh_link_los.hip.hpp"')
    assert link.index('#include "fh_link_los.hip.hpp"') > max(m.end() for m in re.finditer(r"__global__", link))
    los = strip(open(os.path.join(csrc, "fh_link_los.hip.hpp")).read())
    assert sorted(set(re.findall(r"__global__[^\n]*?\b(\w+_kernel)\s*\(", los))) == ["link_los_hook_kernel", "link_los_narrow_kernel"]
    for k in ("link_los_narrow_kernel", "link_los_hook_kernel", "link_boxes_kernel", "link_init_kernel", "link_jump_kernel"):
        assert "fh::" + k in capi_text, k
    for other in os.listdir(csrc):
        if other.endswith(".hpp") and other != "fh_link_los.hip.hpp":
            assert "link_los_" not in strip(open(os.path.join(csrc, other)).read()), other


def test_every_argument_rule_in_prologue_order(built):
    """Null context, null params, range, passes, n, n_views, the grid: the clauses of fh_fleet_link_groups_device in its order; then the
    map; then FH_ERR_DEVICE on a context without a device (never a CPU path)."""
    from faster_amd import capi

    L = capi.lib()
    h = ctypes.c_void_p()
    assert L.fh_create(ctypes.byref(h), 1 << 20) == DEV and h.value
    buf = np.zeros(8192, dtype=np.uint8)
    d = abi.ptr(buf)

    def grid(res=1.0, dims=(40, 36, 12)):
        g = np.zeros(1, dtype=abi.voxel_grid_dtype)
        g["origin"], g["res"], g["dims"] = (0.1, 0.2, 0.3), res, dims
        return g

    def par(**kw):
        p = np.ascontiguousarray(abi.default_link_params(1.2)).reshape(1)
        for k, v in kw.items():
            p[k] = v
        return p

    def call(ctx=h, vmap=None, p=par(), veh=d, n=1, view_of=None, n_views=4, g=grid(), labels=d, info=d):
        return L.fh_fleet_link_groups_los_device(ctx, vmap, None if p is None else abi.ptr(p), veh, n, view_of, n_views,
                                                 None if g is None else abi.ptr(g), labels, info)

    def plain(ctx=h, p=par(), veh=d, n=1, view_of=None, n_views=4, g=grid(), labels=d, info=d):
        return L.fh_fleet_link_groups_device(ctx, None if p is None else abi.ptr(p), veh, n, view_of, n_views, None if g is None else abi.ptr(g),
                                             labels, info)

    nan, inf = float("nan"), float("inf")
    try:
        # 1. the clauses of fh_fleet_link_groups_device, each alone, with a null map: the map is judged after them
        assert call(ctx=None) == ARG and call(ctx=None, p=None) == ARG and call(p=None) == ARG
        broken = [dict(p=par(range=v)) for v in (nan, inf, -inf, 0.0, -0.0, -1e-300, -1.0)]
        broken += [dict(p=par(passes=v)) for v in (0, -1, 1025, 1 << 30)]
        broken += [dict(n=-1), dict(n_views=0), dict(n_views=-5), dict(g=None), dict(g=grid(res=0.0)), dict(g=grid(res=nan))]
        broken += [dict(g=grid(dims=dims)) for dims in ((0, 36, 12), (40, 0, 12), (40, 36, -1), (1024, 1024, 2), (1 << 16, 1 << 16, 1 << 16))]
        for kw in broken:
            assert call(**kw) == ARG and plain(**kw) == ARG, kw
        # 2. every one of them passes: the null map is an argument error where the plain entry point goes on to the missing device
        for kw in (dict(), dict(p=par(range=1e-300)), dict(p=par(range=1e300)), dict(p=par(passes=1)), dict(p=par(passes=1024)), dict(n_views=1),
                   dict(g=grid(dims=(1, 1, 1))), dict(g=grid(dims=(1024, 1024, 1))), dict(n=0), dict(veh=None, labels=None, info=None),
                   dict(n=0, veh=None, labels=None, info=None)):
            assert call(**kw) == ARG and plain(**kw) == DEV, kw
    finally:
        L.fh_destroy(h)
    assert L.fh_abi_version() == 9
    with pytest.raises(capi.FasterHipError):
        capi.Context.fleet_link_groups_los_device(None, None, np.zeros(4), None, 1, None, 1, None, None, None)
