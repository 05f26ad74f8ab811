"""CPU-side checks of the radio link's entry points (fh_fleet_link_groups_device, fh_fleet_link_merge_device): declared in
include/fasterhip_link.h and not in fasterhip.h, the header compiles alone as C99 and C++11, exported, bound in faster_amd/capi.py and on
Fleet, the struct layout and the constants of the header equal faster_amd/abi.py, FH_ABI_VERSION stays, and every clause of both
prologues in the stated order, with no CPU path."""
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
NEW = ["fh_fleet_link_groups_device", "fh_fleet_link_merge_device"]
OK, ARG, DEV = 0, -1, -2


@pytest.fixture(scope="module")
def built():
    from faster_amd import build as fb

    fb.build_all()
    return fb


def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(fh_[a-z_0-9]+)\s*\(", text))


def test_entry_points_are_declared_in_their_own_header_which_compiles_alone(tmp_path):
    assert set(NEW) == _declared(LINK_HDR)
    assert not set(NEW) & _declared(HDR)   # fasterhip.h is pinned to capi.SYMBOLS (tests/test_abi.py): the new ones stay out of it
    assert "link" not in re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S).lower()   # nothing was added to fasterhip.h
    assert int(re.search(r"#define FH_ABI_VERSION (\d+)", open(HDR).read()).group(1)) == abi.FH_ABI_VERSION == 9
    src = "#include \"fasterhip_link.h\"\nint main(void) {\n" + "".join("  (void)%s;\n" % n for n in NEW) + "  return 0;\n}\n"
    for lang, std, comp in (("c", "-std=c99", "gcc"), ("c++", "-std=c++11", "g++")):
        f = tmp_path / ("probe." + ("c" if lang == "c" else "cpp"))
        f.write_text(src)
        r = subprocess.run([comp, "-fsyntax-only", "-x", lang, std, "-Wall", "-pedantic", "-I", INC, str(f)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr.strip(), (lang, r.stderr[-2000:])


def test_struct_layout_and_constants_of_the_header_equal_abi_py(tmp_path):
    """sizeof and every offsetof, printed by a C program compiled against the header."""
    dt = abi.link_params_dtype
    lines = ['  printf("size %d\\n", (int)sizeof(fh_link_params));']
    lines += ['  printf("%s %%d\\n", (int)offsetof(fh_link_params, %s));' % (k, k) for k in dt.names]
    consts = ["FH_LINK_MAX_PASSES", "FH_LINK_MAX_CELLS", "FH_LINK_DEFAULT_PASSES"]
    lines += ['  printf("%s %%d\\n", (int)%s);' % (k, k) for k in consts]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"fasterhip_link.h\"\nint main(void) {\n" + "\n".join(lines)
                   + "\n  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", INC, str(src), "-o", str(exe)])
    got = dict((k, int(v)) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()))
    assert got["size"] == dt.itemsize == 32
    for k in dt.names:
        assert got[k] == dt.fields[k][1], k
    for k in consts:
        assert got[k] == getattr(abi, k), k
    assert (abi.FH_LINK_MAX_PASSES, abi.FH_LINK_MAX_CELLS) == (1024, 1 << 20)


def test_symbols_are_exported_and_bound(built):
    from faster_amd import capi
    from faster_amd.fleet import Fleet

    L = ctypes.CDLL(built.SO)
    for name in NEW:
        assert hasattr(L, name), name
    assert sorted(capi.LINK_SYMBOLS) == sorted(NEW)
    others = (set(capi.SYMBOLS) | set(capi.OCCUPANCY_SYMBOLS) | set(capi.CERTIFY_SYMBOLS) | set(capi.AUDIT_SYMBOLS) | set(capi.SEPARATION_SYMBOLS)
              | set(capi.TRAFFIC_SYMBOLS) | set(capi.TRAFFIC_TIMED_SYMBOLS) | set(capi.CHECK_SYMBOLS) | set(capi.ROUNDS_SYMBOLS)
              | set(capi.VIEW_SUBSET_SYMBOLS))
    assert not set(NEW) & others
    for name in ("fleet_link_groups_device", "fleet_link_merge_device"):
        assert hasattr(capi.Context, name), name
    for name in ("link", "link_records"):
        assert hasattr(Fleet, name), name
    assert LINK_HDR in built.DEPS   # (a change of the header rebuilds the library)
    assert os.path.join(ROOT, "faster_amd", "csrc", "fh_link.hip.hpp") in built.DEPS
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "capi.LINK_SYMBOLS" in entry   # build() touches the new symbols
    p = abi.default_link_params(1.25)
    assert (float(p["range"]), int(p["passes"])) == (1.25, abi.FH_LINK_DEFAULT_PASSES) and not p["reserved"].any()


def test_the_kernels_come_last_in_the_code_object():
    """fh_link.hip.hpp is included after every other device header and defines no kernel of another header again."""
    text = open(os.path.join(ROOT, "faster_amd", "csrc", "fh_capi.hip")).read()
    device = re.findall(r'#include "(fh_\w+\.hip\.hpp)"', text)
    assert device[-1] == "fh_link.hip.hpp" and device[-2] == "fh_rounds.hip.hpp"
    link = open(os.path.join(ROOT, "faster_amd", "csrc", "fh_link.hip.hpp")).read()
    kernels = sorted(set(re.findall(r"\b(\w+_kernel)\s*\(", re.sub(r"//[^\n]*", "", link))))
    assert kernels == ["link_boxes_kernel", "link_hook_kernel", "link_init_kernel", "link_jump_kernel", "link_merge_flags_kernel",
                       "link_merge_mask_kernel", "link_narrow_kernel"]
    for other in device[:-1]:
        body = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "faster_amd", "csrc", other)).read())
        assert not set(kernels) & set(re.findall(r"\b(\w+_kernel)\s*\(", body)), other


def test_every_argument_rule_in_prologue_order(built):
    """Groups: null context, null params, range, passes, n, n_views, the grid, then FH_ERR_DEVICE on a context without a device (never a
    CPU path); n == 0 and the pointers are looked at after the device.  Merge: null context, n_views, the stride when flags are given,
    the words when masks are given, then the device; null labels after it."""
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

    def call(ctx=h, p=par(), veh=d, n=1, view_of=None, n_views=4, g=grid(), labels=d, info=d):
        return L.fh_fleet_link_groups_device(ctx, None if p is None else abi.ptr(p), veh, n, view_of, n_views, None if g is None else abi.ptr(g),
                                             labels, info)

    nan, inf = float("nan"), float("inf")
    try:
        # 1. the context, then the params
        assert call(ctx=None) == ARG and call(ctx=None, p=None) == ARG and call(p=None) == ARG and call(p=None, g=None, n=-1) == ARG
        # 2. the numbers, each alone
        for v in (nan, inf, -inf, 0.0, -0.0, -1e-300, -1.0):
            assert call(p=par(range=v)) == ARG, v
        for v in (0, -1, 1025, 1 << 30):
            assert call(p=par(passes=v)) == ARG, v
        assert call(n=-1) == ARG
        assert call(n_views=0) == ARG and call(n_views=-5) == ARG
        # 3. the grid
        assert call(g=None) == ARG
        assert call(g=grid(res=0.0)) == ARG and call(g=grid(res=-1.0)) == ARG and call(g=grid(res=nan)) == ARG
        for dims in ((0, 36, 12), (40, 0, 12), (40, 36, -1)):
            assert call(g=grid(dims=dims)) == ARG, dims
        assert call(g=grid(dims=(1024, 1024, 2))) == ARG and call(g=grid(dims=(1 << 20, 1, 2))) == ARG   # more than FH_LINK_MAX_CELLS
        assert call(g=grid(dims=(1 << 16, 1 << 16, 1 << 16))) == ARG                   # (a product that does not fit 32 bits)
        # in order: every rule is an argument error before the missing device, whatever comes later; with n == 0 and no pointers too
        for broken in (dict(p=par(range=nan)), dict(p=par(passes=0)), dict(n=-1), dict(n_views=0), dict(g=grid(dims=(0, 36, 12)))):
            kw = dict(n=0, veh=None, labels=None, info=None)
            kw.update(broken)
            assert call(**kw) == ARG, broken
        # 4. every rule passes: the device is looked at next, then n == 0 and the pointers
        assert call() == DEV
        assert call(p=par(range=1e-300)) == DEV and call(p=par(range=1e300)) == DEV
        assert call(p=par(passes=1)) == DEV and call(p=par(passes=1024)) == DEV
        assert call(n_views=1) == DEV
        assert call(g=grid(dims=(1, 1, 1))) == DEV and call(g=grid(dims=(1024, 1024, 1))) == DEV   # exactly FH_LINK_MAX_CELLS
        assert call(n=0) == DEV
        assert call(veh=None, labels=None, info=None) == DEV

        def merge(ctx=h, labels=d, n_views=4, flags=d, stride=16, nbytes=16, mask=d, words=5, shared=2):
            return L.fh_fleet_link_merge_device(ctx, labels, n_views, flags, stride, nbytes, mask, words, shared)

        assert merge(ctx=None) == ARG and merge(ctx=None, n_views=0) == ARG
        assert merge(n_views=0) == ARG and merge(n_views=-1) == ARG
        assert merge(stride=15, nbytes=16) == ARG and merge(stride=0, nbytes=1) == ARG
        assert merge(words=-1, shared=0) == ARG and merge(shared=-1) == ARG and merge(shared=6) == ARG
        # a table that is not given is not judged
        assert merge(flags=None, stride=15, nbytes=16) == DEV
        assert merge(mask=None, words=-1, shared=9) == DEV
        # in order: an argument error before the missing device, null labels after it
        assert merge(labels=None, n_views=0) == ARG and merge(labels=None, stride=1, nbytes=2) == ARG and merge(labels=None, shared=6) == ARG
        assert merge() == DEV and merge(labels=None) == DEV
        assert merge(stride=16, nbytes=16) == DEV and merge(stride=107, nbytes=105) == DEV and merge(nbytes=0, stride=0) == DEV
        assert merge(shared=0) == DEV and merge(shared=5) == DEV and merge(words=0, shared=0) == DEV
        assert merge(flags=None, mask=None) == DEV
    finally:
        L.fh_destroy(h)
    assert L.fh_abi_version() == 9
    with pytest.raises(capi.FasterHipError):
        capi.Context.fleet_link_groups_device(None, np.zeros(4), None, 1, None, 1, None, None, None)
