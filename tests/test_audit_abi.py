"""CPU-side checks of the plan audit's entry point (fh_fleet_audit_device): declared in include/fasterhip_audit.h and not in fasterhip.h,
the header compiles alone as C99 and C++11, exported, bound in faster_amd/capi.py, the struct layouts of the header equal the dtypes of
faster_amd/abi.py, and every argument rule in the order of the prologue, with no CPU path."""
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
AUDIT_HDR = os.path.join(INC, "fasterhip_audit.h")
NEW = ["fh_fleet_audit_device"]
OK, ARG, DEV = 0, -1, -2


@pytest.fixture(scope="module")
def built():
    from faster_amd import build as fb

    fb.build_all()
    return fb


def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(fh_[a-z_0-9]+)\s*\(", text))


def test_entry_point_is_declared_in_its_own_header_which_compiles_alone(tmp_path):
    assert set(NEW) <= _declared(AUDIT_HDR)
    assert not set(NEW) & _declared(HDR)   # fasterhip.h is pinned to capi.SYMBOLS (tests/test_abi.py): the new one stays out of it
    assert "fasterhip_audit.h" in open(HDR).read()   # (the fleet block points to it)
    assert int(re.search(r"#define FH_ABI_VERSION (\d+)", open(HDR).read()).group(1)) == abi.FH_ABI_VERSION == 9
    src = "#include \"fasterhip_audit.h\"\nint main(void) {\n" + "".join("  (void)%s;\n" % n for n in NEW) + "  return 0;\n}\n"
    for lang, std, comp in (("c", "-std=c99", "gcc"), ("c++", "-std=c++11", "g++")):
        f = tmp_path / ("probe." + ("c" if lang == "c" else "cpp"))
        f.write_text(src)
        r = subprocess.run([comp, "-fsyntax-only", "-x", lang, std, "-Wall", "-pedantic", "-I", INC, str(f)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr.strip(), (lang, r.stderr[-2000:])


def test_struct_layouts_and_constants_of_the_header_equal_abi_py(tmp_path):
    """sizeof and every offsetof, printed by a C program compiled against the header."""
    fields = {"fh_audit_params": (abi.audit_params_dtype, 32), "fh_plan_audit": (abi.plan_audit_dtype, 64)}
    lines = []
    for s, (dt, _) in fields.items():
        lines.append('  printf("%s %%d\\n", (int)sizeof(%s));' % (s, s))
        lines += ['  printf("%s.%s %%d\\n", (int)offsetof(%s, %s));' % (s, k, s, k) for k in dt.names]
    consts = ["BAD_PLAN", "NO_VIEW", "NOT_FINITE", "UNKNOWN", "OCCUPIED", "LIST_POINTS", "SLAB_CELLS"]
    lines += ['  printf("FH_AUDIT_%s %%d\\n", (int)FH_AUDIT_%s);' % (k, k) for k in consts]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"fasterhip_audit.h\"\nint main(void) {\n" + "\n".join(lines) + "\n  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", INC, str(src), "-o", str(exe)])
    got = dict((k, int(v)) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()))
    for s, (dt, size) in fields.items():
        assert got[s] == dt.itemsize == size, s
        for k in dt.names:
            assert got["%s.%s" % (s, k)] == dt.fields[k][1], (s, k)
    for k in consts:
        assert got["FH_AUDIT_" + k] == getattr(abi, "FH_AUDIT_" + k), k
    assert [getattr(abi, "FH_AUDIT_" + k) for k in consts[:5]] == [1, 2, 4, 8, 16]
    assert abi.FH_AUDIT_LIST_POINTS >= 128 and abi.FH_AUDIT_LIST_POINTS % 64 == 0 and abi.FH_AUDIT_SLAB_CELLS % 64 == 0


def test_symbol_is_exported_and_bound(built):
    from faster_amd import capi
    from faster_amd.fleet import Fleet

    L = ctypes.CDLL(built.SO)
    for name in NEW:
        assert hasattr(L, name), name
    assert sorted(capi.AUDIT_SYMBOLS) == sorted(NEW)
    others = set(capi.SYMBOLS) | set(capi.OCCUPANCY_SYMBOLS) | set(capi.CERTIFY_SYMBOLS)
    assert not set(NEW) & others
    assert len(others) == len(capi.SYMBOLS) + len(capi.OCCUPANCY_SYMBOLS) + len(capi.CERTIFY_SYMBOLS)   # the four lists are disjoint
    assert hasattr(capi.Context, "fleet_audit_device") and hasattr(Fleet, "audit")


def test_every_argument_rule_in_prologue_order(built):
    """null context, then the arguments, then FH_ERR_DEVICE on a context without a device (never a CPU path); n == 0 and the pointers are
    looked at after the device."""
    from faster_amd import capi

    L = capi.lib()
    h = ctypes.c_void_p()
    assert L.fh_create(ctypes.byref(h), 1 << 20) == DEV and h.value
    buf = np.zeros(8192, dtype=np.uint8)
    d = abi.ptr(buf)

    def grid(res=0.25, dims=(40, 36, 12)):
        g = np.zeros(1, dtype=abi.voxel_grid_dtype)
        g["origin"], g["res"], g["dims"] = (0.1, 0.2, 0.3), res, dims
        return g

    def par(**kw):
        p = np.ascontiguousarray(abi.default_audit_params(0.42)).reshape(1)
        for k, v in kw.items():
            p[k] = v
        return p

    cells = 40 * 36 * 12

    def call(ctx=h, p=par(), n=1, max_states=8, g=grid(), flags=d, view_stride=cells, n_views=1, cloud=d, n_cloud=64, mask=d, mask_words=2, veh=d,
             plans=d, out=d):
        return L.fh_fleet_audit_device(ctx, None if p is None else abi.ptr(p), veh, plans, n, max_states, None if g is None else abi.ptr(g), flags,
                                       view_stride, None, n_views, cloud, n_cloud, mask, mask_words, out)

    nan, inf = float("nan"), float("inf")
    try:
        assert call(ctx=None) == ARG
        assert call(ctx=None, n=-1) == ARG
        assert call(p=None) == ARG
        for k in ("r_unknown", "r_occupied", "cap"):
            for v in (nan, -1e-300, -1.0, inf, -inf):
                assert call(p=par(**{k: v})) == ARG, (k, v)
        assert call(p=par(cap=0.0, r_unknown=0.0, r_occupied=0.0)) == ARG            # cap <= 0
        assert call(p=par(r_unknown=0.85)) == ARG and call(p=par(r_occupied=0.85)) == ARG   # a radius above cap = 0.84
        assert call(p=par(stride=0)) == ARG and call(p=par(stride=-3)) == ARG and call(p=par(count=-1)) == ARG
        assert call(n=-1) == ARG and call(max_states=0) == ARG
        # with d_flags: the grid, cap <= 64 res, n_views, view_stride
        assert call(g=None) == ARG
        assert call(g=grid(res=0.0)) == ARG and call(g=grid(res=-1.0)) == ARG
        for dims in ((0, 36, 12), (40, 0, 12), (40, 36, -1)):
            assert call(g=grid(dims=dims)) == ARG, dims
        assert call(g=grid(res=0.013)) == ARG                                        # cap = 0.84 > 64 * 0.013
        assert call(n_views=0) == ARG
        assert call(view_stride=cells - 1) == ARG
        # with d_point_mask: the row holds a bit per point, n_views
        assert call(n_cloud=65) == ARG
        assert call(flags=None, g=None, n_views=0) == ARG
        # in order: an argument error wins over the missing device, whatever comes later
        assert call(p=par(stride=0), n=0, veh=None) == ARG
        # every rule passes: the device is looked at next, then n == 0 and the pointers
        assert call() == DEV
        assert call(view_stride=0) == DEV and call(view_stride=cells + 7) == DEV     # one grid for the fleet; a stride larger than a view
        assert call(p=par(r_unknown=0.0, r_occupied=0.84)) == DEV                   # zero and cap itself are radii
        assert call(g=grid(res=0.84 / 64.0 * 1.001)) == DEV
        assert call(flags=None, g=None, mask=None, n_views=0, cloud=None, n_cloud=0) == DEV   # no side at all is a call
        assert call(flags=None, g=None, mask=None, n_views=0, n_cloud=65) == DEV    # without masks nothing is asked of mask_words
        assert call(n=0) == DEV
        assert call(veh=None, plans=None, out=None) == DEV
    finally:
        L.fh_destroy(h)
    with pytest.raises(capi.FasterHipError):
        capi.Context.fleet_audit_device(None, np.zeros(4), None, None, 1, 8, None)
