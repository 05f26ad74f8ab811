"""CPU-side checks of the commit check's entry points (fh_fleet_backup_device, fh_fleet_check_device, fh_fleet_revert_device): declared
in include/fasterhip_check.h and not in fasterhip.h, the header compiles alone as C99 and C++11, exported, bound in faster_amd/capi.py,
the struct layouts of the header equal the dtypes of faster_amd/abi.py, and every argument rule in the order of the prologue, with no CPU
path."""
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
CHECK_HDR = os.path.join(INC, "fasterhip_check.h")
NEW = ["fh_fleet_backup_device", "fh_fleet_check_device", "fh_fleet_revert_device"]
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
    assert set(NEW) <= _declared(CHECK_HDR)
    assert not set(NEW) & _declared(HDR)   # fasterhip.h is pinned to capi.SYMBOLS (tests/test_abi.py): the new ones stay out of it
    assert "fasterhip_check.h" in open(HDR).read()   # (the fleet block points to it)
    assert int(re.search(r"#define FH_ABI_VERSION (\d+)", open(HDR).read()).group(1)) == abi.FH_ABI_VERSION == 9
    src = "#include \"fasterhip_check.h\"\nint main(void) {\n" + "".join("  (void)%s;\n" % n for n in NEW) + "  return 0;\n}\n"
    for lang, std, comp in (("c", "-std=c99", "gcc"), ("c++", "-std=c++11", "g++")):
        f = tmp_path / ("probe." + ("c" if lang == "c" else "cpp"))
        f.write_text(src)
        r = subprocess.run([comp, "-fsyntax-only", "-x", lang, std, "-Wall", "-pedantic", "-I", INC, str(f)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr.strip(), (lang, r.stderr[-2000:])


def test_struct_layouts_and_constants_of_the_header_equal_abi_py(tmp_path):
    """sizeof and every offsetof, printed by a C program compiled against the header."""
    fields = {"fh_check_params": (abi.check_params_dtype, 32), "fh_plan_check": (abi.plan_check_dtype, 32)}
    lines = []
    for s, (dt, _) in fields.items():
        lines.append('  printf("%s %%d\\n", (int)sizeof(%s));' % (s, s))
        lines += ['  printf("%s.%s %%d\\n", (int)offsetof(%s, %s));' % (s, k, s, k) for k in dt.names]
    consts = ["FH_CHECK_BAD_PLAN", "FH_CHECK_NOT_FINITE", "FH_CHECK_CANDIDATE", "FH_CHECK_CONFLICT", "FH_CHECK_LIST_OTHERS", "FH_CHECK_MAX_CELLS",
              "FH_FLEET_STAGE_CONFLICT"]
    lines += ['  printf("%s %%d\\n", (int)%s);' % (k, k) for k in consts]
    lines += ['  printf("vehicle %d\\n", (int)sizeof(fh_vehicle));', '  printf("vehicle.stage %d\\n", (int)offsetof(fh_vehicle, stage));']
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"fasterhip_check.h\"\nint main(void) {\n" + "\n".join(lines)
                   + "\n  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", INC, str(src), "-o", str(exe)])
    got = dict((k, int(v)) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()))
    for s, (dt, size) in fields.items():
        assert got[s] == dt.itemsize == size, s
        for k in dt.names:
            assert got["%s.%s" % (s, k)] == dt.fields[k][1], (s, k)
    for k in consts:
        assert got[k] == getattr(abi, k), k
    assert [getattr(abi, k) for k in consts] == [1, 4, 16, 32, 256, 1 << 20, 7]
    assert abi.FH_CHECK_LIST_OTHERS >= 256 and abi.FH_CHECK_LIST_OTHERS % 128 == 0   # (it is emptied when it cannot take 128 more)
    # the new stage is no stage of fasterhip.h, and the revert patches it as the low half of a word of 8 bytes
    old = (abi.FH_FLEET_STAGE_NONE, abi.FH_FLEET_STAGE_NO_PATH, abi.FH_FLEET_STAGE_NO_WHOLE, abi.FH_FLEET_STAGE_NO_SAFE, abi.FH_FLEET_STAGE_COMMITTED,
           abi.FH_FLEET_STAGE_OVERFLOW)
    assert abi.FH_FLEET_STAGE_CONFLICT not in old
    assert got["vehicle"] == abi.vehicle_dtype.itemsize and got["vehicle"] % 8 == 0
    assert got["vehicle.stage"] == abi.vehicle_dtype.fields["stage"][1] and got["vehicle.stage"] % 8 == 0 and abi.state_dtype.itemsize % 16 == 0


def test_symbols_are_exported_and_bound(built):
    from faster_amd import capi
    from faster_amd.fleet import Fleet

    L = ctypes.CDLL(built.SO)
    for name in NEW:
        assert hasattr(L, name), name
    assert sorted(capi.CHECK_SYMBOLS) == sorted(NEW)
    others = (set(capi.SYMBOLS) | set(capi.OCCUPANCY_SYMBOLS) | set(capi.CERTIFY_SYMBOLS) | set(capi.AUDIT_SYMBOLS) | set(capi.SEPARATION_SYMBOLS)
              | set(capi.TRAFFIC_SYMBOLS))
    assert not set(NEW) & others
    for name in ("fleet_backup_device", "fleet_check_device", "fleet_revert_device"):
        assert hasattr(capi.Context, name), name
    assert hasattr(Fleet, "enable_check") and hasattr(Fleet, "check_records")
    assert os.path.join(INC, "fasterhip_check.h") in built.DEPS   # (a change of the header rebuilds the library)
    p = abi.default_check_params(0.6)
    assert (float(p["r"]), int(p["stride"]), int(p["count"])) == (0.6, 1, 0) and not p["reserved"].any()


def test_every_argument_rule_in_prologue_order(built):
    """null context, null params, the numbers of the params, n and max_states, the grid, then FH_ERR_DEVICE on a context without a
    device (never a CPU path); n == 0 and the pointers are looked at after the device."""
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
        p = np.ascontiguousarray(abi.default_check_params(0.84)).reshape(1)
        for k, v in kw.items():
            p[k] = v
        return p

    def call(ctx=h, p=par(), n=1, max_states=8, g=grid(), veh=d, plans=d, bveh=d, bplans=d, out=d):
        return L.fh_fleet_check_device(ctx, None if p is None else abi.ptr(p), veh, plans, bveh, bplans, n, max_states,
                                       None if g is None else abi.ptr(g), out)

    nan, inf = float("nan"), float("inf")
    bad_grid = grid(dims=(0, 36, 12))
    try:
        # 1. the context, then the params
        assert call(ctx=None) == ARG
        assert call(ctx=None, p=None) == ARG
        assert call(p=None) == ARG
        assert call(p=None, g=None, n=-1) == ARG
        # 2. the numbers
        for v in (nan, -1e-300, -1.0, inf, -inf):
            assert call(p=par(r=v)) == ARG, v
        assert call(p=par(stride=0)) == ARG and call(p=par(stride=-3)) == ARG and call(p=par(count=-1)) == ARG
        assert call(n=-1) == ARG and call(max_states=0) == ARG
        # 3. the grid
        assert call(g=None) == ARG
        assert call(g=grid(res=0.0)) == ARG and call(g=grid(res=-1.0)) == ARG and call(g=grid(res=nan)) == ARG
        for dims in ((0, 36, 12), (40, 0, 12), (40, 36, -1)):
            assert call(g=grid(dims=dims)) == ARG, dims
        assert call(g=grid(dims=(1024, 1024, 2))) == ARG and call(g=grid(dims=(1 << 20, 1, 2))) == ARG   # more than FH_CHECK_MAX_CELLS
        assert call(g=grid(dims=(1 << 16, 1 << 16, 1 << 16))) == ARG                   # (a product that does not fit 32 bits)
        # in order: an argument error wins over the missing device, whatever comes later
        assert call(p=par(stride=0), n=0, veh=None) == ARG
        assert call(g=bad_grid, n=0, veh=None) == ARG
        # 4. every rule passes: the device is looked at next, 5. / 6. then n == 0 and the pointers
        assert call() == DEV
        assert call(p=par(r=0.0)) == DEV                                               # zero is a radius
        assert call(p=par(count=5, stride=7)) == DEV
        assert call(g=grid(dims=(1, 1, 1))) == DEV and call(g=grid(dims=(1024, 1024, 1))) == DEV   # exactly FH_CHECK_MAX_CELLS
        assert call(n=0) == DEV
        assert call(veh=None, plans=None, bveh=None, bplans=None, out=None) == DEV
        # backup and revert: the context, n and max_states, then the device; the pointers after it
        for f, args in ((L.fh_fleet_backup_device, lambda n, ms, a=d: (a, a, n, ms, a, a)),
                        (L.fh_fleet_revert_device, lambda n, ms, a=d: (a, a, a, n, ms, a, a))):
            assert f(None, *args(1, 8)) == ARG and f(None, *args(-1, 0)) == ARG
            assert f(h, *args(-1, 8)) == ARG and f(h, *args(1, 0)) == ARG and f(h, *args(0, 0, None)) == ARG
            assert f(h, *args(1, 8)) == DEV and f(h, *args(0, 8)) == DEV and f(h, *args(1, 8, None)) == DEV
    finally:
        L.fh_destroy(h)
    with pytest.raises(capi.FasterHipError):
        capi.Context.fleet_check_device(None, np.zeros(4), None, None, None, None, 1, 8, None, None)
