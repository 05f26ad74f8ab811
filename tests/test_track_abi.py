"""CPU-side checks of fh_fleet_obstacle_track_device: declared in include/fasterhip_track.h and in no other header, the header compiles
alone as C99 and C++11, exported, bound in faster_amd/capi.py in a list of its own and on Fleet, the struct layouts and constants of the
header equal faster_amd/abi.py, the kernel is a file of its own behind the link headers, and every argument rule that can be reached
without a device in the order of the prologue (the two rules that need a map need a device: tests/test_gpu_track.py)."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from faster_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "fasterhip_track.h")
NEW = ["fh_fleet_obstacle_track_device"]
OK, ARG, DEV = 0, -1, -2
STRUCTS = {"fh_track_params": "track_params_dtype", "fh_obstacle_track": "obstacle_track_dtype"}
CONSTANTS = ("FH_TRACK_HISTORY", "FH_TRACK_SEEN", "FH_TRACK_LOST", "FH_TRACK_RESET", "FH_TRACK_STALE", "FH_TRACK_BAD_FIT")


@pytest.fixture(scope="module")
def built():
    from faster_amd import build as fb

    fb.build_all()
    return fb


def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(fh_[a-z_0-9]+)\s*\(", text))


def test_the_entry_point_is_declared_in_its_own_header_which_compiles_alone(tmp_path):
    assert set(NEW) == _declared(HDR)
    for other in sorted(os.listdir(INC)):
        if other != "fasterhip_track.h":
            assert not set(NEW) & _declared(os.path.join(INC, other)), other
    code = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    assert re.findall(r'#include "([^"]+)"', code) == ["fasterhip_obstacles.h", "fasterhip_link_los.h"]
    assert int(re.search(r"#define FH_ABI_VERSION (\d+)", open(os.path.join(INC, "fasterhip.h")).read()).group(1)) == abi.FH_ABI_VERSION == 9
    src = "#include \"fasterhip_track.h\"\nint main(void) {\n" + "".join("  (void)%s;\n" % n for n in NEW) + "  return 0;\n}\n"
    for lang, std, comp in (("c", "-std=c99", "gcc"), ("c++", "-std=c++11", "g++")):
        f = tmp_path / ("probe." + ("c" if lang == "c" else "cpp"))
        f.write_text(src)
        r = subprocess.run([comp, "-fsyntax-only", "-x", lang, std, "-Wall", "-pedantic", "-I", INC, str(f)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr.strip(), (lang, r.stderr[-2000:])


def test_struct_layouts_and_constants_of_the_header_equal_abi_py(tmp_path):
    """sizeof and every offsetof, printed by a C program compiled against the header."""
    lines = []
    for s, d in STRUCTS.items():
        lines.append('  printf("%s %%d\\n", (int)sizeof(%s));' % (s, s))
        lines += ['  printf("%s.%s %%d\\n", (int)offsetof(%s, %s));' % (s, k, s, k) for k in getattr(abi, d).names]
    lines += ['  printf("%s %%d\\n", (int)%s);' % (k, k) for k in CONSTANTS]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"fasterhip_track.h\"\nint main(void) {\n" + "\n".join(lines) + "\n  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", INC, str(src), "-o", str(exe)])
    got = dict((k, int(v)) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()))
    sizes = {"fh_track_params": 64, "fh_obstacle_track": 320}
    for s, d in STRUCTS.items():
        dt = getattr(abi, d)
        assert got[s] == dt.itemsize == sizes[s], s
        for k in dt.names:
            assert got["%s.%s" % (s, k)] == dt.fields[k][1], (s, k)
    assert abi.track_params_dtype.names == ("r_detect", "dc", "gate", "grow", "max_age", "fit", "min_obs", "reserved")
    assert abi.obstacle_track_dtype.names == ("tick", "pos", "radius", "count", "head", "flags", "reserved")
    assert abi.obstacle_track_dtype["tick"].shape == (8,) and abi.obstacle_track_dtype["pos"].shape == (8, 3)
    for k in CONSTANTS:
        assert got[k] == getattr(abi, k), k
    assert [getattr(abi, k) for k in CONSTANTS] == [8, 1, 2, 4, 8, 16]
    p = abi.default_track_params(6.0, 0.01)
    assert (float(p["r_detect"]), float(p["dc"]), float(p["gate"]), float(p["grow"]), int(p["max_age"]), int(p["fit"]), int(p["min_obs"])) == (
        6.0, 0.01, 0.0, 0.0, 0, 4, 2) and not p["reserved"].any()


def test_the_symbol_is_exported_and_bound(built):
    from faster_amd import capi
    from faster_amd.fleet import Fleet

    L = ctypes.CDLL(built.SO)
    for name in NEW:
        assert hasattr(L, name), name
    assert capi.TRACK_SYMBOLS == NEW
    for k in [k for k in dir(capi) if k.endswith("SYMBOLS") and k != "TRACK_SYMBOLS"]:
        assert not set(NEW) & set(getattr(capi, k)), k
    assert hasattr(capi.Context, "fleet_obstacle_track_device")
    sig = inspect.signature(Fleet.enable_tracking).parameters
    assert list(sig)[1:] == ["truth", "r_detect", "los", "fit", "min_obs", "max_age", "gate", "grow"]
    assert [sig[k].default for k in list(sig)[3:]] == [True, 4, 2, 0, 0.0, 0.0]
    for name in ("set_truth", "track", "track_records"):
        assert callable(getattr(Fleet, name))
    assert HDR in built.DEPS and os.path.join(ROOT, "faster_amd", "csrc", "fh_track.hip.hpp") in built.DEPS
    assert "capi.TRACK_SYMBOLS" in open(os.path.join(ROOT, "__graft_entry__.py")).read()   # build() touches the new symbol


def test_the_kernel_is_a_file_of_its_own_behind_the_link_headers():
    """fh_capi.hip names no device header more: fh_link.hip.hpp ends with the line of sight's header and that one with the tracker's, so
    the kernel lies behind every kernel of before.  One plain kernel, no LDS, the ray test of the link as it is, FP contraction off,
    and no atomics but the integer adds into info."""
    csrc = os.path.join(ROOT, "faster_amd", "csrc")
    strip = lambda text: re.sub(r"//[^\n]*", "", text)   # noqa: E731
    device = re.findall(r'#include "(fh_\w+\.hip\.hpp)"', open(os.path.join(csrc, "fh_capi.hip")).read())
    assert "fh_track.hip.hpp" not in device and device[-1] == "fh_link.hip.hpp"
    los = strip(open(os.path.join(csrc, "fh_link_los.hip.hpp")).read())
    assert los.rstrip().endswith('#include "fh_track.hip.hpp"')
    assert los.index('#include "fh_track.hip.hpp"') > max(m.end() for m in re.finditer(r"__global__", los))
    body = strip(open(os.path.join(csrc, "fh_track.hip.hpp")).read())
    assert re.findall(r"__global__[^\n]*?\b(\w+_kernel)\s*\(", body) == ["track_kernel"]
    assert not re.search(r"template\s*<[^>]*>\s*__global__", body) and "__shared__" not in body
    assert "#pragma clang fp contract(off)" in body and "ray_blocked(" in body and "fhw::" in body
    assert re.findall(r"\batomic\w+", body) == ["atomicAdd"] * 4 and len(re.findall(r"atomicAdd\(a\.info \+ \d, 1ull\)", body)) == 4
    assert "fh::track_kernel" in open(os.path.join(csrc, "fh_capi.hip")).read()
    for other in os.listdir(csrc):
        if other not in ("fh_track.hip.hpp", "fh_capi.hip"):
            assert "track_kernel" not in strip(open(os.path.join(csrc, other)).read()), other


def test_every_argument_rule_in_prologue_order(built):
    """Clauses 1 to 11 of the header in its order; clauses 12 and 13 need a map, which needs a device.  A context without a device
    answers FH_ERR_ARG for every broken rule and FH_ERR_DEVICE (never a CPU path) when none is, so the order is shown from the other
    side: with everything before a clause right and everything after it wrong the answer is FH_ERR_ARG, and mending the clauses one by
    one from the first on turns it into FH_ERR_DEVICE only with the last.  m == 0 and the pointers are looked at after the device."""
    from faster_amd import capi

    L = capi.lib()
    h = ctypes.c_void_p()
    assert L.fh_create(ctypes.byref(h), 1 << 20) == DEV and h.value
    buf = np.zeros(8192, dtype=np.uint8)
    d = abi.ptr(buf)

    def par(**kw):
        p = np.ascontiguousarray(abi.default_track_params(6.0, 0.01, fit=4, min_obs=2, max_age=50, gate=1.0, grow=0.1)).reshape(1)
        for k, v in kw.items():
            p[k] = v
        return p

    def call(ctx=h, vmap=None, p=par(), truth=d, m=3, t0=5, tick=7, veh=d, n=2, tracks=d, est=d, seer=d, info=d):
        return L.fh_fleet_obstacle_track_device(ctx, vmap, None if p is None else abi.ptr(p), truth, m, t0, tick, veh, n, tracks, est, seer, info)

    nan, inf = float("nan"), float("inf")
    try:
        # 1. the context or the params
        assert call(ctx=None) == ARG and call(ctx=None, p=None) == ARG and call(p=None) == ARG
        # 2. r_detect and 3. dc: NaN, infinite or <= 0
        for k in ("r_detect", "dc"):
            for v in (nan, inf, -inf, 0.0, -0.0, -1.0, -1e-300):
                assert call(p=par(**{k: v})) == ARG, (k, v)
            assert call(p=par(**{k: 1e-300})) == DEV and call(p=par(**{k: 1e300})) == DEV
        # 4. gate and 5. grow: NaN, infinite or negative; zero is "off"
        for k in ("gate", "grow"):
            for v in (nan, inf, -inf, -1e-300, -3.0):
                assert call(p=par(**{k: v})) == ARG, (k, v)
            assert call(p=par(**{k: 0.0})) == DEV
        # 6. max_age, 7. fit, 8. min_obs
        assert call(p=par(max_age=-1)) == ARG and call(p=par(max_age=-(1 << 63))) == ARG
        assert call(p=par(max_age=0)) == DEV and call(p=par(max_age=(1 << 63) - 1)) == DEV
        for k in ("fit", "min_obs"):
            for v in (0, -1, 9, (1 << 31) - 1, -(1 << 31)):
                assert call(p=par(**{k: v})) == ARG, (k, v)
            assert call(p=par(**{k: 1})) == DEV and call(p=par(**{k: 8})) == DEV
        # 9. n and m, 10. and 11. the two clocks
        assert call(n=-1) == ARG and call(m=-1) == ARG
        for k in ("t0", "tick"):
            for v in (-1, -(1 << 63), (1 << 62) + 1, (1 << 63) - 1):
                assert call(**{k: v}) == ARG, (k, v)
            assert call(**{k: 0}) == DEV and call(**{k: 1 << 62}) == DEV
        # the order
        broken = [("r_detect", nan), ("dc", nan), ("gate", nan), ("grow", nan), ("max_age", -1), ("fit", 0), ("min_obs", 9)]
        good = dict((k, par()[k][0]) for k, _ in broken)
        for c in range(len(broken) + 1):
            p = par(**dict([(k, good[k]) for k, _ in broken[:c]] + broken[c:]))
            assert call(p=p, n=-1, t0=-1, tick=-1, truth=None) == ARG, c      # (clauses 9, 10 and 11 still broken)
            assert call(p=p, t0=-1, tick=-1, truth=None) == ARG, c            # (clauses 10 and 11 still broken)
            assert call(p=p, tick=-1, truth=None) == ARG, c                   # (clause 11 still broken)
            assert call(p=p, truth=None, veh=None, tracks=None, est=None, seer=None, info=None) == (DEV if c == len(broken) else ARG), c
        # an argument error wins over the missing device, over m == 0 and over the pointers
        assert call(p=par(fit=0), m=0, truth=None) == ARG and call(tick=-1, n=0, veh=None) == ARG
        # every rule passes: the device is looked at next, then m == 0 and the pointers
        assert call() == DEV and call(m=0) == DEV and call(n=0, veh=None) == DEV
        assert call(truth=None, veh=None, tracks=None, est=None, seer=None, info=None) == DEV
    finally:
        L.fh_destroy(h)
    with pytest.raises(capi.FasterHipError):
        capi.Context.fleet_obstacle_track_device(None, None, np.zeros(4), None, 1, 0, 0, None, 1, None, None, None, None)
    with pytest.raises(capi.FasterHipError):   # (a record of the obstacle stage is not taken for this one)
        capi.Context.fleet_obstacle_track_device(None, None, abi.default_obstacle_params(4, 2, 6.0, 0.01), None, 1, 0, 0, None, 1, None, None, None, None)
