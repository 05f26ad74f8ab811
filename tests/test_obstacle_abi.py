"""CPU-side checks of the moving-obstacle entry points (fh_fleet_obstacles_device, fh_fleet_obstacle_audit_device): declared in
include/fasterhip_obstacles.h and in no other header, the header compiles alone as C99 and C++11, exported, bound in faster_amd/capi.py
in a tuple of their own, the struct layouts and constants of the header equal faster_amd/abi.py, and every argument rule in the order of
the prologue, which comes before the device is looked at: no GPU is needed, and there is no CPU path."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from faster_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "fasterhip_obstacles.h")
NEW = ["fh_fleet_obstacles_device", "fh_fleet_obstacle_audit_device"]
OK, ARG, DEV = 0, -1, -2
STRUCTS = {"fh_obstacle": "obstacle_dtype", "fh_obstacle_params": "obstacle_params_dtype",
           "fh_obstacle_audit_params": "obstacle_audit_params_dtype", "fh_plan_obstacle_audit": "plan_obstacle_audit_dtype"}


@pytest.fixture(scope="module")
def built():
    from faster_amd import build as fb

    fb.build_all()
    return fb


def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(fh_[a-z_0-9]+)\s*\(", text))


def test_entry_points_are_declared_in_their_own_header_which_compiles_alone(tmp_path):
    assert set(NEW) == _declared(HDR)
    for other in sorted(os.listdir(INC)):
        if other != "fasterhip_obstacles.h":
            assert not set(NEW) & _declared(os.path.join(INC, other)), other
    assert '#include "fasterhip_traffic_timed.h"' in open(HDR).read()
    assert int(re.search(r"#define FH_ABI_VERSION (\d+)", open(os.path.join(INC, "fasterhip.h")).read()).group(1)) == abi.FH_ABI_VERSION == 9
    src = "#include \"fasterhip_obstacles.h\"\nint main(void) {\n" + "".join("  (void)%s;\n" % n for n in NEW) + "  return 0;\n}\n"
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
    for k in ("FH_OBSTACLE_ON", "FH_OBSTACLE_MAX_SAMPLES", "FH_OBSTACLE_AUDIT_CHUNK", "FH_OBSTACLE_BAD_PLAN", "FH_OBSTACLE_NOT_FINITE",
              "FH_OBSTACLE_HIT"):
        lines.append('  printf("%s %%d\\n", (int)%s);' % (k, k))
    lines.append('  printf("FH_OBSTACLE_MAX_TICK %lld\\n", (long long)FH_OBSTACLE_MAX_TICK);')
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"fasterhip_obstacles.h\"\nint main(void) {\n" + "\n".join(lines)
                   + "\n  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", INC, str(src), "-o", str(exe)])
    got = dict((k, int(v)) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()))
    sizes = {"fh_obstacle": 64, "fh_obstacle_params": 64, "fh_obstacle_audit_params": 32, "fh_plan_obstacle_audit": 64}
    for s, d in STRUCTS.items():
        dt = getattr(abi, d)
        assert got[s] == dt.itemsize == sizes[s], s
        for k in dt.names:
            assert got["%s.%s" % (s, k)] == dt.fields[k][1], (s, k)
    assert abi.obstacle_dtype.names == ("p0", "v", "radius", "flags", "reserved")
    assert abi.obstacle_params_dtype.names == ("range", "r_detect", "dc", "samples", "stride", "points", "first_point", "first_instant", "window",
                                               "reserved")
    assert abi.obstacle_audit_params_dtype.names == ("r", "dc", "stride", "count", "reserved")
    assert abi.plan_obstacle_audit_dtype.names == ("flags", "n_tested", "first", "first_obstacle", "worst", "worst_obstacle", "n_hit", "reserved",
                                                   "min_d2", "reserved_d")
    for k in ("FH_OBSTACLE_ON", "FH_OBSTACLE_MAX_SAMPLES", "FH_OBSTACLE_AUDIT_CHUNK", "FH_OBSTACLE_BAD_PLAN", "FH_OBSTACLE_NOT_FINITE",
              "FH_OBSTACLE_HIT", "FH_OBSTACLE_MAX_TICK"):
        assert got[k] == getattr(abi, k), k
    assert (abi.FH_OBSTACLE_ON, abi.FH_OBSTACLE_MAX_SAMPLES, abi.FH_OBSTACLE_MAX_TICK) == (1, 512, 1 << 62)
    # the audit's flags are the separation header's numbers: its rules are taken word for word
    assert (abi.FH_OBSTACLE_BAD_PLAN, abi.FH_OBSTACLE_NOT_FINITE, abi.FH_OBSTACLE_HIT) == (abi.FH_SEP_BAD_PLAN, abi.FH_SEP_NOT_FINITE, abi.FH_SEP_NEAR)
    p = abi.default_obstacle_params(8, 2, 1.5, 0.01)
    assert (int(p["points"]), float(p["r_detect"]), int(p["window"]), int(p["first_instant"]), int(p["first_point"])) == (7, 0.0, 0, 0, 0)
    q = abi.default_obstacle_audit_params(0.3, 0.01)
    assert (float(q["r"]), float(q["dc"]), int(q["stride"]), int(q["count"])) == (0.3, 0.01, 1, 0)


def test_symbols_are_exported_and_bound(built):
    from faster_amd import capi
    from faster_amd.fleet import Fleet
    import inspect

    L = ctypes.CDLL(built.SO)
    for name in NEW:
        assert hasattr(L, name), name
    assert sorted(capi.OBSTACLE_SYMBOLS) == sorted(NEW)
    others = (set(capi.SYMBOLS) | set(capi.OCCUPANCY_SYMBOLS) | set(capi.CERTIFY_SYMBOLS) | set(capi.AUDIT_SYMBOLS)
              | set(capi.SEPARATION_SYMBOLS) | set(capi.TRAFFIC_SYMBOLS) | set(capi.TRAFFIC_TIMED_SYMBOLS) | set(capi.CHECK_SYMBOLS))
    assert not set(NEW) & others
    assert hasattr(capi.Context, "fleet_obstacles_device") and hasattr(capi.Context, "fleet_obstacle_audit_device")
    sig = inspect.signature(Fleet.enable_obstacles).parameters
    assert list(sig)[1:] == ["obstacles", "samples", "stride", "range", "r_detect", "points", "window", "first_instant"]
    assert sig["r_detect"].default == 0.0 and sig["points"].default == 7 and sig["window"].default == 0 and sig["first_instant"].default is None
    sig = inspect.signature(Fleet.obstacle_audit).parameters
    assert sig["r"].default is None and sig["stride"].default == 1 and sig["count"].default == 0
    for name in ("set_obstacles", "obstacles"):
        assert callable(getattr(Fleet, name))
    assert HDR in built.DEPS and os.path.join(ROOT, "faster_amd", "csrc", "fh_obstacles.hip.hpp") in built.DEPS
    assert "capi.OBSTACLE_SYMBOLS" in open(os.path.join(ROOT, "__graft_entry__.py")).read()


def test_device_code_is_a_file_of_its_own_that_leaves_traffic_alone():
    csrc = os.path.join(ROOT, "faster_amd", "csrc")
    strip = lambda s: re.sub(r"//[^\n]*", "", s)  # noqa: E731
    body = strip(open(os.path.join(csrc, "fh_obstacles.hip.hpp")).read())
    kernels = sorted(set(re.findall(r"__global__[^\n]*?\b(\w+_kernel)\s*\(", body)))
    assert kernels == ["obstacle_audit_kernel", "obstacle_mask1_kernel", "obstacle_mask7_kernel", "obstacle_observers_kernel",
                       "obstacle_points1_kernel", "obstacle_points7_kernel"]
    assert not re.search(r"template\s*<[^>]*>\s*__global__", body)   # plain kernels, as in fh_traffic.hip.hpp
    assert '#include "fh_traffic.hip.hpp"' in body and '#include "fh_traffic_timed.hip.hpp"' in body
    assert "#pragma clang fp contract(off)" in body and "atomic" not in body
    for name in ("traffic_rows<PPS>", "TrafficBox", "cell_box_margin", "plan_bad_extent", "plan_finite", "fhw::"):
        assert name in body, name
    capi_text = strip(open(os.path.join(csrc, "fh_capi.hip")).read())
    includes = re.findall(r'#include "([^"]+)"', capi_text)
    assert includes.index("fh_obstacles.hip.hpp") == includes.index("fh_traffic_timed.hip.hpp") + 1
    for other in os.listdir(csrc):   # no other file of the device code knows of it
        if other not in ("fh_obstacles.hip.hpp", "fh_capi.hip"):
            assert "obstacle_" not in strip(open(os.path.join(csrc, other)).read()).lower(), other


def test_every_argument_rule_of_the_stage_in_prologue_order(built):
    """The thirteen clauses of fh_fleet_obstacles_device in the header's order; then FH_ERR_DEVICE on a context without a device (never
    a CPU path); n == 0, m == 0 and the pointers are looked at after the device.  A context without a device answers FH_ERR_ARG for
    every broken rule, so the order itself is shown from the other side: with everything before a clause right and everything after it
    wrong the answer is FH_ERR_ARG, and mending the clauses one by one from the first on turns it into FH_ERR_DEVICE only with the
    last."""
    from faster_amd import capi

    L = capi.lib()
    h = ctypes.c_void_p()
    assert L.fh_create(ctypes.byref(h), 1 << 20) == DEV and h.value
    buf = np.zeros(8192, dtype=np.uint8)
    d = abi.ptr(buf)

    def par(**kw):
        p = np.ascontiguousarray(abi.default_obstacle_params(4, 2, 6.0, 0.01, r_detect=3.0, points=7, first_point=64, first_instant=9, window=1)).reshape(1)
        for k, v in kw.items():
            p[k] = v
        return p

    def call(ctx=h, p=par(), m=3, tick0=5, n=2, max_states=8, n_cloud=64 + 3 * 4 * 7, mask_words=5, obs=d, veh=d, plans=d, cloud=d, mask=d):
        return L.fh_fleet_obstacles_device(ctx, None if p is None else abi.ptr(p), obs, m, tick0, veh, plans, n, max_states, cloud, n_cloud, mask,
                                           mask_words)

    nan, inf = float("nan"), float("inf")
    try:
        # 1. the context or the params
        assert call(ctx=None) == ARG and call(ctx=None, p=None) == ARG and call(p=None) == ARG
        # 2. range: NaN, infinite or <= 0
        for v in (nan, inf, -inf, 0.0, -0.0, -1.0, -1e-300):
            assert call(p=par(range=v)) == ARG, v
        # 3. r_detect: NaN, infinite or negative (zero is "no detection")
        for v in (nan, inf, -inf, -1e-300, -3.0):
            assert call(p=par(r_detect=v)) == ARG, v
        assert call(p=par(r_detect=0.0)) == DEV
        # 4. dc: NaN, infinite or <= 0
        for v in (nan, inf, -inf, 0.0, -0.01):
            assert call(p=par(dc=v)) == ARG, v
        # 5. samples and the cap: 512 is served, 513 is not
        assert call(p=par(samples=0)) == ARG and call(p=par(samples=-4)) == ARG
        big = dict(m=1, n_cloud=64 + 513 * 7, mask_words=(64 + 513 * 7 + 31) // 32)
        assert call(p=par(samples=abi.FH_OBSTACLE_MAX_SAMPLES), **big) == DEV
        assert call(p=par(samples=abi.FH_OBSTACLE_MAX_SAMPLES + 1), **big) == ARG
        assert call(p=par(samples=(1 << 31) - 1), **big) == ARG
        # 6. stride, 7. points, 8. first_point, 9. first_instant, 10. window
        assert call(p=par(stride=0)) == ARG and call(p=par(stride=-1)) == ARG
        for v in (0, 2, 6, 8, -1, -7):
            assert call(p=par(points=v)) == ARG, v
        assert call(p=par(first_point=-32)) == ARG and call(p=par(first_point=33)) == ARG and call(p=par(first_point=16)) == ARG
        assert call(p=par(first_instant=-1)) == ARG and call(p=par(first_instant=-(1 << 31))) == ARG
        assert call(p=par(window=-1)) == ARG and call(p=par(window=-(1 << 31))) == ARG
        # 11. n, m, max_states, and n S in 31 bits
        assert call(n=-1) == ARG and call(m=-1) == ARG and call(max_states=0) == ARG and call(max_states=-5) == ARG
        assert call(p=par(samples=512), n=1 << 22, **big) == ARG and call(p=par(samples=512), n=(1 << 22) - 1, **big) == DEV
        # 12. the clock
        assert call(tick0=-1) == ARG and call(tick0=-(1 << 63)) == ARG and call(tick0=(1 << 62) + 1) == ARG and call(tick0=(1 << 63) - 1) == ARG
        assert call(tick0=0) == DEV and call(tick0=1 << 62) == DEV
        # 13. the points must fit the cloud and the masks: 64 + 3 * 4 * 7 = 148 points, 5 words; in 64 bits
        assert call(n_cloud=147) == ARG and call(mask_words=4) == ARG and call(n_cloud=0) == ARG and call(mask_words=-1) == ARG
        assert call(p=par(points=1), n_cloud=75) == ARG and call(p=par(points=1), mask_words=2) == ARG   # 64 + 12 = 76 points, 3 words
        assert call(p=par(samples=512, first_point=0), m=(1 << 31) - 1, n_cloud=(1 << 31) - 1, mask_words=(1 << 31) - 1) == ARG   # 2^40 samples
        assert call(p=par(samples=512, first_point=0, points=1), m=1 << 23, n_cloud=(1 << 31) - 1, mask_words=(1 << 31) - 1) == ARG   # 2^32: wraps to 0
        assert call(p=par(samples=512, first_point=(1 << 31) - 32, points=1), m=1, n_cloud=(1 << 31) - 1, mask_words=(1 << 31) - 1) == ARG
        # the order: clause c broken together with every later one is FH_ERR_ARG; mended from the first on, the device shows at the end
        broken = [("range", nan), ("r_detect", nan), ("dc", nan), ("samples", 513), ("stride", 0), ("points", 3), ("first_point", -1),
                  ("first_instant", -1), ("window", -1)]
        good = dict((k, par()[k][0]) for k, _ in broken)
        for c in range(len(broken) + 1):
            p = par(**dict([(k, good[k]) for k, _ in broken[:c]] + broken[c:]))
            assert call(p=p, n=-1, tick0=-1, n_cloud=0, veh=None) == ARG, c       # (clauses 11, 12 and 13 still broken)
            assert call(p=p, tick0=-1, n_cloud=0, veh=None) == ARG, c             # (clauses 12 and 13 still broken)
            assert call(p=p, n_cloud=0, veh=None) == ARG, c                       # (clause 13 still broken)
            assert call(p=p, obs=None, veh=None, plans=None, cloud=None, mask=None) == (DEV if c == len(broken) else ARG), c
        # an argument error wins over the missing device, over n == 0, m == 0 and over the pointers
        assert call(p=par(window=-1), n=0, veh=None) == ARG and call(p=par(window=-1), m=0, obs=None) == ARG
        assert call(n_cloud=147, veh=None, mask=None) == ARG
        # every rule passes: the device is looked at next, then n == 0, m == 0 and the pointers
        assert call() == DEV
        assert call(p=par(points=1), n_cloud=76, mask_words=3) == DEV
        assert call(p=par(stride=(1 << 31) - 1, samples=1, first_point=0, first_instant=(1 << 31) - 1, window=(1 << 31) - 1), n_cloud=21, mask_words=1) == DEV
        assert call(n=0) == DEV and call(m=0, n_cloud=64, mask_words=2) == DEV and call(m=0, n_cloud=0, mask_words=0, p=par(first_point=0)) == DEV
        assert call(obs=None, veh=None, plans=None, cloud=None, mask=None) == DEV
    finally:
        L.fh_destroy(h)
    with pytest.raises(capi.FasterHipError):
        capi.Context.fleet_obstacles_device(None, np.zeros(4), None, 1, 0, None, None, 1, 8, None, 0, None, 0)
    with pytest.raises(capi.FasterHipError):   # (a record of the timed traffic is not taken for this one)
        capi.Context.fleet_obstacles_device(None, abi.default_traffic_timed_params(4, 2, 6.0), None, 1, 0, None, None, 1, 8, None, 0, None, 0)


def test_every_argument_rule_of_the_audit_in_prologue_order(built):
    from faster_amd import capi

    L = capi.lib()
    h = ctypes.c_void_p()
    assert L.fh_create(ctypes.byref(h), 1 << 20) == DEV and h.value
    buf = np.zeros(8192, dtype=np.uint8)
    d = abi.ptr(buf)

    def par(**kw):
        p = np.ascontiguousarray(abi.default_obstacle_audit_params(0.3, 0.01, stride=2, count=5)).reshape(1)
        for k, v in kw.items():
            p[k] = v
        return p

    def call(ctx=h, p=par(), m=3, tick0=5, n=2, max_states=8, obs=d, veh=d, plans=d, out=d):
        return L.fh_fleet_obstacle_audit_device(ctx, None if p is None else abi.ptr(p), obs, m, tick0, veh, plans, n, max_states, out)

    nan, inf = float("nan"), float("inf")
    try:
        assert call(ctx=None) == ARG and call(p=None) == ARG
        for v in (nan, inf, -inf, -1e-300, -0.3):
            assert call(p=par(r=v)) == ARG, v
        assert call(p=par(r=0.0)) == DEV
        for v in (nan, inf, -inf, 0.0, -0.01):
            assert call(p=par(dc=v)) == ARG, v
        assert call(p=par(stride=0)) == ARG and call(p=par(stride=-1)) == ARG and call(p=par(count=-1)) == ARG
        assert call(n=-1) == ARG and call(m=-1) == ARG and call(max_states=0) == ARG
        assert call(tick0=-1) == ARG and call(tick0=(1 << 62) + 1) == ARG and call(tick0=1 << 62) == DEV
        broken = [("r", nan), ("dc", nan), ("stride", 0), ("count", -1)]
        good = dict((k, par()[k][0]) for k, _ in broken)
        for c in range(len(broken) + 1):
            p = par(**dict([(k, good[k]) for k, _ in broken[:c]] + broken[c:]))
            assert call(p=p, n=-1, tick0=-1, veh=None) == ARG, c
            assert call(p=p, tick0=-1, veh=None) == ARG, c
            assert call(p=p, obs=None, veh=None, plans=None, out=None) == (DEV if c == len(broken) else ARG), c
        assert call(p=par(count=-1), n=0, veh=None) == ARG
        assert call() == DEV and call(n=0) == DEV and call(m=0, obs=None) == DEV and call(obs=None, veh=None, plans=None, out=None) == DEV
    finally:
        L.fh_destroy(h)
    with pytest.raises(capi.FasterHipError):   # (a record of the stage is not taken for the audit's)
        capi.Context.fleet_obstacle_audit_device(None, abi.default_obstacle_params(4, 2, 6.0, 0.01), None, 1, 0, None, None, 1, 8, None)
