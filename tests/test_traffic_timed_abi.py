"""CPU-side checks of the time-aware traffic entry point (fh_fleet_traffic_timed_device): declared in include/fasterhip_traffic_timed.h and
in no other header, the header compiles alone as C99 and C++11, exported, bound in faster_amd/capi.py in a tuple of its own, the struct
layout and the constant of the header equal faster_amd/abi.py, and every argument rule in the order of the prologue, with no CPU path."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from faster_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
TIMED_HDR = os.path.join(INC, "fasterhip_traffic_timed.h")
NEW = ["fh_fleet_traffic_timed_device"]
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
    assert set(NEW) <= _declared(TIMED_HDR)
    for other in ("fasterhip.h", "fasterhip_traffic.h"):   # (both pinned: tests/test_abi.py, tests/test_traffic_abi.py)
        assert not set(NEW) & _declared(os.path.join(INC, other)), other
    assert '#include "fasterhip_traffic.h"' in open(TIMED_HDR).read()
    assert int(re.search(r"#define FH_ABI_VERSION (\d+)", open(os.path.join(INC, "fasterhip.h")).read()).group(1)) == abi.FH_ABI_VERSION == 9
    src = "#include \"fasterhip_traffic_timed.h\"\nint main(void) {\n" + "".join("  (void)%s;\n" % n for n in NEW) + "  return 0;\n}\n"
    for lang, std, comp in (("c", "-std=c99", "gcc"), ("c++", "-std=c++11", "g++")):
        f = tmp_path / ("probe." + ("c" if lang == "c" else "cpp"))
        f.write_text(src)
        r = subprocess.run([comp, "-fsyntax-only", "-x", lang, std, "-Wall", "-pedantic", "-I", INC, str(f)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr.strip(), (lang, r.stderr[-2000:])


def test_struct_layout_and_constants_of_the_header_equal_abi_py(tmp_path):
    """sizeof and every offsetof, printed by a C program compiled against the header."""
    s, dt = "fh_traffic_timed_params", abi.traffic_timed_params_dtype
    lines = ['  printf("%s %%d\\n", (int)sizeof(%s));' % (s, s)]
    lines += ['  printf("%s.%s %%d\\n", (int)offsetof(%s, %s));' % (s, k, s, k) for k in dt.names]
    lines += ['  printf("MAX %d\\n", (int)FH_TRAFFIC_TIMED_MAX_SAMPLES);']
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"fasterhip_traffic_timed.h\"\nint main(void) {\n" + "\n".join(lines)
                   + "\n  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", INC, str(src), "-o", str(exe)])
    got = dict((k, int(v)) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()))
    assert got[s] == dt.itemsize == 48
    for k in dt.names:
        assert got["%s.%s" % (s, k)] == dt.fields[k][1], k
    assert got["MAX"] == abi.FH_TRAFFIC_TIMED_MAX_SAMPLES == 512
    assert dt.names == ("range", "hull", "samples", "stride", "rule", "first_point", "first_instant", "window", "reserved")
    assert dt.fields["reserved"][0].shape == (2,)
    for k in ("range", "hull", "samples", "stride", "rule", "first_point"):   # (the common fields lie where fh_traffic_params has them)
        assert dt.fields[k][1] == abi.traffic_params_dtype.fields[k][1], k


def test_symbol_is_exported_and_bound(built):
    from faster_amd import capi
    from faster_amd.fleet import Fleet
    import inspect

    L = ctypes.CDLL(built.SO)
    for name in NEW:
        assert hasattr(L, name), name
    assert sorted(capi.TRAFFIC_TIMED_SYMBOLS) == sorted(NEW)
    others = (set(capi.SYMBOLS) | set(capi.OCCUPANCY_SYMBOLS) | set(capi.CERTIFY_SYMBOLS) | set(capi.AUDIT_SYMBOLS)
              | set(capi.SEPARATION_SYMBOLS) | set(capi.TRAFFIC_SYMBOLS) | set(capi.CHECK_SYMBOLS))
    assert not set(NEW) & others
    assert capi.TRAFFIC_SYMBOLS == ["fh_fleet_traffic_device"]
    assert hasattr(capi.Context, "fleet_traffic_timed_device")
    sig = inspect.signature(Fleet.enable_traffic).parameters
    assert sig["timed"].default is False and sig["window"].default == 0 and sig["first_instant"].default is None
    assert TIMED_HDR in built.DEPS   # (a change of the header rebuilds the library)
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "capi.TRAFFIC_TIMED_SYMBOLS" in entry


def test_every_argument_rule_in_prologue_order(built):
    """null context or params, range, hull, samples (and the cap), stride, rule, first_point, first_instant, window, n and max_states, the
    extent of the traffic in the cloud and in the masks; then FH_ERR_DEVICE on a context without a device (never a CPU path); n == 0 and
    the pointers are looked at after the device.  A context without a device answers FH_ERR_ARG for every broken rule, so the order
    itself is shown from the other side: with everything BEFORE a clause right and everything after it wrong the answer is FH_ERR_ARG,
    and mending the clauses one by one from the first on turns FH_ERR_ARG into FH_ERR_DEVICE only with the last."""
    from faster_amd import capi

    L = capi.lib()
    h = ctypes.c_void_p()
    assert L.fh_create(ctypes.byref(h), 1 << 20) == DEV and h.value
    buf = np.zeros(8192, dtype=np.uint8)
    d = abi.ptr(buf)

    def par(**kw):
        p = np.ascontiguousarray(abi.default_traffic_timed_params(4, 2, 6.0, hull=0.3, first_point=64, first_instant=9, window=1)).reshape(1)
        for k, v in kw.items():
            p[k] = v
        return p

    def call(ctx=h, p=par(), n=3, max_states=8, n_cloud=64 + 3 * 4 * 7, mask_words=5, veh=d, plans=d, cloud=d, mask=d):
        return L.fh_fleet_traffic_timed_device(ctx, None if p is None else abi.ptr(p), veh, plans, n, max_states, cloud, n_cloud, mask, mask_words)

    nan, inf = float("nan"), float("inf")
    try:
        # 1. the context or the params
        assert call(ctx=None) == ARG
        assert call(ctx=None, p=None) == ARG
        assert call(p=None) == ARG
        # 2. range: NaN, infinite or <= 0
        for v in (nan, inf, -inf, 0.0, -0.0, -1.0, -1e-300):
            assert call(p=par(range=v)) == ARG, v
        # 3. hull: NaN, infinite or negative (zero is one point per sample)
        for v in (nan, inf, -inf, -1e-300, -0.3):
            assert call(p=par(hull=v)) == ARG, v
        # 4. samples and the cap: 512 is served, 513 is not
        assert call(p=par(samples=0)) == ARG and call(p=par(samples=-4)) == ARG
        big = dict(n=1, n_cloud=64 + 513 * 7, mask_words=(64 + 513 * 7 + 31) // 32)
        assert call(p=par(samples=abi.FH_TRAFFIC_TIMED_MAX_SAMPLES), **big) == DEV
        assert call(p=par(samples=abi.FH_TRAFFIC_TIMED_MAX_SAMPLES + 1), **big) == ARG
        assert call(p=par(samples=(1 << 31) - 1), **big) == ARG
        # 5. stride, 6. rule, 7. first_point, 8. first_instant, 9. window
        assert call(p=par(stride=0)) == ARG and call(p=par(stride=-1)) == ARG
        assert call(p=par(rule=2)) == ARG and call(p=par(rule=-1)) == ARG
        assert call(p=par(first_point=-32)) == ARG and call(p=par(first_point=33)) == ARG and call(p=par(first_point=16)) == ARG
        assert call(p=par(first_instant=-1)) == ARG and call(p=par(first_instant=-(1 << 31))) == ARG
        assert call(p=par(window=-1)) == ARG and call(p=par(window=-(1 << 31))) == ARG
        # 10. n and max_states
        assert call(n=-1) == ARG and call(max_states=0) == ARG and call(max_states=-5) == ARG
        # 11. the traffic must fit the cloud and the masks: 64 + 3 * 4 * 7 = 148 points, 5 words; in 64 bits
        assert call(n_cloud=147) == ARG and call(mask_words=4) == ARG and call(n_cloud=0) == ARG and call(mask_words=-1) == ARG
        assert call(p=par(hull=0.0), n_cloud=75) == ARG and call(p=par(hull=0.0), mask_words=2) == ARG   # 64 + 12 = 76 points, 3 words
        assert call(p=par(samples=512, first_point=0), n=(1 << 31) - 1, n_cloud=(1 << 31) - 1, mask_words=(1 << 31) - 1) == ARG   # 2^40 samples
        assert call(p=par(samples=512, first_point=0, hull=0.0), n=1 << 23, n_cloud=(1 << 31) - 1, mask_words=(1 << 31) - 1) == ARG   # 2^32: wraps to 0
        assert call(p=par(samples=512, first_point=(1 << 31) - 32, hull=0.0), n=1, n_cloud=(1 << 31) - 1, mask_words=(1 << 31) - 1) == ARG
        # the order: clause c broken together with every later one is FH_ERR_ARG; mended from the first on, the device shows at the end
        broken = [("range", nan), ("hull", nan), ("samples", 513), ("stride", 0), ("rule", 7), ("first_point", -1), ("first_instant", -1), ("window", -1)]
        good = dict((k, par()[k][0]) for k, _ in broken)
        for c in range(len(broken) + 1):
            p = par(**dict([(k, good[k]) for k, _ in broken[:c]] + broken[c:]))
            assert call(p=p, n=-1, max_states=0, n_cloud=0, veh=None) == ARG, c            # (clauses 10 and 11 still broken)
            assert call(p=p, n=3, max_states=8, n_cloud=0, veh=None) == ARG, c             # (clause 11 still broken)
            assert call(p=p, veh=None, plans=None, cloud=None, mask=None) == (DEV if c == len(broken) else ARG), c
        # an argument error wins over the missing device, over n == 0 and over the pointers
        assert call(p=par(window=-1), n=0, veh=None) == ARG
        assert call(n_cloud=147, n=3, veh=None, mask=None) == ARG
        # every rule passes: the device is looked at next, then n == 0 and the pointers
        assert call() == DEV
        assert call(p=par(hull=0.0), n_cloud=76, mask_words=3) == DEV
        assert call(p=par(rule=1, stride=(1 << 31) - 1, samples=1, first_point=0, first_instant=(1 << 31) - 1, window=(1 << 31) - 1), n_cloud=21, mask_words=1) == DEV
        assert call(n=0, n_cloud=64, mask_words=2) == DEV and call(n=0, n_cloud=0, mask_words=0, p=par(first_point=0)) == DEV
        assert call(veh=None, plans=None, cloud=None, mask=None) == DEV
    finally:
        L.fh_destroy(h)
    with pytest.raises(capi.FasterHipError):
        capi.Context.fleet_traffic_timed_device(None, np.zeros(4), None, None, 1, 8, None, 0, None, 0)
    with pytest.raises(capi.FasterHipError):   # (a record of the untimed struct is not taken for a timed one)
        capi.Context.fleet_traffic_timed_device(None, abi.default_traffic_params(4, 2, 6.0), None, None, 1, 8, None, 0, None, 0)
