"""CPU-side checks of the traffic entry point (fh_fleet_traffic_device): declared in include/fasterhip_traffic.h and not in fasterhip.h,
the header compiles alone as C99 and C++11, exported, bound in faster_amd/capi.py, the struct layout of the header equals the dtype of
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
TRAFFIC_HDR = os.path.join(INC, "fasterhip_traffic.h")
NEW = ["fh_fleet_traffic_device"]
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
    assert set(NEW) <= _declared(TRAFFIC_HDR)
    assert not set(NEW) & _declared(HDR)   # fasterhip.h is pinned to capi.SYMBOLS (tests/test_abi.py): the new one stays out of it
    assert int(re.search(r"#define FH_ABI_VERSION (\d+)", open(HDR).read()).group(1)) == abi.FH_ABI_VERSION == 9
    src = "#include \"fasterhip_traffic.h\"\nint main(void) {\n" + "".join("  (void)%s;\n" % n for n in NEW) + "  return 0;\n}\n"
    for lang, std, comp in (("c", "-std=c99", "gcc"), ("c++", "-std=c++11", "g++")):
        f = tmp_path / ("probe." + ("c" if lang == "c" else "cpp"))
        f.write_text(src)
        r = subprocess.run([comp, "-fsyntax-only", "-x", lang, std, "-Wall", "-pedantic", "-I", INC, str(f)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr.strip(), (lang, r.stderr[-2000:])


def test_struct_layout_and_constants_of_the_header_equal_abi_py(tmp_path):
    """sizeof and every offsetof, printed by a C program compiled against the header."""
    s, dt = "fh_traffic_params", abi.traffic_params_dtype
    lines = ['  printf("%s %%d\\n", (int)sizeof(%s));' % (s, s)]
    lines += ['  printf("%s.%s %%d\\n", (int)offsetof(%s, %s));' % (s, k, s, k) for k in dt.names]
    consts = ["ALL", "YIELD_TO_LOWER"]
    lines += ['  printf("FH_TRAFFIC_%s %%d\\n", (int)FH_TRAFFIC_%s);' % (k, k) for k in consts]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"fasterhip_traffic.h\"\nint main(void) {\n" + "\n".join(lines)
                   + "\n  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", INC, str(src), "-o", str(exe)])
    got = dict((k, int(v)) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()))
    assert got[s] == dt.itemsize == 48
    for k in dt.names:
        assert got["%s.%s" % (s, k)] == dt.fields[k][1], k
    assert [got["FH_TRAFFIC_" + k] for k in consts] == [abi.FH_TRAFFIC_ALL, abi.FH_TRAFFIC_YIELD_TO_LOWER] == [0, 1]
    assert dt.names == ("range", "hull", "samples", "stride", "rule", "first_point", "reserved")


def test_symbol_is_exported_and_bound(built):
    from faster_amd import capi
    from faster_amd.fleet import Fleet

    L = ctypes.CDLL(built.SO)
    for name in NEW:
        assert hasattr(L, name), name
    assert sorted(capi.TRAFFIC_SYMBOLS) == sorted(NEW)
    others = (set(capi.SYMBOLS) | set(capi.OCCUPANCY_SYMBOLS) | set(capi.CERTIFY_SYMBOLS) | set(capi.AUDIT_SYMBOLS)
              | set(capi.SEPARATION_SYMBOLS))
    assert not set(NEW) & others
    assert hasattr(capi.Context, "fleet_traffic_device") and hasattr(Fleet, "enable_traffic") and hasattr(Fleet, "traffic")
    assert os.path.join(INC, "fasterhip_traffic.h") in built.DEPS   # (a change of the header rebuilds the library)


def test_every_argument_rule_in_prologue_order(built):
    """null context, null params, range, hull, samples, stride, rule, first_point, n, max_states, the extent of the traffic in the cloud
    and in the masks; then FH_ERR_DEVICE on a context without a device (never a CPU path); n == 0 and the pointers are looked at after
    the device.  Each clause is shown to win over every later one by a call that breaks all later ones too."""
    from faster_amd import capi

    L = capi.lib()
    h = ctypes.c_void_p()
    assert L.fh_create(ctypes.byref(h), 1 << 20) == DEV and h.value
    buf = np.zeros(8192, dtype=np.uint8)
    d = abi.ptr(buf)

    def par(**kw):
        p = np.ascontiguousarray(abi.default_traffic_params(4, 2, 6.0, hull=0.3, first_point=64)).reshape(1)
        for k, v in kw.items():
            p[k] = v
        return p

    def call(ctx=h, p=par(), n=3, max_states=8, n_cloud=64 + 3 * 4 * 7, mask_words=5, veh=d, plans=d, cloud=d, mask=d):
        return L.fh_fleet_traffic_device(ctx, None if p is None else abi.ptr(p), veh, plans, n, max_states, cloud, n_cloud, mask, mask_words)

    nan, inf = float("nan"), float("inf")
    try:
        # 1. the context, then the params
        assert call(ctx=None) == ARG
        assert call(ctx=None, p=None) == ARG
        assert call(p=None) == ARG
        # 2. range: NaN, infinite or <= 0
        for v in (nan, inf, -inf, 0.0, -0.0, -1.0, -1e-300):
            assert call(p=par(range=v)) == ARG, v
        # 3. hull: NaN, infinite or negative (zero is one point per sample)
        for v in (nan, inf, -inf, -1e-300, -0.3):
            assert call(p=par(hull=v)) == ARG, v
        # 4. samples, 5. stride, 6. rule, 7. first_point
        assert call(p=par(samples=0)) == ARG and call(p=par(samples=-4)) == ARG
        assert call(p=par(stride=0)) == ARG and call(p=par(stride=-1)) == ARG
        assert call(p=par(rule=2)) == ARG and call(p=par(rule=-1)) == ARG
        assert call(p=par(first_point=-32)) == ARG and call(p=par(first_point=33)) == ARG and call(p=par(first_point=16)) == ARG
        # 8. n, 9. max_states
        assert call(n=-1) == ARG and call(max_states=0) == ARG and call(max_states=-5) == ARG
        # 10. the traffic must fit the cloud and the masks: 64 + 3 * 4 * 7 = 148 points, 5 words
        assert call(n_cloud=147) == ARG and call(mask_words=4) == ARG and call(n_cloud=0) == ARG and call(mask_words=-1) == ARG
        assert call(p=par(hull=0.0), n_cloud=75) == ARG and call(p=par(hull=0.0), mask_words=2) == ARG   # 64 + 12 = 76 points, 3 words
        assert call(p=par(samples=1 << 30, first_point=0), n=1 << 30, n_cloud=(1 << 31) - 1, mask_words=(1 << 31) - 1) == ARG   # (64 bits)
        assert call(p=par(samples=(1 << 31) - 1, first_point=0), n=(1 << 31) - 1, n_cloud=1, mask_words=1) == ARG
        # in order: an argument error wins over the missing device, whatever comes later
        assert call(p=par(range=nan, hull=nan, samples=0, stride=0, rule=7, first_point=-1), n=-1, max_states=0, n_cloud=0) == ARG
        assert call(p=par(stride=0), n=0, veh=None) == ARG
        assert call(n_cloud=147, n=3, veh=None, mask=None) == ARG
        # every rule passes: the device is looked at next, then n == 0 and the pointers
        assert call() == DEV
        assert call(p=par(hull=0.0), n_cloud=76, mask_words=3) == DEV
        assert call(p=par(rule=1, stride=1000, samples=1, first_point=0), n_cloud=21, mask_words=1) == DEV
        assert call(n=0, n_cloud=64, mask_words=2) == DEV and call(n=0, n_cloud=0, mask_words=0, p=par(first_point=0)) == DEV
        assert call(veh=None, plans=None, cloud=None, mask=None) == DEV
    finally:
        L.fh_destroy(h)
    with pytest.raises(capi.FasterHipError):
        capi.Context.fleet_traffic_device(None, np.zeros(4), None, None, 1, 8, None, 0, None, 0)
