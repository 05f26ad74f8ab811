"""CPU-side checks of the certificate entry points (fh_certify_batch_device, fh_certify_batch): declared in include/fasterhip_certify.h and
not in fasterhip.h, the header compiles alone as C99 and C++11, exported, bound in faster_amd/capi.py, the struct layouts of the header
equal the dtypes of faster_amd/abi.py, and the argument prologue in the order of tests/test_abi_return_codes.py with no CPU path."""
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
CERT_HDR = os.path.join(INC, "fasterhip_certify.h")
NEW = ["fh_certify_batch_device", "fh_certify_batch"]
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
    assert set(NEW) <= _declared(CERT_HDR)
    assert not set(NEW) & _declared(HDR)   # fasterhip.h is pinned to capi.SYMBOLS (tests/test_abi.py): the new ones stay out of it
    assert int(re.search(r"#define FH_ABI_VERSION (\d+)", open(HDR).read()).group(1)) == abi.FH_ABI_VERSION == 9
    src = "#include \"fasterhip_certify.h\"\nint main(void) {\n" + "".join("  (void)%s;\n" % n for n in NEW) + "  return 0;\n}\n"
    for lang, std, comp in (("c", "-std=c99", "gcc"), ("c++", "-std=c++11", "g++")):
        f = tmp_path / ("probe." + ("c" if lang == "c" else "cpp"))
        f.write_text(src)
        r = subprocess.run([comp, "-fsyntax-only", "-x", lang, std, "-Wall", "-pedantic", "-I", INC, str(f)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr.strip(), (lang, r.stderr[-2000:])


def test_struct_layouts_of_the_header_equal_the_dtypes(tmp_path):
    """sizeof and every offsetof, printed by a C program compiled against the header."""
    fields = {"fh_certificate": (abi.certificate_dtype, 128), "fh_certify_tol": (abi.certify_tol_dtype, 32)}
    lines = []
    for s, (dt, _) in fields.items():
        lines.append('  printf("%s %%d\\n", (int)sizeof(%s));' % (s, s))
        lines += ['  printf("%s.%s %%d\\n", (int)offsetof(%s, %s));' % (s, k, s, k) for k in dt.names]
    flags = ["UNSOLVED", "BAD_INPUT", "NOT_FINITE", "CORRIDOR", "ASSIGNMENT", "X0", "XF", "CONTINUITY", "BOX", "COST"]
    lines += ['  printf("FH_CERT_%s %%d\\n", (int)FH_CERT_%s);' % (k, k) for k in flags]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"fasterhip_certify.h\"\nint main(void) {\n" + "\n".join(lines) + "\n  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", INC, str(src), "-o", str(exe)])
    got = dict((k, int(v)) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()))
    for s, (dt, size) in fields.items():
        assert got[s] == dt.itemsize == size, s
        for k in dt.names:
            assert got["%s.%s" % (s, k)] == dt.fields[k][1], (s, k)
    for k in flags:
        assert got["FH_CERT_" + k] == getattr(abi, "FH_CERT_" + k), k
    assert [getattr(abi, "FH_CERT_" + k) for k in flags] == [1 << i for i in range(10)]


def test_symbols_are_exported_and_bound(built):
    from faster_amd import capi
    from faster_amd.fleet import Fleet

    L = ctypes.CDLL(built.SO)
    for name in NEW:
        assert hasattr(L, name), name
    assert sorted(capi.CERTIFY_SYMBOLS) == sorted(NEW)
    assert not set(NEW) & set(capi.SYMBOLS) and not set(NEW) & set(capi.OCCUPANCY_SYMBOLS)
    for method in ("certify_batch", "certify_batch_device"):
        assert hasattr(capi.Context, method), method
    for method in ("certify", "faces"):
        assert hasattr(Fleet, method), method


def test_the_argument_prologue_in_order(built):
    """null context, then the arguments (n < 0, n_faces < 0, a tolerance that is negative or NaN), then FH_ERR_DEVICE on a context without
    a device — never a CPU path; n == 0 and the pointers are looked at after the device."""
    from faster_amd import capi

    L = capi.lib()
    h = ctypes.c_void_p()
    assert L.fh_create(ctypes.byref(h), 1 << 20) == DEV and h.value
    buf = np.zeros(8192, dtype=np.uint8)
    d = abi.ptr(buf)
    good = abi.ptr(np.ascontiguousarray(abi.certify_tol(1e-9)).reshape(1))
    try:
        for fn in (L.fh_certify_batch_device, L.fh_certify_batch):
            assert fn(None, d, d, 4, d, 1, None, d) == ARG
            assert fn(None, d, d, 4, d, -1, None, d) == ARG
            assert fn(h, d, d, 4, d, -1, None, d) == ARG
            assert fn(h, d, d, -1, d, 1, None, d) == ARG
            for k in abi.certify_tol_dtype.names:
                for v in (-1e-300, -1.0, float("nan"), -float("inf")):
                    t = np.ascontiguousarray(abi.certify_tol(1e-9)).reshape(1)
                    t[k] = v
                    assert fn(h, d, d, 4, d, 1, abi.ptr(t), d) == ARG, (k, v)
            assert fn(h, d, d, 4, d, 1, None, d) == DEV
            assert fn(h, d, d, 4, d, 1, good, d) == DEV
            t = np.ascontiguousarray(abi.certify_tol(0.0, float("inf"), 0.0, 0.0)).reshape(1)   # zero and +inf are tolerances
            assert fn(h, d, d, 4, d, 1, abi.ptr(t), d) == DEV
            assert fn(h, d, d, 4, d, 0, None, d) == DEV          # (an empty batch is looked at after the device)
            assert fn(h, None, None, 4, None, 1, None, None) == DEV   # (pointers too)
    finally:
        L.fh_destroy(h)
    with pytest.raises(capi.FasterHipError):
        capi.Context._certify_tol(np.zeros(4))
