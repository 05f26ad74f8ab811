"""CPU-side checks of the priority rounds' entry points (fh_fleet_round_classes_device, fh_fleet_round_gate_device): declared in
include/fasterhip_rounds.h and not in fasterhip.h, the header compiles alone as C99 and C++11, exported, bound in faster_amd/capi.py,
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
ROUNDS_HDR = os.path.join(INC, "fasterhip_rounds.h")
NEW = ["fh_fleet_round_classes_device", "fh_fleet_round_gate_device"]
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
    assert set(NEW) <= _declared(ROUNDS_HDR)
    assert not set(NEW) & _declared(HDR)   # fasterhip.h is pinned to capi.SYMBOLS (tests/test_abi.py): the new ones stay out of it
    assert int(re.search(r"#define FH_ABI_VERSION (\d+)", open(HDR).read()).group(1)) == abi.FH_ABI_VERSION == 9
    src = "#include \"fasterhip_rounds.h\"\nint main(void) {\n" + "".join("  (void)%s;\n" % n for n in NEW) + "  return 0;\n}\n"
    for lang, std, comp in (("c", "-std=c99", "gcc"), ("c++", "-std=c++11", "g++")):
        f = tmp_path / ("probe." + ("c" if lang == "c" else "cpp"))
        f.write_text(src)
        r = subprocess.run([comp, "-fsyntax-only", "-x", lang, std, "-Wall", "-pedantic", "-I", INC, str(f)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr.strip(), (lang, r.stderr[-2000:])


def test_struct_layouts_and_constants_of_the_header_equal_abi_py(tmp_path):
    """sizeof and every offsetof, printed by a C program compiled against the header."""
    fields = {"fh_round_params": (abi.round_params_dtype, 32), "fh_plan_round": (abi.plan_round_dtype, 16)}
    lines = []
    for s, (dt, _) in fields.items():
        lines.append('  printf("%s %%d\\n", (int)sizeof(%s));' % (s, s))
        lines += ['  printf("%s.%s %%d\\n", (int)offsetof(%s, %s));' % (s, k, s, k) for k in dt.names]
    consts = ["FH_ROUNDS_MAX", "FH_ROUNDS_LIST", "FH_ROUNDS_MAX_PASSES", "FH_ROUNDS_MAX_CELLS", "FH_ROUND_RESTORE", "FH_ROUND_RETRY",
              "FH_ROUND_OVERFLOW", "FH_ROUND_UNSETTLED", "FH_ROUND_NOT_FINITE", "FH_ROUND_BAD_PLAN"]
    lines += ['  printf("%s %%d\\n", (int)%s);' % (k, k) for k in consts]
    lines += ['  printf("vehicle.active %d\\n", (int)offsetof(fh_vehicle, active));']
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"fasterhip_rounds.h\"\nint main(void) {\n" + "\n".join(lines)
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
    assert [getattr(abi, k) for k in consts] == [64, 64, 1024, 1 << 20, -1, -2, 1, 2, 4, 8]
    # round_class and decided_pass are one aligned word of 8 bytes
    assert (got["fh_plan_round.round_class"], got["fh_plan_round.decided_pass"]) == (0, 4)
    assert got["vehicle.active"] == abi.vehicle_dtype.fields["active"][1]


def test_symbols_are_exported_and_bound(built):
    from faster_amd import capi
    from faster_amd.fleet import Fleet

    L = ctypes.CDLL(built.SO)
    for name in NEW:
        assert hasattr(L, name), name
    assert sorted(capi.ROUNDS_SYMBOLS) == sorted(NEW)
    others = (set(capi.SYMBOLS) | set(capi.OCCUPANCY_SYMBOLS) | set(capi.CERTIFY_SYMBOLS) | set(capi.AUDIT_SYMBOLS) | set(capi.SEPARATION_SYMBOLS)
              | set(capi.TRAFFIC_SYMBOLS) | set(capi.TRAFFIC_TIMED_SYMBOLS) | set(capi.CHECK_SYMBOLS))
    assert not set(NEW) & others
    for name in ("fleet_round_classes_device", "fleet_round_gate_device"):
        assert hasattr(capi.Context, name), name
    for name in ("enable_rounds", "round_records", "check_records_by_round"):
        assert hasattr(Fleet, name), name
    assert ROUNDS_HDR in built.DEPS   # (a change of the header rebuilds the library)
    p = abi.default_round_params(1.2, 3)
    assert (float(p["reach"]), int(p["rounds"]), int(p["passes"]), int(p["stride"]), int(p["count"])) == (1.2, 3, 32, 1, 0) and not p["reserved"].any()


def test_every_argument_rule_in_prologue_order(built):
    """null context, null params, the numbers of the params in the header's order, n and max_states, the grid, then FH_ERR_DEVICE on a
    context without a device (never a CPU path); n == 0 and the pointers are looked at after the device."""
    from faster_amd import capi

    L = capi.lib()
    h = ctypes.c_void_p()
    assert L.fh_create(ctypes.byref(h), 1 << 20) == DEV and h.value
    buf = np.zeros(8192, dtype=np.uint8)
    buf2 = np.zeros(64, dtype=np.uint8)
    d, d2 = abi.ptr(buf), abi.ptr(buf2)

    def grid(res=1.0, dims=(40, 36, 12)):
        g = np.zeros(1, dtype=abi.voxel_grid_dtype)
        g["origin"], g["res"], g["dims"] = (0.1, 0.2, 0.3), res, dims
        return g

    def par(**kw):
        p = np.ascontiguousarray(abi.default_round_params(1.2, 3)).reshape(1)
        for k, v in kw.items():
            p[k] = v
        return p

    def call(ctx=h, p=par(), n=1, max_states=8, g=grid(), veh=d, plans=d, out=d):
        return L.fh_fleet_round_classes_device(ctx, None if p is None else abi.ptr(p), veh, plans, n, max_states, None if g is None else abi.ptr(g),
                                               out)

    nan, inf = float("nan"), float("inf")
    try:
        # 1. the context, then the params
        assert call(ctx=None) == ARG and call(ctx=None, p=None) == ARG and call(p=None) == ARG and call(p=None, g=None, n=-1) == ARG
        # 2. the numbers, each alone
        for v in (nan, -1e-300, -1.0, inf, -inf):
            assert call(p=par(reach=v)) == ARG, v
        for v in (0, -1, 65, 1 << 30):
            assert call(p=par(rounds=v)) == ARG, v
        for v in (-1, 1025):
            assert call(p=par(passes=v)) == ARG, v
        assert call(p=par(stride=0)) == ARG and call(p=par(stride=-3)) == ARG and call(p=par(count=-1)) == ARG
        assert call(n=-1) == ARG and call(max_states=0) == ARG
        # 3. the grid
        assert call(g=None) == ARG
        assert call(g=grid(res=0.0)) == ARG and call(g=grid(res=-1.0)) == ARG and call(g=grid(res=nan)) == ARG
        for dims in ((0, 36, 12), (40, 0, 12), (40, 36, -1)):
            assert call(g=grid(dims=dims)) == ARG, dims
        assert call(g=grid(dims=(1024, 1024, 2))) == ARG and call(g=grid(dims=(1 << 20, 1, 2))) == ARG   # more than FH_ROUNDS_MAX_CELLS
        assert call(g=grid(dims=(1 << 16, 1 << 16, 1 << 16))) == ARG                   # (a product that does not fit 32 bits)
        # in order: every rule is an argument error before the missing device, whatever comes later; with all of them broken too
        for broken in (dict(p=par(reach=nan)), dict(p=par(rounds=0)), dict(p=par(passes=-1)), dict(p=par(stride=0)), dict(p=par(count=-1)),
                       dict(n=-1), dict(max_states=0), dict(g=grid(dims=(0, 36, 12)))):
            kw = dict(n=0, veh=None)
            kw.update(broken)
            assert call(**kw) == ARG, broken
        # 4. every rule passes: the device is looked at next, 5. / 6. then n == 0 and the pointers
        assert call() == DEV
        assert call(p=par(reach=0.0)) == DEV                                           # zero is a reach
        assert call(p=par(rounds=1)) == DEV and call(p=par(rounds=64)) == DEV
        assert call(p=par(passes=0)) == DEV and call(p=par(passes=1024)) == DEV
        assert call(p=par(count=5, stride=7)) == DEV
        assert call(g=grid(dims=(1, 1, 1))) == DEV and call(g=grid(dims=(1024, 1024, 1))) == DEV   # exactly FH_ROUNDS_MAX_CELLS
        assert call(n=0) == DEV
        assert call(veh=None, plans=None, out=None) == DEV

        # the gate: the context; round, n and the two active arrays being one; then the device; the pointers after it
        def gate(ctx=h, rounds=d, rnd=0, begin=d, n=1, veh=d, active=d2):
            return L.fh_fleet_round_gate_device(ctx, rounds, rnd, begin, n, veh, active)

        assert gate(ctx=None) == ARG and gate(ctx=None, rnd=-3) == ARG
        assert gate(rnd=-3) == ARG and gate(rnd=64) == ARG and gate(rnd=1 << 30) == ARG and gate(n=-1) == ARG
        assert gate(begin=d, active=d) == ARG and gate(begin=None, active=None) == ARG
        assert gate(rnd=-3, n=0, veh=None) == ARG
        for rnd in (0, 63, abi.FH_ROUND_RESTORE, abi.FH_ROUND_RETRY):
            assert gate(rnd=rnd) == DEV, rnd
        assert gate(n=0) == DEV and gate(rounds=None) == DEV and gate(veh=None) == DEV and gate(begin=None) == DEV
    finally:
        L.fh_destroy(h)
    with pytest.raises(capi.FasterHipError):
        capi.Context.fleet_round_classes_device(None, np.zeros(4), None, None, 1, 8, None, None)
