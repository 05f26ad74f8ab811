"""CPU-side checks of the fleet entry points (fh_fleet_*, fh_map_plan_batch_radius_device): declared in include/fasterhip.h, exported by
the library, fh_vehicle / fh_fleet_params laid out as faster_amd/abi.py describes them, and no CPU path without a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from faster_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "fasterhip.h")
NEW = ["fh_map_plan_batch_radius_device", "fh_fleet_init_device", "fh_fleet_begin_device", "fh_fleet_commit_device", "fh_fleet_next_goals_device"]


@pytest.fixture(scope="module")
def built():
    from faster_amd import build as fb

    fb.build_all()
    return fb


def test_new_entry_points_are_declared():
    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    declared = set(re.findall(r"\b(fh_[a-z_0-9]+)\s*\(", text))
    for name in NEW:
        assert name in declared, name
    for name in ("fh_vehicle", "fh_fleet_params", "FH_FLEET_STAGE_OVERFLOW", "FH_VEHICLE_GOAL_REACHED"):
        assert name in text, name


def test_header_with_the_fleet_declarations_compiles_alone(tmp_path):
    """A C99 and a C++11 translation unit that include only fasterhip.h and name every new entry point and struct."""
    src = "#include \"fasterhip.h\"\nfh_vehicle v; fh_fleet_params fp;\nint main(void) {\n" + "".join("  (void)%s;\n" % n for n in NEW) + \
          "  return (int)sizeof(v) + (int)sizeof(fp) + FH_FLEET_STAGE_OVERFLOW;\n}\n"
    for lang, std, comp in (("c", "-std=c99", "gcc"), ("c++", "-std=c++11", "g++")):
        f = tmp_path / ("probe." + ("c" if lang == "c" else "cpp"))
        f.write_text(src)
        r = subprocess.run([comp, "-fsyntax-only", "-x", lang, std, "-Wall", "-pedantic", "-I", os.path.dirname(HDR), str(f)], capture_output=True,
                           text=True)
        assert r.returncode == 0 and not r.stderr.strip(), (lang, r.stderr[-2000:])


def test_new_symbols_are_exported(built):
    from faster_amd import capi

    L = ctypes.CDLL(built.SO)
    for name in NEW:
        assert hasattr(L, name), name
        assert name in capi.SYMBOLS, name


def test_vehicle_and_fleet_params_layouts_match_the_numpy_dtypes(tmp_path):
    """sizeof / offsetof of every field of fh_vehicle and fh_fleet_params as gcc lays them out == abi.vehicle_dtype / abi.fleet_params_dtype."""
    checks = []
    for struct, dt in (("fh_vehicle", abi.vehicle_dtype), ("fh_fleet_params", abi.fleet_params_dtype)):
        checks.append(("sizeof(%s)" % struct, dt.itemsize))
        for name in dt.names:
            checks.append(("offsetof(%s, %s)" % (struct, name), dt.fields[name][1]))
    checks += [("offsetof(fh_fleet_params, rule.drone_radius)", abi.fleet_params_dtype.fields["rule"][1] + abi.pair_rule_dtype.fields["drone_radius"][1]),
               ("offsetof(fh_vehicle, state.jerk)", abi.vehicle_dtype.fields["state"][1] + abi.state_dtype.fields["jerk"][1])]
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"fasterhip.h\"\nint main(void) {\n" + \
          "".join("  printf(\"%%zu\\n\", (size_t)%s);\n" % expr for expr, _ in checks) + "  return 0;\n}\n"
    (tmp_path / "layout.c").write_text(src)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.dirname(HDR), str(tmp_path / "layout.c"), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    for (expr, want), g in zip(checks, got):
        assert g == want, (expr, g, want)
    assert len(got) == len(checks)


def test_default_fleet_params_are_the_reference_yaml():
    p = abi.default_fleet_params()
    assert p["delta_t"] == 10 and p["goal_radius"] == 0.3 and p["ra"] == 4.0 and (p["wdx"], p["wdy"], p["wdz"]) == (20.0, 20.0, 4.0)
    assert p["gamma_whole"] == p["gammap_whole"] == p["gamma_safe"] == p["gammap_safe"] == 20.0
    assert p["rule"]["mode"] == 2 and p["rule"]["drone_radius"] == 0.42


def test_fleet_entry_points_without_a_device(built):
    """Arguments are checked first (FH_ERR_ARG = -1), then the missing device is reported (FH_ERR_DEVICE = -2): never a CPU path."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from faster_amd import capi

    L = capi.lib()
    h = ctypes.c_void_p()
    assert L.fh_create(ctypes.byref(h), -1) == -2 and h.value
    dummy = np.zeros(64)
    d = abi.ptr(dummy)
    p = abi.default_fleet_params().reshape(1)
    bad = p.copy()
    bad["rule"]["mode"] = 0       # the fleet needs FASTER's rule for R (mode 1 or 2)
    pp, pb = abi.ptr(p), abi.ptr(bad)
    try:
        assert L.fh_fleet_init_device(h, pb, d, d, 4, 8, d, d) == -1
        assert L.fh_fleet_init_device(h, pp, d, d, 4, 8, d, d) == -2
        assert L.fh_fleet_begin_device(h, pp, d, d, 4, 0, d, d, d, d, d, d) == -1   # max_states
        assert L.fh_fleet_begin_device(h, pp, d, d, 4, 8, d, d, d, d, d, d) == -2
        assert L.fh_fleet_commit_device(h, pb, d, d, 4, 8, d, d, d, d, d) == -1
        assert L.fh_fleet_commit_device(h, pp, d, d, 4, 8, d, d, d, d, d) == -2
        assert L.fh_fleet_next_goals_device(h, d, d, 4, 8, 0, 1, d) == -1          # ticks
        assert L.fh_fleet_next_goals_device(h, d, d, 4, 8, 3, 1, d) == -2
        assert L.fh_map_plan_batch_radius_device(None, d, d, d, None, 4, 8, 0.0, 0, d, d, None) == -1
    finally:
        L.fh_destroy(h)
