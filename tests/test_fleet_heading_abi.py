"""CPU-side checks of the fleet's heading (fh_heading, fh_yaw_params, fh_fleet_heading_init_device, fh_fleet_set_headings_device,
fh_fleet_set_goals_device, fh_fleet_next_goals_yaw_device, fh_fleet_sense_fov_device): declared in include/fasterhip.h with the layout
of the numpy dtypes, exported and bound; the Python restatement of the yaw tick (tests/heading_model.py) equals a g++ build of
fhreplan::Planner tick by tick; the forward sensor model on an empty map is its closed form; and the inputs of the GPU yaw test keep
clear of every threshold at which the last bit of atan2 could decide."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from faster_amd import abi

import heading_model as hm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "fasterhip.h")
NEW = ["fh_fleet_heading_init_device", "fh_fleet_set_headings_device", "fh_fleet_set_goals_device", "fh_fleet_next_goals_yaw_device",
       "fh_fleet_sense_fov_device"]


@pytest.fixture(scope="module")
def built():
    from faster_amd import build as fb

    fb.build_all()
    return fb


def test_heading_entry_points_are_declared_and_the_header_compiles_alone(tmp_path):
    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    declared = set(re.findall(r"\b(fh_[a-z_0-9]+)\s*\(", text))
    for name in NEW:
        assert name in declared, name
    assert re.search(r"FH_VEHICLE_YAWING\s*=\s*3\b", text)
    src = "#include \"fasterhip.h\"\nint main(void) {\n" + "".join("  (void)%s;\n" % n for n in NEW) + "  return FH_VEHICLE_YAWING - 3;\n}\n"
    for lang, std, comp in (("c", "-std=c99", "gcc"), ("c++", "-std=c++11", "g++")):
        f = tmp_path / ("probe." + ("c" if lang == "c" else "cpp"))
        f.write_text(src)
        r = subprocess.run([comp, "-fsyntax-only", "-x", lang, std, "-Wall", "-pedantic", "-I", os.path.dirname(HDR), str(f)], capture_output=True,
                           text=True)
        assert r.returncode == 0 and not r.stderr.strip(), (lang, r.stderr[-2000:])


def test_the_header_states_the_forward_sensor_and_the_yaw_tick():
    text = " ".join(open(HDR).read().replace("\n *", " ").split())
    for phrase in ("f = c dx + s dy, l = c dy - s dx, u = dz", "f > 0 and fabs(l) <= f tan_half_h and fabs(u) <= f tan_half_v",
                   "diff = fmod(diff + pi, 2 pi)", "|diff| < 0.04", "1 <= ticks <= 65536", "GOAL_REACHED becomes YAWING"):
        assert phrase in text, phrase
    assert "Not supported: yaw" not in text and "the fleet has no yaw" not in text


def test_struct_layouts_equal_the_numpy_dtypes(tmp_path):
    fields = {"fh_heading": abi.heading_dtype, "fh_yaw_params": abi.yaw_params_dtype}
    lines = ["#include <stdio.h>", "#include <stddef.h>", "#include \"fasterhip.h\"", "int main(void) {"]
    for struct, dt in fields.items():
        lines.append("  printf(\"%s %%zu\\n\", sizeof(%s));" % (struct, struct))
        for name in dt.names:
            lines.append("  printf(\"%s.%s %%zu\\n\", offsetof(%s, %s));" % (struct, name, struct, name))
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.dirname(HDR), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for struct, dt in fields.items():
        assert int(got[struct]) == dt.itemsize and dt.itemsize % 8 == 0, (struct, got[struct], dt.itemsize)
        for name in dt.names:
            assert int(got["%s.%s" % (struct, name)]) == dt.fields[name][1], (struct, name)
    assert abi.heading_dtype.itemsize % 16 == 0
    assert abi.FH_VEHICLE_YAWING == 3 == hm.YAWING
    yp = abi.default_yaw_params()
    assert (float(yp["w_max"]), float(yp["alpha_filter_dyaw"]), float(yp["dc"])) == (4.0, 0.0, 0.01)


def test_heading_symbols_are_exported_and_bound(built):
    from faster_amd import capi
    from faster_amd.fleet import Fleet

    L = ctypes.CDLL(built.SO)
    for name in NEW:
        assert hasattr(L, name), name
        assert name in capi.SYMBOLS, name
    for method in ("fleet_heading_init_device", "fleet_set_headings_device", "fleet_set_goals_device", "fleet_next_goals_yaw_device",
                   "fleet_sense_fov_device"):
        assert hasattr(capi.Context, method), method
    for method in ("enable_heading", "set_goals", "headings", "goal_yaw"):
        assert hasattr(Fleet, method), method


def test_heading_entry_points_without_a_device(built):
    """Arguments first (FH_ERR_ARG = -1), then the missing device (FH_ERR_DEVICE = -2): never a CPU path.  Attaching records only stores
    a pointer, so it succeeds without a device, as setting views does."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from faster_amd import capi

    L = capi.lib()
    h = ctypes.c_void_p()
    assert L.fh_create(ctypes.byref(h), -1) == -2 and h.value
    dummy = np.zeros(4096, dtype=np.uint8)
    d = abi.ptr(dummy)
    g = np.zeros(1, dtype=abi.voxel_grid_dtype)
    g["origin"], g["res"], g["dims"] = (0, 0, 0), 0.2, (8, 8, 4)
    par = abi.default_fleet_params()
    yp = abi.default_yaw_params()
    bad_yp = yp.copy()
    bad_yp["dc"] = 0.0
    fake_map = ctypes.c_void_p(1)
    try:
        assert L.fh_fleet_set_headings_device(None, d, 4) == -1
        assert L.fh_fleet_set_headings_device(h, d, 0) == -1
        assert L.fh_fleet_set_headings_device(h, d, 4) == 0 and L.fh_fleet_set_headings_device(h, None, 0) == 0
        assert L.fh_fleet_heading_init_device(h, None, -1, d) == -1
        assert L.fh_fleet_heading_init_device(h, None, 4, d) == -2
        assert L.fh_fleet_set_goals_device(h, None, d, d, None, 4) == -1
        assert L.fh_fleet_set_goals_device(h, abi.ptr(par), d, d, None, 4) == -2
        for ticks in (0, -1, 65537):
            assert L.fh_fleet_next_goals_yaw_device(h, abi.ptr(yp), d, d, d, 4, 8, ticks, 1, d, d) == -1, ticks
        assert L.fh_fleet_next_goals_yaw_device(h, abi.ptr(bad_yp), d, d, d, 4, 8, 1, 1, d, d) == -1
        assert L.fh_fleet_next_goals_yaw_device(h, None, d, d, d, 4, 8, 1, 1, d, d) == -1
        for ticks in (1, 65536):
            assert L.fh_fleet_next_goals_yaw_device(h, abi.ptr(yp), d, d, d, 4, 8, ticks, 1, d, d) == -2, ticks
        for th, tv in ((0.0, 0.5), (1.0, 0.0), (-1.0, 0.5), (float("nan"), 0.5), (1.0, float("inf"))):
            assert L.fh_fleet_sense_fov_device(h, fake_map, 3.0, abi.ptr(g), d, 256, None, 4, d, 4, d, th, tv) == -1, (th, tv)
        assert L.fh_fleet_sense_fov_device(h, fake_map, 3.0, abi.ptr(g), d, 256, None, 4, d, 4, None, 1.0, 0.5) == -1   # no headings
        assert L.fh_fleet_sense_fov_device(h, fake_map, 3.0, abi.ptr(g), d, 256, None, 4, d, 4, d, 1.0, 0.5) == -2
    finally:
        L.fh_destroy(h)


# ---- the yaw tick: the Python model against fhreplan::Planner built by g++ ----
def planner_ticks(tmp_path, cases):
    """tests/cpp/test_heading_yaw.cpp on `cases`: per case the list of (yaw, dyaw, status) per tick."""
    host = os.path.join(ROOT, "faster_amd", "host")
    src, exe = os.path.join(ROOT, "tests", "cpp", "test_heading_yaw.cpp"), str(tmp_path / "test_heading_yaw")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", host, src,
                           os.path.join(host, "corridor_frontend.cpp"), "-fopenmp", "-o", exe])
    inp, outp = tmp_path / "yaw_cases.bin", tmp_path / "yaw_cases.out"
    with open(inp, "wb") as f:
        f.write(np.array([len(cases)], dtype=np.int32).tobytes())
        for c in cases:
            f.write(np.array([c["status"], len(c["plan_xy"]), c["ticks"], c["follow"]], dtype=np.int32).tobytes())
            f.write(np.array([c["alpha"], c["w_max"], c["dc"], c["yaw"], c["previous_yaw"], c["dyaw_filtered"], c["g_term"][0], c["g_term"][1],
                              c["look_at"][0], c["look_at"][1]], dtype=np.float64).tobytes())
            f.write(np.asarray(c["plan_xy"], dtype=np.float64).tobytes())
    r = subprocess.run([exe, str(inp), str(outp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = np.fromfile(outp, dtype=np.float64).reshape(-1, 3)
    out, pos = [], 0
    for c in cases:
        out.append(raw[pos:pos + c["ticks"]])
        pos += c["ticks"]
    assert pos == len(raw)
    return out


def test_the_yaw_model_equals_the_host_planner_tick_by_tick(tmp_path):
    """600 random sequences: all four statuses, alpha 0 and 0.92, follow on and off, plans of 1 .. 30 states, 1 .. 80 ticks, targets in
    every direction (some exactly behind or exactly ahead: diff = +-pi, 0).  yaw, dyaw and status after EVERY tick are equal, bit for bit."""
    rng = np.random.default_rng(20)
    cases = []
    for k in range(600):
        n_plan = int(rng.integers(1, 31))
        start = rng.uniform(-5, 5, size=2)
        plan_xy = start + np.cumsum(rng.uniform(-0.05, 0.05, size=(n_plan, 2)), axis=0)
        yaw = float(rng.uniform(-7, 7))
        c = {"status": k % 4, "plan_xy": plan_xy, "ticks": int(rng.integers(1, 81)), "follow": int(rng.integers(0, 2)), "alpha": (0.0, 0.92)[(k // 4) % 2],
             "w_max": 4.0, "dc": 0.01, "yaw": yaw, "previous_yaw": yaw + float(rng.uniform(-0.1, 0.1)), "dyaw_filtered": float(rng.uniform(-4, 4)),
             "g_term": rng.uniform(-8, 8, size=2), "look_at": rng.uniform(-8, 8, size=2)}
        if k % 25 == 0:   # exactly ahead / behind along x from a plan that does not move in y: atan2 = 0 or pi, yaw = 0
            c["plan_xy"] = np.stack([np.linspace(0, 0.3, n_plan), np.zeros(n_plan)], axis=1)
            c["yaw"] = c["previous_yaw"] = 0.0
            c["g_term"] = c["look_at"] = np.array([5.0 if k % 50 == 0 else -5.0, 0.0])
        cases.append(c)
    got = planner_ticks(tmp_path, cases)
    seen, transitions = set(), 0
    for c, g in zip(cases, got):
        h = {"yaw": c["yaw"], "previous_yaw": c["previous_yaw"], "dyaw_filtered": c["dyaw_filtered"], "goal_yaw": 0.0, "goal_dyaw": 0.0,
             "look_at": [float(c["look_at"][0]), float(c["look_at"][1]), 0.0]}
        st, log, _ = hm.yaw_ticks(c["status"], h, [float(c["g_term"][0]), float(c["g_term"][1])], [tuple(map(float, p)) for p in c["plan_xy"]],
                                  c["ticks"], c["follow"], c["w_max"], c["alpha"], c["dc"])
        want = np.array([(y, d, float(s)) for y, d, s in log])
        assert want.tobytes() == g.tobytes(), (c["status"], c["alpha"], c["follow"], want[:3], g[:3])
        seen.add((c["status"], c["alpha"], c["follow"]))
        transitions += int(c["status"] == hm.YAWING and st == hm.TRAVELING)
    assert len(seen) == 16 and transitions > 20, (len(seen), transitions)


def test_angle_wrap_and_the_goal_reached_tick():
    assert hm.angle_wrap(0.0) == 0.0 and hm.angle_wrap(3 * math.pi) == hm.angle_wrap(math.pi) == -math.pi
    assert abs(hm.angle_wrap(-3.5) - (2 * math.pi - 3.5)) < 1e-15
    h = {"yaw": 0.3, "previous_yaw": 0.7, "dyaw_filtered": 1.5, "goal_yaw": 0.0, "goal_dyaw": 0.0, "look_at": [1.0, 1.0, 0.0]}
    st, log, near = hm.yaw_ticks(hm.GOAL_REACHED, h, [0.0, 0.0], [(0.0, 0.0)], 3, 1, 4.0, 0.0, 0.01)
    assert st == hm.GOAL_REACHED and log == [(0.7, 0.0, hm.GOAL_REACHED)] * 3 and h["dyaw_filtered"] == 1.5 and h["yaw"] == 0.7 and near == 0
    # YAWING straight at the goal: TRAVELING on the first tick, and the tick still turns by w_max dc
    h = {"yaw": 0.0, "previous_yaw": 0.0, "dyaw_filtered": 0.0, "goal_yaw": 0.0, "goal_dyaw": 0.0, "look_at": [0.0, 9.0, 0.0]}
    st, log, near = hm.yaw_ticks(hm.YAWING, h, [5.0, 0.01], [(0.0, 0.0)], 1, 0, 4.0, 0.0, 0.01)
    assert st == hm.TRAVELING and log == [(0.04, 4.0, hm.TRAVELING)] and h["yaw"] == 0.0 and near == 0


def test_set_goals_model():
    v = np.zeros(4, dtype=abi.vehicle_dtype)
    v["status"] = [0, 1, 2, 3]
    v["state"]["pos"] = [[0, 0, 1], [1, 1, 1], [2, 2, 1], [3, 3, 1]]
    goals = np.array([[1.0, 0.5, 1.2], [30.0, 2.0, 1.0], [2.0, -20.0, 1.5], [3.5, 3.0, 9.0]])
    out = hm.set_goals(v, goals, None, (8.0, 8.0, 4.0))
    assert list(out["status"]) == [0, 1, 3, 3]
    assert np.array_equal(out["g_term"], goals)
    assert np.array_equal(out["goal"][0], goals[0])                       # inside the box: itself
    assert out["goal"][1][0] == 5.0 and out["goal"][2][1] == -2.0 and out["goal"][3][2] == 3.0   # on the face crossed
    masked = hm.set_goals(v, goals, [0, 0, 1, 0], (8.0, 8.0, 4.0))
    assert list(masked["status"]) == [0, 1, 3, 3] and np.array_equal(masked["g_term"][[0, 1, 3]], v["g_term"][[0, 1, 3]])


# ---- the forward sensor model on an empty map, dir = (1, 0): the closed form ----
@pytest.mark.parametrize("th,tv", [(1.0, 0.5), (0.1, 0.1), (50.0, 50.0)])
def test_forward_model_on_an_empty_map_is_the_closed_form(th, tv):
    res, dims, origin = 0.25, (12, 40, 40), np.array([0.1, -0.05, 0.02])
    occ = np.zeros(dims, dtype=np.int8)
    view = np.ones(dims, dtype=np.uint8)
    p = np.array([5.13, 4.96, 1.41])
    hidden, out = hm.sense_fov(view[None], None, [p], [(1.0, 0.0)], th, tv, 3.0, origin, res, occ, origin, res)
    iz, iy, ix = np.meshgrid(np.arange(dims[0]), np.arange(dims[1]), np.arange(dims[2]), indexing="ij")
    dx, dy, dz = (ix + 0.5) * res + origin[0] - p[0], (iy + 0.5) * res + origin[1] - p[1], (iz + 0.5) * res + origin[2] - p[2]
    in_range = np.sqrt(dx * dx + dy * dy + dz * dz) < 3.0
    want = in_range & (dx > 0) & (np.abs(dy) <= dx * th) & (np.abs(dz) <= dx * tv)
    assert hidden == 0 and want.sum() > 10 and out == int((in_range & ~want).sum()) > 0
    assert np.array_equal(view == 0, want)
    # every cleared cell lies in the box the kernel scans, which is not the whole sphere for a narrow sensor
    (lx, hx), (ly, hy), (lz, hz) = hm.scan_box(p, (1.0, 0.0), th, tv, 3.0)
    assert (dx[want] >= lx).all() and (dx[want] <= hx).all() and (dy[want] >= ly).all() and (dy[want] <= hy).all()
    assert (dz[want] >= lz).all() and (dz[want] <= hz).all() and lx == 0.0
    # dir = None is the omnidirectional model; a dir that is not finite sees nothing
    import sense_model

    a, b = np.ones(dims, dtype=np.uint8), np.ones(dims, dtype=np.uint8)
    hm.sense_fov(a[None], None, [p], None, th, tv, 3.0, origin, res, occ, origin, res)
    sense_model.sense(b[None], None, [p], 3.0, origin, res, occ, origin, res)
    assert np.array_equal(a, b) and np.array_equal(a == 0, in_range)
    c = np.ones(dims, dtype=np.uint8)
    hm.sense_fov(c[None], None, [p], [(float("nan"), 0.0)], th, tv, 3.0, origin, res, occ, origin, res)
    assert c.all()


def test_the_scan_box_holds_the_frustum_for_any_heading():
    rng = np.random.default_rng(3)
    for _ in range(200):
        a = float(rng.uniform(-math.pi, math.pi))
        th, tv, r = float(rng.choice([0.1, 0.5, 1.0, 3.0, 50.0])), float(rng.choice([0.1, 0.5, 50.0])), 3.0
        c, s = math.cos(a), math.sin(a)
        d = rng.uniform(-r, r, size=(4000, 3))
        f, l = c * d[:, 0] + s * d[:, 1], c * d[:, 1] - s * d[:, 0]
        keep = (np.linalg.norm(d, axis=1) < r) & (f > 0) & (np.abs(l) <= f * th) & (np.abs(d[:, 2]) <= f * tv)
        box = hm.scan_box((0, 0, 0), (c, s), th, tv, r)
        for ax in range(3):
            assert (d[keep, ax] >= box[ax][0] - 1e-12).all() and (d[keep, ax] <= box[ax][1] + 1e-12).all(), (a, th, tv, ax)


def test_gpu_yaw_inputs_keep_clear_of_every_threshold():
    """The condition the GPU yaw test rests on (tests/test_gpu_fleet_heading.py): on its inputs no tick has a wrapped diff within 1e-9
    of 0, +-0.04 or +-pi, so a last-bit difference between the device's atan2 and the host's cannot change a result.  The seed
    (heading_model.YAW_SEED) was chosen so that this holds; the inputs still hold what the test is about."""
    case = hm.yaw_case()
    assert len(case["status"]) == 257 and set(case["status"]) == {0, 1, 2, 3} and case["size"].min() == 1 and case["size"].max() == 40
    total, ended = 0, 0
    for ticks in hm.YAW_TICKS:
        for follow in (0, 1):
            for alpha in (0.0, 0.92):
                st, _, near = hm.yaw_case_model(case, ticks, follow, alpha)
                total += near
                ended += int(((case["status"] == hm.YAWING) & (st == hm.TRAVELING)).sum())
                if ticks == 1:
                    assert ((case["status"] == hm.YAWING) & (st == hm.YAWING)).any()   # (some still turning)
    assert total == 0, total
    assert ended > 0
