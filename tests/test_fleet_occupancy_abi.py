"""CPU-side checks of occupied space per view (fh_map_read_views_device, fh_map_plan_batch_radius_views_device,
fh_set_point_views_device, fh_fleet_observe_device): declared in include/fasterhip_occupancy.h, exported, bound in faster_amd/capi.py, their
argument prologue in the order of tests/test_abi_return_codes.py and no CPU path without a device; and the numpy restatement of
observing (tests/occupancy_model.py) on cases built by hand."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from faster_amd import abi

import occupancy_model as om

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "fasterhip.h")
OCC_HDR = os.path.join(ROOT, "include", "fasterhip_occupancy.h")
NEW = ["fh_map_read_views_device", "fh_map_plan_batch_radius_views_device", "fh_set_point_views_device", "fh_fleet_observe_device"]
OK, ARG, DEV = 0, -1, -2


@pytest.fixture(scope="module")
def built():
    from faster_amd import build as fb

    fb.build_all()
    return fb


def test_occupancy_entry_points_are_declared_and_the_header_compiles_alone(tmp_path):
    text = re.sub(r"/\*.*?\*/", "", open(OCC_HDR).read(), flags=re.S)
    declared = set(re.findall(r"\b(fh_[a-z_0-9]+)\s*\(", text))
    for name in NEW:
        assert name in declared, name
    src = "#include \"fasterhip_occupancy.h\"\nint main(void) {\n" + "".join("  (void)%s;\n" % n for n in NEW) + "  return 0;\n}\n"
    for lang, std, comp in (("c", "-std=c99", "gcc"), ("c++", "-std=c++11", "g++")):
        f = tmp_path / ("probe." + ("c" if lang == "c" else "cpp"))
        f.write_text(src)
        r = subprocess.run([comp, "-fsyntax-only", "-x", lang, std, "-Wall", "-pedantic", "-I", os.path.dirname(HDR), str(f)], capture_output=True,
                           text=True)
        assert r.returncode == 0 and not r.stderr.strip(), (lang, r.stderr[-2000:])


def test_the_header_states_the_model_and_its_limit():
    text = " ".join(open(HDR).read().replace("\n *", " ").split())
    assert "Not supported: a map of occupied space per vehicle" not in text
    for phrase in ("bit k & 31 of word k >> 5", "floor((x - origin) / res) per axis", "is never observed", "Nothing is ever cleared",
                   "the caller chooses the world inflation accordingly", "words_per_view * 4 + mask_words * 4"):
        assert phrase in text, phrase
    assert int(re.search(r"#define FH_ABI_VERSION (\d+)", open(HDR).read()).group(1)) == abi.FH_ABI_VERSION >= 9


def test_occupancy_symbols_are_exported_and_bound(built):
    from faster_amd import capi
    from faster_amd.fleet import Fleet

    L = ctypes.CDLL(built.SO)
    for name in NEW:
        assert hasattr(L, name), name
        assert name in capi.OCCUPANCY_SYMBOLS, name
    for method in ("set_point_views_device", "fleet_observe_device"):
        assert hasattr(capi.Context, method), method
    for method in ("read_views_device", "plan_batch_radius_views_device", "view_occupancy"):
        assert hasattr(capi.Map, method), method
    for method in ("set_point_views", "observe", "point_masks"):
        assert hasattr(Fleet, method), method


def test_the_argument_prologue_in_order(built):
    """null context, then n_views <= 0, then mask_words * 32 < n_cloud, then — every argument in order — FH_ERR_DEVICE on a context
    without a device: never a CPU path.  Attaching masks only records pointers, so it succeeds without a device, as attaching views does;
    the corridor entry points then check the masks against their cloud before they ask for the device."""
    from faster_amd import capi

    L = capi.lib()
    h = ctypes.c_void_p()
    assert L.fh_create(ctypes.byref(h), 1 << 20) == DEV and h.value
    buf = np.zeros(4096, dtype=np.uint8)
    d = abi.ptr(buf)
    g = np.zeros(1, dtype=abi.voxel_grid_dtype)
    g["origin"], g["res"], g["dims"] = (0, 0, 0), 0.2, (8, 8, 4)
    bad = g.copy()
    bad["res"] = 0.0
    gp, bbox = abi.ptr(g), abi.ptr(np.array([2.0, 2.0, 1.0]))
    cells, center = np.array([8, 8, 4], dtype=np.int32), np.zeros(3)
    try:
        # fh_fleet_observe_device(ctx, grid, flags, stride, view_of, n_views, cloud, n_cloud, mask, mask_words)
        assert L.fh_fleet_observe_device(None, gp, d, 256, None, 4, d, 64, d, 2) == ARG
        assert L.fh_fleet_observe_device(None, gp, d, 256, None, 0, d, 65, d, 2) == ARG
        assert L.fh_fleet_observe_device(h, gp, d, 256, None, 0, d, 64, d, 2) == ARG
        assert L.fh_fleet_observe_device(h, gp, d, 256, None, -1, d, 64, d, 2) == ARG
        assert L.fh_fleet_observe_device(h, gp, d, 256, None, 4, d, 65, d, 2) == ARG      # 2 words hold 64 bits
        assert L.fh_fleet_observe_device(h, gp, d, 256, None, 4, d, -1, d, 2) == ARG
        assert L.fh_fleet_observe_device(h, abi.ptr(bad), d, 256, None, 4, d, 64, d, 2) == ARG
        assert L.fh_fleet_observe_device(h, None, d, 256, None, 4, d, 64, d, 2) == ARG
        assert L.fh_fleet_observe_device(h, gp, d, 255, None, 4, d, 64, d, 2) == ARG      # stride smaller than a view
        assert b"view_stride" in L.fh_last_error(h)
        assert L.fh_fleet_observe_device(h, gp, d, 256, None, 4, d, 64, d, 2) == DEV
        assert L.fh_fleet_observe_device(h, gp, d, 256, None, 4, d, 0, d, 0) == DEV       # (an empty cloud is looked at after the device)
        assert L.fh_fleet_observe_device(h, gp, None, 256, None, 4, None, 64, None, 2) == DEV   # (pointers too)
        # fh_set_point_views_device(ctx, mask, mask_words, view_of, n_views)
        assert L.fh_set_point_views_device(None, d, 2, None, 4) == ARG
        assert L.fh_set_point_views_device(h, d, 2, None, 0) == ARG
        assert L.fh_set_point_views_device(h, d, 0, None, 4) == ARG
        assert L.fh_set_point_views_device(h, d, 2, None, 4) == OK
        # attached: 2 words cover 64 points
        corridor = lambda n_cloud: L.fh_corridor_batch_device(h, d, n_cloud, d, d, 4, 8, 4, bbox, 0.05, 0.0, 96, d, d, d, None)  # noqa: E731
        safe = lambda n_cloud: L.fh_safe_corridor_batch_device(h, d, d, d, d, 4, d, d, n_cloud, gp, 4, 0.5, 3, bbox, 0.05, 0.0, 96, 6, d, d, None, None)  # noqa: E731
        assert corridor(64) == DEV and corridor(65) == ARG and b"point masks" in L.fh_last_error(h)
        assert corridor(-1) == ARG and safe(64) == DEV and safe(65) == ARG
        assert L.fh_solve_pairs_device(h, d, d, 4, 10, 64, 0.5, 0.2, 3, d, d, d, d) == DEV   # (the refusal needs the device's checks first, as for views)
        assert L.fh_set_point_views_device(h, None, 0, None, 0) == OK                      # detached
        assert corridor(65) == DEV and safe(65) == DEV
        # the map entry points: no map exists without a device, so what they say to no map
        assert L.fh_map_read_views_device(None, d, 64, d, 2, 4, abi.ptr(cells), 0.2, abi.ptr(center), 0.0, 3.0, 0.3) == ARG
        assert L.fh_map_plan_batch_radius_views_device(None, d, d, d, None, 4, 16, 0.0, 0, d, d, d, None, 4) == ARG
        assert L.fh_map_view_occupancy(None, 0, d) == ARG
    finally:
        L.fh_destroy(h)


# ---- the numpy model on cases built by hand: a lattice of 4 x 3 x 2 cells of 0.5 m from (1, 1, 0) ----
def test_model_bit_layout_round_trip():
    rng = np.random.default_rng(3)
    for n in (1, 31, 32, 33, 64, 65):
        known = rng.random((3, n)) < 0.5
        m = om.pack(known)
        assert m.shape == (3, (n + 31) // 32) and m.dtype == np.uint32
        assert np.array_equal(om.unpack(m, n), known)
        for v in range(3):
            for k in range(n):
                assert bool((int(m[v, k >> 5]) >> (k & 31)) & 1) == bool(known[v, k])


def test_model_faces_outside_and_not_finite():
    origin, res = np.array([1.0, 1.0, 0.0]), 0.5
    views = np.ones((2, 2, 3, 4), dtype=np.uint8)
    views[0, 0, 0, 0] = 0            # view 0 knows cell (0, 0, 0) and cell (3, 2, 1)
    views[0, 1, 2, 3] = 0
    views[1] = 0                     # view 1 knows everything
    cloud = np.array([[1.0, 1.0, 0.0],        # on the lower faces of cell (0, 0, 0): belongs to it
                      [1.5, 1.0, 0.0],        # on the face between (0, 0, 0) and (1, 0, 0): belongs to (1, 0, 0)
                      [1.25, 1.25, 0.25],     # inside (0, 0, 0)
                      [3.0, 2.5, 1.0],        # on the upper faces of the lattice: outside
                      [2.99, 2.49, 0.99],     # inside (3, 2, 1)
                      [0.999, 1.2, 0.2],      # outside, below x
                      [np.nan, 1.2, 0.2], [1.2, np.inf, 0.2], [1.2, 1.2, -np.inf]])
    mask = np.zeros((2, 1), dtype=np.uint32)
    om.observe(mask, views, cloud, origin, res)
    assert [bool(b) for b in om.unpack(mask, len(cloud))[0]] == [True, False, True, False, True, False, False, False, False]
    assert [bool(b) for b in om.unpack(mask, len(cloud))[1]] == [True, True, True, False, True, False, False, False, False]
    before = mask.copy()
    views[:] = 1                     # forgetting voxels clears nothing
    om.observe(mask, views, cloud, origin, res)
    assert np.array_equal(mask, before)
