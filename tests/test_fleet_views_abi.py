"""CPU-side checks of unknown-voxel views and sensing (fh_set_unknown_views_device, fh_fleet_sense_device): declared in
include/fasterhip.h, exported by the library, bound in faster_amd/capi.py, no CPU path without a device; and the numpy restatement of the
sensor model (tests/sense_model.py), which the GPU tests compare the device against byte for byte, on cases built by hand."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from faster_amd import abi

import sense_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "fasterhip.h")
NEW = ["fh_set_unknown_views_device", "fh_fleet_sense_device", "fh_set_sense_staging", "fh_map_occupancy_bits_device"]


@pytest.fixture(scope="module")
def built():
    from faster_amd import build as fb

    fb.build_all()
    return fb


def test_view_entry_points_are_declared_and_the_header_compiles_alone(tmp_path):
    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    declared = set(re.findall(r"\b(fh_[a-z_0-9]+)\s*\(", text))
    for name in NEW:
        assert name in declared, name
    src = "#include \"fasterhip.h\"\nint main(void) {\n" + "".join("  (void)%s;\n" % n for n in NEW) + "  return 0;\n}\n"
    for lang, std, comp in (("c", "-std=c99", "gcc"), ("c++", "-std=c++11", "g++")):
        f = tmp_path / ("probe." + ("c" if lang == "c" else "cpp"))
        f.write_text(src)
        r = subprocess.run([comp, "-fsyntax-only", "-x", lang, std, "-Wall", "-pedantic", "-I", os.path.dirname(HDR), str(f)], capture_output=True,
                           text=True)
        assert r.returncode == 0 and not r.stderr.strip(), (lang, r.stderr[-2000:])


def test_the_header_states_the_sensor_model():
    text = " ".join(open(HDR).read().replace("\n *", " ").split())
    for phrase in ("|q - p| < r_sense", "K = max(1, ceil(|q - p| / (0.5 res_map)))", "a point outside the map is free", "the map cell of q itself", "knowledge only grows",
                   "NOT supported with views"):
        assert phrase in text, phrase


def test_view_symbols_are_exported_and_bound(built):
    from faster_amd import capi

    L = ctypes.CDLL(built.SO)
    for name in NEW:
        assert hasattr(L, name), name
        assert name in capi.SYMBOLS, name
    for method in ("set_unknown_views_device", "fleet_sense_device", "set_sense_staging"):
        assert hasattr(capi.Context, method), method
    from faster_amd.fleet import Fleet

    for method in ("set_unknown_views", "sense", "views"):
        assert hasattr(Fleet, method), method


def test_view_entry_points_without_a_device(built):
    """Arguments are checked first (FH_ERR_ARG = -1), then the missing device is reported (FH_ERR_DEVICE = -2): never a CPU path.  Setting
    views only records pointers, so it succeeds on a context without a device, like fh_set_unknown_grid_device; what it refuses, it refuses."""
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
    bad = g.copy()
    bad["res"] = 0.0
    fake_map = ctypes.c_void_p(1)   # (never dereferenced: without a device the call returns before the map is read)
    try:
        assert L.fh_set_unknown_views_device(None, abi.ptr(g), d, 256, None, 4) == -1
        assert L.fh_set_unknown_views_device(h, abi.ptr(g), d, 255, None, 4) == -1      # stride smaller than a view
        assert b"view_stride" in L.fh_last_error(h)
        assert L.fh_set_unknown_views_device(h, abi.ptr(g), d, 256, None, 0) == -1      # no views
        assert L.fh_set_unknown_views_device(h, abi.ptr(bad), d, 256, None, 4) == -1
        assert L.fh_set_unknown_views_device(h, None, d, 256, None, 4) == -1
        assert L.fh_set_unknown_views_device(h, abi.ptr(g), d, 256, None, 4) == 0
        assert L.fh_set_unknown_views_device(h, None, None, 0, None, 0) == 0            # back to none
        assert L.fh_set_sense_staging(h, 2) == -1 and L.fh_set_sense_staging(h, 0) == 0 and L.fh_set_sense_staging(None, 1) == -1
        assert L.fh_fleet_sense_device(h, None, 3.0, abi.ptr(g), d, 256, None, 4, d, 4) == -1                 # no map
        assert L.fh_fleet_sense_device(h, fake_map, 0.0, abi.ptr(g), d, 256, None, 4, d, 4) == -1             # r_sense
        assert L.fh_fleet_sense_device(h, fake_map, float("nan"), abi.ptr(g), d, 256, None, 4, d, 4) == -1
        assert L.fh_fleet_sense_device(h, fake_map, 3.0, abi.ptr(bad), d, 256, None, 4, d, 4) == -1           # the lattice
        assert L.fh_fleet_sense_device(h, fake_map, 3.0, abi.ptr(g), d, 255, None, 4, d, 4) == -1             # the stride
        assert L.fh_fleet_sense_device(h, fake_map, 3.0, abi.ptr(g), d, 256, None, 0, d, 4) == -1             # no views
        assert L.fh_fleet_sense_device(h, fake_map, 3.0, abi.ptr(g), d, 256, None, 4, d, 4) == -2
        assert L.fh_map_occupancy_bits_device(None, d, None) == -1
    finally:
        L.fh_destroy(h)


# ---- the numpy sensor model on cases built by hand: lattice = map = 20 x 20 x 5 cells of 0.5 m from the origin ----
RES, DIMS = 0.5, (5, 20, 20)   # [nz][ny][nx]
ORIGIN = np.zeros(3)


def centres():
    iz, iy, ix = np.meshgrid(np.arange(DIMS[0]), np.arange(DIMS[1]), np.arange(DIMS[2]), indexing="ij")
    return np.stack([(ix + 0.5) * RES, (iy + 0.5) * RES, (iz + 0.5) * RES], axis=-1)


def test_model_open_space_clears_exactly_the_sphere():
    view = np.ones(DIMS, dtype=np.uint8)
    occ = np.zeros(DIMS, dtype=np.int8)
    p = np.array([5.1, 4.9, 1.2])
    hidden = sense_model.sense(view[None], None, [p], 2.0, ORIGIN, RES, occ, ORIGIN, RES)
    inside = np.linalg.norm(centres() - p, axis=-1) < 2.0
    assert hidden == 0 and inside.sum() > 100
    assert np.array_equal(view == 0, inside)


def test_model_a_wall_hides_what_is_behind_it_and_its_first_layer_becomes_known():
    view = np.ones(DIMS, dtype=np.uint8)
    occ = np.zeros(DIMS, dtype=np.int8)
    occ[:, :, 12:14] = 100            # a wall two cells thick across the whole map: x in [6, 7)
    p = np.array([4.25, 5.25, 1.25])  # a cell centre, 1.75 m in front of the wall
    hidden = sense_model.sense(view[None], None, [p], 4.0, ORIGIN, RES, occ, ORIGIN, RES)
    in_range = np.linalg.norm(centres() - p, axis=-1) < 4.0
    assert hidden > 0
    assert (view[:, :, :12][in_range[:, :, :12]] == 0).all()          # everything in front of the wall and in range is seen
    # the wall's first layer becomes known where the ray meets it first: straight ahead and around (a slanted ray passes through a
    # neighbouring cell of the wall before it reaches its end point, so the far parts of the first layer stay unknown)
    assert view[2, 10, 12] == 0 and (view[:, 7:14, 12] == 0).all()
    assert (view[:, :, 13:][in_range[:, :, 13:]] == 1).all()          # its second layer and everything behind it stay unknown
    assert in_range[:, :, 14:].any()
    assert (view[~in_range] == 1).all()
    before = view.copy()
    sense_model.sense(view[None], None, [p], 4.0, ORIGIN, RES, occ, ORIGIN, RES)   # looking again changes nothing
    assert np.array_equal(view, before)


def test_model_vehicle_outside_the_lattice_and_tiny_range():
    occ = np.zeros(DIMS, dtype=np.int8)
    view = np.ones(DIMS, dtype=np.uint8)
    # far outside: nothing; just outside: the part of the sphere that reaches in (a ray is free where it runs outside the map)
    sense_model.sense(view[None], None, [np.array([-30.0, 4.0, 1.0])], 3.0, ORIGIN, RES, occ, ORIGIN, RES)
    assert view.all()
    p = np.array([-1.0, 4.0, 1.0])
    sense_model.sense(view[None], None, [p], 3.0, ORIGIN, RES, occ, ORIGIN, RES)
    inside = np.linalg.norm(centres() - p, axis=-1) < 3.0
    assert inside.any() and np.array_equal(view == 0, inside)
    # r_sense smaller than a cell: only a centre closer than r_sense — none from a corner, the vehicle's own cell from near its centre
    view = np.ones(DIMS, dtype=np.uint8)
    sense_model.sense(view[None], None, [np.array([5.0, 5.0, 1.0])], 0.2, ORIGIN, RES, occ, ORIGIN, RES)
    assert view.all()
    sense_model.sense(view[None], None, [np.array([5.3, 5.2, 1.2])], 0.2, ORIGIN, RES, occ, ORIGIN, RES)
    assert (view == 0).sum() == 1 and view[2, 10, 10] == 0
    # not a finite position: nothing
    sense_model.sense(view[None], None, [np.array([np.nan, 5.0, 1.0])], 3.0, ORIGIN, RES, occ, ORIGIN, RES)
    assert (view == 0).sum() == 1


def test_model_shared_views_take_the_union_and_flags_never_come_back():
    occ = np.zeros(DIMS, dtype=np.int8)
    occ[:, 8:12, 10] = 100
    pos = [np.array([3.0, 5.0, 1.0]), np.array([7.5, 5.0, 1.0]), np.array([3.0, 5.0, 1.0])]
    views = np.ones((2,) + DIMS, dtype=np.uint8)
    sense_model.sense(views, [0, 0, 1], pos, 2.5, ORIGIN, RES, occ, ORIGIN, RES)
    alone = np.ones((3,) + DIMS, dtype=np.uint8)
    sense_model.sense(alone, None, pos, 2.5, ORIGIN, RES, occ, ORIGIN, RES)
    assert np.array_equal(views[0], alone[0] & alone[1]) and np.array_equal(views[1], alone[2])
    assert not np.array_equal(views[0], views[1])
    before = views.copy()
    sense_model.sense(views, [0, 0, 1], [q + 0.4 for q in pos], 2.5, ORIGIN, RES, occ, ORIGIN, RES)
    assert not ((before == 0) & (views != 0)).any() and (views != before).any()
