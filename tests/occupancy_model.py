"""numpy restatement of fh_fleet_observe_device (include/fasterhip.h) and the bit layout of the point masks: row v of mask [n_views][words]
uint32 holds bit k & 31 of word k >> 5 for cloud point k.  The GPU tests compare the device's masks with this, every word."""
import numpy as np


def words_for(n_cloud):
    return (int(n_cloud) + 31) // 32


def pack(known, words=None):
    """bool [n_views][n_cloud] -> uint32 [n_views][words]"""
    known = np.atleast_2d(np.asarray(known, dtype=bool))
    words = words_for(known.shape[1]) if words is None else words
    padded = np.zeros((known.shape[0], words * 32), dtype=np.uint8)
    padded[:, :known.shape[1]] = known
    return np.packbits(padded, axis=1, bitorder="little").view("<u4").reshape(known.shape[0], words).copy()


def unpack(mask, n_cloud):
    """uint32 [n_views][words] -> bool [n_views][n_cloud]"""
    mask = np.ascontiguousarray(np.atleast_2d(mask), dtype="<u4")
    return np.unpackbits(mask.view(np.uint8), axis=1, bitorder="little")[:, :n_cloud].astype(bool)


def observe(mask, views, cloud, origin, res):
    """ORs into mask [n_views][words] the points of `cloud` whose voxel (floor((x - origin) / res) per axis, in double) lies inside the
    lattice of views [n_views][nz][ny][nx] and is known there (flag byte 0).  Points outside and points that are not finite: never."""
    cloud = np.asarray(cloud, dtype=np.float64).reshape(-1, 3)
    nz, ny, nx = views.shape[1:]
    with np.errstate(invalid="ignore"):
        f = np.floor((cloud - np.asarray(origin, dtype=np.float64)) / float(res))
        inside = (f[:, 0] >= 0) & (f[:, 0] < nx) & (f[:, 1] >= 0) & (f[:, 1] < ny) & (f[:, 2] >= 0) & (f[:, 2] < nz)   # (NaN and infinity fail)
    idx = np.where(inside[:, None], f, 0.0).astype(np.int64)
    seen = (views[:, idx[:, 2], idx[:, 1], idx[:, 0]] == 0) & inside[None, :]
    mask |= pack(seen, mask.shape[1])
    return seen
